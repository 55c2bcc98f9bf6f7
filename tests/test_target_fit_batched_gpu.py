"""scaml_target_mll_batched_f64 / scaml_target_fit_batched_f64 on the MI355X against the single-problem entry points called per
problem: a workgroup of the batched launch runs the instruction sequence the single-problem kernel runs on that problem, on the same
numbers, so the comparison is torch.equal -- ragged sizes, sizes on both sides of the matrix-core limit (n = 112), both
factorisations, S = 1, a problem that is indefinite by construction, and replay from a HIP graph."""
import pytest
import torch

from scamlgp_amd import _lib, hyper, ops
from tests._target_problem import make_target_problem, raw_start

pytestmark = pytest.mark.gpu


def _problem_on_device(prob, device):
    spec = hyper.target_gp_spec()
    return ops.TargetFitProblem(prob["source_means"].to(device), prob["source_covs"].to(device), prob["X"].to(device), prob["y"].to(device),
                                prob["m_all"], prob["s_all"], spec, hyper.GammaPrior(1.0, 1.0), 1e-10, prob["kind"])


@pytest.fixture(params=["matrix-core", "column-by-column"])
def fit_path(request):
    was = _lib.lib.scaml_debug_target_fit_path(1 if request.param == "column-by-column" else 0)
    yield request.param
    _lib.lib.scaml_debug_target_fit_path(was)


def _batch(device, sizes, T, D, kind, B, n_src=16):
    probs = [make_target_problem(n, T, D, kind, seed=31 + s, n_src=n_src) for s, n in enumerate(sizes)]
    tps = [_problem_on_device(p, device) for p in probs]
    z = torch.stack([raw_start(D, T, seed=40 + s, B=B) for s in range(len(sizes))]).to(device)
    return probs, tps, z


CASES = [((5, 12, 12), 4, 3, 1), ((1, 7, 33, 20), 3, 2, 0), ((80, 79, 64), 32, 6, 1), ((112, 113, 40), 5, 3, 1)]


@pytest.mark.parametrize("sizes,T,D,kind", CASES)
def test_batched_objective_equals_the_single_problem_entry(device, fit_path, sizes, T, D, kind):
    _, tps, z = _batch(device, sizes, T, D, kind, B=3)
    batch = ops.TargetFitBatch(tps)
    assert batch.n_max == max(sizes) and batch.n_points.tolist() == list(sizes)
    out = ops.target_mll_batched(batch, z)
    assert out["value"].shape == (len(sizes), 3) and out["grad"].shape == (len(sizes), 3, D + 2 + T)
    assert not bool(out["info"].any()) and bool(torch.isfinite(out["value"]).all())
    for s, tp in enumerate(tps):
        one = ops.target_mll(tp, z[s])
        for k in ("value", "grad", "info", "jitter"):
            assert torch.equal(out[k][s], one[k]), (s, k, (out[k][s] - one[k]).abs().max())


@pytest.mark.parametrize("sizes,T,D,kind", CASES[:3])
def test_batched_refit_equals_the_single_problem_refit(device, fit_path, sizes, T, D, kind):
    _, tps, z0 = _batch(device, sizes, T, D, kind, B=3)
    res = ops.target_fit_batched(ops.TargetFitBatch(tps), z0)
    stats = res["stats"].cpu()
    assert bool((stats[..., 2] != 4).all()) and bool((stats[..., 0] >= 1).all())
    for s, tp in enumerate(tps):
        one = ops.target_fit(tp, z0[s])
        for k in ("z", "value", "stats", "info", "jitter"):
            assert torch.equal(res[k][s], one[k]), (s, k, res[k][s], one[k])


def test_one_study_reproduces_the_single_entry_point(device):
    _, tps, z = _batch(device, (24,), 6, 4, 1, B=4)
    batch = ops.TargetFitBatch(tps)
    a, b = ops.target_mll_batched(batch, z), ops.target_mll(tps[0], z[0])
    assert torch.equal(a["value"][0], b["value"]) and torch.equal(a["grad"][0], b["grad"])
    fa, fb = ops.target_fit_batched(batch, z), ops.target_fit(tps[0], z[0])
    assert torch.equal(fa["z"][0], fb["z"]) and torch.equal(fa["value"][0], fb["value"]) and torch.equal(fa["stats"][0], fb["stats"])


def test_result_layouts_are_the_documented_ones_and_the_starts_are_left_alone(device):
    """What the docstrings of the four ``ops.target_*`` wrappers promise: keys, shapes and dtypes of the results, fresh tensors, and
    z0 unchanged by a refit (the wrappers optimise a copy)."""
    (S, B), T, D = (2, 2), 4, 3
    _, tps, z = _batch(device, (5, 12), T, D, 1, B=B)
    P = D + 2 + T
    batch, z_before = ops.TargetFitBatch(tps), z.clone()
    f64, i32 = torch.float64, torch.int32
    for lead, mll, fit in (((), ops.target_mll(tps[1], z[1]), ops.target_fit(tps[1], z[1])),
                           ((S,), ops.target_mll_batched(batch, z), ops.target_fit_batched(batch, z))):
        want_mll = dict(value=((*lead, B), f64), grad=((*lead, B, P), f64), info=((*lead, B), i32), jitter=((*lead, B), f64))
        want_fit = dict(z=((*lead, B, P), f64), value=((*lead, B), f64), info=((*lead, B), i32), jitter=((*lead, B), f64),
                        stats=((*lead, B, 4), i32))
        for out, want in ((mll, want_mll), (fit, want_fit)):
            assert list(out) == list(want)
            for k, (shape, dtype) in want.items():
                assert tuple(out[k].shape) == shape and out[k].dtype == dtype and out[k].device == z.device, k
                assert out[k].is_contiguous(), k
        assert bool((fit["stats"][..., 0] >= 1).all()) and bool((fit["stats"][..., 3] == 0).all())
        z_in = z[1] if lead == () else z
        assert not torch.equal(fit["z"], z_in) and fit["z"].data_ptr() != z_in.data_ptr()   # the optimiser moved, on its own copy
    assert torch.equal(z, z_before)


def test_an_indefinite_problem_fails_alone(device, fit_path):
    """Problem 1 is indefinite by construction, as tests/test_target_fit_gpu.py builds it: duplicated target points, a source term of
    -6e-8 on the diagonal under 1e-8 noise -- and a NaN weight in one of its starts, which no jitter saves.  That row answers
    info > 0 / NaN / zero gradient; the other start of the problem passes with jitter 1e-7; the neighbours are untouched.  The refit
    moves a start's weights into the box first (a NaN weight becomes the lower bound), so there the NaN sits in a lengthscale."""
    probs = [make_target_problem(12, 3, 2, 0, seed=4 + s) for s in range(3)]
    w = 0.1
    bad = probs[1]
    bad["X"][5] = bad["X"][4]
    bad["X"][7] = bad["X"][4]
    c = 6e-8 * bad["s_all"] ** 2 / (3 * w * w)
    bad["source_covs"] = -c * torch.eye(12, dtype=torch.float64).unsqueeze(-1).repeat(1, 1, 3)
    tps = [_problem_on_device(p, device) for p in probs]
    z = torch.stack([raw_start(2, 3, seed=s, B=2) for s in range(3)])
    z[1, :, 3] = -40.0    # raw noise -> 1e-8
    z[1, :, 2] = 5.0      # outputscale ~ 99
    z[1, :, 4:] = w
    z[1, 1, 4] = float("nan")
    z = z.to(device)
    out = ops.target_mll_batched(ops.TargetFitBatch(tps), z)
    assert out["info"][1, 0].item() == 0 and out["jitter"][1, 0].item() == 1e-7
    assert out["info"][1, 1].item() > 0 and bool(torch.isnan(out["value"][1, 1])) and not bool(out["grad"][1, 1].any())
    for s in (0, 2):
        one = ops.target_mll(tps[s], z[s])
        assert not bool(out["info"][s].any()) and torch.equal(out["value"][s], one["value"]) and torch.equal(out["grad"][s], one["grad"])
    z[1, 1, 4] = w
    z[1, 1, 0] = float("nan")
    fit = ops.target_fit_batched(ops.TargetFitBatch(tps), z)
    assert fit["stats"][1, 1, 2].item() == 4 and bool(torch.isnan(fit["value"][1, 1])) and fit["info"][1, 1].item() > 0
    assert bool(torch.isfinite(fit["value"][1, 0])) and fit["stats"][1, 0, 2].item() != 4
    for s in (0, 2):
        one = ops.target_fit(tps[s], z[s])
        assert bool(torch.isfinite(fit["value"][s]).all())
        assert torch.equal(fit["z"][s], one["z"]) and torch.equal(fit["value"][s], one["value"]) and torch.equal(fit["stats"][s], one["stats"])


def test_batched_refit_is_stream_capturable(device):
    """No host synchronisation inside: the refit of all problems replays from a HIP graph on new targets."""
    _, tps, z0 = _batch(device, (20, 33, 27), 5, 3, 1, B=2)
    batch = ops.TargetFitBatch(tps)
    eager = ops.target_fit_batched(batch, z0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.target_fit_batched(batch, z0)            # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.target_fit_batched(batch, z0)
    y2 = (batch.y * 0.9 + 0.05).contiguous()
    batch.y.copy_(y2)                                # new targets in the captured buffers
    g.replay()
    torch.cuda.synchronize()
    ref = ops.target_fit_batched(batch, z0)
    for k in ("z", "value", "stats"):
        assert torch.equal(out[k], ref[k]), k
    assert float((out["value"] - eager["value"]).abs().max()) > 0.0


def test_argument_contract(device):
    _, tps, z = _batch(device, (5, 9), 3, 2, 0, B=2)
    batch = ops.TargetFitBatch(tps)
    with pytest.raises(ValueError):
        ops.target_mll_batched(batch, z[0])
    with pytest.raises(ValueError):
        ops.target_mll_batched(batch, z[:1])
    other = _problem_on_device(make_target_problem(5, 4, 2, 0), device)
    with pytest.raises(ValueError):
        ops.TargetFitBatch([tps[0], other])
    assert ops.TargetFitBatch.supported(80, 32, 6) and not ops.TargetFitBatch.supported(4000, 3, 2)
