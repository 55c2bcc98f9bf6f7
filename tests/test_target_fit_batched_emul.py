"""CPU checks of the BATCHED target-fit entry (csrc/gp_target_fit.hip: tf_main_batched, the body of scaml_target_fit_batched_kernel)
through a single-threaded host build of the same source (tests/host_emul/target_fit_batched_emul.cpp): S = 3 problems of ragged
size in the (S, ...) layouts of include/scaml_gp.h (8b) -- value and gradient of every (problem, start) against torch autograd
through the oracle's target_train_mll, with the tolerances tests/test_target_fit_emul.py uses for one problem, and against the
single-problem emulation of the same source, problem by problem.  What the slices past n_s hold must not matter: they are filled with
NaN.  The parallel execution is what tests/test_target_fit_batched_gpu.py covers."""
import ctypes

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests._host_emul import DP, IP, build, ptr as _p
from tests._target_problem import TARGET_SPEC, make_target_problem, oracle_mll_and_grad, pack_lower, raw_start


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "target_fit_batched_emul")
    lib.emul_target_fit_batched.restype = ctypes.c_int
    lib.emul_target_fit_batched.argtypes = [DP, DP, DP, DP, IP, DP, DP, DP, DP] + [ctypes.c_int] * 9 + [ctypes.c_double, ctypes.c_double,
                                                                                                    DP, DP, IP, DP, IP]
    lib.emul_target_fit_single.restype = ctypes.c_int
    lib.emul_target_fit_single.argtypes = [DP, DP, DP, DP, ctypes.c_double, ctypes.c_double, DP, DP] + [ctypes.c_int] * 8 + [
        ctypes.c_double, ctypes.c_double, DP, DP, IP, DP, IP]
    for f in (lib.emul_target_fit_batched_lds_doubles, lib.emul_target_fit_problem_lds_doubles):
        f.restype, f.argtypes = ctypes.c_longlong, [ctypes.c_int] * 5
    return lib


def pack_batch(probs, fill=float("nan")):
    """The (S, ...) layouts of (8b) from a list of problem dicts; everything past a problem's n_s is `fill`."""
    S, T, D = len(probs), probs[0]["T"], probs[0]["D"]
    n_max = max(p["n"] for p in probs)
    e_max = n_max * (n_max + 1) // 2
    mt = np.full((S, T, n_max), fill)
    cp = np.full((S, T, e_max), fill)
    X = np.full((S, n_max, D), fill)
    y = np.full((S, n_max), fill)
    for s, p in enumerate(probs):
        n = p["n"]
        mt[s, :, :n] = p["source_means"].transpose(0, 1).numpy()
        cp[s, :, :n * (n + 1) // 2] = pack_lower(p["source_covs"]).numpy()
        X[s, :n] = p["X"].numpy()
        y[s, :n] = p["y"].numpy()
    return dict(means_t=mt, covs_p=cp, X=X, y=y, n_points=np.array([p["n"] for p in probs], dtype=np.int32),
                m_all=np.array([p["m_all"] for p in probs]), s_all=np.array([p["s_all"] for p in probs]), S=S, T=T, D=D, n_max=n_max)


def call_batched(lib, probs, z, mode, max_iter=200, history=10, n_points=None):
    b = pack_batch(probs)
    S, B, P = z.shape
    kind = probs[0]["kind"]
    zz = np.ascontiguousarray(z.numpy().copy())
    spec = np.array(TARGET_SPEC, dtype=np.float64)
    value, grad = np.zeros((S, B)), np.zeros((S, B, P))
    info, jit, stats = np.zeros((S, B), dtype=np.int32), np.zeros((S, B)), np.zeros((S, B, 4), dtype=np.int32)
    npts = b["n_points"] if n_points is None else np.asarray(n_points, dtype=np.int32)
    rc = lib.emul_target_fit_batched(_p(b["means_t"]), _p(b["covs_p"]), _p(b["X"]), _p(b["y"]), _p(npts), _p(b["m_all"]), _p(b["s_all"]),
                                     _p(spec), _p(zz), S, B, b["n_max"], b["T"], b["D"], kind, mode, max_iter, history, 1e-5, 2.2e-9,
                                     _p(value), _p(grad), _p(info), _p(jit), _p(stats))
    assert rc == 0
    return dict(value=value, grad=grad, info=info, jitter=jit, stats=stats, z=zz)


def call_single(lib, prob, z, mode, max_iter=200, history=10):
    B, P = z.shape
    arr = lambda t: np.ascontiguousarray(t.numpy(), dtype=np.float64)   # noqa: E731
    mt, cp = arr(prob["source_means"].transpose(0, 1).contiguous()), arr(pack_lower(prob["source_covs"]))
    X, y, spec, zz = arr(prob["X"]), arr(prob["y"]), np.array(TARGET_SPEC, dtype=np.float64), arr(z.clone())
    value, grad = np.zeros(B), np.zeros((B, P))
    info, jit, stats = np.zeros(B, dtype=np.int32), np.zeros(B), np.zeros((B, 4), dtype=np.int32)
    rc = lib.emul_target_fit_single(_p(mt), _p(cp), _p(X), _p(y), prob["m_all"], prob["s_all"], _p(spec), _p(zz), B, prob["n"], prob["T"],
                                    prob["D"], prob["kind"], mode, max_iter, history, 1e-5, 2.2e-9, _p(value), _p(grad), _p(info), _p(jit),
                                    _p(stats))
    assert rc == 0
    return dict(value=value, grad=grad, info=info, jitter=jit, stats=stats, z=zz)


def ragged_problems(sizes=(5, 12, 12), T=4, D=3, kind=1):
    return [make_target_problem(n, T, D, kind, seed=10 + s) for s, n in enumerate(sizes)]


def starts(S, B, D, T):
    return torch.stack([raw_start(D, T, seed=20 + s, B=B) for s in range(S)])


@pytest.mark.parametrize("kind", [0, 1])
def test_ragged_batch_matches_oracle_autograd_and_the_single_problem_entry(emul, kind):
    probs = ragged_problems(kind=kind)
    S, B, T, D = 3, 2, 4, 3
    z = starts(S, B, D, T)
    out = call_batched(emul, probs, z, mode=0)
    assert not out["info"].any()
    for s in range(S):
        one = call_single(emul, probs[s], z[s], mode=0)
        # the same source on the same numbers in the same order: equal, not close
        assert np.array_equal(out["value"][s], one["value"]) and np.array_equal(out["grad"][s], one["grad"]), s
        assert np.array_equal(out["jitter"][s], one["jitter"])
        for b in range(B):
            val, g = oracle_mll_and_grad(probs[s], z[s, b])
            np.testing.assert_allclose(out["value"][s, b], float(val), rtol=1e-9)
            np.testing.assert_allclose(out["grad"][s, b], g.numpy(), rtol=1e-6, atol=1e-9)


def test_ragged_batch_refit_equals_the_single_problem_refit(emul):
    probs = ragged_problems()
    S, B, T, D = 3, 2, 4, 3
    z0 = starts(S, B, D, T)
    out = call_batched(emul, probs, z0, mode=1)
    assert (out["stats"][..., 2] != 4).all() and (out["stats"][..., 0] >= 1).all()
    for s in range(S):
        one = call_single(emul, probs[s], z0[s], mode=1)
        assert np.array_equal(out["z"][s], one["z"]) and np.array_equal(out["value"][s], one["value"]), s
        assert np.array_equal(out["stats"][s], one["stats"]) and np.array_equal(out["info"][s], one["info"])
        for b in range(B):   # the reported value is the oracle's objective at the returned point
            val, _ = oracle_mll_and_grad(probs[s], torch.from_numpy(out["z"][s, b]))
            np.testing.assert_allclose(out["value"][s, b], float(val), rtol=1e-8)


def test_single_study_batch_is_the_single_problem(emul):
    prob = make_target_problem(7, 3, 2, 1, seed=7)
    z = raw_start(2, 3, seed=7, B=2)
    out, one = call_batched(emul, [prob], z.unsqueeze(0), mode=0), call_single(emul, prob, z, mode=0)
    assert np.array_equal(out["value"][0], one["value"]) and np.array_equal(out["grad"][0], one["grad"])


def test_a_count_out_of_range_answers_nan_for_that_problem_only(emul):
    probs = ragged_problems()
    S, B, T, D = 3, 2, 4, 3
    z = starts(S, B, D, T)
    good = call_batched(emul, probs, z, mode=0)
    for bad_n in (0, 13):
        out = call_batched(emul, probs, z, mode=0, n_points=[5, bad_n, 12])
        assert (out["info"][1] == -1).all() and np.isnan(out["value"][1]).all() and not out["grad"][1].any()
        for s in (0, 2):
            assert np.array_equal(out["value"][s], good["value"][s]) and np.array_equal(out["grad"][s], good["grad"][s])
    fit = call_batched(emul, probs, z, mode=1, n_points=[5, 0, 12])
    assert (fit["stats"][1, :, 2] == 4).all() and np.array_equal(fit["z"][1], z[1].numpy())


def test_batched_lds_request_covers_every_problem_size(emul):
    """The counts live in device memory, so the launch asks for the largest footprint any 1 <= n <= n_max can have -- with the
    matrix-core factorisation that is not always the footprint at n_max (112 -> 113 drops from tiles to packed triangles)."""
    for T, D, waves in ((32, 6, 8), (3, 2, 8), (200, 16, 8), (5, 3, 1)):
        for may in (0, 1):
            worst = 0
            for n_max in range(1, 129):
                worst = max(worst, emul.emul_target_fit_problem_lds_doubles(n_max, T, D, waves, may))
                assert emul.emul_target_fit_batched_lds_doubles(n_max, T, D, waves, may) == worst, (n_max, T, D, waves, may)
