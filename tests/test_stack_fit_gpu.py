"""GPU tests of the source-stack fit on the device (scaml_stack_fit_f64 / ops.stack_fit / utils._fit_stack(driver="device")):
one round against SourceGPStack.objective, whole fits against the host driver from identical starts, chunking, the blocked
fit beyond 256 points, a stack with duplicate points, and the model on top."""
import os

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import _lib, model as M, ops, synthetic, utils

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _stack(name, device):
    """Stacks shaped like the golden cases c2r / c3r / c5r, one ragged stack, one beyond 256 points per task."""
    if name == "c2r":
        d, kind = synthetic.branin_task_stack(3, 64, seed=2, noise_std=1.0), O.KIND_RBF
    elif name == "c3r":
        d, kind = synthetic.smooth_field_task_stack(3, 64, 8, seed=3), O.KIND_MATERN52
    elif name == "c5r":
        d, kind = synthetic.hartmann6_task_stack(2, 64, seed=5), O.KIND_MATERN52
    elif name == "ragged":
        d, kind = synthetic.branin_task_stack(3, 64, seed=7, noise_std=1.0), O.KIND_MATERN52
    elif name == "n384":
        d, kind = synthetic.hartmann6_task_stack(8, 384, seed=1), O.KIND_MATERN52
    else:
        raise KeyError(name)
    T = d["X"].shape[0]
    ns = [48, 64, 33][:T] if name == "ragged" else [d["X"].shape[1]] * T
    Xs = [torch.from_numpy(d["X"][t][:ns[t]]) for t in range(T)]
    Ys = [torch.from_numpy(d["Y"][t][:ns[t]]).unsqueeze(-1) for t in range(T)]
    return M.SourceGPStack(list(range(T)), Xs, Ys, kind=kind, device=device)


def _no_worse(f_dev, f_host):
    """Every task: the device driver's chosen objective (minimised) is no worse than the host driver's within 1e-3 max(1, |f|)."""
    for t, (a, b) in enumerate(zip(f_dev.tolist(), f_host.tolist())):
        assert a <= b + 1e-3 * max(1.0, abs(b)), (t, a, b)


def _fit_both(name, device, restarts, seed, max_iter=200):
    host, dev = _stack(name, device), _stack(name, device)
    torch.manual_seed(seed)
    utils._fit_stack(host, restarts, max_iter=max_iter)
    torch.manual_seed(seed)
    utils.optimize_marginal_likelihood(dev, restarts, max_iter=max_iter, driver="device")
    return host, dev


def test_one_round_matches_the_stack_objective(device):
    """n_evals = 1 evaluates z itself: value and the state's gradient against SourceGPStack.objective at the same z -- the same
    fit and gradient kernels underneath; only the tile sums, the chain rule and the prior terms are computed elsewhere.
    Measured on the MI355X: value 3.9e-16 relative, gradient 9.3e-16 absolute (the order of the sum over the tiles)."""
    stack = _stack("c3r", device)
    reps = 2
    torch.manual_seed(0)
    z0 = utils._stack_starts(stack, reps - 1)
    c = stack._replicated(reps)
    B, N, D = c["X"].shape
    z = z0.clone()
    value = torch.empty(B, dtype=torch.float64, device=device)
    stats = torch.zeros(B, 4, dtype=torch.int32, device=device)
    nbytes = _lib.lib.scaml_stack_fit_workspace_bytes(B, N, D, 10)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    rc = _lib.lib.scaml_stack_fit_f64(c["X"].data_ptr(), c["y"].data_ptr(), None, ops.stack_spec_host(stack.spec), z.data_ptr(), B, N, D,
                                      stack.kind, 1, 0, 200, 10, 1e-5, 2.2e-9, value.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    f_ref, g_ref = stack.objective(z0, reps)
    stride = (4 + 2 * 10) * (D + 2) + 10 + 16
    state = ws[: B * stride * 8].view(torch.float64).reshape(B, stride)
    g = state[:, D + 2:2 * (D + 2)]
    print("one round: max rel value diff", float(((-value - f_ref) / f_ref).abs().max()), "max abs grad diff", float((g - g_ref).abs().max()))
    assert stats[:, 1].tolist() == [1] * B and stats[:, 0].tolist() == [1] * B
    assert torch.equal(z, z0)                                             # the start point is the accepted point
    torch.testing.assert_close(-value, f_ref, rtol=1e-12, atol=0)
    torch.testing.assert_close(g, g_ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name,restarts", [("c2r", 2), ("c3r", 2), ("c5r", 2), ("ragged", 2), ("n384", 1)])
def test_device_driver_against_host_driver(device, name, restarts):
    """Whole fits from identical starts (same seed): per task no worse than the host driver, every problem stopped, and the
    reported value is the stack's objective at the returned point."""
    max_iter = 30 if name == "n384" else 200
    host, dev = _fit_both(name, device, restarts, seed=11, max_iter=max_iter)
    info = dev.last_fit_info
    print(name, "host", (-host.last_fit_info["objective"]).tolist(), "device", (-info["objective"]).tolist(), "evals", info["n_eval"],
          host.last_fit_info["n_eval"])
    _no_worse(-info["objective"], -host.last_fit_info["objective"])
    assert bool((info["stats"][:, 2] != 0).all())
    # value = objective at the returned point
    reps = 1 + restarts
    torch.manual_seed(11)
    z0 = utils._stack_starts(_stack(name, device), restarts)
    c = dev._replicated(reps)
    res = ops.stack_fit(c["X"], c["y"], c["npts"], dev.spec, z0, dev.kind, max_iter=max_iter)
    f_at, _ = dev.objective(res["z"], reps)
    assert bool((res["stats"][:, 2] != 4).all())
    torch.testing.assert_close(-res["value"], f_at, rtol=1e-8, atol=0)
    assert bool((res["stats"][:, 1] <= 1 + max_iter * 20).all())


@pytest.mark.parametrize("name", ["c2r", "ragged"])
def test_chunking_does_not_change_the_result(device, name):
    stack = _stack(name, device)
    reps = 3
    torch.manual_seed(5)
    z0 = utils._stack_starts(stack, reps - 1)
    c = stack._replicated(reps)
    out = [ops.stack_fit(c["X"], c["y"], c["npts"], stack.spec, z0, stack.kind, max_iter=40, evals_per_call=k) for k in (1, 7, 100000)]
    assert out[0]["n_calls"] > out[1]["n_calls"] > out[2]["n_calls"] == 1
    for o in out[1:]:
        assert torch.equal(o["z"], out[0]["z"]) and torch.equal(o["value"], out[0]["value"])
        assert torch.equal(o["stats"][:, :3], out[0]["stats"][:, :3])
    assert bool((out[0]["stats"][:, 2] != 0).all())


def _duplicates_fixture():
    g = np.load(os.path.join(GOLDEN, "edge_duplicates_jitter_T3_N32_rbf.npz"))
    ns = [int(v) for v in g["n_points"]]
    Xs = [torch.from_numpy(g["X"][t, :ns[t]]) for t in range(3)]
    Ys = [torch.from_numpy(g["y"][t, :ns[t]] * g["y_std"][t] + g["y_mean"][t]).unsqueeze(-1) for t in range(3)]
    dup = [len(np.unique(g["X"][t, :ns[t]], axis=0)) < ns[t] for t in range(3)]
    return Xs, Ys, int(g["kind"]), dup


def test_stack_with_duplicate_points(device):
    """Duplicate points: some evaluations need the in-kernel jitter ladder or fail.  Every problem stops, a problem that did not
    fail at its start point has a finite value, and the tasks without duplicates reach the host driver's objective."""
    Xs, Ys, kind, dup = _duplicates_fixture()
    assert any(dup) and not all(dup)
    host, dev = (M.SourceGPStack([0, 1, 2], Xs, Ys, kind=kind, device=device) for _ in range(2))
    torch.manual_seed(3)
    z0 = utils._stack_starts(dev, 2)
    c = dev._replicated(3)
    res = ops.stack_fit(c["X"], c["y"], c["npts"], dev.spec, z0, kind)
    status = res["stats"][:, 2]
    print("duplicates: status", status.tolist(), "value", res["value"].tolist())
    assert bool((status != 0).all())
    assert bool(torch.isfinite(res["value"].cpu()[status != 4]).all())
    torch.manual_seed(3)
    utils._fit_stack(host, 2)
    torch.manual_seed(3)
    utils._fit_stack(dev, 2, driver="device")
    f_dev, f_host = -dev.last_fit_info["objective"], -host.last_fit_info["objective"]
    for t in range(3):
        if not dup[t]:
            _no_worse(f_dev[t:t + 1], f_host[t:t + 1])
    # the public entry with the device driver gives a usable model
    meta = {f"t{t}": M.SupervisedDataset(Xs[t], Ys[t]) for t in range(3)}
    gps = M.meta_fit_scamlgp(meta, covar_module=M.KernelSpec(kind), num_restarts_log_likelihood=2, seed=3, device=device,
                             fit_options={"driver": "device"})
    st = gps["t0"]._stack
    assert "stats" in st.last_fit_info and bool((st.last_fit_info["stats"][:, 2] != 0).all())
    xq = torch.rand(5, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    p = gps["t1"].posterior(xq)
    assert bool(torch.isfinite(p.mvn.mean).all()) and bool((p.mvn.variance > 0).all())


def test_scamlgp_posterior_on_a_device_fitted_stack_matches_the_oracle(device):
    """End to end: sources fitted by the device driver, ScaMLGP on top, posterior against the oracle at the fitted theta."""
    d = synthetic.branin_task_stack(3, 64, seed=2, noise_std=1.0)
    meta = {f"task{t}": M.SupervisedDataset(torch.from_numpy(d["X"][t]), torch.from_numpy(d["Y"][t]).unsqueeze(-1)) for t in range(3)}
    gps = M.meta_fit_scamlgp(meta, num_restarts_log_likelihood=2, seed=7, device=device, fit_options=dict(driver="device"))
    stack = gps["task0"]._stack
    g = torch.Generator().manual_seed(5)
    Xt = torch.rand(7, 2, dtype=torch.float64, generator=g)
    yt = torch.tensor(synthetic.branin(-5 + 15 * Xt[:, 0].numpy(), 15 * Xt[:, 1].numpy()), dtype=torch.float64).unsqueeze(-1)
    model = M.ScaMLGP(Xt, yt, gps)
    w = torch.tensor([0.4, 0.3, 0.6], dtype=torch.float64)
    model.weights = w
    xq = torch.rand(11, 2, dtype=torch.float64, generator=g)
    post = model.eval().posterior(xq)
    mus, covs = [], []
    xall = torch.cat([Xt, xq])
    for t in range(3):
        X, y, th = stack.X[t].cpu(), stack.y[t].cpu(), stack.theta[t].cpu()
        fit = O.gp_fit(X, y, th, stack.kind)
        mu, cov = O.source_posterior(xall, X, th, stack.kind, fit["L"], fit["alpha"], float(stack.y_mean[t]), float(stack.y_std[t]))
        mus.append(mu)
        covs.append(cov)
    mu_j, cov_j = O.target_prior(torch.stack(mus), torch.stack(covs), w)
    mu_ref, S_ref = O.target_posterior(xq, Xt, yt.squeeze(-1), mu_j, cov_j, model.theta.cpu(), O.KIND_RBF, float(model.m_all), float(model.s_all))
    torch.testing.assert_close(post.mean.squeeze(-1).cpu(), mu_ref, rtol=1e-4, atol=1e-4 * float(mu_ref.abs().max()))
    torch.testing.assert_close(post.variance.squeeze(-1).cpu(), S_ref.diagonal(), rtol=1e-4, atol=1e-4 * float(S_ref.abs().max()))
