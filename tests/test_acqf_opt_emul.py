"""CPU checks of the device-side acquisition optimiser's step kernel (csrc/gp_acqf_opt.h) through a single-threaded host build of the
same source (tests/host_emul/acqf_opt_emul.cpp: test infrastructure, never part of the library).  The state machine of ONE start is
``hyper.batched_lbfgs(bounds=...)`` run on that start alone: fed the same (f, g) it has the same iteration count, evaluation count,
stop reason and -- the sums run in the same order, no product is contracted -- the same accepted points, bit for bit.  The
parallel execution (lane broadcasts, the evaluation launches in between) is what tests/test_acqf_opt_gpu.py covers on the MI355X."""
import ctypes

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from scamlgp_amd import hyper as H
from tests._host_emul import DP as dp, IP as ip, build, ptr
from tests.test_hyper_bounds import h6_starts, neg_hartmann6

F64 = torch.float64
RUNNING, CONVERGED, FTOL, STALLED, FAILED, MAXITER, PADDING = range(7)
CONTINUE = 1
EVAL_FN = ctypes.CFUNCTYPE(None)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "acqf_opt_emul")
    lib.emul_acqf_opt_state_doubles.restype, lib.emul_acqf_opt_state_doubles.argtypes = ctypes.c_longlong, [ctypes.c_int] * 2
    lib.emul_acqf_opt_max_d.restype, lib.emul_acqf_opt_max_d.argtypes = ctypes.c_int, []
    lib.emul_acqf_opt_call.restype = None
    lib.emul_acqf_opt_call.argtypes = ([dp, dp, ip, dp, dp, dp, dp, dp, ip, dp, dp, ip] + [ctypes.c_int] * 6 + [ctypes.c_double] * 3
                                       + [ctypes.c_int, ctypes.c_uint, EVAL_FN])
    return lib


def _drive(emul, fun, x0, bounds=(0.0, 1.0), group=None, max_iter=200, history=10, gtol=1e-5, ftol=2.2e-9, max_ls=20, c1=1e-4,
           per_call=1, state_fill=0.0):
    """The chunk loop of ``StudiesAcquisition.optimize`` on the CPU.  ``fun(points (B, P) tensor) -> (f (B,), g (B, P))`` is the
    MINIMISED function (what ``hyper.batched_lbfgs`` takes); the step kernel is handed the maximised one, -f and -g (a negation is
    exact).  Returns the final outputs, the state bytes, the accepted points after every call (``path``: with ``per_call=1`` one
    entry per round) and every point the function was asked for per round (``asked``: (Xq, group_live) copies)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, D = x0.shape
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds[0], dtype=np.float64), (D,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds[1], dtype=np.float64), (D,)))
    group = np.zeros(B, dtype=np.int32) if group is None else np.ascontiguousarray(group, dtype=np.int32)
    G = int(max(group.max() + 1, 1))
    state = np.full((B, emul.emul_acqf_opt_state_doubles(D, history)), state_fill)
    value, grad = np.zeros(B), np.zeros((B, D))
    Xq, x, f = np.zeros((B, D)), np.zeros((B, D)), np.zeros(B)
    live = np.zeros(B, dtype=np.int32)
    stats = np.zeros((B, 4), dtype=np.int32)
    asked = []

    def evaluate():
        asked.append((Xq.copy(), live.copy()))
        fv, gv = fun(torch.from_numpy(Xq.copy()))
        # what the evaluation kernels give a row whose group is negative: zeros
        value[:] = np.where(live >= 0, -fv.numpy(), 0.0)
        grad[:] = np.where(live[:, None] >= 0, -gv.numpy(), 0.0)

    cb = EVAL_FN(evaluate)
    budget = 1 + max_iter * max_ls
    rounds = calls = 0
    path = []
    while True:
        k = min(per_call, budget - rounds)
        emul.emul_acqf_opt_call(ptr(value), ptr(grad), ptr(group), ptr(x0), ptr(lo), ptr(hi), ptr(state), ptr(Xq), ptr(live), ptr(x), ptr(f),
                                ptr(stats), B, G, D, max_iter, history, max_ls, gtol, ftol, c1, k, CONTINUE if calls else 0, cb)
        rounds += k
        calls += 1
        path.append((x.copy(), f.copy(), stats.copy()))
        if not (stats[:, 2] == RUNNING).any() or rounds >= budget:
            break
    return dict(x=x, f=f, stats=stats, state=state, Xq=Xq, live=live, rounds=rounds, path=path, asked=asked)


def _host_alone(fun, x0, bounds, **kw):
    """``hyper.batched_lbfgs(bounds=...)`` on ONE start, with the accepted point after every iteration and why it stopped."""
    path = []
    res = H.batched_lbfgs(fun, x0, bounds=bounds, callback=lambda it, x, f, done: path.append((it, x[0].clone(), float(f[0]), bool(done[0]))), **kw)
    if bool(res.failed[0]):
        reason = FAILED
    elif bool(res.converged[0]):
        reason = CONVERGED
    elif not path[-1][3]:
        reason = MAXITER
    elif len(path) > 1 and torch.equal(path[-1][1], path[-2][1]):
        reason = STALLED     # (an accepted step has slope < 0: it moves the point)
    else:
        reason = FTOL
    return res, path, reason


def _accepted_points(res):
    """The accepted point whenever an iteration ended (the iteration counter moved on, or the start stopped): what the host
    optimiser's ``callback`` sees."""
    out, it_prev = [], 0
    for x, _, stats in res["path"]:
        it, status = int(stats[0, 0]), int(stats[0, 2])
        if it != it_prev or status != RUNNING:
            out.append(x[0].copy())
        it_prev = it
        if status != RUNNING:
            break
    return out


def _same_as_host(emul, fun, x0, bounds, **kw):
    for b in range(x0.shape[0]):
        fun_b = (lambda x, b=b: fun(x, b))
        ref, path, reason = _host_alone(fun_b, x0[b:b + 1], bounds, **kw)
        res = _drive(emul, fun_b, x0[b:b + 1].numpy(), bounds=tuple(np.asarray(v) for v in bounds), **kw)
        assert res["stats"][0, :3].tolist() == [ref.n_iter, ref.n_eval, reason], (b, res["stats"][0].tolist(), ref.n_iter, ref.n_eval, reason)
        pts = _accepted_points(res)
        assert len(pts) == len(path), (b, len(pts), len(path))
        for (it, xr, _, _), xe in zip(path, pts):
            np.testing.assert_array_equal(xe, xr.numpy(), err_msg=f"start {b}, iteration {it}")
        np.testing.assert_array_equal(res["x"][0], ref.x[0].numpy())
        if reason != FAILED:
            assert res["f"][0] == -float(ref.f[0])      # the maximised value at the accepted point


def _quadratic_case():
    # the data of test_separable_quadratic_ends_at_the_clipped_optimum
    gen = torch.Generator().manual_seed(0)
    c = torch.rand(16, 6, dtype=F64, generator=gen) * 2.0 - 0.5
    c[0] = torch.tensor([0.2, 0.4, 0.5, 0.6, 0.7, 0.9], dtype=F64)
    c[1] = torch.tensor([-0.3, 1.4, -1.0, 2.0, 1.1, -0.1], dtype=F64)
    c[2] = torch.tensor([0.5, 0.5, 1.5, 0.5, 0.5, 0.5], dtype=F64)
    a = 0.5 + 3.0 * torch.rand(16, 6, dtype=F64, generator=gen)
    x0 = torch.rand(16, 6, dtype=F64, generator=gen)
    return a, c, x0


def _rowsum(t):
    acc = t[:, 0]
    for j in range(1, t.shape[1]):
        acc = acc + t[:, j]
    return acc


def test_iterates_match_the_host_optimiser_on_the_separable_quadratic(emul):
    a, c, x0 = _quadratic_case()
    fun = lambda x, b: (_rowsum(a[b:b + 1] * (x - c[b:b + 1]) ** 2), 2.0 * a[b:b + 1] * (x - c[b:b + 1]))   # noqa: E731
    _same_as_host(emul, fun, x0, (0.0, 1.0), max_iter=200, gtol=1e-10, ftol=0.0)
    # (P,) bounds and starts outside the box
    lo, hi = torch.full((6,), 0.25, dtype=F64), torch.tensor([0.75, 0.75, 0.75, 2.0, 2.0, 2.0], dtype=F64)
    _same_as_host(emul, fun, x0 * 3.0 - 1.0, (lo, hi), max_iter=200, gtol=1e-10, ftol=0.0)


@pytest.mark.parametrize("max_iter", [100, 200, 60])
def test_iterates_match_the_host_optimiser_on_hartmann6(emul, max_iter):
    _same_as_host(emul, lambda x, b: neg_hartmann6(x), h6_starts(), (0.0, 1.0), max_iter=max_iter)


def _rosenbrock(scale):
    def fun(x, b):
        x = x.clone().requires_grad_(True)
        f = (scale[b] * (x[:, 1:] - x[:, :-1] ** 2) ** 2 + (1 - x[:, :-1]) ** 2).sum(-1)
        (g,) = torch.autograd.grad(f.sum(), x)
        return f.detach(), g
    return fun


def test_iterates_match_the_host_optimiser_on_the_rosenbrock_family_in_a_wide_box(emul):
    B, P = 7, 4
    _same_as_host(emul, _rosenbrock(torch.linspace(1.0, 20.0, B, dtype=F64)), torch.zeros(B, P, dtype=F64), (-10.0, 10.0), max_iter=500,
                  gtol=1e-8, ftol=0.0)


def _quad(c, a=1.0):
    c = torch.as_tensor(c, dtype=F64).reshape(1, -1)
    return lambda x, b=0: (_rowsum(a * (x - c) ** 2), 2.0 * a * (x - c))


def test_a_start_outside_the_box_is_projected(emul):
    res = _drive(emul, _quad([0.3, 0.6, 0.5]), [[-2.0, 7.0, 0.5]], gtol=1e-10, ftol=0.0)
    np.testing.assert_array_equal(res["asked"][0][0], [[0.0, 1.0, 0.5]])     # the first point evaluated is the projected start
    assert res["stats"][0, 2] == CONVERGED
    np.testing.assert_allclose(res["x"][0], [0.3, 0.6, 0.5], rtol=0, atol=1e-9)


def test_a_start_on_a_face_with_the_gradient_pointing_outward_is_held_there(emul):
    res = _drive(emul, _quad([-0.5, 0.7]), [[0.0, 0.2]], gtol=1e-10, ftol=0.0)
    assert res["stats"][0, 2] == CONVERGED and res["stats"][0, 0] >= 1       # the projected-gradient rule, after real iterations
    for Xq, _ in res["asked"]:
        assert Xq[0, 0] == 0.0                                               # never leaves the face
    np.testing.assert_allclose(res["x"][0], [0.0, 0.7], rtol=0, atol=1e-9)
    # the gradient there still points outward: only its projection is small
    _, g = _quad([-0.5, 0.7])(torch.from_numpy(res["x"]))
    assert float(g[0, 0]) == 1.0
    _same_as_host(emul, _quad([-0.5, 0.7]), torch.tensor([[0.0, 0.2]], dtype=F64), (0.0, 1.0), gtol=1e-10, ftol=0.0)


def test_an_optimum_in_a_corner(emul):
    res = _drive(emul, _quad([1.5, -0.5, 2.0]), [[0.4, 0.6, 0.5]], gtol=1e-10, ftol=0.0)
    assert res["stats"][0, 2] == CONVERGED
    np.testing.assert_array_equal(res["x"][0], [1.0, 0.0, 1.0])


@pytest.mark.parametrize("D", [1, 15])
def test_smallest_and_largest_dimension(emul, D):
    assert emul.emul_acqf_opt_max_d() == 15
    gen = torch.Generator().manual_seed(D)
    c = torch.rand(1, D, dtype=F64, generator=gen) * 2.0 - 0.5
    a = 0.5 + 3.0 * torch.rand(1, D, dtype=F64, generator=gen)
    x0 = torch.rand(1, D, dtype=F64, generator=gen)
    fun = lambda x, b=0: (_rowsum(a * (x - c) ** 2), 2.0 * a * (x - c))   # noqa: E731
    _same_as_host(emul, fun, x0, (0.0, 1.0), max_iter=200, gtol=1e-10, ftol=0.0)
    res = _drive(emul, fun, x0.numpy(), gtol=1e-10, ftol=0.0)
    np.testing.assert_allclose(res["x"], c.clamp(0.0, 1.0).numpy(), rtol=0, atol=1e-8)


def test_history_overflow_wraps_the_ring(emul):
    fun = _rosenbrock(torch.tensor([10.0], dtype=F64))
    x0 = torch.full((1, 6), -0.5, dtype=F64)
    kw = dict(max_iter=500, history=3, gtol=1e-8, ftol=0.0)
    _same_as_host(emul, fun, x0, (-2.0, 2.0), **kw)
    res = _drive(emul, lambda x: fun(x, 0), x0.numpy(), bounds=(-2.0, 2.0), **kw)
    assert res["stats"][0, 3] == 3 and res["stats"][0, 0] > 3 * 3            # three pairs held, far more than three accepted
    np.testing.assert_allclose(res["x"], np.ones((1, 6)), rtol=0, atol=1e-5)


def test_max_iter_cuts_off(emul):
    fun = _rosenbrock(torch.tensor([10.0], dtype=F64))
    x0 = torch.full((1, 4), -0.5, dtype=F64)
    res = _drive(emul, lambda x: fun(x, 0), x0.numpy(), bounds=(-2.0, 2.0), max_iter=5, gtol=1e-8, ftol=0.0)
    assert res["stats"][0, 0] == 5 and res["stats"][0, 2] == MAXITER
    _same_as_host(emul, fun, x0, (-2.0, 2.0), max_iter=5, gtol=1e-8, ftol=0.0)
    # max_iter = 0: one evaluation, no step
    res = _drive(emul, lambda x: fun(x, 0), x0.numpy(), bounds=(-2.0, 2.0), max_iter=0)
    assert res["stats"][0, :3].tolist() == [0, 1, MAXITER]
    np.testing.assert_array_equal(res["x"], x0.numpy())


def _nan_beyond_two(x, b=0):
    f = torch.where(x[:, 0] > 2.0, torch.full_like(x[:, 0], float("nan")), _rowsum((x - 1.0) ** 2))
    return f, 2 * (x - 1.0)


def test_a_nonfinite_start_fails_and_stays_at_the_projected_start(emul):
    res = _drive(emul, _nan_beyond_two, [[7.0, -20.0]], bounds=(-10.0, 5.0))
    assert res["stats"][0, :3].tolist() == [0, 1, FAILED]
    np.testing.assert_array_equal(res["x"][0], [5.0, -10.0])
    assert res["f"][0] == -np.inf and res["live"][0] == -1
    _same_as_host(emul, _nan_beyond_two, torch.tensor([[7.0, -20.0]], dtype=F64), (-10.0, 5.0))
    # a non-finite gradient alone fails the start too
    res = _drive(emul, lambda x: (_rowsum(x * x), torch.full_like(x, float("inf"))), [[0.5, 0.5]])
    assert res["stats"][0, 2] == FAILED


def test_a_nonfinite_region_met_in_the_line_search_shrinks_the_step(emul):
    # the first steepest-descent trial (length 1) overshoots the optimum at 0.6 into x_0 < 0.55, where the function is NaN
    c = torch.tensor([[0.6, 0.6]], dtype=F64)

    def fun(x, b=0):
        f = torch.where(x[:, 0] < 0.55, torch.full_like(x[:, 0], float("nan")), _rowsum((x - c) ** 2))
        return f, 2.0 * (x - c)

    x0 = torch.tensor([[1.4, 0.9]], dtype=F64)
    seen = []

    def watched(x):
        out = fun(x)
        seen.append(out[0].clone())
        return out

    res = _drive(emul, watched, x0.numpy(), bounds=(-10.0, 10.0), gtol=1e-8, ftol=0.0)
    assert not bool(torch.isfinite(seen[1]).all())                               # the region was met by the first trial
    assert res["stats"][0, 2] == CONVERGED and res["stats"][0, 1] > res["stats"][0, 0] + 1   # and cost an extra trial
    np.testing.assert_allclose(res["x"], c.numpy(), rtol=0, atol=1e-6)
    _same_as_host(emul, fun, x0, (-10.0, 10.0), gtol=1e-8, ftol=0.0)


def test_a_padding_row_never_moves_and_never_reports_running(emul):
    a, c, x0 = _quadratic_case()
    x0 = (x0[:4] * 3.0 - 1.0).numpy()
    fun = lambda x: (_rowsum(a[:4] * (x - c[:4]) ** 2), 2.0 * a[:4] * (x - c[:4]))   # noqa: E731
    group = np.array([0, -1, 1, 0], dtype=np.int32)
    res = _drive(emul, fun, x0, group=group, gtol=1e-10, ftol=0.0)
    for x, _, stats in res["path"]:
        assert stats[1].tolist() == [0, 0, PADDING, 0]
        np.testing.assert_array_equal(x[1], np.clip(x0[1], 0.0, 1.0))
    for _, live in res["asked"]:
        assert live[1] == -1
    assert res["f"][1] == 0.0
    # the real rows are what they are on their own, and hand their group on while they run
    assert res["asked"][0][1].tolist() == [0, -1, 1, 0]
    assert (res["live"] == -1).all() and (res["stats"][[0, 2, 3], 2] != RUNNING).all()
    for b in (0, 2, 3):
        alone = _drive(emul, lambda x, b=b: (_rowsum(a[b:b + 1] * (x - c[b:b + 1]) ** 2), 2.0 * a[b:b + 1] * (x - c[b:b + 1])), x0[b:b + 1],
                       gtol=1e-10, ftol=0.0)
        np.testing.assert_array_equal(res["x"][b], alone["x"][0])
        assert res["stats"][b].tolist() == alone["stats"][0].tolist()


def test_a_stopped_start_is_no_longer_evaluated(emul):
    """Starts do not wait for each other: each hands -1 to the evaluation kernels from the round after its stop."""
    x0 = h6_starts()[:6].numpy()
    res = _drive(emul, neg_hartmann6, x0, max_iter=60)
    n_eval = res["stats"][:, 1]
    assert len(set(n_eval.tolist())) > 1
    asked_live = np.array([(live >= 0) for _, live in res["asked"]])       # (rounds, B)
    np.testing.assert_array_equal(asked_live.sum(0), n_eval)


@pytest.mark.parametrize("fill", [0.0, np.nan])
def test_chunking_does_not_change_the_state(emul, fill):
    x0 = h6_starts()[:5].numpy() * 1.4 - 0.2
    group = np.array([0, 0, -1, 1, 1], dtype=np.int32)
    kw = dict(group=group, max_iter=30, history=4, state_fill=fill)
    one = _drive(emul, neg_hartmann6, x0, per_call=1, **kw)
    for per_call in (3, 1 + 30 * 20):
        res = _drive(emul, neg_hartmann6, x0, per_call=per_call, **kw)
        assert res["rounds"] >= one["rounds"]
        for k in ("x", "f", "stats", "Xq", "live"):
            np.testing.assert_array_equal(res[k], one[k], err_msg=k)
        # (what a reset leaves untouched -- pairs not yet held, a padding row's gradient -- is the caller's: NaN here, never read)
        np.testing.assert_array_equal(res["state"], one["state"])
        if fill == 0.0:
            assert res["state"].tobytes() == one["state"].tobytes()


def test_python_state_stride_matches_header(emul):
    from scamlgp_amd import ops

    for D in range(1, 16):
        for history in range(1, 17):
            assert ops.studies_acqf_opt_state_doubles(D, history) == emul.emul_acqf_opt_state_doubles(D, history)
