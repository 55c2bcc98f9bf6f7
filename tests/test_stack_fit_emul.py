"""CPU checks of the source-stack fit's step kernel (csrc/gp_stack_fit.hip) through a single-threaded host build of the same
source (tests/host_emul/stack_fit_emul.cpp: test infrastructure, never part of the library): ``sf_objective`` against the
oracle's training objective, ``sf_advance`` against the cases tests/test_hyper.py states for ``hyper.batched_lbfgs``, and the
whole loop -- emulated step around the oracle's marginal likelihood -- against ``hyper.batched_lbfgs`` on golden stacks.  The
parallel execution (wave reductions, the launches in between) is what tests/test_stack_fit_gpu.py covers on the MI355X."""
import ctypes
import os

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from oracle import gp_oracle as O
from scamlgp_amd import hyper as H
from tests._host_emul import DP as dp, IP as ip, ROOT, build, ptr

GOLDEN = os.path.join(ROOT, "tests", "golden")

SPEC = H.source_gp_spec()
# Interval bounds, then (kind, p1, p2): Gamma(3, 6), Gamma(2, 0.15), LogNormal(-8, 2)  (scamlgp/model.py:25-33, 36-70)
SPEC15 = np.array([1e-4, 1e2, 1e-4, 1e2, 1e-8, 1e-2, 1, 3.0, 6.0, 1, 2.0, 0.15, 2, -8.0, 2.0], dtype=np.float64)
_LOG_2PI = float(np.log(2.0 * np.pi))

_d = _i = ptr   # (float64 arrays -> dp, int32 arrays -> ip)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "stack_fit_emul")
    lib.emul_stack_fit_state_doubles.restype, lib.emul_stack_fit_state_doubles.argtypes = ctypes.c_longlong, [ctypes.c_int] * 2
    lib.emul_stack_objective.restype = None
    lib.emul_stack_objective.argtypes = [dp, dp, ip, dp, ctypes.c_int, dp, dp, ip, ctypes.c_int, ctypes.c_int, dp, dp]
    lib.emul_stack_reset.restype = None
    lib.emul_stack_reset.argtypes = [dp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
    lib.emul_stack_advance.restype = None
    lib.emul_stack_advance.argtypes = [dp, dp, dp] + [ctypes.c_int] * 5 + [ctypes.c_double] * 3 + [dp, dp, dp, ip]
    return lib


def _bounds(D):
    return [(1e-4, 1e2)] * D + [(1e-4, 1e2), (1e-8, 1e-2)]


def _oracle_mll_and_theta_grad(X, y, theta, kind):
    """mll WITHOUT priors (divided by n) and its gradient w.r.t. the constrained parameters, by autograd through the oracle's
    differentiable kernel matrix; raises if the matrix is not positive definite."""
    th = theta.clone().requires_grad_(True)
    n, D = X.shape
    K = O._kernel_matrix_grad(X, th, kind) + th[D + 1] * torch.eye(n, dtype=X.dtype)
    L = torch.linalg.cholesky(K)
    v = torch.linalg.solve_triangular(L, y.unsqueeze(-1), upper=False)
    mll = -0.5 * ((v * v).sum() + 2.0 * torch.log(torch.diagonal(L)).sum() + n * _LOG_2PI) / n
    (g,) = torch.autograd.grad(mll, th)
    return float(mll.detach()), g.numpy()


def _objective(emul, mll, info, partials, theta, raw, n):
    B, tiles, P = partials.shape
    f, g = np.zeros(B), np.zeros((B, P))
    emul.emul_stack_objective(_d(SPEC15), _d(np.ascontiguousarray(mll)), _i(np.ascontiguousarray(info, dtype=np.int32)),
                              _d(np.ascontiguousarray(partials)), tiles, _d(np.ascontiguousarray(theta)),
                              _d(np.ascontiguousarray(raw)), _i(np.ascontiguousarray(n, dtype=np.int32)), B, P - 2, _d(f), _d(g))
    return f, g


# raw points: ordinary, close to the lower end of every interval, close to the upper end
@pytest.mark.parametrize("kind", [O.KIND_RBF, O.KIND_MATERN52])
@pytest.mark.parametrize("raw_row", [[-5.0, -4.5, -6.0, -4.0, -3.0], [-12.0, -11.0, -12.5, -11.5, -12.0], [-2.5, -3.0, -2.0, 12.0, 12.0]])
def test_objective_matches_oracle_with_priors(emul, kind, raw_row):
    """sf_objective fed with the oracle's mll (no priors) and d mll / d theta split over fake tiles = the oracle's full training
    objective and its raw gradient (both prior families: Gamma on lengthscales / outputscale, LogNormal on the noise)."""
    rng = np.random.default_rng(3)
    n, D, tiles = 9, 3, 5
    X = torch.from_numpy(rng.random((n, D)))
    y = torch.from_numpy(rng.standard_normal(n))
    raw = torch.tensor(raw_row, dtype=torch.float64)
    val, g_raw, theta = O.mll_value_and_grad_raw(X, y, raw, kind, _bounds(D), with_priors=True)
    mll, g_theta = _oracle_mll_and_theta_grad(X, y, theta, kind)
    # the gradient kernel's partials sum to 2 n d mll / d theta: random split over the tiles
    w = rng.random((tiles, D + 2))
    partials = (w / w.sum(0)) * (2.0 * n * g_theta)
    f, g = _objective(emul, np.array([mll]), [0], partials[None], theta.numpy()[None], raw.numpy()[None], [n])
    np.testing.assert_allclose(f[0], -float(val), rtol=1e-9)
    np.testing.assert_allclose(g[0], -g_raw.numpy(), rtol=1e-6, atol=1e-9)
    # any non-zero status (a failed pivot, or a negative one) has no value and a zero gradient
    for info in (3, -1):
        f, g = _objective(emul, np.array([mll]), [info], partials[None], theta.numpy()[None], raw.numpy()[None], [n])
        assert not np.isfinite(f[0]) and not g.any()


def _drive(emul, fun, x0, max_iter=200, history=10, gtol=1e-5, ftol=2.2e-9, max_ls=20):
    """The round loop of scaml_stack_fit_f64 on the CPU: fun(points (B, P)) -> (f (B,), g (B, P)) stands for fit + gradient +
    sf_objective, the emulated sf_advance turns every evaluation into the next trial point."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, P = x0.shape
    state = np.zeros((B, emul.emul_stack_fit_state_doubles(P, history)))
    xt, x, fx = np.zeros((B, P)), np.zeros((B, P)), np.zeros(B)
    stats = np.zeros((B, 3), dtype=np.int32)
    emul.emul_stack_reset(_d(state), _d(x0), B, P, history, _d(xt))
    rounds = 0
    while rounds < 1 + max_iter * max_ls:
        f, g = fun(xt.copy())
        emul.emul_stack_advance(_d(state), _d(np.ascontiguousarray(f)), _d(np.ascontiguousarray(g)), B, P, history, max_iter, max_ls,
                                gtol, ftol, 1e-4, _d(xt), _d(x), _d(fx), _i(stats))
        rounds += 1
        if (stats[:, 2] != 0).all():
            break
    return dict(x=x, f=fx, stats=stats, rounds=rounds)


def test_advance_on_rosenbrock_family(emul):
    """The first case of tests/test_hyper.py, with its bounds: all converged, x within 1e-5 of 1, f < 1e-10."""
    B, P = 7, 4
    scale = torch.linspace(1.0, 20.0, B, dtype=torch.float64)

    def fun(xn):
        x = torch.from_numpy(xn).requires_grad_(True)
        f = (scale[:, None] * (x[:, 1:] - x[:, :-1] ** 2) ** 2 + (1 - x[:, :-1]) ** 2).sum(-1)
        (g,) = torch.autograd.grad(f.sum(), x)
        return f.detach().numpy(), g.numpy()

    res = _drive(emul, fun, np.full((B, P), -0.5), max_iter=500, gtol=1e-8, ftol=0.0)
    assert np.isin(res["stats"][:, 2], (1, 2)).all(), res["stats"]
    np.testing.assert_allclose(res["x"], np.ones((B, P)), rtol=0, atol=1e-5)
    assert res["f"].max() < 1e-10
    # problems no longer wait for each other: each stops after its own number of evaluations
    assert len(set(res["stats"][:, 1].tolist())) > 1


def test_advance_handles_nonfinite_regions_and_flags_failures(emul):
    """The second case of tests/test_hyper.py: failed flags [False, False, True], the first two reach 1 within 1e-4."""
    def fun(xn):
        x = torch.from_numpy(xn)
        f = torch.where(x[:, 0] > 2.0, torch.full_like(x[:, 0], float("nan")), ((x - 1.0) ** 2).sum(-1))
        return f.numpy(), (2 * (x - 1.0)).numpy()

    x0 = np.array([[0.0, 0.0], [1.9, 5.0], [3.0, 0.0]])
    res = _drive(emul, fun, x0)
    assert (res["stats"][:, 2] == 4).tolist() == [False, False, True]
    assert (res["stats"][:, 2] != 0).all()
    np.testing.assert_allclose(res["x"][:2], np.ones((2, 2)), rtol=0, atol=1e-4)
    np.testing.assert_array_equal(res["x"][2], x0[2])   # the failed problem stays at its start point
    assert np.isinf(res["f"][2])


def test_advance_is_batched_lbfgs_per_problem(emul):
    """Per problem the state machine IS hyper.batched_lbfgs run on that problem alone: same iterates (to rounding: the sums
    are taken in another order), same iteration and evaluation counts."""
    scale = torch.linspace(1.0, 20.0, 3, dtype=torch.float64)
    for b in range(3):
        def fun_t(x):
            x = x.clone().requires_grad_(True)
            f = (scale[b] * (x[:, 1:] - x[:, :-1] ** 2) ** 2 + (1 - x[:, :-1]) ** 2).sum(-1)
            (g,) = torch.autograd.grad(f.sum(), x)
            return f.detach(), g

        x0 = torch.full((1, 4), -0.5, dtype=torch.float64)
        for max_iter in (8, 500):   # stopped by max_iter; converged by the gradient rule
            ref = H.batched_lbfgs(fun_t, x0, max_iter=max_iter, gtol=1e-8, ftol=0.0)
            res = _drive(emul, lambda xn: tuple(t.numpy() for t in fun_t(torch.from_numpy(xn))), x0.numpy(), max_iter=max_iter, gtol=1e-8,
                         ftol=0.0)
            assert bool(ref.converged[0]) == (max_iter == 500)
            assert res["stats"][0].tolist() == [ref.n_iter, ref.n_eval, 1 if max_iter == 500 else 5]
            np.testing.assert_allclose(res["x"], ref.x.numpy(), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("fixture,seed", [("ref_meta1d_quartic_T2_N7_rbf.npz", 0), ("c1_branin_T4_N32_rbf.npz", 0)])
def test_whole_loop_reaches_the_batched_lbfgs_optimum_on_golden_stacks(emul, fixture, seed):
    """Emulated step (sf_objective + sf_advance) around the oracle's marginal likelihood, warm start + two prior-sampled starts
    per task: for EVERY task the best-of-starts objective is no worse than what hyper.batched_lbfgs reaches on the oracle's full
    objective from the same starts, within 1e-3 max(1, |f|)."""
    g = np.load(os.path.join(GOLDEN, fixture))
    kind, T = int(g["kind"]), g["X"].shape[0]
    D = g["X"].shape[2]
    ns = [int(v) for v in g["n_points"]]
    Xs = [torch.from_numpy(g["X"][t, :ns[t]]) for t in range(T)]
    ys = [torch.from_numpy(g["y"][t, :ns[t]]) for t in range(T)]
    torch.manual_seed(seed)
    reps = 3
    starts = [SPEC.to_raw(SPEC.init_theta(D)).repeat(T, 1)]
    for _ in range(reps - 1):
        starts.append(SPEC.to_raw(SPEC.sample_prior((T,), D)))
    x0 = torch.cat(starts, 0)   # problem b = rep * T + task
    B = x0.shape[0]
    n_b = np.array([ns[b % T] for b in range(B)], dtype=np.int32)

    def oracle_fun(x):   # the reference objective: oracle value and autograd gradient, priors included
        f, gr = torch.full((B,), float("nan"), dtype=torch.float64), torch.zeros(B, D + 2, dtype=torch.float64)
        for b in range(B):
            try:
                val, gb, _ = O.mll_value_and_grad_raw(Xs[b % T], ys[b % T], x[b], kind, _bounds(D), with_priors=True)
                f[b], gr[b] = -val, -gb
            except RuntimeError:   # not positive definite at this trial point
                pass
        return f, gr

    def emul_fun(xn):    # what the device computes per round: fit (mll, info), gradient partials, then sf_objective
        raw = torch.from_numpy(xn)
        theta = SPEC.to_theta(raw)
        mll, info, part = np.zeros(B), np.zeros(B, dtype=np.int32), np.zeros((B, 2, D + 2))
        for b in range(B):
            try:
                mll[b], gth = _oracle_mll_and_theta_grad(Xs[b % T], ys[b % T], theta[b], kind)
                part[b, 0], part[b, 1] = 0.25 * 2.0 * n_b[b] * gth, 0.75 * 2.0 * n_b[b] * gth
            except RuntimeError:
                info[b] = 1
        return _objective(emul, mll, info, part, theta.numpy(), xn, n_b)

    ref = H.batched_lbfgs(oracle_fun, x0)
    res = _drive(emul, emul_fun, x0.numpy())
    assert (res["stats"][:, 2] != 0).all()
    f_ref = torch.where(ref.failed | ~torch.isfinite(ref.f), torch.full_like(ref.f, float("inf")), ref.f).reshape(reps, T).min(0).values.numpy()
    f_dev = np.where((res["stats"][:, 2] == 4) | ~np.isfinite(res["f"]), np.inf, res["f"]).reshape(reps, T).min(0)
    assert np.isfinite(f_ref).all()
    for t in range(T):
        assert f_dev[t] <= f_ref[t] + 1e-3 * max(1.0, abs(f_ref[t])), (t, f_dev[t], f_ref[t], res["stats"].tolist())


def test_python_state_stride_matches_header(emul):
    """``ops.stack_fit`` reads the gradient out of the per-problem state at the head of the workspace: the stride it uses is the
    header's ``stack_fit_state_doubles`` for every P = D + 2 and history the kernel takes."""
    from scamlgp_amd import ops

    for P in range(3, 65):
        for history in range(1, 17):
            assert ops.stack_fit_state_doubles(P, history) == emul.emul_stack_fit_state_doubles(P, history)
