"""Joint q-point Monte-Carlo acquisition on the MI355X: the joint GRAD source pass (scaml_posterior_linv_grad_joint_f64, (5g)), the
acquisition kernel (scaml_target_qacqf_f64, (7p)), ScaMLGP.joint_acqf, the acquisition classes and ScaMLGPBOLoop.suggest_batch.

  (5g) against (5d): per batch, (5d) called with Xa = cat(Xt, batch) and VA = cat(VA_train, V_batch) is an independent route to the
       same rows -- 1e-9 max|ref|, the suite's figure for two device routes.
  (7p) / joint_acqf against torch autograd through the ORACLE on the CPU in fp64 (source_posterior(full_cov) -> target_prior ->
       target_posterior -> Cholesky -> Monte-Carlo value): _close's rule, rtol 1e-4 and atol 1e-4 max|ref| (the project's north star,
       as tests/test_posterior_grad_gpu.py).  The reference itself is held to cond(Sigma) <= 1e4 and to a margin of 1e-6
       sqrt(max Sigma_jj) between every sample's two best entries and from the kinks (tests/_qacqf_ref.py); the seeds were picked
       on the CPU so that both hold.  Measured worst ratios: profiles/qacqf_notes.md.
  The kernel's own arithmetic is held to an a-priori per-element fp64 bound, on planted arrays at the shape edges, by
  tests/test_qacqf_bounds_gpu.py (tests/_qacqf_bounds.py; figures in profiles/qacqf_bounds_notes.md).

Shapes: T = 3 with one pruned weight, ragged n_points (32, 20, 17) at N = 32; D in {2, 15}; q in {1, 2, 3, 8}; B in {1, 5};
n in {1, 17}, and n = 88 with q = 8 on a T = 2, N = 96 stack (Ma + q = 96, the last row of the covariance block); S in {1, 300, 512};
both kernel families for sources and target; both codes."""
import math

import pytest
import torch

from scamlgp_amd import _lib, ops, utils
from scamlgp_amd.bo import ScaMLGPBOLoop
from tests import _qacqf_ref as R
from tests._qacqf_problem import JointProblem

pytestmark = pytest.mark.gpu

#        ns            D   n   B  q  kind_s kind_t S    seed
CASES = [((32, 20, 17), 2, 17, 5, 3, 0, 0, 300, 1),
         ((32, 32, 32), 15, 1, 1, 8, 1, 1, 512, 1),
         ((32, 32, 32), 2, 17, 5, 1, 1, 1, 1, 2),
         ((32, 32, 32), 2, 1, 1, 2, 0, 1, 300, 1),
         ((96, 96), 15, 88, 1, 8, 1, 0, 300, 1),
         ((32, 20, 17), 15, 17, 5, 2, 1, 0, 512, 1)]
_IDS = [f"N{max(c[0])}{'r' if len(set(c[0])) > 1 else ''}-D{c[1]}-n{c[2]}-B{c[3]}-q{c[4]}-S{c[7]}" for c in CASES]
_BUILT = {}


def _problem(case, device):
    """A case's problem, its model on the GPU and its base samples: built once, shared, never changed."""
    if case not in _BUILT:
        ns, D, n, B, q, ks, kt, S, seed = case
        p = JointProblem(ns, D, n, B, q, ks, kt, seed)
        eps = torch.randn(S, q, dtype=torch.float64, generator=torch.Generator().manual_seed(100 + seed))
        _BUILT[case] = (p, p.model(device), eps)
    return _BUILT[case]


def _close(got, ref, what, rtol=1e-4):
    tol = rtol * float(ref.abs().max())
    print(f"{what}: worst |got - ref| / (rtol |ref| + atol) = {float(((got - ref).abs() / (rtol * ref.abs() + tol + 1e-300)).max()):.3g}")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=tol + 1e-300)


def _route(got, ref, what):
    """Two device routes to the same numbers: 1e-9 of the reference's largest entry."""
    tol = 1e-9 * float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"{what}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, what


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_joint_pass_against_the_concatenated_route(device, case):
    p, (stack, model), _ = _problem(case, device)
    T, N, D, n, B, q = stack.T, stack.N, p.D, p.n, p.B, p.q
    Mq, f = B * q, stack.fit
    Xq = p.X.reshape(Mq, D).to(device)
    args = (stack.X, stack.theta, stack.kind)
    VQ = ops.source_posteriors(Xq, *args, f["L"], f["Linv_diag"], f["alpha"], stack.y_mean, stack.y_std, n_points=stack.n_points,
                               want_var=False, keep_V=True, Linv=f["Linv"])["V"]
    VA = model._train_VA()
    out = ops.source_posteriors_grad_joint(Xq, q, model.train_X, *args, f["Linv"], f["alpha"], VA, VQ, stack.y_mean, stack.y_std, stack.n_points)
    cov = out["cov"].reshape(T, n + q, Mq, 16)
    for b in range(B):
        sl = slice(b * q, (b + 1) * q)
        ref = ops.source_posteriors_grad(Xq[sl], torch.cat([model.train_X, Xq[sl]]), *args, f["Linv"], f["alpha"], stack.y_mean, stack.y_std,
                                         stack.n_points, torch.cat([VA, VQ[:, :, sl]], -1).contiguous())
        _route(cov[:, :, sl], ref["cov"].reshape(T, n + q, q, 16), f"batch {b} cov")
        _route(out["mu"][:, sl], ref["mu"], f"batch {b} mu")
        _route(out["var"][:, sl], ref["var"], f"batch {b} var")
    # the row of the point itself: var in column 0, half of var's derivative in the others; the columns past D are zero
    for j in range(Mq):
        own = cov[:, n + j % q, j]
        _route(own[:, 0], out["var"][:, j, 0], f"point {j} own row, value")
        _route(own[:, 1:1 + D], 0.5 * out["var"][:, j, 1:1 + D], f"point {j} own row, derivative")
    assert not bool(cov[..., 1 + D:].any())


def test_joint_pass_writes_its_rows_only(device):
    """A sentinel fill, one task at a time (T = 1: no next task's rows behind the block that a stray write could hide in).  The
    epilogue stages ceil((Ma + q) / 16) strips of 16 rows; the guard behind the (Ma + q, Mq * 16) block holds the 16 nas - (Ma + q)
    rows that the staged strips reach past it.  Every entry of the block is written, nothing in the guard is."""
    p, (stack, model), _ = _problem(CASES[0], device)
    N, D, n, q = stack.N, p.D, p.n, p.q
    Mq, f = p.B * q, stack.fit
    Xq = p.X.reshape(Mq, D).to(device)
    VQ = ops.source_posteriors(Xq, stack.X, stack.theta, stack.kind, f["L"], f["Linv_diag"], f["alpha"], stack.y_mean, stack.y_std,
                               n_points=stack.n_points, want_var=False, keep_V=True, Linv=f["Linv"])["V"]
    VA = model._train_VA()
    rows, staged = n + q, 16 * ((n + q + 15) // 16)
    assert staged > rows   # (20 rows in two strips: 12 guard rows)
    P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    theta = stack.theta.contiguous()
    for t in range(stack.T):
        one = [x[t:t + 1].contiguous() for x in (stack.X, theta, f["Linv"], f["alpha"], stack.y_mean, stack.y_std, stack.n_points, VA, VQ)]
        Xs, th, Li, al, ym, ys, npts, va, vq = one
        buf = torch.full((staged, Mq * 16), -77.0, dtype=torch.float64, device=device)
        mu = torch.full((1, Mq, 16), -77.0, dtype=torch.float64, device=device)
        var = mu.clone()
        with torch.cuda.device(device):
            rc = _lib.lib.scaml_posterior_linv_grad_joint_f64(P(Xq), P(model.train_X), P(Xs), P(th), P(Li), P(al), P(ym), P(ys), P(npts), P(va),
                                                              P(vq), 1, N, Mq, n, q, D, stack.kind, P(mu), P(var), P(buf), 0,
                                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize(device)
        assert bool((buf[rows:] == -77.0).all())
        assert not bool((buf[:rows] == -77.0).any()) and not bool((mu == -77.0).any()) and not bool((var == -77.0).any())


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB], ids=["qEI", "qUCB"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_joint_acqf_against_oracle_autograd(device, case, acqf):
    p, (stack, model), eps = _problem(case, device)
    par = p.best_f() if acqf == R.ACQF_EI else 4.0
    v_ref, g_ref = p.reference(eps, acqf, par)   # (asserts the two conditions on every batch)
    assert float(g_ref.abs().max()) > 0
    out = model.joint_acqf_full(p.X, acqf, par, eps, want_grad=True)
    assert not bool(out["info"].any()) and not bool(out["jitter"].any())
    _close(out["value"].cpu(), v_ref, "value")
    _close(out["grad"].cpu(), g_ref, "grad")
    # (a second run of the whole chain: the source pass adds its waves' shares of a mean with LDS atomics, whose order may differ from
    #  run to run by a rounding -- only the kernel itself, below, is held to the bit)
    v_only, none = model.joint_acqf(p.X, acqf, par, eps)
    assert none is None
    torch.testing.assert_close(v_only, out["value"], rtol=1e-10, atol=1e-10 * float(out["value"].abs().max()))
    # two calls of the kernel on the same inputs: bit for bit
    kw = model.joint_acqf_inputs(p.X, eps)
    kw.pop("shape")
    once, again = (ops.target_qacqf(acqf=acqf, acqf_param=par, **kw) for _ in range(2))
    assert torch.equal(again["value"], once["value"]) and torch.equal(again["grad"], once["grad"])
    assert torch.equal(again["jitter"], once["jitter"]) and torch.equal(again["info"], once["info"])


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB], ids=["qEI", "qUCB"])
def test_q1_is_the_composition_of_the_posterior_gradients(device, acqf):
    p, (stack, model), _ = _problem(CASES[2], device)
    eps = torch.randn(300, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    par = p.best_f() if acqf == R.ACQF_EI else 4.0
    X = p.X.to(device)
    mu, var, dmu, dvar = model.posterior_with_grad(X.reshape(-1, p.D))
    sigma, e = var.sqrt().unsqueeze(-1), eps.to(device).reshape(1, -1)                 # (B, 1), (1, S)
    dsig = dvar / (2.0 * sigma)
    if acqf == R.ACQF_EI:
        g = par - (mu.unsqueeze(-1) + sigma * e)
        on = (g > 0).to(torch.float64)
        v_ref = (g * on).mean(-1)
        g_ref = -(on.mean(-1, keepdim=True) * dmu) - (on * e).mean(-1, keepdim=True) * dsig
    else:
        c = math.sqrt(par * math.pi / 2.0)
        v_ref = (c * sigma * e.abs()).mean(-1) - mu
        g_ref = -dmu + c * e.abs().mean() * dsig
    v, g = model.joint_acqf(X, acqf, par, eps, want_grad=True)
    torch.testing.assert_close(v, v_ref, rtol=1e-9, atol=1e-9 * float(v_ref.abs().max()))
    torch.testing.assert_close(g.reshape(-1, p.D), g_ref, rtol=1e-9, atol=1e-9 * float(g_ref.abs().max()))


def test_a_batch_with_two_equal_points(device):
    p, (stack, model), eps = _problem(CASES[0], device)
    X = p.X.clone()
    X[0, 1] = X[0, 0]
    par = p.best_f()
    out = model.joint_acqf_full(X, R.ACQF_EI, par, eps, want_grad=True)
    jit = out["jitter"].cpu()
    assert not bool(out["info"].any())
    assert all(float(j) in R.LADDER for j in jit)
    print("jitter of the singular batch:", float(jit[0]))
    mu, Sigma = p.joint_posterior(X[0])
    # (the reference's own Sigma is singular to rounding: with the jitter 0 its second pivot is +-1e-19, and torch.linalg.cholesky
    #  refuses the minus; the factor of a semidefinite matrix, the limit of the jittered ones, is what both sides approximate)
    ref = R.mc_value_semidefinite(mu.detach(), 0.5 * (Sigma + Sigma.T).detach(), eps, par, float(jit[0]))
    assert float(out["value"][0]) == pytest.approx(float(ref), rel=1e-6)


def test_a_nan_coordinate_stays_in_its_batch(device):
    p, (stack, model), eps = _problem(CASES[0], device)
    # the kernel: one set of inputs, then the same with one coordinate of batch 2 replaced -- that batch is NaN, the others bit for bit
    kw = model.joint_acqf_inputs(p.X, eps)
    kw.pop("shape")
    base = ops.target_qacqf(acqf=R.ACQF_UCB, acqf_param=4.0, **kw)
    kw["Xq"] = kw["Xq"].clone()
    kw["Xq"][2 * p.q + 1, 0] = float("nan")
    out = ops.target_qacqf(acqf=R.ACQF_UCB, acqf_param=4.0, **kw)
    grad, grad0 = out["grad"].reshape(p.B, p.q, p.D), base["grad"].reshape(p.B, p.q, p.D)
    assert math.isnan(float(out["value"][2])) and bool(torch.isnan(grad[2]).all())
    for b in (0, 1, 3, 4):
        assert torch.equal(out["value"][b], base["value"][b]) and torch.equal(grad[b], grad0[b])
    clean = model.joint_acqf_full(p.X, R.ACQF_UCB, 4.0, eps, want_grad=True)
    # the whole chain (the source pass answers NaN in that point's strips): the same, the others to the source pass's rounding
    X = p.X.clone()
    X[2, 1, 0] = float("nan")
    out = model.joint_acqf_full(X, R.ACQF_UCB, 4.0, eps, want_grad=True)
    assert math.isnan(float(out["value"][2])) and bool(torch.isnan(out["grad"][2]).all())
    keep = [0, 1, 3, 4]
    torch.testing.assert_close(out["value"][keep], clean["value"][keep], rtol=1e-10, atol=0)
    torch.testing.assert_close(out["grad"][keep], clean["grad"][keep], rtol=1e-10, atol=1e-10 * float(clean["grad"].abs().max()))


def test_refusals_of_the_python_layers(device):
    p, (stack, model), eps = _problem(CASES[0], device)
    with pytest.raises(NotImplementedError):
        model.fantasize(p.X[0, :1], 4).joint_acqf(p.X, R.ACQF_EI, 0.0, eps)
    with pytest.raises(ValueError):
        model.joint_acqf(p.X, ops.ACQF_LOGEI, 0.0, eps)                      # a joint LogEI is not defined
    with pytest.raises(ValueError):
        model.joint_acqf(p.X, R.ACQF_EI, 0.0, eps[:, :2])                    # base samples of another q
    af = utils.qExpectedImprovement(model, p.best_f(), num_samples=32, generator=torch.Generator().manual_seed(0))
    v1, v2 = af(p.X), af(p.X)
    assert af.q == p.q and af.model is model and v1.shape == (p.B,)
    torch.testing.assert_close(v1, v2, rtol=1e-10, atol=0)   # fixed base samples: the same function at every call
    v, g = af.value_and_grad(p.X)
    assert g.shape == p.X.shape
    torch.testing.assert_close(v, v1, rtol=1e-10, atol=0)


def test_suggest_batch(device):
    p = JointProblem((32, 32, 32), 2, 12, 1, 3, 0, 0, seed=4)
    stack, model = p.model(device)
    gps = model.source_gps

    def loop(**kw):
        lp = ScaMLGPBOLoop(gps, 2, raw_samples=64, num_restarts=4, af_max_iter=15, seed=1, num_mc_samples=64, **kw)
        lp.record(p.Xt, p.yt.squeeze(-1))
        lp.model.weights = p.w.clone()
        return lp

    for acquisition in ("ucb", "ei"):
        lp = loop(acquisition=acquisition, max_pending_evaluations=3)
        X = lp.suggest_batch(3)
        assert X.shape == (3, 2) and bool(((X >= 0) & (X <= 1)).all())
        assert lp.pending.shape[0] == 3
        # the result is at least as good as the best raw batch: the same draws, scored by the same acquisition function
        # (a second loop with the same seed replays the draws: the base samples first, then the raw batches)
        lp2 = loop(acquisition=acquisition)
        af = lp2.joint_acquisition_function(3)
        cand = torch.rand(64, 3, 2, dtype=torch.float64, generator=lp2.gen)
        best_raw = float(af(cand).max())
        v = float(af(X.unsqueeze(0))[0])
        assert v >= best_raw - 1e-6 * max(1.0, abs(v))
        with pytest.raises(NotImplementedError):
            lp.suggest_batch(1)                                              # points are pending
    with pytest.raises(ValueError):
        loop(acquisition="logei").suggest_batch(2)
    with pytest.raises(ValueError):
        loop(max_pending_evaluations=2).suggest_batch(3)                     # q > k
    lp = loop()
    X = lp.suggest_batch(2)
    assert X.shape == (2, 2) and lp.pending.shape[0] == 0                    # no bookkeeping without max_pending_evaluations
    # one idle worker: q = 1 takes the joint route too
    for acquisition in ("ucb", "ei"):
        lp = loop(acquisition=acquisition, max_pending_evaluations=2)
        X = lp.suggest_batch(1)
        assert X.shape == (1, 2) and bool(((X >= 0) & (X <= 1)).all()) and lp.pending.shape[0] == 1
    # ... and a q = 1 joint function reads a flat list of points as the analytic functions do
    af = loop().joint_acquisition_function(1)
    pts = torch.rand(5, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    torch.testing.assert_close(af(pts), af(pts.unsqueeze(1)), rtol=1e-10, atol=0)
