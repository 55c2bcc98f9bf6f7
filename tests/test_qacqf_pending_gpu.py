"""Joint q-point Monte-Carlo acquisition with evaluations pending on the MI355X: the acquisition kernel
(scaml_target_qacqf_pending_f64, (7q)), ScaMLGP.joint_acqf(X_pending=...), the acquisition classes and
ScaMLGPBOLoop(joint_pending="joint").suggest_batch.

  The new route (the pending points as LEADING points of the source pass, B q strips) against the concatenated route
  ``joint_acqf(cat(X, X_pending))`` at q' = q + p (every pending point a batch mate, B (q + p) strips; code that the oracle already
  holds): value and the q moving points' gradient to 1e-9 max|ref|, the suite's figure for two device routes.
  Both against torch autograd through the ORACLE on the CPU in fp64: _close's rule, rtol 1e-4 and atol 1e-4 max|ref|.  The reference
  is held to cond(Sigma) <= 1e4 on the (q + p)-point joint and to the margin of 1e-6 sqrt(max Sigma_jj) of every sample from a tie
  and from a kink (tests/_qacqf_ref.py), every batch of every case, both codes; the seed was picked on the CPU so that both hold.
  Measured worst ratios: profiles/qacqf_pending_notes.md.
  The kernel's own arithmetic is held to an a-priori per-element fp64 bound, on planted arrays at the shape edges, by
  tests/test_qacqf_bounds_gpu.py (tests/_qacqf_bounds.py; figures in profiles/qacqf_bounds_notes.md).

Shapes: T = 3 with one pruned weight, ragged n_points (32, 20, 17) at N = 32; D in {2, 15}; (q, p) in {(2, 1), (1, 7), (3, 5), (4, 4),
(7, 1), (1, 1)}; B in {1, 3, 5}; n in {1, 17}, and n = 88 with (3, 5) on a T = 2, N = 96 stack (n + p + q = 96, the last row of the
covariance block); S in {1, 300, 512}; both kernel families for sources and target; both codes."""
import copy
import math

import pytest
import torch

from scamlgp_amd import ops, utils
from scamlgp_amd.bo import OptimizerNotReady, ScaMLGPBOLoop
from tests import _qacqf_ref as R
from tests._qacqf_problem import JointProblem

pytestmark = pytest.mark.gpu

SEED = 1
#        ns            D   n   B  q  p  kind_s kind_t S
CASES = [((32, 20, 17), 2, 17, 5, 2, 1, 0, 0, 300),
         ((32, 32, 32), 15, 1, 1, 1, 7, 1, 1, 512),
         ((96, 96), 15, 88, 1, 3, 5, 1, 0, 300),
         ((32, 20, 17), 15, 17, 5, 4, 4, 1, 0, 512),
         ((32, 32, 32), 2, 17, 5, 7, 1, 0, 1, 1),
         ((32, 32, 32), 2, 1, 3, 1, 1, 0, 1, 300)]
_IDS = [f"N{max(c[0])}{'r' if len(set(c[0])) > 1 else ''}-D{c[1]}-n{c[2]}-B{c[3]}-q{c[4]}-p{c[5]}-S{c[8]}" for c in CASES]
LIVE = [CASES[i] for i in (1, 2, 3, 5)]   # the cases in which pending entries win samples: evidence for the pending terms
CODES = [R.ACQF_EI, R.ACQF_UCB]
_BUILT, _REF = {}, {}


def _problem(case, device):
    """A case's problem (the last p points of every batch are the pending set), its model on the GPU, the pending points and the base
    samples: built once, shared, never changed."""
    if case not in _BUILT:
        ns, D, n, B, q, p, ks, kt, S = case
        pr = JointProblem(ns, D, n, B, q + p, ks, kt, SEED)
        Xp = torch.rand(p, D, dtype=torch.float64, generator=torch.Generator().manual_seed(500 + SEED))
        pr.X = torch.cat([pr.X[:, :q], Xp.expand(B, p, D)], 1).contiguous()
        eps = torch.randn(S, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(100 + SEED))
        _BUILT[case] = (pr, pr.model(device), Xp, eps)
    return _BUILT[case]


def _par(pr, acqf):
    return pr.best_f() if acqf == R.ACQF_EI else 4.0


def _reference(case, device, acqf):
    """Oracle autograd of the (q + p)-point statement, both conditions asserted on every batch: value (B,) and the moving points'
    gradient (B, q, D).  Computed once per (case, code)."""
    if (case, acqf) not in _REF:
        pr, _, _, eps = _problem(case, device)
        v, g = pr.reference(eps, acqf, _par(pr, acqf))
        _REF[case, acqf] = (v, g[:, :case[4]].contiguous())
    return _REF[case, acqf]


def _close(got, ref, what, rtol=1e-4):
    tol = rtol * float(ref.abs().max())
    print(f"{what}: worst |got - ref| / (rtol |ref| + atol) = {float(((got - ref).abs() / (rtol * ref.abs() + tol + 1e-300)).max()):.3g}")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=tol + 1e-300)


def _route(got, ref, what):
    """Two device routes to the same numbers: 1e-9 of the reference's largest entry."""
    tol = 1e-9 * float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"{what}: err {err:.3e} tol {tol:.3e} ratio {err / tol if tol > 0 else 0.0:.3g}")
    assert err <= tol, what


def _pending_kw(model, pr, q, Xp, eps):
    kw = model.joint_acqf_inputs(pr.X[:, :q], eps, X_pending=Xp)
    kw.pop("shape")
    return kw


@pytest.mark.parametrize("acqf", CODES, ids=["qEI", "qUCB"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_pending_route_against_the_concatenated_route(device, case, acqf):
    pr, (stack, model), Xp, eps = _problem(case, device)
    q, par = case[4], _par(pr, acqf)
    cat = model.joint_acqf_full(pr.X, acqf, par, eps, want_grad=True)
    out = model.joint_acqf_full(pr.X[:, :q], acqf, par, eps, want_grad=True, X_pending=Xp)
    assert out["grad"].shape == (pr.B, q, pr.D)
    _route(out["value"], cat["value"], "value")
    _route(out["grad"], cat["grad"][:, :q], "grad")
    assert torch.equal(out["info"], cat["info"]) and torch.equal(out["jitter"], cat["jitter"])
    assert not bool(out["info"].any())
    # the dict joint_pending made of the points is what the acquisition classes pass: the same numbers (to the source pass's rounding)
    v, g = model.joint_acqf(pr.X[:, :q], acqf, par, eps, want_grad=True, X_pending=model.joint_pending(Xp))
    _route(v, out["value"], "value, prepared pending set")
    _route(g, out["grad"], "grad, prepared pending set")
    v_only, none = model.joint_acqf(pr.X[:, :q], acqf, par, eps, X_pending=Xp)
    assert none is None
    _route(v_only, out["value"], "value only")


@pytest.mark.parametrize("acqf", CODES, ids=["qEI", "qUCB"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_pending_route_against_oracle_autograd(device, case, acqf):
    pr, (stack, model), Xp, eps = _problem(case, device)
    q, par = case[4], _par(pr, acqf)
    v_ref, g_ref = _reference(case, device, acqf)   # (asserts the two conditions on every batch)
    assert float(g_ref.abs().max()) > 0
    out = model.joint_acqf_full(pr.X[:, :q], acqf, par, eps, want_grad=True, X_pending=Xp)
    assert not bool(out["info"].any()) and not bool(out["jitter"].any())
    _close(out["value"].cpu(), v_ref, "value")
    _close(out["grad"].cpu(), g_ref, "grad")


@pytest.mark.parametrize("acqf", CODES, ids=["qEI", "qUCB"])
@pytest.mark.parametrize("case", LIVE, ids=[_IDS[i] for i in (1, 2, 3, 5)])
def test_the_pending_terms_are_live_in_the_reference(device, case, acqf):
    """Not vacuous: in the reference pending entries win samples, and the moving points' gradient differs from the gradient WITHOUT the
    pending points by more than 1e-2 max|ref| -- a kernel that ignored the pending columns of Sbar, Zp or the mixed dP could not pass
    the comparison above."""
    pr, _, _, eps = _problem(case, device)
    q, par = case[4], _par(pr, acqf)
    pend = mov = 0
    for b in range(pr.B):
        with torch.no_grad():
            mu, Sg = pr.joint_posterior(pr.X[b])
        u, g, _ = R.utilities(mu, 0.5 * (Sg + Sg.T), eps, acqf, par)
        j = (g if acqf == R.ACQF_EI else u).argmax(-1)
        pend, mov = pend + int((j >= q).sum()), mov + int((j < q).sum())
    print(f"a pending entry wins {pend} samples, a moving one {mov}")
    assert pend > 0
    _, g_ref = _reference(case, device, acqf)
    free = copy.copy(pr)
    free.q, free.X = q, pr.X[:, :q].contiguous()
    _, g_free = free.reference(eps[:, :q].contiguous(), acqf, par, check=False)
    diff = float((g_ref - g_free).abs().max()) / float(g_ref.abs().max())
    print(f"the gradient with / without the pending points differs by {diff:.3g} of max|ref|")
    assert diff > 1e-2


def test_both_kinds_of_winner_in_one_case_per_code(device):
    """... and in at least one case per code some samples are won by a pending entry and some by a moving one."""
    for acqf in CODES:
        found = False
        for case in LIVE:
            pr, _, _, eps = _problem(case, device)
            q, par = case[4], _par(pr, acqf)
            for b in range(pr.B):
                with torch.no_grad():
                    mu, Sg = pr.joint_posterior(pr.X[b])
                u, g, _ = R.utilities(mu, 0.5 * (Sg + Sg.T), eps, acqf, par)
                j = (g if acqf == R.ACQF_EI else u).argmax(-1)
                found = found or (bool((j >= q).any()) and bool((j < q).any()))
        assert found, acqf


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_two_calls_agree_bit_for_bit_and_p0_is_7p(device, case):
    pr, (stack, model), Xp, eps = _problem(case, device)
    q = case[4]
    kw = _pending_kw(model, pr, q, Xp, eps)
    for acqf in CODES:
        once, again = (ops.target_qacqf_pending(acqf=acqf, acqf_param=_par(pr, acqf), **kw) for _ in range(2))
        for k in ("value", "grad", "jitter", "info"):
            assert torch.equal(again[k], once[k]), k
    # no pending points: (7p)'s inputs through the new entry point give (7p)'s bits
    kw0 = model.joint_acqf_inputs(pr.X, eps)
    kw0.pop("shape")
    none = dict(Xp=torch.empty(0, pr.D, dtype=torch.float64, device=device), Zp=None, mu_p=None, Sigma_pp=None)
    for acqf in CODES:
        want = ops.target_qacqf(acqf=acqf, acqf_param=_par(pr, acqf), **kw0)
        got = ops.target_qacqf_pending(acqf=acqf, acqf_param=_par(pr, acqf), **kw0, **none)
        for k in ("value", "grad", "jitter", "info"):
            assert torch.equal(got[k], want[k]), k
        assert bool(torch.isfinite(got["value"]).all())


def test_a_moving_point_equal_to_a_pending_point(device):
    case = CASES[0]
    pr, (stack, model), Xp, eps = _problem(case, device)
    q = case[4]
    X = pr.X.clone()
    X[0, 1] = Xp[0]
    par = pr.best_f()
    out = model.joint_acqf_full(X[:, :q], R.ACQF_EI, par, eps, want_grad=True, X_pending=Xp)
    jit = out["jitter"].cpu()
    assert not bool(out["info"].any())
    assert all(float(j) in R.LADDER for j in jit)
    print("jitter of the singular batch:", float(jit[0]))
    mu, Sigma = pr.joint_posterior(X[0])
    # (the reference's own Sigma is singular to rounding: the factor of a semidefinite matrix, the limit of the jittered ones, is what
    #  both sides approximate -- tests/test_qacqf_gpu.py::test_a_batch_with_two_equal_points)
    ref = R.mc_value_semidefinite(mu.detach(), 0.5 * (Sigma + Sigma.T).detach(), eps, par, float(jit[0]))
    assert float(out["value"][0]) == pytest.approx(float(ref), rel=1e-6)


def test_nan_containment(device):
    case = CASES[0]
    pr, (stack, model), Xp, eps = _problem(case, device)
    q, B, D = case[4], pr.B, pr.D
    nan = float("nan")
    # the kernel: one set of inputs, then the same with one coordinate of batch 2 replaced -- that batch is NaN, the others bit for bit
    kw = _pending_kw(model, pr, q, Xp, eps)
    base = ops.target_qacqf_pending(acqf=R.ACQF_UCB, acqf_param=4.0, **kw)
    assert bool(torch.isfinite(base["value"]).all()) and bool(torch.isfinite(base["grad"]).all())
    bad = dict(kw, Xq=kw["Xq"].clone())
    bad["Xq"][2 * q + 1, 0] = nan
    out = ops.target_qacqf_pending(acqf=R.ACQF_UCB, acqf_param=4.0, **bad)
    grad, grad0 = out["grad"].reshape(B, q, D), base["grad"].reshape(B, q, D)
    assert math.isnan(float(out["value"][2])) and bool(torch.isnan(grad[2]).all())
    for b in (0, 1, 3, 4):
        assert torch.equal(out["value"][b], base["value"][b]) and torch.equal(grad[b], grad0[b])
    # a NaN anywhere in the pending set's arrays: every batch, the pending set being shared
    for name in ("Xp", "Zp", "mu_p", "Sigma_pp"):
        bad = dict(kw)
        bad[name] = kw[name].clone()
        bad[name].reshape(-1)[-1] = nan
        out = ops.target_qacqf_pending(acqf=R.ACQF_UCB, acqf_param=4.0, **bad)
        assert bool(torch.isnan(out["value"]).all()) and bool(torch.isnan(out["grad"]).all()), name
    # the whole chain: a NaN coordinate in a moving point stays in its batch, the others to the source pass's rounding ...
    clean = model.joint_acqf_full(pr.X[:, :q], R.ACQF_UCB, 4.0, eps, want_grad=True, X_pending=Xp)
    X = pr.X[:, :q].clone()
    X[2, 1, 0] = nan
    out = model.joint_acqf_full(X, R.ACQF_UCB, 4.0, eps, want_grad=True, X_pending=Xp)
    assert math.isnan(float(out["value"][2])) and bool(torch.isnan(out["grad"][2]).all())
    keep = [0, 1, 3, 4]
    torch.testing.assert_close(out["value"][keep], clean["value"][keep], rtol=1e-10, atol=0)
    torch.testing.assert_close(out["grad"][keep], clean["grad"][keep], rtol=1e-10, atol=1e-10 * float(clean["grad"].abs().max()))
    # ... and one in a pending point reaches every batch
    bad_p = Xp.clone()
    bad_p[0, 1] = nan
    out = model.joint_acqf_full(pr.X[:, :q], R.ACQF_UCB, 4.0, eps, want_grad=True, X_pending=bad_p)
    assert bool(torch.isnan(out["value"]).all()) and bool(torch.isnan(out["grad"]).all())


def test_refusals_and_the_acquisition_classes(device):
    case = CASES[3]   # q = 4, p = 4
    pr, (stack, model), Xp, eps = _problem(case, device)
    q = case[4]
    five = torch.cat([Xp, Xp[:1] + 0.01])
    with pytest.raises(NotImplementedError, match="q \\+ p <= 8"):
        model.joint_acqf(pr.X[:, :q], R.ACQF_EI, 0.0, torch.zeros(4, q + 5, dtype=torch.float64), X_pending=five)     # q + p = 9
    with pytest.raises(ValueError):
        model.joint_acqf(pr.X[:, :q], R.ACQF_EI, 0.0, eps[:, :q], X_pending=Xp)              # base samples of q, not q + p, columns
    with pytest.raises(NotImplementedError):
        model.fantasize(Xp[:1], 4).joint_acqf(pr.X[:, :q], R.ACQF_EI, 0.0, eps, X_pending=Xp)
    # n + p + q beyond the covariance block: n = 27 on an N = 32 stack leaves room for 5 points
    tight = JointProblem((32, 32, 32), 2, 27, 1, 2, 0, 0, seed=1)
    _, tight_model = tight.model(device)
    with pytest.raises(NotImplementedError, match="n \\+ p \\+ q <= 32"):
        tight_model.joint_acqf(tight.X, R.ACQF_EI, 0.0, torch.zeros(4, 6, dtype=torch.float64), X_pending=Xp[:, :2].contiguous())
    # an empty pending set takes the path without pending points: base samples of q columns, the same launches
    v0 = model.joint_acqf(pr.X, R.ACQF_EI, 0.3, eps)[0]
    torch.testing.assert_close(model.joint_acqf(pr.X, R.ACQF_EI, 0.3, eps, X_pending=Xp[:0])[0], v0, rtol=1e-10, atol=0)
    # the classes: the draws are (num_samples, 8) whatever p is, a batch reads the leading q + p columns
    g1, g2 = torch.Generator().manual_seed(0), torch.Generator().manual_seed(0)
    af = utils.qExpectedImprovement(model, pr.best_f(), num_samples=32, generator=g1, X_pending=Xp)
    af0 = utils.qExpectedImprovement(model, pr.best_f(), num_samples=32, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    v1, v2 = af(pr.X[:, :q]), af(pr.X[:, :q])
    assert af.q == q and af.p == 4 and af.base_samples.shape == (32, 8) and v1.shape == (pr.B,)
    assert torch.equal(af.base_samples, af0._eps)
    torch.testing.assert_close(v1, v2, rtol=1e-10, atol=0)
    v, g = af.value_and_grad(pr.X[:, :q])
    assert g.shape == (pr.B, q, pr.D)
    torch.testing.assert_close(v, v1, rtol=1e-10, atol=0)
    want = model.joint_acqf(pr.X[:, :q], R.ACQF_EI, pr.best_f(), af.base_samples, X_pending=Xp)[0]
    torch.testing.assert_close(v, want, rtol=1e-10, atol=0)
    with pytest.raises(NotImplementedError, match="q \\+ p <= 8"):
        utils.qUpperConfidenceBound(model, 4.0, num_samples=8, q=5, X_pending=Xp)


def test_suggest_batch_with_points_pending(device):
    pr = JointProblem((32, 32, 32), 2, 12, 1, 3, 0, 0, seed=4)
    stack, model = pr.model(device)
    gps = model.source_gps

    def loop(**kw):
        lp = ScaMLGPBOLoop(gps, 2, raw_samples=64, num_restarts=4, af_max_iter=15, seed=1, num_mc_samples=64, num_restarts_log_likelihood=1, **kw)
        lp.record(pr.Xt, pr.yt.squeeze(-1))
        lp.model.weights = pr.w.clone()
        return lp

    for acquisition in ("ucb", "ei"):
        lp = loop(acquisition=acquisition, max_pending_evaluations=4, joint_pending="joint")
        X1 = lp.suggest_batch(2)
        assert X1.shape == (2, 2) and lp.pending.shape[0] == 2
        X2 = lp.suggest_batch(2)                                           # two points pending
        assert X2.shape == (2, 2) and bool(((X2 >= 0) & (X2 <= 1)).all())
        assert lp.pending.shape[0] == 4 and torch.equal(lp.pending, torch.cat([X1, X2]))
        # the result is at least as good as the best raw batch: a twin loop with the same seed replays the draws of both calls (the
        # base samples first, then the raw batches), and the same acquisition function, X_pending included, scores both
        lp2 = loop(acquisition=acquisition, max_pending_evaluations=4, joint_pending="joint")
        lp2.suggest_batch(2)   # (its generator is now where lp's was before the second call; its points may differ from X1 by a rounding)
        af = lp2.joint_acquisition_function(2, X_pending=X1)
        assert af.p == 2
        cand = torch.rand(64, 2, 2, dtype=torch.float64, generator=lp2.gen)
        best_raw = float(af(cand).max())
        v = float(af(X2.unsqueeze(0))[0])
        print(f"{acquisition}: value {v:.6g}, best raw batch {best_raw:.6g}")
        assert v >= best_raw - 1e-6 * max(1.0, abs(v))
        with pytest.raises(OptimizerNotReady):
            lp.suggest_batch(1)                                            # p >= k
        lp.report(torch.cat([X1, X2]), torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64))
        assert lp.pending.shape[0] == 0
    lp = loop(max_pending_evaluations=4, joint_pending="joint")
    lp.suggest_batch(2)
    with pytest.raises(ValueError):
        lp.suggest_batch(3)                                                # q + p > k
    with pytest.raises(NotImplementedError):
        lp_default = loop(max_pending_evaluations=4)
        lp_default.suggest_batch(2)
        lp_default.suggest_batch(1)                                        # the default still refuses
