"""The value-only route of the joint q-point acquisition on the MI355X: the value-layout joint source pass
(scaml_posterior_linv_cov_joint_f64, (5h)), the value-only acquisition kernel (scaml_target_qacqf_value_f64, (7r)),
ScaMLGP.joint_acqf_value, score_mode="value_pass" of the acquisition classes and ScaMLGPBOLoop(joint_score_mode="value_pass").

  (5h) against the joint GRAD pass (5g) at the same points: mu, var and all Ma + q rows of cov against column 16 j of (5g)'s outputs
  to 1e-9 max|ref|, the suite's figure for two device routes (tests/test_qacqf_gpu.py holds (5g) to (5d) at it); mate rows of padding
  columns are zero.
  joint_acqf_value_full against joint_acqf_full's value at the same figure, jitter and info equal, none set.
  Against torch autograd through the ORACLE on the CPU in fp64: _close's rule, rtol 1e-4 and atol 1e-4 max|ref|.  The reference is held
  to cond(Sigma) <= 1e4 and to the tie and kink margins (tests/_qacqf_ref.py) on every batch of every case, both codes, at seed 1.
  Measured worst ratios: profiles/qacqf_value_notes.md.
  The kernel's own arithmetic is held to an a-priori per-element fp64 bound, on planted arrays at the shape edges, by
  tests/test_qacqf_bounds_gpu.py (tests/_qacqf_bounds.py; figures in profiles/qacqf_bounds_notes.md).

Shapes, by where the packing and the extra tile can go wrong (bps = 16 // q batches per strip):
  (32, 20, 17) D 2  n 17 B 6  q 3 p 0   bps 5, one padding column, the second strip holds one batch; N = 32 with nas = NB: the extra image
  (32, 32, 32) D 15 n 1  B 3  q 8 p 0   bps 2, n = 1
  (32, 20, 17) D 15 n 17 B 4  q 5 p 3   bps 3, pending
  (32, 32, 32) D 2  n 17 B 17 q 1 p 0   q = 1, 17 columns
  (96, 96)     D 15 n 88 B 2  q 7 p 1   n + p + q = 96, Ma = 89: six leading tiles plus the Gram tile, two padding columns
  (32, 32, 32) D 2  n 17 B 16 q 2 p 6   two strips exactly full, q + p = 8"""
import math

import pytest
import torch

from scamlgp_amd import ops, utils
from scamlgp_amd.bo import ScaMLGPBOLoop
from tests import _qacqf_ref as R
from tests._qacqf_problem import JointProblem

pytestmark = pytest.mark.gpu

SEED = 1
#        ns            D   n   B  q  p  kind_s kind_t S
CASES = [((32, 20, 17), 2, 17, 6, 3, 0, 0, 0, 300),
         ((32, 32, 32), 15, 1, 3, 8, 0, 1, 1, 512),
         ((32, 20, 17), 15, 17, 4, 5, 3, 1, 0, 300),
         ((32, 32, 32), 2, 17, 17, 1, 0, 0, 1, 1),
         ((96, 96), 15, 88, 2, 7, 1, 1, 0, 300),
         ((32, 32, 32), 2, 17, 16, 2, 6, 0, 1, 300)]
_IDS = [f"N{max(c[0])}{'r' if len(set(c[0])) > 1 else ''}-D{c[1]}-n{c[2]}-B{c[3]}-q{c[4]}-p{c[5]}-S{c[8]}" for c in CASES]
CODES = [R.ACQF_EI, R.ACQF_UCB]
_BUILT, _REF = {}, {}


def _problem(case, device):
    """A case's problem (the last p points of every batch are the pending set), its model on the GPU, the pending points (None with
    p = 0) and the base samples: built once, shared, never changed."""
    if case not in _BUILT:
        ns, D, n, B, q, p, ks, kt, S = case
        pr = JointProblem(ns, D, n, B, q + p, ks, kt, SEED)
        Xp = torch.rand(p, D, dtype=torch.float64, generator=torch.Generator().manual_seed(500 + SEED))
        pr.X = torch.cat([pr.X[:, :q], Xp.expand(B, p, D)], 1).contiguous()
        eps = torch.randn(S, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(100 + SEED))
        _BUILT[case] = (pr, pr.model(device), Xp if p > 0 else None, eps)
    return _BUILT[case]


def _par(pr, acqf):
    return pr.best_f() if acqf == R.ACQF_EI else 4.0


def _reference(case, device, acqf):
    """Oracle values of the (q + p)-point statement, both conditions asserted on every batch.  Computed once per (case, code)."""
    if (case, acqf) not in _REF:
        pr, _, _, eps = _problem(case, device)
        _REF[case, acqf] = pr.reference(eps, acqf, _par(pr, acqf))[0]
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


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_value_layout_pass_against_the_grad_layout_pass(device, case):
    pr, (stack, model), Xp, eps = _problem(case, device)
    ns, D, n, B, q, p = case[:6]
    st, f = model._stack, model._stack.fit
    X = pr.X[:, :q].to(device)
    Xq = X.reshape(B * q, D).contiguous()
    if Xp is None:
        Xa, VA = model.train_X, model._train_VA()
    else:
        pend = model.joint_pending(Xp)
        Xa, VA = pend["Xa"], pend["VA"]
    Ma, Mq = int(VA.shape[-1]), B * q
    assert Ma == n + p
    src = (st.X, st.theta, st.kind)
    VQ = ops.source_posteriors(Xq, *src, f["L"], f["Linv_diag"], f["alpha"], st.y_mean, st.y_std, n_points=st.n_points, want_var=False,
                               keep_V=True, Linv=f["Linv"])["V"]
    g = ops.source_posteriors_grad_joint(Xq, q, Xa, *src, f["Linv"], f["alpha"], VA, VQ, st.y_mean, st.y_std, st.n_points)
    packed = ops.qacqf_value_pack(X)
    Mp = packed.shape[0]
    assert Mp == 16 * -(-B // (16 // q))
    v = ops.source_posteriors_cov_joint(packed, B, q, Xa, *src, f["Linv"], f["alpha"], VA, st.y_mean, st.y_std, st.n_points)
    assert v["mu"].shape == (st.T, Mp) and v["var"].shape == (st.T, Mp) and v["cov"].shape == (st.T, Ma + q, Mp)
    cols = ops.qacqf_value_column_map(B, q).reshape(-1).to(device)
    _route(v["mu"][:, cols], g["mu"][:, :, 0], "mu")
    _route(v["var"][:, cols], g["var"][:, :, 0], "var")
    cov_g = g["cov"].reshape(st.T, Ma + q, Mq, 16)[..., 0]
    _route(v["cov"][:, :Ma][:, :, cols], cov_g[:, :Ma], "cov, leading rows")
    _route(v["cov"][:, Ma:][:, :, cols], cov_g[:, Ma:], "cov, mate rows")
    assert bool(torch.isfinite(v["cov"]).all()) and bool(torch.isfinite(v["mu"]).all()) and bool(torch.isfinite(v["var"]).all())
    pad = torch.ones(Mp, dtype=torch.bool, device=device)
    pad[cols] = False
    assert int(pad.sum()) == Mp - Mq
    assert not bool(v["cov"][:, Ma:][:, :, pad].any()), "mate rows of padding columns are zero"
    # the point's own mate row is its variance
    own = ops.qacqf_value_column_map(B, q).to(device)
    for r in range(q):
        _route(v["cov"][:, Ma + r, own[:, r]], v["var"][:, own[:, r]], f"own row {r} / var")


@pytest.mark.parametrize("acqf", CODES, ids=["qEI", "qUCB"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_value_route_against_the_gradient_route_and_the_oracle(device, case, acqf):
    pr, (stack, model), Xp, eps = _problem(case, device)
    q, par = case[4], _par(pr, acqf)
    X = pr.X[:, :q]
    want = model.joint_acqf_full(X, acqf, par, eps, want_grad=False, X_pending=Xp)
    out = model.joint_acqf_value_full(X, acqf, par, eps, X_pending=Xp)
    assert set(out) == {"value", "jitter", "info"} and out["value"].shape == (pr.B,)
    _route(out["value"], want["value"], "value / joint_acqf_full")
    assert torch.equal(out["info"], want["info"]) and torch.equal(out["jitter"], want["jitter"])
    assert not bool(out["info"].any()) and not bool(out["jitter"].any())
    assert torch.equal(model.joint_acqf_value(X, acqf, par, eps, X_pending=Xp).isfinite(), torch.ones(pr.B, dtype=torch.bool, device=device))
    _close(out["value"].cpu(), _reference(case, device, acqf), "value / oracle")   # (asserts the two conditions on every batch)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_two_calls(device, case):
    pr, (stack, model), Xp, eps = _problem(case, device)
    q = case[4]
    X = pr.X[:, :q]
    kw = model.joint_acqf_value_inputs(X, eps, X_pending=Xp)
    assert kw.pop("shape") == (pr.B, q, pr.D)
    assert ("Xp" in kw) == (Xp is not None)
    for acqf in CODES:
        # the kernel on the same tensors: bit for bit
        once, again = (ops.target_qacqf_value(acqf=acqf, acqf_param=_par(pr, acqf), **kw) for _ in range(2))
        for k in ("value", "jitter", "info"):
            assert torch.equal(again[k], once[k]), k
        # the model method: the source pass's mu / var go through LDS float atomics
        a, b = (model.joint_acqf_value(X, acqf, _par(pr, acqf), eps, X_pending=Xp) for _ in range(2))
        torch.testing.assert_close(a, b, rtol=1e-10, atol=0)
        torch.testing.assert_close(a, once["value"], rtol=1e-10, atol=0)
    # an empty call, and an empty pending set
    assert model.joint_acqf_value(X[:0], R.ACQF_EI, 0.0, eps, X_pending=Xp).shape == (0,)
    if Xp is None:
        v = model.joint_acqf_value(X, R.ACQF_UCB, 4.0, eps, X_pending=torch.empty(0, pr.D, dtype=torch.float64))
        torch.testing.assert_close(v, model.joint_acqf_value(X, R.ACQF_UCB, 4.0, eps), rtol=1e-10, atol=0)


def test_containment_inside_a_shared_strip(device):
    case = CASES[0]   # batches 0 .. 4 share the first strip, batch 5 has the second
    pr, (stack, model), Xp, eps = _problem(case, device)
    q = case[4]
    for acqf in CODES:
        par = _par(pr, acqf)
        clean = model.joint_acqf_value(pr.X[:, :q], acqf, par, eps)
        assert bool(torch.isfinite(clean).all())
        X = pr.X[:, :q].clone()
        X[1, 2, 0] = float("nan")
        X[5, 0, 1] = float("inf")
        v = model.joint_acqf_value(X, acqf, par, eps)
        assert torch.isnan(v).tolist() == [False, True, False, False, False, True]
        keep = [0, 2, 3, 4]
        torch.testing.assert_close(v[keep], clean[keep], rtol=1e-10, atol=0)
    # the source pass alone: the bad point's own column is NaN, every other column of its strip -- its batch mates' leading rows, mu and
    # var included -- is what it was
    st, f = model._stack, model._stack.fit
    args = (model.train_X, st.X, st.theta, st.kind, f["Linv"], f["alpha"], model._train_VA(), st.y_mean, st.y_std, st.n_points)
    good = ops.source_posteriors_cov_joint(ops.qacqf_value_pack(pr.X[:, :q].to(device)), pr.B, q, *args)
    bad = ops.source_posteriors_cov_joint(ops.qacqf_value_pack(X.to(device)), pr.B, q, *args)
    cols = ops.qacqf_value_column_map(pr.B, q)
    c_nan, c_inf, n = int(cols[1, 2]), int(cols[5, 0]), case[2]
    for c in (c_nan, c_inf):
        assert bool(torch.isnan(bad["mu"][:, c]).all()) and bool(torch.isnan(bad["var"][:, c]).all()) and bool(torch.isnan(bad["cov"][:, :, c]).all())
    others = [c for c in range(good["mu"].shape[1]) if c not in (c_nan, c_inf)]
    torch.testing.assert_close(bad["mu"][:, others], good["mu"][:, others], rtol=1e-10, atol=0)
    torch.testing.assert_close(bad["var"][:, others], good["var"][:, others], rtol=1e-10, atol=0)
    assert torch.equal(bad["cov"][:, :n][:, :, others], good["cov"][:, :n][:, :, others])   # (the leading rows are ordered sums)
    foreign = [c for c in others if c not in cols[1].tolist() and c not in cols[5].tolist()]
    assert torch.equal(bad["cov"][:, n:][:, :, foreign], good["cov"][:, n:][:, :, foreign])   # mate rows of the other batches


def test_chunking_and_the_classes(device):
    case = CASES[5]   # 16 batches of 2 with 6 pending: two strips
    pr, (stack, model), Xp, eps = _problem(case, device)
    q = case[4]
    X = pr.X[:, :q]
    g1, g2 = torch.Generator().manual_seed(0), torch.Generator().manual_seed(0)
    af_g = utils.qExpectedImprovement(model, pr.best_f(), num_samples=64, generator=g1, X_pending=Xp)
    af_v = utils.qExpectedImprovement(model, pr.best_f(), num_samples=64, generator=g2, X_pending=Xp, score_mode="value_pass")
    assert af_g.score_mode == "grad_pass" and af_v.score_mode == "value_pass" and torch.equal(g1.get_state(), g2.get_state())
    assert torch.equal(af_g._eps, af_v._eps)   # (the draws; q is fixed by the first batch)
    whole = af_v(X)
    assert af_v.q == q and af_v.p == case[5] and af_v.base_samples.shape == (64, 8)
    assert af_v._value_pass_step() >= pr.B and whole.shape == (pr.B,)
    _route(whole, af_g(X), "qEI __call__, value_pass / grad_pass")
    # the cap lowered on the instance: a strip (8 batches) per call, two calls
    af_v.SCORE_COV_CAP_BYTES = 1
    assert af_v._value_pass_step() == 8 < pr.B
    torch.testing.assert_close(af_v(X), whole, rtol=1e-10, atol=0)
    torch.testing.assert_close(af_v(X[:11]), whole[:11], rtol=1e-10, atol=0)   # (a last chunk that is not full)
    # value_and_grad is the gradient route in both modes
    (v1, d1), (v2, d2) = af_g.value_and_grad(X), af_v.value_and_grad(X)
    torch.testing.assert_close(v2, v1, rtol=1e-10, atol=0)
    torch.testing.assert_close(d2, d1, rtol=1e-10, atol=1e-10 * float(d1.abs().max()))
    # qUCB, no pending points, q fixed by the first batch; a flat (M, D) list with q = 1
    pr0, (_, model0), _, _ = _problem(CASES[0], device)
    u_g, u_v = (utils.qUpperConfidenceBound(model0, 4.0, num_samples=32, generator=torch.Generator().manual_seed(3), score_mode=m)
                for m in ("grad_pass", "value_pass"))
    _route(u_v(pr0.X), u_g(pr0.X), "qUCB __call__, value_pass / grad_pass")
    s_g, s_v = (utils.qUpperConfidenceBound(model0, 4.0, num_samples=32, generator=torch.Generator().manual_seed(3), q=1, score_mode=m)
                for m in ("grad_pass", "value_pass"))
    flat = pr0.X.reshape(-1, pr0.D)
    _route(s_v(flat), s_g(flat), "qUCB q = 1 on a flat list")
    # the refusals are joint_acqf's, raised before anything is launched
    with pytest.raises(ValueError, match="LogEI"):
        model.joint_acqf_value(X, ops.ACQF_LOGEI, 0.0, eps, X_pending=Xp)
    with pytest.raises(ValueError):
        model.joint_acqf_value(X, R.ACQF_EI, 0.0, eps[:, :q], X_pending=Xp)              # base samples of q, not q + p, columns
    with pytest.raises(NotImplementedError, match="q \\+ p <= 8"):
        model.joint_acqf_value(pr.X[:, :3], R.ACQF_EI, 0.0, torch.zeros(4, 9, dtype=torch.float64), X_pending=Xp)
    with pytest.raises(NotImplementedError):
        model.fantasize(Xp[:1], 4).joint_acqf_value(X, R.ACQF_EI, 0.0, eps, X_pending=Xp)
    tight = JointProblem((32, 32, 32), 2, 27, 1, 2, 0, 0, seed=1)   # n = 27 on an N = 32 stack leaves room for 5 points
    _, tight_model = tight.model(device)
    with pytest.raises(NotImplementedError, match="n \\+ p \\+ q <= 32"):
        tight_model.joint_acqf_value(tight.X, R.ACQF_EI, 0.0, torch.zeros(4, 6, dtype=torch.float64), X_pending=Xp[:4, :2].contiguous())


def test_suggest_batch_in_value_pass_mode(device):
    pr = JointProblem((32, 32, 32), 2, 12, 1, 3, 0, 0, seed=4)
    stack, model = pr.model(device)
    gps = model.source_gps

    def loop(mode, acquisition):
        lp = ScaMLGPBOLoop(gps, 2, raw_samples=64, num_restarts=4, af_max_iter=15, seed=1, num_mc_samples=64, num_restarts_log_likelihood=1,
                           acquisition=acquisition, max_pending_evaluations=5, joint_pending="joint", joint_score_mode=mode)
        lp.record(pr.Xt, pr.yt.squeeze(-1))
        lp.model.weights = pr.w.clone()
        return lp

    for acquisition in ("ucb", "ei"):
        lp_v, lp_g, lp_r = (loop(m, acquisition) for m in ("value_pass", "grad_pass", "value_pass"))
        assert lp_v.joint_score_mode == "value_pass" and lp_v.joint_acquisition_function(3).score_mode == "value_pass"
        lp_g.joint_acquisition_function(3), lp_r.joint_acquisition_function(3)   # (the same draws from every generator)
        pend = None
        for q in (3, 2):   # without points pending, then with the three of the first call
            Xv, Xg = lp_v.suggest_batch(q), lp_g.suggest_batch(q)
            assert Xv.shape == (q, 2) and bool(torch.isfinite(Xv).all()) and bool(((Xv >= 0) & (Xv <= 1)).all())
            assert torch.equal(lp_v.gen.get_state(), lp_g.gen.get_state())   # the two modes consume the same draws
            # a third loop replays the draws: every raw batch scores finite, and the result is at least as good as the best of them
            af = lp_r.joint_acquisition_function(q, X_pending=pend)
            cand = torch.rand(64, q, 2, dtype=torch.float64, generator=lp_r.gen)
            vals = af(cand)
            assert bool(torch.isfinite(vals).all())
            v = float(af(Xv.unsqueeze(0))[0])
            print(f"{acquisition} q={q}: value {v:.6g}, best raw batch {float(vals.max()):.6g}")
            assert math.isfinite(v) and v >= float(vals.max()) - 1e-6 * max(1.0, abs(v))
            lp_r.gen.set_state(lp_v.gen.get_state())
            lp_g.pending = lp_v.pending.clone()   # (the twin goes on from the same pending set: its own points may differ by a rounding)
            pend = lp_v.pending.clone()
        assert lp_v.pending.shape[0] == 5
