"""CPU checks of the ARITHMETIC of the joint q-point acquisition kernel with evaluations pending (csrc/gp_qacqf.h: qa_batch<true>,
the body of scaml_target_qacqf_pending_kernel, include/scaml_gp.h (7q)) through a host build of the same source
(tests/host_emul/qacqf_pending_emul.cpp).

One synthetic prior with analytic covariance (``Problem`` of tests/test_qacqf_emul.py) at q' = q + p points per batch, the last p of
every batch being the same pending points, stated two ways:
  the concatenated route -- (7p)'s host build ``emul_qacqf`` at q' = q + p, every pending point a batch mate -- and torch autograd
  of the definition (tests/_qacqf_ref.py); from both the value and the first q gradient rows are the reference;
  the pending route -- the moving points alone in the value path, the pending points as leading points of the GRAD-layout sums
  (rows n + k), Zp, mu_p, Sigma_pp -- through ``emul_qacqf_pending``.
Tolerance: 1e-9 max|ref| per array, the figure of tests/test_qacqf_emul.py (the estimate Q^2 u cond is 7e-11 at Q = 8, cond = 1e4).
The reference is held to cond(Knn) <= 1e4, cond(Sigma) <= 1e4 on the (q + p)-point joint and to the margin of every sample from a tie
and from a kink (``assert_well_posed``), every batch, no sample left out.  Measured worst ratios: profiles/qacqf_pending_notes.md."""
import ctypes
import math

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests import _qacqf_ref as R
from tests._host_emul import DP, IP, build, ptr as _p
from tests.test_qacqf_emul import Problem, batch_reference, run_batch

NAN = float("nan")
_I, _F = ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """(the pending build, (7p)'s build)"""
    lib = build(tmp_path_factory, "qacqf_pending_emul")
    lib.emul_qacqf_pending.restype = _I
    lib.emul_qacqf_pending.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 11 + [_I, _F] + [_I] * 7 + [DP, DP, DP, IP]
    lib.emul_qacqf_pending_lds_doubles.restype, lib.emul_qacqf_pending_lds_doubles.argtypes = ctypes.c_longlong, [_I] * 4
    lib.emul_qacqf_pending_plan.restype, lib.emul_qacqf_pending_plan.argtypes = None, [_I] * 5 + [ctypes.POINTER(ctypes.c_longlong)]
    ref = build(tmp_path_factory, "qacqf_emul")
    ref.emul_qacqf.restype = _I
    ref.emul_qacqf.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 7 + [_I, _F] + [_I] * 6 + [DP, DP, DP, IP]
    return lib, ref


def pending_problem(B, q, p, D, n, kind, seed):
    """``Problem`` at q + p points per batch, the last p of every batch replaced by batch 0's: the pending set."""
    prob = Problem(B, q + p, D, n, kind, seed)
    prob.X[:, q:] = prob.X[0, q:].clone()
    return prob


def pending_inputs(prob, q, p):
    """What (7q) takes, by autograd of the prior alone: the value path over the B q moving points, the GRAD-layout sums with the
    pending points as leading points (rows n + k) in front of the mates (rows n + p + r), and the pending set's own pieces."""
    n, D, B, s = prob.n, prob.D, prob.B, prob.s
    Mq = B * q
    Xm, Xp = prob.X[:, :q].reshape(Mq, D).contiguous(), prob.X[0, q:].contiguous()
    Knn, alpha = prob.train()
    Knq = prob.cov_s(prob.Xt, Xm) / s ** 2 + R.kernel(prob.Xt, Xm, prob.theta, prob.kind)
    Z = torch.linalg.solve(Knn, Knq)
    mean_q = (prob.mean_s(Xm) - prob.m) / s
    var_q = torch.diagonal(prob.cov_s(Xm, Xm)) / s ** 2 + prob.theta[D]
    X = Xm.clone().requires_grad_(True)
    mates = Xm.reshape(B, 1, q, D).expand(B, q, q, D).reshape(Mq, q, D)
    rows = n + p + q
    anchors = torch.cat([prob.Xt.unsqueeze(0).expand(Mq, n, D), Xp.unsqueeze(0).expand(Mq, p, D), mates], 1).detach()   # (Mq, rows, D)
    cov = prob.cov_s(anchors, X.unsqueeze(1))[:, :, 0]
    eye = torch.eye(rows, dtype=torch.float64).unsqueeze(1).expand(rows, Mq, rows)
    (dcov,) = torch.autograd.grad(cov, X, eye, is_grads_batched=True)
    mean = prob.mean_s(X)
    (dmean,) = torch.autograd.grad(mean.sum(), X)
    var = prob.cov_s(X.unsqueeze(1), X.unsqueeze(1))[:, 0, 0]
    (dvar,) = torch.autograd.grad(var.sum(), X)
    cov_g, mu_g, var_g = torch.zeros(rows, Mq, 16, dtype=torch.float64), torch.zeros(Mq, 16, dtype=torch.float64), torch.zeros(Mq, 16, dtype=torch.float64)
    cov_g[:, :, 0], cov_g[:, :, 1:1 + D] = cov.detach().T, dcov
    mu_g[:, 0], mu_g[:, 1:1 + D] = mean.detach(), dmean
    var_g[:, 0], var_g[:, 1:1 + D] = var.detach(), dvar
    out = dict(Knq=Knq, Z=Z, alpha=alpha, mean_q=mean_q, var_q=var_q, cov_g=cov_g.reshape(rows, Mq * 16), mu_g=mu_g.reshape(-1),
               var_g=var_g.reshape(-1), Xt=prob.Xt, Xq=Xm, theta=prob.theta, Xp=Xp)
    if p > 0:
        Knp = prob.cov_s(prob.Xt, Xp) / s ** 2 + R.kernel(prob.Xt, Xp, prob.theta, prob.kind)
        mu_p, Sigma_pp = prob.joint(Xp)
        out.update(Zp=torch.linalg.solve(Knn, Knp), mu_p=mu_p, Sigma_pp=Sigma_pp)
    return out


def run_pending(lib, inp, prob, q, p, eps, acqf, par, info=None):
    a = {k: np.ascontiguousarray(v.detach().numpy(), dtype=np.float64) for k, v in inp.items()}
    B, D, n = prob.B, prob.D, prob.n
    value, grad, jit = np.full(B, 7.0), np.full((B * q, D), 7.0), np.full(B, 7.0)
    info_out = np.full(B, 7, dtype=np.int32)
    e = np.ascontiguousarray(eps.numpy())
    pend = [_p(a[k]) if p > 0 else None for k in ("Xp", "Zp", "mu_p", "Sigma_pp")]
    rc = lib.emul_qacqf_pending(_p(a["Knq"]), _p(a["Z"]), _p(a["alpha"]), _p(a["mean_q"]), _p(a["var_q"]), prob.m, prob.s,
                                _p(info) if info is not None else None, _p(a["cov_g"]), _p(a["mu_g"]), _p(a["var_g"]), _p(a["Xt"]),
                                _p(a["Xq"]), _p(a["theta"]), _p(e), *pend, acqf, par, n, B * q, q, p, eps.shape[0], D, prob.kind,
                                _p(value), _p(grad), _p(jit), _p(info_out))
    assert rc == 0
    return torch.from_numpy(value), torch.from_numpy(grad).reshape(B, q, D), torch.from_numpy(jit), torch.from_numpy(info_out)


def acqf_param(prob, acqf):
    """qEI: best_f two standard deviations above the largest mean (nearly every sample improves); qUCB: beta = 4."""
    if acqf != R.ACQF_EI:
        return 4.0
    with torch.no_grad():
        js = [prob.joint(prob.X[b]) for b in range(prob.B)]
        return max(float(mu.max()) + 2.0 * math.sqrt(float(torch.diagonal(Sg).max())) for mu, Sg in js)


WORST = {"ratio": 0.0}


def _ratio(got, ref, what):
    """|got - ref| against 1e-9 max|ref|; the ratio is printed before it is asserted."""
    tol = 1e-9 * float(ref.abs().max())
    err = float((got - ref).abs().max())
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: err {err:.3e} tol {tol:.3e} ratio {ratio:.3g} (worst so far {WORST['ratio']:.3g})")
    assert ratio <= 1.0, what


#         B  q  p  D   n   S    kind     every (q, p), n, S, D and kind of the list is met; n = 88 with (3, 5): n + p + q = 96
CASES = [(2, 1, 1, 2, 1, 1, 0),
         (1, 1, 7, 15, 17, 512, 1),
         (2, 2, 3, 2, 17, 7, 1),
         (2, 2, 3, 15, 17, 300, 0),
         (2, 4, 4, 15, 1, 300, 0),
         (2, 4, 4, 2, 17, 512, 1),
         (2, 7, 1, 2, 17, 300, 1),
         (2, 7, 1, 15, 1, 7, 0),
         (1, 3, 5, 15, 88, 512, 0)]
# the seeds are picked where the reference itself is well posed: the first candidate of this case has cond(Sigma) = 2e4 under qUCB
RESEED = {((2, 7, 1, 2, 17, 300, 1), R.ACQF_UCB): 1000}


def _seed(case, acqf):
    B, q, p, D, n, S, kind = case
    return 11 * (q + p) + n + acqf + 100 * q + RESEED.get((case, acqf), 0)


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
@pytest.mark.parametrize("B,q,p,D,n,S,kind", CASES)
def test_pending_against_the_concatenated_route_and_autograd(emul, B, q, p, D, n, S, kind, acqf):
    lib, ref = emul
    prob = pending_problem(B, q, p, D, n, kind, seed=_seed((B, q, p, D, n, S, kind), acqf))
    eps = torch.randn(S, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(q + p + S))
    cat = prob.kernel_inputs()
    assert cat["cond_Knn"] <= R.COND_MAX
    par = acqf_param(prob, acqf)
    # (b) torch autograd of the definition at q + p points (asserts both conditions on every batch); the pending rows are dropped
    v_ad, g_ad = batch_reference(prob, eps, acqf, par)
    assert float(g_ad[:, :q].abs().max()) > 0
    # (a) (7p)'s host build over the concatenated batches
    v_cat, g_cat, jit_cat, info_cat = run_batch(ref, cat, prob, eps, acqf, par)
    assert not info_cat.any() and not jit_cat.any()
    v, g, jit, info = run_pending(lib, pending_inputs(prob, q, p), prob, q, p, eps, acqf, par)
    assert not info.any() and not jit.any()
    tag = f"B={B} q={q} p={p} D={D} n={n} S={S} kind={kind} acqf={acqf}"
    _ratio(v, v_cat, tag + " value / concatenated")
    _ratio(g, g_cat[:, :q], tag + " grad / concatenated")
    _ratio(v, v_ad, tag + " value / autograd")
    _ratio(g, g_ad[:, :q], tag + " grad / autograd")


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
def test_the_pending_terms_are_live(emul, acqf):
    """Not vacuous: in the reference of this case pending entries win some samples and moving entries others, and the moving points'
    gradient differs from the one WITHOUT the pending points by more than 1e-2 max|ref| -- a kernel that ignored the pending columns of
    Sbar, Zp or the mixed dP could not agree with the reference.  The kernel is then held to that reference."""
    lib, _ = emul
    B, q, p, D, n, S, kind = 2, 2, 3, 15, 17, 300, 0
    prob = pending_problem(B, q, p, D, n, kind, seed=_seed((B, q, p, D, n, S, kind), acqf))
    eps = torch.randn(S, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(q + p + S))
    par = acqf_param(prob, acqf)
    pend_wins = mov_wins = 0
    for b in range(B):
        with torch.no_grad():
            mu, Sigma = prob.joint(prob.X[b])
        u, g, _ = R.utilities(mu, Sigma, eps, acqf, par)
        j = (g if acqf == R.ACQF_EI else u).argmax(-1)   # (qEI: the entries that compete are best_f - f_j before the clamp)
        pend_wins, mov_wins = pend_wins + int((j >= q).sum()), mov_wins + int((j < q).sum())
    print(f"acqf={acqf}: a pending entry wins {pend_wins} samples, a moving one {mov_wins}")
    assert pend_wins > 0 and mov_wins > 0
    v_ref, g_ref = batch_reference(prob, eps, acqf, par)
    free = Problem(B, q, D, n, kind, seed=0)   # the same prior and training set, the moving points alone
    for k in ("A", "b", "c", "l", "Xt", "y", "m", "s", "theta"):
        setattr(free, k, getattr(prob, k))
    free.X = prob.X[:, :q].clone()
    _, g_free = batch_reference(free, eps[:, :q].contiguous(), acqf, par)
    diff = float((g_ref[:, :q] - g_free).abs().max()) / float(g_ref[:, :q].abs().max())
    print(f"acqf={acqf}: gradient with / without the pending points differs by {diff:.3g} of max|ref|")
    assert diff > 1e-2
    v, g, _, _ = run_pending(lib, pending_inputs(prob, q, p), prob, q, p, eps, acqf, par)
    _ratio(v, v_ref, f"live acqf={acqf} value")
    _ratio(g, g_ref[:, :q], f"live acqf={acqf} grad")


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
@pytest.mark.parametrize("B,q,D,n,S,kind", [(2, 3, 2, 5, 7, 0), (1, 1, 2, 1, 1, 1), (2, 2, 3, 17, 300, 1), (1, 8, 15, 88, 512, 0)])
def test_without_pending_points_the_bits_are_those_of_7p(emul, B, q, D, n, S, kind, acqf):
    lib, ref = emul
    prob = Problem(B, q, D, n, kind, seed=11 * q + n + acqf)
    eps = torch.randn(S, q, dtype=torch.float64, generator=torch.Generator().manual_seed(q + S))
    inp = prob.kernel_inputs()
    par = acqf_param(prob, acqf)
    want = run_batch(ref, inp, prob, eps, acqf, par)
    inp = {k: v for k, v in inp.items() if isinstance(v, torch.Tensor)}
    inp["Xp"] = torch.empty(0, D, dtype=torch.float64)
    got = run_pending(lib, inp, prob, q, 0, eps, acqf, par)
    for a, b in zip(got, want):
        assert np.array_equal(a.numpy(), b.numpy())
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


def test_nan_rules_and_failures(emul):
    lib, _ = emul
    B, q, p = 3, 2, 2
    prob = pending_problem(B, q, p, 2, 5, 0, seed=2)
    eps = torch.randn(16, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    inp = pending_inputs(prob, q, p)
    v0, g0, jit0, info0 = run_pending(lib, inp, prob, q, p, eps, R.ACQF_EI, 0.5)
    assert bool(torch.isfinite(v0).all()) and bool(torch.isfinite(g0).all()) and not info0.any()
    # two calls: bit for bit
    again = run_pending(lib, inp, prob, q, p, eps, R.ACQF_EI, 0.5)
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(again, (v0, g0, jit0, info0)))
    # a failed target factorisation: everything is NaN
    v, g, jit, info = run_pending(lib, inp, prob, q, p, eps, R.ACQF_EI, 0.5, info=np.ones(1, dtype=np.int32))
    assert bool(torch.isnan(v).all()) and bool(torch.isnan(g).all()) and bool(torch.isnan(jit).all()) and bool((info == 1).all())
    # a NaN coordinate in a moving point of batch 1: that batch is NaN, the others are bit for bit what they were
    bad = dict(inp)
    bad["Xq"] = inp["Xq"].clone()
    bad["Xq"][1 * q + 1, 1] = NAN
    v, g, _, _ = run_pending(lib, bad, prob, q, p, eps, R.ACQF_EI, 0.5)
    assert math.isnan(float(v[1])) and bool(torch.isnan(g[1]).all())
    for b in (0, 2):
        assert float(v[b]) == float(v0[b]) and torch.equal(g[b], g0[b])
    # a NaN anywhere in the pending set's arrays: every batch is NaN (Sigma_pp: an entry of the upper triangle, which is not read)
    for name, idx in (("Xp", (1, 0)), ("Zp", (4, 1)), ("mu_p", (0,)), ("Sigma_pp", (0, 1))):
        bad = dict(inp)
        bad[name] = inp[name].detach().clone()
        bad[name][idx] = NAN
        v, g, _, _ = run_pending(lib, bad, prob, q, p, eps, R.ACQF_UCB, 4.0)
        assert bool(torch.isnan(v).all()) and bool(torch.isnan(g).all()), name


def test_plan_and_footprint(emul):
    lib, _ = emul
    out = (ctypes.c_longlong * 3)()
    for n, q, p in ((88, 3, 5), (88, 1, 7), (88, 7, 1), (88, 8, 0), (95, 1, 0)):   # n + p + q = 96, q + p <= 8
        lib.emul_qacqf_pending_plan(5, n, q, p, 512, out)
        assert (out[0], out[1]) == (5, 256)
        assert out[2] == lib.emul_qacqf_pending_lds_doubles(n, q, p, 512) and out[2] * 8 <= 160 * 1024   # the largest shapes fit the LDS
