"""CPU checks of the ARITHMETIC of the joint q-point acquisition kernel (csrc/gp_qacqf.h: qa_tail and qa_batch, the body of
csrc/gp_qacqf.hip, include/scaml_gp.h (7p)) through a host build of the same source (tests/host_emul/qacqf_emul.cpp) against torch
fp64 autograd of the definitions (tests/_qacqf_ref.py: torch.linalg.cholesky, the samples, the two utilities).

The tail (everything from "Sigma, mu given" onwards: the jitter ladder, the sampling, qEI / qUCB and the adjoint up to mubar and
Sigmabar) for q in {1, 2, 3, 8} x S in {1, 7, 300, 512} x both codes.  The inputs are seeded so that the reference itself satisfies
cond(Sigma) <= 1e4 and keeps every sample 1e-6 sqrt(max Sigma_jj) away from a tie of its two best entries and from the kinks; both
are asserted on the reference, no sample is left out.  Tolerance: 1e-9 max|ref| per array -- the estimate q^2 u cond is 7e-11 at
q = 8, cond = 1e4, u = 1.1e-16, a margin of about 14.  (Measured worst ratio error / tolerance: profiles/qacqf_notes.md.)

The whole batch (qa_batch: the joint posterior from the value path and the joint GRAD pass's sums, the tail, the input gradient)
against autograd through a synthetic source prior with analytic covariance; cond(Knn) <= 1e4 is asserted too, same tolerance."""
import ctypes
import math

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests import _qacqf_ref as R
from tests._host_emul import DP, IP, build, ptr as _p

NAN = float("nan")
_I, _F = ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "qacqf_emul")
    lib.emul_qacqf_tail.restype = _I
    lib.emul_qacqf_tail.argtypes = [DP, DP, DP, _I, _I, _I, _F, DP, DP, DP, DP, IP]
    lib.emul_qacqf.restype = _I
    lib.emul_qacqf.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 7 + [_I, _F] + [_I] * 6 + [DP, DP, DP, IP]
    lib.emul_qacqf_lds_doubles.restype, lib.emul_qacqf_lds_doubles.argtypes = ctypes.c_longlong, [_I] * 3
    lib.emul_qacqf_plan.restype, lib.emul_qacqf_plan.argtypes = None, [_I] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    return lib


def run_tail(emul, mu, Sigma, eps, acqf, par):
    q, S = mu.numel(), eps.shape[0]
    Sg, m, e = (np.ascontiguousarray(t.numpy(), dtype=np.float64) for t in (Sigma, mu, eps))
    value, jit = np.full(1, 7.0), np.full(1, 7.0)
    mubar, Sbar = np.full(q, 7.0), np.full((q, q), 7.0)
    info = np.full(1, 7, dtype=np.int32)
    assert emul.emul_qacqf_tail(_p(Sg), _p(m), _p(e), q, S, acqf, par, _p(value), _p(mubar), _p(Sbar), _p(jit), _p(info)) == 0
    return float(value[0]), torch.from_numpy(mubar), torch.from_numpy(Sbar), float(jit[0]), int(info[0])


def tail_inputs(q, S, acqf, seed, bulk=False):
    """mu, Sigma with eigenvalues log-spaced over [0.05, 5] (cond 100) under a random rotation, eps, and the acquisition parameter:
    best_f two standard deviations above the largest mean (nearly every sample improves) or, with ``bulk``, at the smallest mean, in the
    bulk of the posterior (a good part of the samples sits on qEI's clamp); beta = 4."""
    g = torch.Generator().manual_seed(seed)
    Qm, _ = torch.linalg.qr(torch.randn(q, q, dtype=torch.float64, generator=g))
    ev = torch.logspace(math.log10(0.05), math.log10(5.0), q, dtype=torch.float64) if q > 1 else torch.tensor([0.7], dtype=torch.float64)
    Sigma = (Qm * ev) @ Qm.T
    Sigma = 0.5 * (Sigma + Sigma.T)
    mu = torch.randn(q, dtype=torch.float64, generator=g)
    eps = torch.randn(S, q, dtype=torch.float64, generator=g)
    par = float(mu.max()) + 2.0 * math.sqrt(float(torch.diagonal(Sigma).max())) if acqf == R.ACQF_EI else 4.0
    if bulk and acqf == R.ACQF_EI:
        par = float(mu.min())
    return mu, Sigma, eps, par


WORST = {"ratio": 0.0}


def _ratio(got, ref, what):
    """|got - ref| against 1e-9 max|ref|; the ratio is printed before it is asserted."""
    tol = 1e-9 * float(ref.abs().max())
    err = float((got - ref).abs().max())
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: err {err:.3e} tol {tol:.3e} ratio {ratio:.3g} (worst so far {WORST['ratio']:.3g})")
    assert ratio <= 1.0, what


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
@pytest.mark.parametrize("S", [1, 7, 300, 512])
@pytest.mark.parametrize("q", [1, 2, 3, 8])
def test_tail_against_autograd(emul, q, S, acqf):
    mu, Sigma, eps, par = tail_inputs(q, S, acqf, seed=1000 * q + S + acqf)
    R.assert_well_posed(mu, Sigma, eps, acqf, par)
    v_ref, gm_ref, gs_ref = R.tail_reference(mu, Sigma, eps, acqf, par)
    v, mubar, Sbar, jit, info = run_tail(emul, mu, Sigma, eps, acqf, par)
    assert info == 0 and jit == 0.0
    assert float(gm_ref.abs().max()) > 0 and float(v_ref.abs()) > 0   # (nothing vacuous: the gradient is live)
    tag = f"q={q} S={S} acqf={acqf}"
    _ratio(torch.tensor([v], dtype=torch.float64), v_ref.reshape(1), tag + " value")
    _ratio(mubar, gm_ref, tag + " mubar")
    _ratio(Sbar, gs_ref, tag + " Sigmabar")
    torch.testing.assert_close(Sbar, Sbar.T, rtol=0, atol=0)


@pytest.mark.parametrize("q,S", [(1, 300), (2, 7), (3, 300), (8, 512)])
def test_tail_with_the_incumbent_in_the_bulk(emul, q, S):
    """qEI with best_f inside the posterior: samples without improvement take the clamped branch (a = 0, no weight on mubar or Cbar)
    next to samples that improve.  Same conditions on the reference, same tolerance."""
    mu, Sigma, eps, par = tail_inputs(q, S, R.ACQF_EI, seed=7000 + 10 * q + S, bulk=True)
    R.assert_well_posed(mu, Sigma, eps, R.ACQF_EI, par)
    u, _, _ = R.utilities(mu, Sigma, eps, R.ACQF_EI, par)
    clamped = int((u.max(-1).values == 0).sum())
    assert 0 < clamped < S, "both branches of the clamp are taken"
    v_ref, gm_ref, gs_ref = R.tail_reference(mu, Sigma, eps, R.ACQF_EI, par)
    v, mubar, Sbar, jit, info = run_tail(emul, mu, Sigma, eps, R.ACQF_EI, par)
    assert info == 0 and jit == 0.0
    tag = f"bulk q={q} S={S} ({clamped} of {S} clamped)"
    _ratio(torch.tensor([v], dtype=torch.float64), v_ref.reshape(1), tag + " value")
    _ratio(mubar, gm_ref, tag + " mubar")
    _ratio(Sbar, gs_ref, tag + " Sigmabar")


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
def test_q1_is_the_closed_form(emul, acqf):
    """q = 1: the factor is sigma and the value is mean_s A(mu + sigma eps_s)."""
    mu, Sigma, eps, par = tail_inputs(1, 300, acqf, seed=5)
    sigma = math.sqrt(float(Sigma))
    f = float(mu) + sigma * eps[:, 0]
    a = (par - f).clamp_min(0.0) if acqf == R.ACQF_EI else math.sqrt(par * math.pi / 2) * (sigma * eps[:, 0]).abs() - float(mu)
    v, _, _, jit, info = run_tail(emul, mu, Sigma, eps, acqf, par)
    assert info == 0 and jit == 0.0
    assert v == pytest.approx(float(a.mean()), rel=1e-13)


def test_ladder_on_exactly_representable_matrices(emul):
    eps = torch.randn(64, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    mu = torch.tensor([0.25, -0.5], dtype=torch.float64)
    par = 1.0
    # singular: the second pivot is 1 - 1 = 0 without jitter; 1e-8 is the first rung that passes
    Sigma = torch.ones(2, 2, dtype=torch.float64)
    v, mubar, Sbar, jit, info = run_tail(emul, mu, Sigma, eps, R.ACQF_EI, par)
    assert info == 0 and jit == 1e-8
    v_ref, gm_ref, gs_ref = R.tail_reference(mu, Sigma, eps, R.ACQF_EI, par, jitter=1e-8)
    # cond(Sigma + 1e-8 I) = 2e8: the estimate q^2 u cond is 9e-8; with the margin of 14 that the well-conditioned cases have, 1.3e-6
    tol = 14 * 4 * 1.1e-16 * 2e8
    assert abs(v - float(v_ref)) <= tol * abs(float(v_ref))
    assert float((mubar - gm_ref).abs().max()) <= tol * float(gm_ref.abs().max())
    assert float((Sbar - gs_ref).abs().max()) <= tol * float(gs_ref.abs().max())
    # indefinite: the second pivot is 1 + j - 4 / (1 + j) < 0 on every rung
    v, mubar, Sbar, jit, info = run_tail(emul, mu, torch.tensor([[1.0, 2.0], [2.0, 1.0]], dtype=torch.float64), eps, R.ACQF_EI, par)
    assert info == 1 and math.isnan(v) and bool(torch.isnan(mubar).all()) and bool(torch.isnan(Sbar).all())
    # a NaN entry
    for bad in (torch.tensor([[NAN, 0.0], [0.0, 1.0]]), torch.tensor([[1.0, NAN], [NAN, 1.0]]), torch.tensor([[1.0, 0.0], [0.0, NAN]])):
        v, mubar, Sbar, jit, info = run_tail(emul, mu, bad.double(), eps, R.ACQF_UCB, 4.0)
        assert math.isnan(v) and bool(torch.isnan(mubar).all()) and bool(torch.isnan(Sbar).all())
    # a NaN mean: the factor is fine, the value is NaN
    v, _, _, _, info = run_tail(emul, torch.tensor([NAN, 0.0], dtype=torch.float64), torch.eye(2, dtype=torch.float64), eps, R.ACQF_EI, par)
    assert info == 0 and math.isnan(v)


def test_plan_and_footprint(emul):
    out = (ctypes.c_longlong * 3)()
    emul.emul_qacqf_plan(5, 88, 8, 512, out)
    assert (out[0], out[1]) == (5, 256)
    assert out[2] == emul.emul_qacqf_lds_doubles(88, 8, 512) and out[2] * 8 <= 160 * 1024   # the largest shape fits the LDS


# ---- the whole batch against autograd through a synthetic source prior -------------------------------------------------------------
class Problem:
    """A target GP over a synthetic weighted source prior: mean_s(x) = 2 sin(x . A + b), cov_s(x, x') = c g(x) g(x') exp(-|x - x'|^2 /
    (2 l^2)) with g(x) = 1 + 0.3 sin(sum x) (original units), noise 3e-2 of the outputscale."""

    def __init__(self, B, q, D, n, kind, seed):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)   # noqa: E731
        self.B, self.q, self.D, self.n, self.kind = B, q, D, n, kind
        self.A, self.b = 2.0 * rnd(D) - 1.0, float(rnd(1))
        self.c, self.l = 0.6, 0.9 * math.sqrt(D)
        self.Xt, self.X = rnd(n, D), rnd(B, q, D)
        self.y = torch.randn(n, dtype=torch.float64, generator=g)
        self.m, self.s = 0.3, 1.7
        self.theta = torch.cat([0.5 * math.sqrt(D) * (0.8 + 0.4 * rnd(D)), torch.tensor([1.3, 0.04], dtype=torch.float64)])

    def mean_s(self, x):
        return 2.0 * torch.sin(x @ self.A + self.b)

    def cov_s(self, xa, xb):
        ga, gb = 1.0 + 0.3 * torch.sin(xa.sum(-1)), 1.0 + 0.3 * torch.sin(xb.sum(-1))
        d2 = ((xa.unsqueeze(-2) - xb.unsqueeze(-3)) ** 2).sum(-1)
        return self.c * ga.unsqueeze(-1) * gb.unsqueeze(-2) * torch.exp(-0.5 * d2 / self.l ** 2)

    def train(self):
        n, s, th = self.n, self.s, self.theta
        Knn = self.cov_s(self.Xt, self.Xt) / s ** 2 + R.kernel(self.Xt, self.Xt, th, self.kind) + th[-1] * torch.eye(n, dtype=torch.float64)
        resid = self.y - (self.mean_s(self.Xt) - self.m) / s
        return Knn, torch.linalg.solve(Knn, resid)

    def joint(self, Xb):
        """mu (q,), Sigma (q, q) of one batch, differentiable in Xb."""
        s, th = self.s, self.theta
        Knn, alpha = self.train()
        Knq = self.cov_s(self.Xt, Xb) / s ** 2 + R.kernel(self.Xt, Xb, th, self.kind)
        P = self.cov_s(Xb, Xb) / s ** 2 + R.kernel(Xb, Xb, th, self.kind)
        mu = self.m + s * ((self.mean_s(Xb) - self.m) / s + Knq.T @ alpha)
        return mu, s ** 2 * (P - Knq.T @ torch.linalg.solve(Knn, Knq))

    def kernel_inputs(self):
        """What (7p) takes: the value path's outputs and the GRAD-layout sums, by autograd of the prior alone."""
        n, q, D, B, s = self.n, self.q, self.D, self.B, self.s
        Mq = B * q
        Xq = self.X.reshape(Mq, D)
        Knn, alpha = self.train()
        Knq = self.cov_s(self.Xt, Xq) / s ** 2 + R.kernel(self.Xt, Xq, self.theta, self.kind)
        Z = torch.linalg.solve(Knn, Knq)
        mean_q = (self.mean_s(Xq) - self.m) / s
        var_q = torch.diagonal(self.cov_s(Xq, Xq)) / s ** 2 + self.theta[D]
        # every GRAD-layout entry depends on its own query point alone: one batched backward per array gives all the derivatives
        X = Xq.clone().requires_grad_(True)
        mates = Xq.reshape(B, 1, q, D).expand(B, q, q, D).reshape(Mq, q, D)                       # point j's batch, mates held fixed
        anchors = torch.cat([self.Xt.unsqueeze(0).expand(Mq, n, D), mates], 1).detach()          # (Mq, n + q, D)
        cov = self.cov_s(anchors, X.unsqueeze(1))[:, :, 0]                                       # (Mq, n + q)
        eye = torch.eye(n + q, dtype=torch.float64).unsqueeze(1).expand(n + q, Mq, n + q)
        (dcov,) = torch.autograd.grad(cov, X, eye, is_grads_batched=True)                         # (n + q, Mq, D)
        mean = self.mean_s(X)
        (dmean,) = torch.autograd.grad(mean.sum(), X)
        var = self.cov_s(X.unsqueeze(1), X.unsqueeze(1))[:, 0, 0]
        (dvar,) = torch.autograd.grad(var.sum(), X)
        cov_g, mu_g, var_g = torch.zeros(n + q, Mq, 16, dtype=torch.float64), torch.zeros(Mq, 16, dtype=torch.float64), torch.zeros(Mq, 16, dtype=torch.float64)
        cov_g[:, :, 0], cov_g[:, :, 1:1 + D] = cov.detach().T, dcov
        mu_g[:, 0], mu_g[:, 1:1 + D] = mean.detach(), dmean
        var_g[:, 0], var_g[:, 1:1 + D] = var.detach(), dvar
        return dict(Knq=Knq, Z=Z, alpha=alpha, mean_q=mean_q, var_q=var_q, cov_g=cov_g.reshape(n + q, Mq * 16), mu_g=mu_g.reshape(-1),
                    var_g=var_g.reshape(-1), Xt=self.Xt, Xq=Xq, theta=self.theta, cond_Knn=float(torch.linalg.cond(Knn)))


def run_batch(emul, inp, prob, eps, acqf, par, info=None, want_grad=True):
    a = {k: np.ascontiguousarray(v.detach().numpy(), dtype=np.float64) for k, v in inp.items() if isinstance(v, torch.Tensor)}
    B, q, D, n = prob.B, prob.q, prob.D, prob.n
    value, grad, jit = np.full(B, 7.0), np.full((B * q, D), 7.0), np.full(B, 7.0)
    info_out = np.full(B, 7, dtype=np.int32)
    e = np.ascontiguousarray(eps.numpy())
    rc = emul.emul_qacqf(_p(a["Knq"]), _p(a["Z"]), _p(a["alpha"]), _p(a["mean_q"]), _p(a["var_q"]), prob.m, prob.s,
                         _p(info) if info is not None else None, _p(a["cov_g"]), _p(a["mu_g"]), _p(a["var_g"]), _p(a["Xt"]), _p(a["Xq"]),
                         _p(a["theta"]), _p(e), acqf, par, n, B * q, q, eps.shape[0], D, prob.kind, _p(value),
                         _p(grad) if want_grad else None, _p(jit), _p(info_out))
    assert rc == 0
    return torch.from_numpy(value), torch.from_numpy(grad).reshape(B, q, D), torch.from_numpy(jit), torch.from_numpy(info_out)


def batch_reference(prob, eps, acqf, par):
    X = prob.X.clone().requires_grad_(True)
    vals = []
    for b in range(prob.B):
        mu, Sigma = prob.joint(X[b])
        R.assert_well_posed(mu.detach(), Sigma.detach(), eps, acqf, par)
        vals.append(R.mc_value(mu, Sigma, eps, acqf, par))
    v = torch.stack(vals)
    (g,) = torch.autograd.grad(v.sum(), X)
    return v.detach(), g


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
@pytest.mark.parametrize("B,q,D,n,S,kind", [(2, 3, 2, 5, 7, 0), (1, 1, 2, 1, 1, 1), (2, 2, 3, 17, 300, 1), (1, 8, 15, 88, 512, 0), (2, 8, 6, 20, 64, 1)])
def test_batch_against_autograd(emul, B, q, D, n, S, kind, acqf):
    prob = Problem(B, q, D, n, kind, seed=11 * q + n + acqf)
    eps = torch.randn(S, q, dtype=torch.float64, generator=torch.Generator().manual_seed(q + S))
    inp = prob.kernel_inputs()
    assert inp["cond_Knn"] <= R.COND_MAX
    with torch.no_grad():   # best_f two standard deviations above the largest mean: nearly every sample improves
        js = [prob.joint(prob.X[b]) for b in range(B)]
        best_f = max(float(mu.max()) + 2.0 * math.sqrt(float(torch.diagonal(Sg).max())) for mu, Sg in js)
    par = best_f if acqf == R.ACQF_EI else 4.0
    v_ref, g_ref = batch_reference(prob, eps, acqf, par)
    assert float(g_ref.abs().max()) > 0
    v, g, jit, info = run_batch(emul, inp, prob, eps, acqf, par)
    assert not info.any() and not jit.any()
    tag = f"B={B} q={q} D={D} n={n} S={S} kind={kind} acqf={acqf}"
    _ratio(v, v_ref, tag + " value")
    _ratio(g, g_ref, tag + " grad")


def test_batch_failures_and_nan(emul):
    prob = Problem(3, 2, 2, 5, 0, seed=2)
    eps = torch.randn(16, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    inp = prob.kernel_inputs()
    v0, g0, _, _ = run_batch(emul, inp, prob, eps, R.ACQF_EI, 0.5)
    # a failed target factorisation: everything is NaN
    v, g, jit, info = run_batch(emul, inp, prob, eps, R.ACQF_EI, 0.5, info=np.ones(1, dtype=np.int32))
    assert bool(torch.isnan(v).all()) and bool(torch.isnan(g).all()) and bool(torch.isnan(jit).all()) and bool((info == 1).all())
    # a NaN coordinate in batch 1: that batch is NaN, the others are bit for bit what they were
    bad = dict(inp)
    bad["Xq"] = inp["Xq"].clone()
    bad["Xq"][3, 1] = NAN
    v, g, _, _ = run_batch(emul, bad, prob, eps, R.ACQF_EI, 0.5)
    assert math.isnan(float(v[1])) and bool(torch.isnan(g[1]).all())
    for b in (0, 2):
        assert float(v[b]) == float(v0[b]) and torch.equal(g[b], g0[b])
    # value only
    v, _, _, _ = run_batch(emul, inp, prob, eps, R.ACQF_EI, 0.5, want_grad=False)
    assert torch.equal(v, v0)
