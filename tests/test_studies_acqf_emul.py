"""CPU checks of the batched target acquisition's ARITHMETIC (csrc/gp_studies_acqf.h: sa_query, the body of
scaml_target_acqf_batched_kernel) through a host build of the same source (tests/host_emul/studies_acqf_emul.cpp) against a torch-fp64
restatement written here: weighted sums over the active tasks -> Knq -> torch.linalg.cholesky solves -> posterior -> UCB / EI ->
torch.autograd for the input gradient.  The source-pass outputs are smooth synthetic functions of the query point with their analytic
derivatives in columns 1 .. D, so autograd through the restatement differentiates the same functions.  G = 3 groups of ragged size
(1, 17, 96), one task pruned in one group only, one padding query, one query whose variance is forced below zero (UCB: clamped at 0,
EI: on the 1e-9 floor; the slope of the clamped term is zero), everything past a group's n_g filled with NaN.  Tolerances: those of
tests/test_target_fit_emul.py against autograd (value rtol 1e-9; gradient rtol 1e-6, atol 1e-9).  The parallel execution is what
tests/test_studies_acqf_gpu.py covers."""
import ctypes
import math

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests._host_emul import BP, DP, IP, build, ptr as _p

NS, T = (1, 17, 96), 3
COUNTS = (2, 3, 2)      # queries per group; then one padding row
LOW_VAR_Q = 3           # a query of group 1 whose source variance is pushed far below zero


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "studies_acqf_emul")
    lib.emul_studies_acqf.restype = ctypes.c_int
    lib.emul_studies_acqf.argtypes = [DP, DP, DP, IP, DP, DP, BP, DP, DP, DP, DP, DP, IP, DP, DP, IP, DP] + [ctypes.c_int] * 7 + [DP] * 4
    return lib


def _kernel(x1, x2, theta, kind):
    """os k((x1 - x2) / l), (n1, n2): gpytorch's RBF / Matern-5/2 (squared distance clamped at 1e-30 before the root)."""
    D = x1.shape[-1]
    d2 = (((x1.unsqueeze(-2) - x2.unsqueeze(-3)) / theta[:D]) ** 2).sum(-1)
    if kind == 0:
        return theta[D] * torch.exp(-0.5 * d2)
    r = torch.sqrt(d2.clamp_min(1e-30)) * math.sqrt(5.0)
    return theta[D] * (1.0 + r + r * r / 3.0) * torch.exp(-r)


class Problem:
    """Synthetic source-pass outputs mu_t(x), var_t(x), cov_{t,a}(x) (smooth in x) and G studies on top of them."""

    def __init__(self, D, kind, seed):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)   # noqa: E731
        self.D, self.kind, self.G, self.n_max = D, kind, len(NS), max(NS)
        self.A, self.b, self.C = rnd(T, D) * 2 - 1, rnd(T), rnd(T, D)
        self.Xt = [rnd(n, D) for n in NS]
        self.theta = [torch.cat([0.4 + rnd(D), 0.5 + rnd(1), 1e-2 + 0.1 * rnd(1)]) for _ in NS]
        self.w = [0.2 + rnd(T) for _ in NS]
        self.active = [torch.ones(T, dtype=torch.bool) for _ in NS]
        self.active[1][2] = False          # one task pruned in one group only
        self.w[1][2] = 0.0
        self.m = [float(rnd(1)) - 0.5 for _ in NS]
        self.s = [0.7 + float(rnd(1)) for _ in NS]
        self.param = {0: [4.0 + 5.0 * float(rnd(1)) for _ in NS], 1: [float(rnd(1)) - 0.3 for _ in NS]}   # beta / best_f
        self.Xq = rnd(sum(COUNTS) + 1, D)
        self.group = np.array([s for s, c in enumerate(COUNTS) for _ in range(c)] + [-1], dtype=np.int32)
        self.off = torch.zeros(self.Xq.shape[0], dtype=torch.float64)
        self.off[LOW_VAR_Q] = -1e3
        # the studies' training blocks: Knn (SPD), its factor and alpha = Knn^-1 resid
        self.Lc, self.alpha = [], []
        for s_, n in enumerate(NS):
            Knn = sum((self.w[s_][t] ** 2) * self.cov_fn(t, s_, self.Xt[s_]) for t in range(T) if self.active[s_][t]) / self.s[s_] ** 2
            Knn = 0.5 * (Knn + Knn.T) + _kernel(self.Xt[s_], self.Xt[s_], self.theta[s_], kind) + self.theta[s_][-1] * torch.eye(n, dtype=torch.float64)
            Lc = torch.linalg.cholesky(Knn)
            self.Lc.append(Lc)
            self.alpha.append(torch.cholesky_solve((rnd(n, 1) - 0.5), Lc).squeeze(-1))

    # the source pass as functions of the query points x (M, D)
    def mu_fn(self, t, x):
        return 2.0 * torch.sin(x @ self.A[t] + self.b[t]) + 0.3 * t

    def var_fn(self, t, x):
        return 2.0 + torch.cos(x @ self.C[t])

    def cov_fn(self, t, s_, x):
        """(n_s, M): Cov(f_t(Xt_s[a]), f_t(x))"""
        d2 = ((self.Xt[s_].unsqueeze(1) - x.unsqueeze(0)) ** 2).sum(-1)
        return 0.3 * (1.0 + 0.1 * t) * torch.exp(-0.5 * d2)

    def arrays(self, acqf, info=(0, 0, 0)):
        """The inputs of (7g): values in column 0, analytic derivatives in columns 1 .. D, zeros behind; NaN past every n_g."""
        D, G, n_max, Mq = self.D, self.G, self.n_max, self.Xq.shape[0]
        nan = float("nan")
        mu, var = np.zeros((T, Mq, 16)), np.zeros((T, Mq, 16))
        cov = np.full((T, n_max, Mq, 16), nan)
        X = self.Xq
        for t in range(T):
            mu[t, :, 0] = self.mu_fn(t, X).numpy()
            mu[t, :, 1:1 + D] = (2.0 * torch.cos(X @ self.A[t] + self.b[t]).unsqueeze(-1) * self.A[t]).numpy()
            var[t, :, 0] = (self.var_fn(t, X) + self.off).numpy()
            var[t, :, 1:1 + D] = (-torch.sin(X @ self.C[t]).unsqueeze(-1) * self.C[t]).numpy()
            for q in range(Mq):
                s_ = int(self.group[q])
                if s_ < 0:
                    continue
                n = NS[s_]
                c = self.cov_fn(t, s_, X[q:q + 1]).squeeze(-1)                       # (n,)
                cov[t, :n, q, :] = 0.0
                cov[t, :n, q, 0] = c.numpy()
                cov[t, :n, q, 1:1 + D] = (-(X[q] - self.Xt[s_]) * c.unsqueeze(-1)).numpy()
        nbm = (n_max + 15) // 16
        Xt, theta = np.full((G, n_max, D), nan), np.zeros((G, D + 2))
        L, W, alpha = np.full((G, n_max, n_max), nan), np.full((G, nbm, 16, 16), nan), np.full((G, n_max), nan)
        for s_, n in enumerate(NS):
            Xt[s_, :n], theta[s_] = self.Xt[s_].numpy(), self.theta[s_].numpy()
            L[s_, :n, :n], alpha[s_, :n] = self.Lc[s_].numpy(), self.alpha[s_].numpy()
            for kb in range((n + 15) // 16):
                c = min(16, n - 16 * kb)
                W[s_, kb, :c, :c] = torch.linalg.inv(self.Lc[s_][16 * kb:16 * kb + c, 16 * kb:16 * kb + c]).numpy()
        return dict(mu=mu, var=var, cov=np.ascontiguousarray(cov.reshape(T, n_max, Mq * 16)), group=self.group, Xq=X.numpy().copy(),
                    w=torch.stack(self.w).numpy().copy(), active=torch.stack(self.active).numpy().astype(np.uint8), Xt=Xt, theta=theta, L=L,
                    Linv_diag=W, alpha=alpha, n_points=np.array(NS, dtype=np.int32), m_all=np.array(self.m), s_all=np.array(self.s),
                    info=np.array(info, dtype=np.int32), acqf_param=np.array(self.param[acqf]))

    def reference(self, acqf, q):
        """(value, grad (D,), mu*, var*) of query q from the restated formulas, the gradient by autograd."""
        s_ = int(self.group[q])
        x = self.Xq[q:q + 1].clone().requires_grad_(True)
        act = [t for t in range(T) if self.active[s_][t]]
        w, m, s, th = self.w[s_], self.m[s_], self.s[s_], self.theta[s_]
        mu_s = sum(w[t] * self.mu_fn(t, x) for t in act).squeeze(0)
        var_s = sum(w[t] ** 2 * (self.var_fn(t, x) + self.off[q]) for t in act).squeeze(0)
        cov_s = sum(w[t] ** 2 * self.cov_fn(t, s_, x) for t in act).squeeze(-1)
        Knq = cov_s / s ** 2 + _kernel(self.Xt[s_], x, th, self.kind).squeeze(-1)
        z = torch.cholesky_solve(Knq.unsqueeze(-1), self.Lc[s_]).squeeze(-1)
        mu = m + s * ((mu_s - m) / s + Knq @ self.alpha[s_])
        var = s ** 2 * (var_s / s ** 2 + th[-2] - Knq @ z)
        par = self.param[acqf][s_]
        if acqf == 0:   # utils.UpperConfidenceBound: -mu + sqrt(beta max(var, 0)), zero slope where the variance is clamped
            val = -mu + torch.where(var > 0, torch.sqrt(par * torch.where(var > 0, var, torch.ones_like(var))), torch.zeros_like(var))
        else:           # utils.ExpectedImprovement: the 1e-9 floor under the root
            sigma = var.clamp_min(1e-9).sqrt()
            u = -(mu - par) / sigma
            val = sigma * (torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi) + u * 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))))
        (g,) = torch.autograd.grad(val, x)
        return float(val.detach()), g.squeeze(0).numpy(), float(mu.detach()), float(var.detach())


def _run(lib, prob, acqf, info=(0, 0, 0), edit=None):
    a = prob.arrays(acqf, info)
    if edit is not None:
        edit(a)
    Mq, D = a["Xq"].shape
    out = dict(value=np.full(Mq, 7.0), grad=np.full((Mq, D), 7.0), mu=np.full(Mq, 7.0), var=np.full(Mq, 7.0))
    order = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha", "n_points", "m_all", "s_all", "info",
             "acqf_param")
    rc = lib.emul_studies_acqf(*[_p(a[k]) for k in order], Mq, prob.G, prob.n_max, T, D, prob.kind, acqf, _p(out["value"]), _p(out["grad"]),
                               _p(out["mu"]), _p(out["var"]))
    assert rc == 0
    return out


@pytest.mark.parametrize("D", [2, 15])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("acqf", [0, 1])
def test_value_and_gradient_match_the_torch_restatement(emul, D, kind, acqf):
    prob = Problem(D, kind, seed=100 + D + kind)
    out = _run(emul, prob, acqf)
    Mq = prob.Xq.shape[0]
    for q in range(Mq - 1):
        val, g, mu, var = prob.reference(acqf, q)
        np.testing.assert_allclose(out["value"][q], val, rtol=1e-9, err_msg=f"value q={q}")
        np.testing.assert_allclose(out["mu"][q], mu, rtol=1e-9)
        np.testing.assert_allclose(out["var"][q], var, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(out["grad"][q], g, rtol=1e-6, atol=1e-9, err_msg=f"gradient q={q}")
    # the clamped query: variance below zero, so UCB is -mu with gradient -dmu, EI sits on the floor with no variance slope
    assert out["var"][LOW_VAR_Q] < 0
    # the padding row
    assert out["value"][-1] == 0.0 and not out["grad"][-1].any() and out["mu"][-1] == 0.0 and out["var"][-1] == 0.0


def test_a_failed_factorisation_is_nan_for_that_group_only(emul):
    prob = Problem(2, 1, seed=5)
    good, bad = _run(emul, prob, 0), _run(emul, prob, 0, info=(0, 3, 0))
    g = prob.group
    for k in ("value", "grad", "mu", "var"):
        assert np.isnan(bad[k][g == 1]).all(), k
        for s_ in (0, 2):
            assert np.array_equal(bad[k][g == s_], good[k][g == s_]), (k, s_)   # bit for bit
        assert np.array_equal(bad[k][g < 0], good[k][g < 0])


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("acqf", [0, 1])
def test_a_non_finite_query_coordinate_is_nan_in_all_its_outputs(emul, kind, acqf):
    """include/scaml_gp.h (7g): one NaN coordinate in a query point whose source-pass columns are all finite (the Matern branch's fmax
    drops the NaN: without the rule only that coordinate's gradient entry showed it, value / mu / var were those of a point at
    distance ~0 from every training point) -- NaN in its value, every entry of its gradient, mu and var; the other queries bit for bit."""
    prob = Problem(6, kind, seed=11)
    q = LOW_VAR_Q + 1          # the last query of group 1 (n = 17)

    def poison(a):
        a["Xq"][q, 2] = float("nan")

    good, bad = _run(emul, prob, acqf), _run(emul, prob, acqf, edit=poison)
    others = np.arange(prob.Xq.shape[0]) != q
    for k in ("value", "grad", "mu", "var"):
        assert np.isnan(bad[k][q]).all(), (k, bad[k][q])
        assert np.array_equal(bad[k][others], good[k][others]), k   # bit for bit


def test_lds_footprint_holds_the_carve(emul):
    emul.emul_studies_acqf_lds_doubles.restype, emul.emul_studies_acqf_lds_doubles.argtypes = ctypes.c_longlong, [ctypes.c_int]
    for n in range(1, 97):
        nb = (n + 15) // 16
        assert emul.emul_studies_acqf_lds_doubles(n) == n * 16 + 32 + 3 * 16 * nb + 256 * nb + n * (n | 1) + 48
    assert emul.emul_studies_acqf_lds_doubles(96) * 8 <= 160 * 1024
