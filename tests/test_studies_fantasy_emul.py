"""CPU checks of the ARITHMETIC of the batched target acquisition for studies with pending evaluations (csrc/gp_studies_acqf.h: sa_block
with the StudiesFantasyParams block, the bodies of the two kernels of csrc/gp_studies_fantasy.hip) through a host build of the same
source (tests/host_emul/studies_fantasy_emul.cpp) against a torch-fp64 restatement written here: that of
tests/test_studies_acqf_emul.py -- its synthetic source-pass outputs with analytic derivative columns, weighted sums over the active
tasks -> Knq -> torch.linalg.cholesky solves -> posterior -- with mean_f A(mu_f, v) over the group's fantasies and torch.autograd for
the input gradient.  Its tolerances: value rtol 1e-9; gradient rtol 1e-6, atol 1e-9.

One call holds groups of (n', F) = (1, 1), (2, 2), (16, 8), (17, 63), (96, 64), a group with info != 0, a group with F_g = 0, one task
pruned in one group only, one padding query, one query whose variance is forced below the clamp, one query with a NaN coordinate;
everything past a group's n_g / F_g is NaN.  The strip layout (R = 16) must give the query layout's values exactly; with F_g = 1
everywhere the outputs must equal, exactly, those of the existing host builds of sa_query and sa_score_strip."""
import ctypes
import math

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests._host_emul import BP, DP, IP, build, ptr as _p
from tests.test_studies_acqf_emul import Problem as _AcqfProblem, T, _kernel

#          (n', F)
GROUPS = ((1, 1), (2, 2), (16, 8), (17, 63), (96, 64), (5, 3), (4, 0))
INFO = (0, 0, 0, 0, 0, 2, 0)      # group 5: its factorisation failed
COUNTS = (2, 2, 3, 3, 2, 1, 1)    # queries per group; then one padding row
PRUNED_GROUP, PRUNED_TASK = 3, 2
LOW_VAR_Q = 8                     # a query of group 3 whose source variance is pushed far below zero
NAN_Q = 6                         # the last query of group 2 gets a NaN coordinate
F_MAX = 64
ORDER = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha_f", "n_fant", "n_points", "m_all", "s_all",
         "info", "acqf_param")
ORDER_ORDINARY = tuple("alpha" if k == "alpha_f" else k for k in ORDER if k != "n_fant")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "studies_fantasy_emul")
    lib.emul_studies_fantasy.restype = ctypes.c_int
    lib.emul_studies_fantasy.argtypes = ([ctypes.c_int] + [DP, DP, DP, IP, DP, DP, BP, DP, DP, DP, DP, DP, IP, IP, DP, DP, IP, DP] + [ctypes.c_int] * 8
                                         + [DP, DP])
    lib.emul_studies_fantasy_lds_doubles.restype, lib.emul_studies_fantasy_lds_doubles.argtypes = ctypes.c_longlong, [ctypes.c_int] * 3
    lib.emul_studies_fantasy_params_bytes.restype, lib.emul_studies_fantasy_params_bytes.argtypes = ctypes.c_longlong, [ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def ordinary(tmp_path_factory):
    """The existing host builds of sa_query (value + gradient) and sa_score_strip."""
    q = build(tmp_path_factory, "studies_acqf_emul")
    q.emul_studies_acqf.restype = ctypes.c_int
    q.emul_studies_acqf.argtypes = [DP, DP, DP, IP, DP, DP, BP, DP, DP, DP, DP, DP, IP, DP, DP, IP, DP] + [ctypes.c_int] * 7 + [DP] * 4
    s = build(tmp_path_factory, "studies_score_emul")
    s.emul_studies_score.restype = ctypes.c_int
    s.emul_studies_score.argtypes = [DP, DP, DP, IP, DP, DP, BP, DP, DP, DP, DP, DP, IP, DP, DP, IP, DP] + [ctypes.c_int] * 7 + [DP] * 3
    return q, s


class Problem(_AcqfProblem):
    """tests/test_studies_acqf_emul.py's synthetic source pass (mu_fn, var_fn, cov_fn) under G studies that are fantasy models."""

    def __init__(self, D, kind, seed, groups=GROUPS):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)   # noqa: E731
        self.groups = groups
        self.NS, self.FS = [n for n, _ in groups], [f for _, f in groups]
        self.D, self.kind, self.G, self.n_max = D, kind, len(groups), max(self.NS)
        self.A, self.b, self.C = rnd(T, D) * 2 - 1, rnd(T), rnd(T, D)
        self.Xt = [rnd(n, D) for n in self.NS]
        self.theta = [torch.cat([0.4 + rnd(D), 0.5 + rnd(1), 1e-2 + 0.1 * rnd(1)]) for _ in self.NS]
        self.w = [0.2 + rnd(T) for _ in self.NS]
        self.active = [torch.ones(T, dtype=torch.bool) for _ in self.NS]
        self.active[PRUNED_GROUP][PRUNED_TASK] = False   # one task pruned in one group only
        self.w[PRUNED_GROUP][PRUNED_TASK] = 0.0
        self.m = [float(rnd(1)) - 0.5 for _ in self.NS]
        self.s = [0.7 + float(rnd(1)) for _ in self.NS]
        self.param = {0: [4.0 + 5.0 * float(rnd(1)) for _ in self.NS], 1: [float(rnd(1)) - 0.3 for _ in self.NS]}   # beta / best_f
        self.Xq = rnd(sum(COUNTS) + 1, D)
        self.group = np.array([s for s, c in enumerate(COUNTS) for _ in range(c)] + [-1], dtype=np.int32)
        self.off = torch.zeros(self.Xq.shape[0], dtype=torch.float64)
        self.off[LOW_VAR_Q] = -1e3
        # the studies' training blocks: Knn (SPD), its factor and the columns alpha_f = Knn^-1 resid_f, which share all rows but the last
        # (the pending ones, where a group has more than one point)
        self.Lc, self.alpha_f = [], []
        for s_, (n, F) in enumerate(groups):
            Knn = sum((self.w[s_][t] ** 2) * self.cov_fn(t, s_, self.Xt[s_]) for t in range(T) if self.active[s_][t]) / self.s[s_] ** 2
            Knn = 0.5 * (Knn + Knn.T) + _kernel(self.Xt[s_], self.Xt[s_], self.theta[s_], kind) + self.theta[s_][-1] * torch.eye(n, dtype=torch.float64)
            Lc = torch.linalg.cholesky(Knn)
            self.Lc.append(Lc)
            cols = max(F, 1)
            resid = (rnd(n, 1) - 0.5).expand(n, cols).clone()
            resid[-max(1, n // 8):] += 0.5 * (rnd(max(1, n // 8), cols) - 0.5)
            self.alpha_f.append(torch.cholesky_solve(resid, Lc))

    def arrays(self, acqf, info=INFO, F_max=F_MAX):
        """The inputs of (7k) in the query layout: values in column 0, analytic derivatives in columns 1 .. D, zeros behind; NaN past every
        n_g and F_g."""
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
                n = self.NS[s_]
                c = self.cov_fn(t, s_, X[q:q + 1]).squeeze(-1)                       # (n,)
                cov[t, :n, q, :] = 0.0
                cov[t, :n, q, 0] = c.numpy()
                cov[t, :n, q, 1:1 + D] = (-(X[q] - self.Xt[s_]) * c.unsqueeze(-1)).numpy()
        nbm = (n_max + 15) // 16
        Xt, theta = np.full((G, n_max, D), nan), np.zeros((G, D + 2))
        L, W, alpha_f = np.full((G, n_max, n_max), nan), np.full((G, nbm, 16, 16), nan), np.full((G, n_max, F_max), nan)
        for s_, (n, F) in enumerate(self.groups):
            Xt[s_, :n], theta[s_] = self.Xt[s_].numpy(), self.theta[s_].numpy()
            L[s_, :n, :n] = self.Lc[s_].numpy()
            alpha_f[s_, :n, :F] = self.alpha_f[s_][:, :F].numpy()
            for kb in range((n + 15) // 16):
                c = min(16, n - 16 * kb)
                W[s_, kb, :c, :c] = torch.linalg.inv(self.Lc[s_][16 * kb:16 * kb + c, 16 * kb:16 * kb + c]).numpy()
        return dict(mu=mu, var=var, cov=np.ascontiguousarray(cov.reshape(T, n_max, Mq * 16)), group=self.group, Xq=X.numpy().copy(),
                    w=torch.stack(self.w).numpy().copy(), active=torch.stack(self.active).numpy().astype(np.uint8), Xt=Xt, theta=theta, L=L,
                    Linv_diag=W, alpha_f=alpha_f, n_fant=np.array(self.FS, dtype=np.int32), n_points=np.array(self.NS, dtype=np.int32),
                    m_all=np.array(self.m), s_all=np.array(self.s), info=np.array(info, dtype=np.int32), acqf_param=np.array(self.param[acqf]))

    def reference(self, acqf, q):
        """(value, grad (D,)) of query q: mean_f A(mu_f, v) from the restated formulas, the gradient by autograd."""
        s_ = int(self.group[q])
        F = self.FS[s_]
        x = self.Xq[q:q + 1].clone().requires_grad_(True)
        act = [t for t in range(T) if self.active[s_][t]]
        w, m, s, th = self.w[s_], self.m[s_], self.s[s_], self.theta[s_]
        mu_s = sum(w[t] * self.mu_fn(t, x) for t in act).squeeze(0)
        var_s = sum(w[t] ** 2 * (self.var_fn(t, x) + self.off[q]) for t in act).squeeze(0)
        cov_s = sum(w[t] ** 2 * self.cov_fn(t, s_, x) for t in act).squeeze(-1)
        Knq = cov_s / s ** 2 + _kernel(self.Xt[s_], x, th, self.kind).squeeze(-1)
        z = torch.cholesky_solve(Knq.unsqueeze(-1), self.Lc[s_]).squeeze(-1)
        mu = m + s * ((mu_s - m) / s + Knq @ self.alpha_f[s_][:, :F])   # (F,)
        var = s ** 2 * (var_s / s ** 2 + th[-2] - Knq @ z)
        par = self.param[acqf][s_]
        if acqf == 0:   # utils.UpperConfidenceBound: -mu + sqrt(beta max(var, 0)), zero slope where the variance is clamped
            val = -mu + torch.where(var > 0, torch.sqrt(par * torch.where(var > 0, var, torch.ones_like(var))), torch.zeros_like(var))
        else:           # utils.ExpectedImprovement: the 1e-9 floor under the root
            sigma = var.clamp_min(1e-9).sqrt()
            u = -(mu - par) / sigma
            val = sigma * (torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi) + u * 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))))
        val = val.mean()
        (g,) = torch.autograd.grad(val, x)
        return float(val.detach()), g.squeeze(0).numpy()


def _strip_arrays(a, group):
    """The value layout of the same problem: one strip per group (then a padding strip) holding the group's queries, the first one
    repeated up to 16.  Returns (arrays, the query of every candidate)."""
    G = int(group.max()) + 1
    qs = []
    for s_ in list(range(G)) + [-1]:
        mine = [q for q in range(len(group)) if group[q] == s_]
        qs += mine + [mine[0]] * (16 - len(mine))
    qs = np.array(qs)
    Tn, Mq = a["mu"].shape[0], len(qs)
    n_max = a["cov"].shape[1]
    cov = a["cov"].reshape(Tn, n_max, -1, 16)
    b = dict(a)
    b.update(mu=np.ascontiguousarray(a["mu"][:, qs, 0]), var=np.ascontiguousarray(a["var"][:, qs, 0]),
             cov=np.ascontiguousarray(cov[:, :, qs, 0]), Xq=np.ascontiguousarray(a["Xq"][qs]),
             group=np.array(list(range(G)) + [-1], dtype=np.int32))
    assert b["mu"].shape == (Tn, Mq)
    return b, qs


def _run(lib, prob, a, strips=False, want_grad=True):
    Mq, D = a["Xq"].shape
    F_max = a["alpha_f"].shape[2]
    out = dict(value=np.full(Mq, 7.0), grad=np.full((Mq, D), 7.0))
    rc = lib.emul_studies_fantasy(int(strips), *[_p(a[k]) for k in ORDER], Mq, prob.G, prob.n_max, F_max, T, D, prob.kind, a["acqf"],
                                  _p(out["value"]), _p(out["grad"]) if want_grad and not strips else None)
    assert rc == 0
    return out


def _arrays(prob, acqf, **kw):
    a = prob.arrays(acqf, **kw)
    a["Xq"][NAN_Q, min(2, prob.D - 1)] = float("nan")   # (after the source-pass columns were formed: they are finite)
    a["acqf"] = acqf
    return a


@pytest.mark.parametrize("D", [1, 6, 15])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("acqf", [0, 1])
def test_value_and_gradient_match_the_torch_restatement(emul, D, kind, acqf):
    prob = Problem(D, kind, seed=300 + D + kind)
    a = _arrays(prob, acqf)
    out = _run(emul, prob, a)
    g = prob.group
    worst_v = worst_g = 0.0
    for q in range(len(g) - 1):
        if g[q] >= 5 or q == NAN_Q:
            continue
        val, gr = prob.reference(acqf, q)
        if val != 0.0:   # (EI far below the incumbent on the variance floor underflows to 0 on both sides)
            worst_v = max(worst_v, abs(out["value"][q] - val) / abs(val))
        worst_g = max(worst_g, float(np.max(np.abs(out["grad"][q] - gr) / (1e-9 + 1e-6 * np.abs(gr)))))
        np.testing.assert_allclose(out["value"][q], val, rtol=1e-9, err_msg=f"value q={q} group {g[q]}")
        np.testing.assert_allclose(out["grad"][q], gr, rtol=1e-6, atol=1e-9, err_msg=f"gradient q={q} group {g[q]}")
    print(f"D={D} kind={kind} acqf={acqf}: max relative value difference {worst_v:.2e}, max gradient difference / (1e-9 + 1e-6 |g|) {worst_g:.2e}")
    # the refusals: a failed factorisation, a count of fantasies outside 1 .. F_max, a NaN coordinate, a padding row
    for k in ("value", "grad"):
        assert np.isnan(out[k][g == 5]).all() and np.isnan(out[k][g == 6]).all() and np.isnan(out[k][NAN_Q]).all(), k
    assert out["value"][-1] == 0.0 and not out["grad"][-1].any()
    # ... and each of them leaves the others alone: the same call without it, bit for bit
    clean = prob.arrays(acqf, info=(0,) * 7)
    clean["acqf"] = acqf
    clean["n_fant"][6] = 1
    clean["alpha_f"][6, :prob.NS[6], 0] = prob.alpha_f[6][:, 0].numpy()
    ref = _run(emul, prob, clean)
    keep = (g < 5) & (np.arange(len(g)) != NAN_Q)
    for k in ("value", "grad"):
        assert np.array_equal(out[k][keep], ref[k][keep]), k
        assert np.isfinite(ref[k][g >= 0]).all(), k
    # value only: the same values
    assert np.array_equal(_run(emul, prob, a, want_grad=False)["value"], out["value"], equal_nan=True)


@pytest.mark.parametrize("D", [1, 6, 15])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("acqf", [0, 1])
def test_the_strip_layout_gives_the_values_of_the_query_layout(emul, D, kind, acqf):
    prob = Problem(D, kind, seed=300 + D + kind)
    a = _arrays(prob, acqf)
    out = _run(emul, prob, a)
    b, qs = _strip_arrays(a, prob.group)
    strip = _run(emul, prob, b, strips=True)
    assert np.array_equal(strip["value"], out["value"][qs], equal_nan=True)
    assert np.isfinite(strip["value"][prob.group[qs] == 4]).all() and not strip["value"][-16:].any()


def test_too_many_fantasies_is_nan_for_that_group_only(emul):
    prob = Problem(6, 1, seed=21)
    a = _arrays(prob, 0)
    good = _run(emul, prob, a)
    a["n_fant"][2] = F_MAX + 1
    bad = _run(emul, prob, a)
    g = prob.group
    for k in ("value", "grad"):
        assert np.isnan(bad[k][g == 2]).all(), k
        assert np.array_equal(bad[k][g != 2], good[k][g != 2], equal_nan=True), k


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("acqf", [0, 1])
def test_one_fantasy_is_the_ordinary_block_bit_for_bit(emul, ordinary, kind, acqf):
    """F_g = 1 everywhere, alpha_f[..., 0] = alpha: the value and gradient of the existing host build of sa_query, the strip values of
    sa_score_strip -- exact equality (also through F_max = 1 and F_max = 64: the row stride of alpha_f does not matter)."""
    groups = tuple((n, 1) for n, _ in GROUPS)
    prob = Problem(6, kind, seed=40 + kind, groups=groups)
    q_lib, s_lib = ordinary
    for F_max in (1, F_MAX):
        a = prob.arrays(acqf, F_max=F_max)
        a["acqf"] = acqf
        a["alpha"] = np.ascontiguousarray(a["alpha_f"][:, :, 0])
        Mq, D = a["Xq"].shape
        ref = dict(value=np.full(Mq, 7.0), grad=np.full((Mq, D), 7.0))
        assert q_lib.emul_studies_acqf(*[_p(a[k]) for k in ORDER_ORDINARY], Mq, prob.G, prob.n_max, T, D, kind, acqf, _p(ref["value"]),
                                       _p(ref["grad"]), None, None) == 0
        out = _run(emul, prob, a)
        assert np.array_equal(out["value"], ref["value"], equal_nan=True) and np.array_equal(out["grad"], ref["grad"], equal_nan=True)
        assert np.isfinite(ref["value"][:-1][prob.group[:-1] != 5]).all()
        b, qs = _strip_arrays(a, prob.group)
        sref = np.full(len(qs), 7.0)
        assert s_lib.emul_studies_score(*[_p(b[k]) for k in ORDER_ORDINARY], len(qs), prob.G, prob.n_max, T, D, kind, acqf, _p(sref), None, None) == 0
        strip = _run(emul, prob, b, strips=True)
        assert np.array_equal(strip["value"], sref, equal_nan=True) and np.array_equal(sref, ref["value"][qs], equal_nan=True)


def test_lds_footprint_and_argument_block(emul):
    """sa_fantasy_lds_doubles: the ordinary block's carve, then A / Amu / Av [F_max], abar [np] and four sums (a query point) or [16][F_max]
    (a strip); n_max = 96 with F_max = 64 fits the launcher's 160 KiB in both layouts.  The ordinary argument block keeps its size."""
    for n in (1, 16, 17, 96):
        nb = (n + 15) // 16
        base1 = n * 16 + 32 + 3 * 16 * nb + 256 * nb + n * (n | 1) + 48
        base16 = n * 16 + 32 + 33 * 16 * nb + 256 * nb + n * (n | 1) + 32
        for F in (1, 8, 64):
            assert emul.emul_studies_fantasy_lds_doubles(0, n, F) == base1 + 3 * F + 16 * nb + 4
            assert emul.emul_studies_fantasy_lds_doubles(1, n, F) == base16 + 16 * F
    assert emul.emul_studies_fantasy_lds_doubles(1, 96, 64) == 16640 and emul.emul_studies_fantasy_lds_doubles(0, 96, 64) == 13044
    assert emul.emul_studies_fantasy_lds_doubles(1, 96, 64) * 8 <= 160 * 1024
    assert emul.emul_studies_fantasy_params_bytes(0) == 21 * 8 + 8 * 4 and emul.emul_studies_fantasy_params_bytes(1) == 23 * 8 + 10 * 4
