"""Synthetic inputs of the strip scoring kernel (include/scaml_gp.h (7i)) shared by tests/test_studies_score_emul.py (host build) and
tests/test_studies_score_gpu.py (device): smooth source-pass outputs mu_t(x), var_t(x), cov_{t,a}(x) as in
tests/test_studies_acqf_emul.py, G studies of ragged size on top of them, a table of candidates in strips of 16, and the same numbers
in both layouts -- the value layout (7i) reads and column 0 of (7g)'s 16-column layout with NaN in columns 1 .. 15.

Planted: rows past a study's n hold NaN (never read); one task is pruned in ONE study and its mu / var / cov hold NaN in that study's
columns (skipped, not multiplied by zero); one padding strip (zeros; its columns hold NaN); one study with info = 1 (NaN for its
candidates); one candidate with a NaN coordinate (NaN for that candidate only).  Not a test module."""
import math

import numpy as np
import torch

NS = (1, 15, 16, 17, 33, 5)      # the last study's factorisation "failed": info = 1
FAILED = 5
PRUNED_STUDY, PRUNED_TASK = 3, 1
NAN_STUDY = 2                    # the study that owns the candidate with a NaN coordinate
ORDER = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha", "n_points", "m_all", "s_all", "info",
         "acqf_param")


def kernel(x1, x2, theta, kind):
    """os k((x1 - x2) / l), (n1, n2): gpytorch's RBF / Matern-5/2 (squared distance clamped at 1e-30 before the root)."""
    D = x1.shape[-1]
    d2 = (((x1.unsqueeze(-2) - x2.unsqueeze(-3)) / theta[:D]) ** 2).sum(-1)
    if kind == 0:
        return theta[D] * torch.exp(-0.5 * d2)
    r = torch.sqrt(d2.clamp_min(1e-30)) * math.sqrt(5.0)
    return theta[D] * (1.0 + r + r * r / 3.0) * torch.exp(-r)


class Problem:
    def __init__(self, T, D, kind, seed, strips=(1, 1, 1, 1, 1, 1)):
        """``strips[g]``: strips of 16 candidates of study g; a padding strip is inserted after the first study's."""
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)   # noqa: E731
        self.T, self.D, self.kind, self.G, self.n_max = T, D, kind, len(NS), max(NS)
        self.A, self.b, self.C = rnd(T, D) * 2 - 1, rnd(T), rnd(T, D)
        self.Xt = [rnd(n, D) for n in NS]
        self.theta = [torch.cat([0.4 + rnd(D), 0.5 + rnd(1), 1e-2 + 0.1 * rnd(1)]) for _ in NS]
        self.w = [0.2 + rnd(T) for _ in NS]
        self.active = [torch.ones(T, dtype=torch.bool) for _ in NS]
        self.active[PRUNED_STUDY][PRUNED_TASK] = False
        self.w[PRUNED_STUDY][PRUNED_TASK] = 0.0
        self.m = [float(rnd(1)) - 0.5 for _ in NS]
        self.s = [0.7 + float(rnd(1)) for _ in NS]
        self.param = {0: [4.0 + 5.0 * float(rnd(1)) for _ in NS], 1: [float(rnd(1)) - 0.3 for _ in NS]}   # beta / best_f
        group = []
        for s_, c in enumerate(strips):
            group += [s_] * c
            if s_ == 0:
                group.append(-1)
        self.group = np.array(group, dtype=np.int32)                 # per strip
        self.Mq = 16 * len(group)
        self.Xq = rnd(self.Mq, D)
        self.nan_q = 16 * int(np.nonzero(self.group == NAN_STUDY)[0][0]) + 5
        self.Lc, self.alpha = [], []
        for s_, n in enumerate(NS):
            Knn = sum((self.w[s_][t] ** 2) * self.cov_fn(t, s_, self.Xt[s_]) for t in range(T) if self.active[s_][t]) / self.s[s_] ** 2
            Knn = 0.5 * (Knn + Knn.T) + kernel(self.Xt[s_], self.Xt[s_], self.theta[s_], kind) + self.theta[s_][-1] * torch.eye(n, dtype=torch.float64)
            Lc = torch.linalg.cholesky(Knn)
            self.Lc.append(Lc)
            self.alpha.append(torch.cholesky_solve((rnd(n, 1) - 0.5), Lc).squeeze(-1))

    def mu_fn(self, t, x):
        return 2.0 * torch.sin(x @ self.A[t] + self.b[t]) + 0.3 * t

    def var_fn(self, t, x):
        return 2.0 + torch.cos(x @ self.C[t])

    def cov_fn(self, t, s_, x):
        """(n_s, M): Cov(f_t(Xt_s[a]), f_t(x))"""
        d2 = ((self.Xt[s_].unsqueeze(1) - x.unsqueeze(0)) ** 2).sum(-1)
        return 0.3 * (1.0 + 0.1 * t) * torch.exp(-0.5 * d2)

    def study_of(self, q):
        return int(self.group[q // 16])

    def arrays(self, acqf, layout):
        """The inputs in ORDER.  ``layout`` "value": mu, var (T, Mq), cov (T, n_max, Mq), group per strip; "grad": mu, var (T, Mq, 16),
        cov (T, n_max, Mq * 16), group per query point, the numbers in column 0 and NaN in columns 1 .. 15."""
        T, D, G, n_max, Mq = self.T, self.D, self.G, self.n_max, self.Mq
        nan = float("nan")
        mu, var, cov = np.full((T, Mq), nan), np.full((T, Mq), nan), np.full((T, n_max, Mq), nan)
        Xq = self.Xq.numpy().copy()
        for s_, n in enumerate(NS):
            cols = np.nonzero(np.repeat(self.group, 16) == s_)[0]
            X = self.Xq[cols]
            for t in range(T):
                if not bool(self.active[s_][t]):
                    continue                                          # the pruned task: NaN stays
                mu[t, cols] = self.mu_fn(t, X).numpy()
                var[t, cols] = self.var_fn(t, X).numpy()
                cov[t][:n, cols] = self.cov_fn(t, s_, X).numpy()
        Xq[self.nan_q, D - 1] = nan
        nbm = (n_max + 15) // 16
        Xt, theta = np.full((G, n_max, D), nan), np.zeros((G, D + 2))
        L, W, alpha = np.full((G, n_max, n_max), nan), np.full((G, nbm, 16, 16), nan), np.full((G, n_max), nan)
        for s_, n in enumerate(NS):
            Xt[s_, :n], theta[s_] = self.Xt[s_].numpy(), self.theta[s_].numpy()
            L[s_, :n, :n], alpha[s_, :n] = self.Lc[s_].numpy(), self.alpha[s_].numpy()
            for kb in range((n + 15) // 16):
                c = min(16, n - 16 * kb)
                W[s_, kb, :c, :c] = torch.linalg.inv(self.Lc[s_][16 * kb:16 * kb + c, 16 * kb:16 * kb + c]).numpy()
        info = np.zeros(G, dtype=np.int32)
        info[FAILED] = 1
        group = self.group
        if layout == "grad":
            m16, v16, c16 = np.full((T, Mq, 16), nan), np.full((T, Mq, 16), nan), np.full((T, n_max, Mq, 16), nan)
            m16[:, :, 0], v16[:, :, 0], c16[:, :, :, 0] = mu, var, cov
            mu, var, cov = m16, v16, np.ascontiguousarray(c16.reshape(T, n_max, Mq * 16))
            group = np.repeat(self.group, 16).astype(np.int32)
        return dict(mu=mu, var=var, cov=np.ascontiguousarray(cov), group=group, Xq=Xq, w=torch.stack(self.w).numpy().copy(),
                    active=torch.stack(self.active).numpy().astype(np.uint8), Xt=Xt, theta=theta, L=L, Linv_diag=W, alpha=alpha,
                    n_points=np.array(NS, dtype=np.int32), m_all=np.array(self.m), s_all=np.array(self.s), info=info,
                    acqf_param=np.array(self.param[acqf]))

    def reference(self, acqf, q):
        """(value, mu*, var*) of candidate q from the restated formulas in torch fp64."""
        s_ = self.study_of(q)
        x = self.Xq[q:q + 1]
        act = [t for t in range(self.T) if self.active[s_][t]]
        w, m, s, th = self.w[s_], self.m[s_], self.s[s_], self.theta[s_]
        mu_s = sum(w[t] * self.mu_fn(t, x) for t in act).squeeze(0)
        var_s = sum(w[t] ** 2 * self.var_fn(t, x) for t in act).squeeze(0)
        cov_s = sum(w[t] ** 2 * self.cov_fn(t, s_, x) for t in act).squeeze(-1)
        Knq = cov_s / s ** 2 + kernel(self.Xt[s_], x, th, self.kind).squeeze(-1)
        z = torch.cholesky_solve(Knq.unsqueeze(-1), self.Lc[s_]).squeeze(-1)
        mu = m + s * ((mu_s - m) / s + Knq @ self.alpha[s_])
        var = s ** 2 * (var_s / s ** 2 + th[-2] - Knq @ z)
        par = self.param[acqf][s_]
        if acqf == 0:
            val = -mu + torch.sqrt(par * var.clamp_min(0.0))
        else:
            sigma = var.clamp_min(1e-9).sqrt()
            u = -(mu - par) / sigma
            val = sigma * (torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi) + u * 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))))
        return float(val), float(mu), float(var)
