"""CPU checks of the ARITHMETIC of the studies' batched fantasy set-up (csrc/gp_studies_condition.h: sc_condition_block and
sc_fantasy_condition, the bodies of the two kernels of csrc/gp_studies_condition.hip, include/scaml_gp.h (7m) / (7n)) through a host build
of the same source (tests/host_emul/studies_condition_emul.cpp) against a torch-fp64 restatement written here.

The restatement takes the PRESENT route on purpose -- the parent's factor L_nn and alpha, the posterior mean K_pn alpha, the Schur
complement K_pp - V^T V with V = L_nn^-1 K_np, a Cholesky of that p x p block for the samples, and one solve of the whole n' system per
fantasy for alpha_f -- so that the test checks the identity "everything follows from one factor of the joint block", not only the code.
Between (7m) and (7n) stands torch.linalg.cholesky of the host build's own K' (what (2) does on the device).

One call holds the groups (n_obs, p, F) of GROUPS: the smallest, the smallest with two fantasies, n' = 16 (ends on a block edge), n' = 17
(straddles a 16-block), pending rows that straddle the block edge, n' = 96 with F = 64 (all limits), an ordinary study (p = 0: column 0
must be the alpha of a plain solve), a group with info != 0, a group with n_fant = 0 and a group of its own with a NaN coordinate in a
pending point.  One task is pruned in one group only.  Everything past a group's n' / p / F holds NaN on the way in and must hold it on
the way out.  Noise >= 1e-2 of the outputscale: no rung of a jitter ladder is needed, and torch's plain ``cholesky`` is asserted to
succeed on every block -- the condition under which the two routes are the same mathematics.

Tolerances: alpha_f, y_fant and mu_p relative 1e-9 of the column's largest entry (the value tolerance of
tests/test_studies_fantasy_emul.py).  K', resid and mean_p are sums of T = 5 products, a distance over D <= 15 coordinates and one
exponential: relative 1e-13 of the block's largest entry is over a hundred roundings of fp64."""
import ctypes

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests._host_emul import BP, DP, IP, build, ptr as _p

T = 5
F_MAX, N_MAX = 64, 96
#          (n_obs, p, F)
GROUPS = ((1, 1, 1), (1, 1, 2), (15, 1, 8), (15, 2, 63), (12, 5, 3), (92, 4, 64), (5, 0, 1), (6, 2, 3), (4, 1, 0), (7, 2, 4))
INFO = (0, 0, 0, 0, 0, 0, 0, 2, 0, 0)   # group 7: its factorisation failed
ORDINARY, INFO_GROUP, NOFANT_GROUP, NAN_GROUP = 6, 7, 8, 9
PRUNED_GROUP, PRUNED_TASK = 3, 2
P_MAX = max(p for _, p, _ in GROUPS)
NAN = float("nan")


def load(tmp_path_factory, out_dir=None):
    lib = build(tmp_path_factory, "studies_condition_emul", out_dir)
    lib.emul_studies_condition_block.restype = ctypes.c_int
    lib.emul_studies_condition_block.argtypes = [DP, DP, IP, DP, BP, DP, DP, DP, IP, IP, DP, DP] + [ctypes.c_int] * 6 + [DP] * 3
    lib.emul_studies_fantasy_condition.restype = ctypes.c_int
    lib.emul_studies_fantasy_condition.argtypes = [DP, DP, DP, IP, IP, IP, DP, IP, DP, DP] + [ctypes.c_int] * 4 + [DP] * 3
    for f in (lib.emul_condition_block_lds_doubles, lib.emul_fantasy_condition_lds_doubles):
        f.restype, f.argtypes = ctypes.c_longlong, [ctypes.c_int] * 2
    lib.emul_condition_plan.restype, lib.emul_condition_plan.argtypes = None, [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    return lib


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return load(tmp_path_factory)


def kernel(xa, xb, theta, kind):
    D = xa.shape[-1]
    d2 = (((xa.unsqueeze(1) - xb.unsqueeze(0)) / theta[:D]) ** 2).sum(-1)
    if kind == 0:
        return theta[D] * torch.exp(-0.5 * d2)
    r = torch.sqrt(d2.clamp_min(1e-30))
    return theta[D] * (1.0 + 5.0 ** 0.5 * r + (5.0 / 3.0) * r * r) * torch.exp(-(5.0 ** 0.5) * r)


class Problem:
    """A synthetic source pass -- per task a smooth mean mu_t(x) = 2 sin(x . A_t + b_t) and a positive-definite covariance
    c_t exp(-|x - x'|^2 / (2 l_t^2)) -- under G studies with pending evaluations."""

    def __init__(self, D, kind, seed, groups=GROUPS, info=INFO):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)   # noqa: E731
        self.D, self.kind, self.groups, self.G, self.info = D, kind, groups, len(groups), info
        self.NO, self.NP, self.FS = [a for a, _, _ in groups], [a + b for a, b, _ in groups], [c for _, _, c in groups]
        self.n_max = max(self.NP)
        self.A, self.b = rnd(T, D) * 2 - 1, rnd(T)
        self.c, self.l = 0.3 + rnd(T), 0.5 + rnd(T)
        self.X = [rnd(n, D) for n in self.NP]
        os_ = [0.5 + rnd(1) for _ in groups]
        self.theta = [torch.cat([0.4 + rnd(D), o, o * (1e-2 + 0.1 * rnd(1))]) for o in os_]   # noise >= 1e-2 outputscale
        self.w = [0.2 + rnd(T) for _ in groups]
        self.active = [torch.ones(T, dtype=torch.bool) for _ in groups]
        if len(groups) > PRUNED_GROUP:
            self.active[PRUNED_GROUP][PRUNED_TASK] = False
            self.w[PRUNED_GROUP][PRUNED_TASK] = 0.0
        self.m = [float(rnd(1)) - 0.5 for _ in groups]
        self.s = [0.7 + float(rnd(1)) for _ in groups]
        self.y = [rnd(n) * 2 - 1 for n in self.NO]
        self.eps = [torch.randn(max(f, 1), n - no, dtype=torch.float64, generator=g) for n, no, f in zip(self.NP, self.NO, self.FS)]   # (F, p)
        self.strips = [(n + 15) // 16 for n in self.NP]
        self.base = np.concatenate([[0], np.cumsum(self.strips)[:-1]]).astype(np.int32)
        self.Mq = 16 * int(sum(self.strips))

    def mu_fn(self, t, x):
        return 2.0 * torch.sin(x @ self.A[t] + self.b[t])

    def cov_fn(self, t, xa, xb):
        return self.c[t] * torch.exp(-0.5 * ((xa.unsqueeze(1) - xb.unsqueeze(0)) ** 2).sum(-1) / self.l[t] ** 2)

    def block_arrays(self, nan_group=None):
        """The inputs of (7m); NaN in everything a study must not read."""
        D, G, n_max, Mq = self.D, self.G, self.n_max, self.Mq
        mu, cov = np.full((T, Mq), NAN), np.full((T, n_max, Mq), NAN)
        Xt, y = np.full((G, n_max, D), NAN), np.full((G, n_max), NAN)
        theta, w, active = np.zeros((G, D + 2)), np.zeros((G, T)), np.zeros((G, T), dtype=np.uint8)
        for s_, n in enumerate(self.NP):
            c0 = 16 * int(self.base[s_])
            for t in range(T):
                mu[t, c0:c0 + n] = self.mu_fn(t, self.X[s_]).numpy()
                cov[t, :n, c0:c0 + n] = self.cov_fn(t, self.X[s_], self.X[s_]).numpy()
            Xt[s_, :n], y[s_, :self.NO[s_]] = self.X[s_].numpy(), self.y[s_].numpy()
            theta[s_], w[s_], active[s_] = self.theta[s_].numpy(), self.w[s_].numpy(), self.active[s_].numpy()
        if len(self.groups) > PRUNED_GROUP:   # a pruned task's numbers are not looked at
            c0, c1 = 16 * int(self.base[PRUNED_GROUP]), 16 * int(self.base[PRUNED_GROUP] + self.strips[PRUNED_GROUP])
            mu[PRUNED_TASK, c0:c1], cov[PRUNED_TASK, :, c0:c1] = NAN, NAN
            w[PRUNED_GROUP, PRUNED_TASK] = NAN
        if nan_group is not None:
            Xt[nan_group, self.NP[nan_group] - 1, D - 1] = NAN   # the last pending point
        return dict(mu=mu, cov=cov, strip_base=self.base.copy(), w=w, active=active, Xt=Xt, theta=theta, y=y,
                    n_points=np.array(self.NP, dtype=np.int32), n_obs=np.array(self.NO, dtype=np.int32),
                    m_all=np.array(self.m), s_all=np.array(self.s))

    def eps_array(self, F_max=F_MAX, p_max=P_MAX):
        eps = np.full((self.G, p_max, F_max), NAN)
        for s_, e in enumerate(self.eps):
            F, p = self.FS[s_], self.NP[s_] - self.NO[s_]
            if F >= 1 and p >= 1:
                eps[s_, :p, :F] = e.numpy().T
        return eps

    # ---- the torch restatement: the present route
    def joint(self, s_):
        """K' (n', n') and mean' (n') of study s_ in standardised units."""
        X, th, s = self.X[s_], self.theta[s_], self.s[s_]
        n = self.NP[s_]
        K = sum(self.w[s_][t] ** 2 * self.cov_fn(t, X, X) for t in range(T) if self.active[s_][t]) / s ** 2
        K = K + kernel(X, X, th, self.kind) + th[-1] * torch.eye(n, dtype=torch.float64)
        mean = (sum(self.w[s_][t] * self.mu_fn(t, X) for t in range(T) if self.active[s_][t]) - self.m[s_]) / s
        return K, mean

    def reference(self, s_):
        """dict(K, resid, mean_p, alpha_f (n', F), y_fant (p, F), mu_p (p)) by the present route; plain Cholesky must succeed on every
        block it factors."""
        def chol(A):
            L, info = torch.linalg.cholesky_ex(A)
            assert int(info) == 0, f"group {s_}: torch's plain cholesky failed -- the input set is ill-chosen"
            return L

        no, n, F = self.NO[s_], self.NP[s_], max(self.FS[s_], 1)
        K, mean = self.joint(s_)
        m, s = self.m[s_], self.s[s_]
        resid_n = self.y[s_] - mean[:no]
        Lnn = chol(K[:no, :no])
        alpha0 = torch.cholesky_solve(resid_n.unsqueeze(-1), Lnn).squeeze(-1)
        out = dict(K=K, resid=torch.cat([resid_n, torch.zeros(n - no, dtype=torch.float64)]), mean_p=mean[no:])
        if n == no:
            out.update(alpha_f=alpha0.unsqueeze(-1), y_fant=None, mu_p=None)
            return out
        mu_t = mean[no:] + K[no:, :no] @ alpha0                                    # posterior mean at the pending points
        V = torch.linalg.solve_triangular(Lnn, K[:no, no:], upper=False)
        Lpp = chol(K[no:, no:] - V.T @ V)                                          # Schur complement, noise included
        y_t = mu_t.unsqueeze(0) + self.eps[s_] @ Lpp.T                             # (F, p) standardised fantasy targets
        R = torch.cat([resid_n.unsqueeze(0).expand(F, no), y_t - mean[no:]], 1)    # (F, n')
        alpha_f = torch.cholesky_solve(R.T.contiguous(), chol(K))                  # one solve of the n' system per fantasy
        out.update(alpha_f=alpha_f, y_fant=(m + s * y_t).T, mu_p=m + s * mu_t)
        return out


def run_block(lib, prob, a):
    G, n_max = prob.G, prob.n_max
    out = dict(Knn=np.full((G, n_max, n_max), NAN), resid=np.full((G, n_max), NAN), mean_p=np.full((G, n_max), NAN))
    order = ("mu", "cov", "strip_base", "w", "active", "Xt", "theta", "y", "n_points", "n_obs", "m_all", "s_all")
    rc = lib.emul_studies_condition_block(*[_p(a[k]) for k in order], prob.Mq, G, n_max, T, prob.D, prob.kind, _p(out["Knn"]), _p(out["resid"]),
                                          _p(out["mean_p"]))
    assert rc == 0
    return out


def factor(prob, blk):
    """What (2) hands on: the factor of the lower triangle of every study's block (NaN outside it), info as the problem plants it."""
    L = np.full((prob.G, prob.n_max, prob.n_max), NAN)
    for s_, n in enumerate(prob.NP):
        A = torch.from_numpy(np.tril(blk["Knn"][s_, :n, :n]))
        A = A + A.tril(-1).T
        if not torch.isfinite(A).all():
            continue
        Lc, info = torch.linalg.cholesky_ex(A)
        assert int(info) == 0
        L[s_, :n, :n] = np.tril(Lc.numpy()) + np.triu(np.full((n, n), NAN), 1)
    return L


def run_fantasy(lib, prob, a, blk, L, eps, info=None, n_fant=None, F_max=F_MAX, p_max=P_MAX):
    G, n_max = prob.G, prob.n_max
    info = np.array(prob.info if info is None else info, dtype=np.int32)
    n_fant = np.array(prob.FS if n_fant is None else n_fant, dtype=np.int32)
    out = dict(alpha_f=np.full((G, n_max, F_max), NAN), y_fant=np.full((G, p_max, F_max), NAN), mu_p=np.full((G, p_max), NAN))
    rc = lib.emul_studies_fantasy_condition(_p(L), _p(blk["resid"]), _p(blk["mean_p"]), _p(a["n_points"]), _p(a["n_obs"]), _p(info), _p(eps),
                                            _p(n_fant), _p(a["m_all"]), _p(a["s_all"]), G, n_max, p_max, F_max, _p(out["alpha_f"]),
                                            _p(out["y_fant"]), _p(out["mu_p"]))
    assert rc == 0
    return out


def _close_cols(got, ref, what, rtol=1e-9):
    """|got - ref| <= rtol * the column's largest |ref| (columns: the last axis; a vector is one column)."""
    got, ref = np.asarray(got), ref.numpy()
    scale = np.abs(ref).max(0, keepdims=True) if ref.ndim == 2 else np.abs(ref).max()
    err = np.abs(got - ref)
    assert np.isfinite(got).all() and (err <= rtol * scale).all(), f"{what}: error / scale {float((err / scale).max()):.3e}"


@pytest.mark.parametrize("kind", [0, 1], ids=["rbf", "matern"])
@pytest.mark.parametrize("D", [1, 6, 15])
def test_one_factor_of_the_joint_block_gives_the_present_routes_fantasies(emul, D, kind):
    prob = Problem(D, kind, seed=100 + 10 * D + kind)
    a = prob.block_arrays(nan_group=NAN_GROUP)
    blk = run_block(emul, prob, a)
    L = factor(prob, blk)
    out = run_fantasy(emul, prob, a, blk, L, prob.eps_array())
    for s_, (no, p, F) in enumerate(GROUPS):
        n = no + p
        # ---- nothing past n' / p / F was written
        assert np.isnan(blk["Knn"][s_, n:]).all() and np.isnan(blk["Knn"][s_, :, n:]).all(), s_
        assert np.isnan(blk["resid"][s_, n:]).all() and np.isnan(blk["mean_p"][s_, :no]).all() and np.isnan(blk["mean_p"][s_, n:]).all(), s_
        assert np.isnan(out["alpha_f"][s_, n:]).all() and np.isnan(out["alpha_f"][s_, :, max(F, 0):]).all(), s_
        assert np.isnan(out["y_fant"][s_, p:]).all() and np.isnan(out["y_fant"][s_, :, max(F, 0):]).all() and np.isnan(out["mu_p"][s_, p:]).all(), s_
        if s_ == NAN_GROUP:   # a NaN coordinate in a pending point: that study's outputs are NaN, all of them
            assert np.isnan(blk["Knn"][s_, :n, :n]).all() and np.isnan(blk["resid"][s_, :n]).all() and np.isnan(blk["mean_p"][s_, no:n]).all()
            assert np.isnan(out["alpha_f"][s_]).all() and np.isnan(out["y_fant"][s_]).all() and np.isnan(out["mu_p"][s_]).all()
            continue
        ref = prob.reference(s_)
        # ---- (7m)
        K = ref["K"].numpy()
        assert np.abs(blk["Knn"][s_, :n, :n] - K).max() <= 1e-13 * np.abs(K).max(), s_
        assert np.array_equal(blk["Knn"][s_, :n, :n], blk["Knn"][s_, :n, :n].T), s_
        assert np.abs(blk["resid"][s_, :n] - ref["resid"].numpy()).max() <= 1e-13 * max(1.0, np.abs(ref["resid"].numpy()).max()), s_
        assert (blk["resid"][s_, no:n] == 0.0).all(), s_
        if p:
            assert np.abs(blk["mean_p"][s_, no:n] - ref["mean_p"].numpy()).max() <= 1e-13 * max(1.0, np.abs(ref["mean_p"].numpy()).max()), s_
        # ---- (7n)
        if s_ in (INFO_GROUP, NOFANT_GROUP):
            assert np.isnan(out["alpha_f"][s_]).all() and np.isnan(out["y_fant"][s_]).all() and np.isnan(out["mu_p"][s_]).all(), s_
            continue
        _close_cols(out["alpha_f"][s_, :n, :F], ref["alpha_f"], f"group {s_} alpha_f")
        if p:
            _close_cols(out["y_fant"][s_, :p, :F], ref["y_fant"], f"group {s_} y_fant")
            _close_cols(out["mu_p"][s_, :p], ref["mu_p"], f"group {s_} mu_p")
        else:   # an ordinary study: nothing of y_fant / mu_p is written
            assert np.isnan(out["y_fant"][s_]).all() and np.isnan(out["mu_p"][s_]).all()


def test_refusals_touch_one_study_only(emul):
    """Counts out of range turn that study's outputs into NaN and leave the neighbours' bits alone."""
    prob = Problem(3, 1, seed=7, groups=GROUPS[:5], info=INFO[:5])
    a = prob.block_arrays()
    blk = run_block(emul, prob, a)
    L = factor(prob, blk)
    eps = prob.eps_array()
    good = run_fantasy(emul, prob, a, blk, L, eps)
    assert all(np.isfinite(good["alpha_f"][s_, :no + p, :F]).all() for s_, (no, p, F) in enumerate(prob.groups))
    cases = [("n_fant", 2, F_MAX + 1), ("n_fant", 2, -1), ("info", 3, -3), ("n_obs", 2, 0), ("n_obs", 4, 18), ("n_points", 1, 0),
             ("n_points", 3, N_MAX + 1)]
    for name, s_, val in cases:
        b = {k: v.copy() for k, v in a.items()}
        kw = {}
        if name in ("n_obs", "n_points"):
            b[name][s_] = val
        else:
            vec = np.array(prob.FS if name == "n_fant" else prob.info, dtype=np.int32)
            vec[s_] = val
            kw[name] = vec
        out = run_fantasy(emul, prob, b, blk, L, eps, **kw)
        no, p, F = prob.groups[s_]
        assert not np.isfinite(out["alpha_f"][s_]).any() and not np.isfinite(out["y_fant"][s_]).any() and not np.isfinite(out["mu_p"][s_]).any(), (name, val)
        for o in range(prob.G):
            if o != s_:
                assert all(np.array_equal(out[k][o], good[k][o], equal_nan=True) for k in out), (name, val, o)
    # an ORDINARY study takes F = 1 only
    prob2 = Problem(3, 0, seed=8, groups=((5, 0, 1), (3, 1, 2)), info=(0, 0))
    a2 = prob2.block_arrays()
    blk2 = run_block(emul, prob2, a2)
    out = run_fantasy(emul, prob2, a2, blk2, factor(prob2, blk2), prob2.eps_array(p_max=1), n_fant=[2, 2], p_max=1)
    assert np.isnan(out["alpha_f"][0, :5, :2]).all() and np.isfinite(out["alpha_f"][1, :4, :2]).all()
    # (7m): n_obs out of range or strips outside the pass's columns: that study's block is NaN, n' out of range: nothing is written
    for name, s_, val in (("n_obs", 2, 0), ("n_obs", 2, 17), ("strip_base", 4, prob.Mq // 16), ("strip_base", 1, -1), ("n_points", 3, 0),
                          ("n_points", 3, N_MAX + 1)):
        b = {k: v.copy() for k, v in a.items()}
        b[name][s_] = val
        got = run_block(emul, prob, b)
        assert np.isnan(got["Knn"][s_]).all() and np.isnan(got["resid"][s_]).all(), (name, val)
        for o in range(prob.G):
            if o != s_:
                assert all(np.array_equal(got[k][o], blk[k][o], equal_nan=True) for k in got), (name, val, o)


def test_launch_plans(emul):
    """A workgroup of 256 threads per study, the LDS of the footprint functions (csrc/gp_dispatch.h)."""
    out = (ctypes.c_longlong * 3)()
    for which, third, lds in ((0, 15, emul.emul_condition_block_lds_doubles), (1, 64, emul.emul_fantasy_condition_lds_doubles)):
        for G, n_max in ((1, 1), (7, 17), (300, 96)):
            emul.emul_condition_plan(which, G, n_max, third, out)
            assert list(out) == [G, 256, lds(n_max, third)]


def test_lds_footprints_at_the_limits(emul):
    assert emul.emul_condition_block_lds_doubles(96, 15) == 96 * 15 + 96
    assert emul.emul_fantasy_condition_lds_doubles(96, 64) == 96 * 97 + 3 * 96 + 96 * 64
    assert emul.emul_fantasy_condition_lds_doubles(96, 64) * 8 <= 160 * 1024
