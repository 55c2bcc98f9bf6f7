"""Long-double reference, a-priori forward error bound and shared assertions for the source-posterior kernels
(gp_posterior_kernel, gp_posterior_linv_kernel plain / COV / GRAD, gp_posterior_cov_kernel, gp_linv_kernel).

The reference consumes the arrays the kernel itself is handed (X, theta, alpha, and L / Linv / V / VA as the device
produced them), so what is compared is the kernel's own arithmetic; the fit's conditioning does not enter.  The tolerance
is a componentwise forward error bound from standard rounding analysis, computed next to the reference.  With u = 2^-53,
g_k = k u / (1 - k u), a' = x / l (scaled points), |.| the Euclidean norm of a scaled point:

  distance   E_d2 = (D + 8) u (|a'| + |q'|)^2          expanded form |a'|^2 + |q'|^2 - 2 a'.q', the worst in the family
  kernel     E_K  = os (S  E_d2 + 4 u |k|)              S  = sup |dk/dd2|     = 1/2 (RBF), 5/6 (Matern-5/2)
  slope      E_dk = os (S' E_d2 + 4 u |dk|)             S' = sup |d2k/dd2^2|  = 1/4 (RBF), 25/12 (Matern-5/2)
             (4 u: exp ~1 ulp, the seeded sqrt <= 1.5 ulp, one rounding each for 1 / l and the product)
  GRAD col   c = 2 os dk (q'_d - a'_d) / l_d:
             E_c  = (2 / l_d) (E_dk |q'_d - a'_d| + os |dk| (2 u (|q'_d| + |a'_d|) + u |q'_d - a'_d|)) + 5 u |c|
             (the difference of two scaled coordinates that carry 2 u each, its own rounding, then the roundings of
              1 / l_d, the three products and the factor's relative error passed on: 5 u of the result)
  mean       E_mu = ys (E_K^T |alpha| + g_{N+4} |K*|^T |alpha|) + 2 u (|ym| + |mu - ym|)
  solve      E_V  = |Linv| E_K + g_{N+4} |Linv| |K*|                      explicit inverse: a matrix product
             E_V  = |L^-1| (E_K + g_{N+4} |L| |V|)                       substitution
  variance   E_var = ys^2 (sum (2 |V| E_V + E_V^2) + g_{N+4} sum V^2 + 2 u os) + 2 u |var|
  d var      E = 2 ys^2 (sum (|V_0| E_Vd + |V_d| E_V0 + E_V0 E_Vd) + g_{N+4} sum |V_0| |V_d|) + 3 u |d var|
  cov        E = ys^2 (E_K(xa, xq) + |VA|^T E_V + g_{N+4} |VA|^T |V| + u (|os k| + |VA^T V|)) + 2 u |cov|
             (VA, and V for scaml_posterior_cov_f64, are inputs: they carry no error term of their own)
  Linv       g_{N+4} |L^-1| |L| |L^-1| componentwise

Terms added to the issue's model, each one rounding of the kernels' last statement: `ys * ys * (...)` is two products
(2 u |var|, 2 u |cov|, with the factor -2 of d var 3 u), and `kv - dot` in the covariance is one subtraction
(u (|os k| + |VA^T V|)).  No constant here is fitted to what a kernel returns.

Every bound is capped: it must not exceed CAP = 1e-8 of the quantity's largest reference magnitude in the task (os ys^2
for variances and covariances).  That is a condition on the INPUTS (a bound that grows loose is an ill-chosen input
set), asserted with every comparison.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the reference needs x87 extended precision (x86-64)"

KIND_RBF, KIND_MATERN52 = 0, 1
U = 2.0 ** -53
CAP = 1e-8
SENTINEL = -7.25e77          # what an output buffer holds before the call
OS = 1.3


def gamma(k: int) -> float:
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------------------------
# input sets, shared by the CPU and the GPU file
Case = namedtuple("Case", "kern T N M D kind Ma ragged std per_task nanq c noise")


def _c(kern, T, N, M, D, kind, Ma=0, ragged=None, std=False, per_task=False, nanq=False, c=0.5, noise=1e-2):
    return Case(kern, T, N, M, D, kind, Ma, ragged, std, per_task, nanq, c, noise)


R, MT = KIND_RBF, KIND_MATERN52
# kern: subst / subst_mean (scaml_posterior_batched_f64), linv (scaml_posterior_linv_f64), cov (scaml_posterior_cov_f64),
# linv_cov (scaml_posterior_linv_cov_f64), grad (scaml_posterior_linv_grad_f64, M = Mq), linvmat / linvmat_lower.
# ragged = k: task t has RAGGED(N)[(t + k) % 5] points.  N: 17 two blocks, odd | 129 NB = 9, odd, mostly padding | 144 NB = 9,
# even, vector loads | 255 odd, NB = 16 | 272 NB = 17, third serpentine round | 512 the limit.  T = 9: second XCD round.
CASES = [
    _c("subst", 9, 17, 1, 1, R, ragged=0, std=True, c=0.3),
    _c("subst", 3, 129, 17, 5, MT, ragged=0, noise=1e-3),
    _c("subst", 2, 144, 16, 4, R, std=True, per_task=True),
    _c("subst", 2, 255, 33, 15, MT, ragged=1, c=0.3),
    _c("subst", 2, 256, 17, 11, R, std=True),                  # X staged in LDS
    _c("subst", 2, 256, 17, 12, MT),                           # X read from memory (posterior_lds_doubles past 160 KiB)
    _c("subst", 2, 272, 16, 4, MT, ragged=2, std=True, noise=1e-3),
    _c("subst", 2, 512, 33, 5, R, ragged=1),
    _c("subst_mean", 9, 129, 17, 17, MT, ragged=0, std=True),
    _c("subst_mean", 2, 255, 1, 4, R, per_task=True, noise=1e-3),
    _c("subst", 2, 129, 33, 4, R, std=True, nanq=True),
    _c("subst", 2, 144, 17, 5, MT, ragged=1, nanq=True),
    _c("linv", 9, 17, 1, 1, MT, ragged=0, c=0.3),
    _c("linv", 9, 129, 17, 5, R, ragged=0, std=True, noise=1e-3),
    _c("linv", 9, 144, 16, 4, MT, ragged=0, per_task=True),
    _c("linv", 3, 255, 33, 15, R, ragged=0, std=True, c=0.3),
    _c("linv", 2, 272, 17, 15, MT),
    _c("linv", 2, 512, 33, 4, MT, ragged=1, std=True, noise=1e-3),
    _c("linv", 2, 129, 16, 17, R, ragged=2),
    _c("linv", 2, 129, 33, 5, R, std=True, nanq=True),
    _c("linv", 2, 255, 17, 4, MT, ragged=1, nanq=True),
    _c("cov", 3, 129, 33, 5, R, Ma=17, ragged=0, std=True),
    _c("cov", 2, 144, 17, 17, MT, Ma=16, per_task=True),
    _c("cov", 2, 17, 1, 1, R, Ma=1, ragged=1, c=0.3),
    _c("linv_cov", 9, 129, 17, 4, R, Ma=1, ragged=0, std=True),
    _c("linv_cov", 3, 144, 16, 5, MT, Ma=16, ragged=0, noise=1e-3),
    _c("linv_cov", 3, 255, 33, 15, R, Ma=17, ragged=1, std=True),
    _c("linv_cov", 2, 272, 97, 4, MT, Ma=96, ragged=1),
    _c("linv_cov", 2, 512, 33, 5, R, Ma=17, std=True, c=0.3),
    _c("linv_cov", 2, 17, 17, 1, R, Ma=17, ragged=1),
    _c("linv_cov", 2, 129, 33, 4, MT, Ma=16, ragged=1, std=True, nanq=True),
    _c("grad", 9, 17, 3, 1, R, Ma=0, ragged=0, std=True, c=0.3),
    _c("grad", 9, 129, 4, 5, MT, Ma=1, ragged=0),
    _c("grad", 3, 144, 3, 4, R, Ma=17, ragged=0, std=True, noise=1e-3),
    _c("grad", 2, 255, 3, 15, MT, Ma=96, ragged=1),
    _c("grad", 2, 272, 2, 5, R, Ma=17, std=True),
    _c("grad", 2, 512, 2, 15, R, Ma=0, ragged=1, c=0.3),
    _c("grad", 2, 129, 3, 4, R, Ma=17, ragged=1, std=True, nanq=True),
    _c("grad", 2, 144, 3, 5, MT, Ma=1, nanq=True),
    _c("linvmat", 9, 17, 0, 1, R, ragged=0),
    _c("linvmat", 3, 129, 0, 5, MT, ragged=0, noise=1e-3),
    _c("linvmat", 2, 144, 0, 4, R),
    _c("linvmat", 2, 255, 0, 15, MT, ragged=1),
    _c("linvmat", 2, 272, 0, 4, R),
    _c("linvmat", 2, 512, 0, 5, MT, ragged=1),
    _c("linvmat_lower", 3, 129, 0, 4, R, ragged=0),
    _c("linvmat_lower", 2, 272, 0, 5, MT, ragged=3),
]


def case_id(c: Case) -> str:
    s = f"{c.kern}-T{c.T}-N{c.N}-M{c.M}-D{c.D}-{'rbf' if c.kind == R else 'matern'}"
    if c.Ma or c.kern == "grad":
        s += f"-Ma{c.Ma}"
    for flag in ("std", "per_task", "nanq"):
        if getattr(c, flag):
            s += "-" + flag
    return s + ("" if c.ragged is None else f"-ragged{c.ragged}")


def ragged_counts(N: int):
    """N, N - 1, a multiple of 16 (inside the matrix, at least 16), 1, 0."""
    return [N, N - 1, max(16, 16 * (N // 32)), 1, 0]


def make_inputs(c: Case) -> dict:
    """fp64 numpy arrays of one case: X in the unit cube, l = c sqrt(D) (0.5 .. 1.5), os = 1.3, a smooth standardised y.  The
    first query point sits exactly on a training point of task 0, the second 1e-7 away from another."""
    rng = np.random.default_rng([CASES.index(c) if c in CASES else 999, c.T, c.N, c.D])
    T, N, M, D = c.T, c.N, c.M, c.D
    X = rng.uniform(size=(T, N, D))
    theta = np.concatenate([c.c * np.sqrt(D) * rng.uniform(0.5, 1.5, size=(T, D)), np.full((T, 1), OS), np.full((T, 1), c.noise)], 1)
    n_points = None if c.ragged is None else np.array([ragged_counts(N)[(t + c.ragged) % 5] for t in range(T)], dtype=np.int32)
    y = np.zeros((T, N))
    for t in range(T):
        n = N if n_points is None else int(n_points[t])
        w = rng.normal(size=D)
        f = np.sin(3.0 * X[t, :n] @ w / np.sqrt(D) + t) + 0.3 * X[t, :n, 0] + 0.05 * rng.normal(size=n)
        y[t, :n] = (f - f.mean()) / f.std() if n > 1 else 0.3
    out = dict(X=X, y=y, theta=theta, n_points=n_points, y_mean=None, y_std=None)
    if c.std:
        out["y_mean"], out["y_std"] = rng.normal(size=T) * 3.0, rng.uniform(0.5, 2.5, size=T)
    if c.kern.startswith("linvmat"):
        return out
    Xq = rng.uniform(size=(T, M, D) if c.per_task else (M, D))
    q0 = Xq[0] if c.per_task else Xq
    q0[0] = X[0, 0]
    if M > 1:
        q0[1] = X[0, min(3, N - 1)] + 1e-7
    if c.nanq:
        q0[M - 2, D - 1] = np.nan          # (for T > 1 per-task sets only task 0 would see it; the NaN cases share Xq)
    out["Xq"] = Xq
    if c.kern == "grad" and c.Ma:
        out["Xa"] = rng.uniform(size=(c.Ma, D))
        out["Xa"][0] = X[0, 1]
    return out


def counts(c: Case, inp: dict):
    return [c.N] * c.T if inp["n_points"] is None else [int(v) for v in inp["n_points"]]


def host_fit(c: Case, inp: dict) -> dict:
    """fp64 numpy stand-in for the DEVICE fit (the CPU file has no device): L, alpha, the inverses of L's 16 x 16 diagonal blocks
    (identity-padded) and Linv, laid out as the library lays them out (zeros / identity past n_t)."""
    T, N, D = c.T, c.N, c.D
    NB = (N + 15) // 16
    L, alpha = np.zeros((T, N, N)), np.zeros((T, N))
    W = np.tile(np.eye(16), (T, NB, 1, 1))
    Linv = np.tile(np.eye(N), (T, 1, 1))
    for t, n in enumerate(counts(c, inp)):
        if n == 0:
            continue
        a = inp["X"][t, :n] / inp["theta"][t, :D]
        d2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)
        K = OS * _kernel(d2, c.kind)[0] + inp["theta"][t, D + 1] * np.eye(n)
        Lt = np.linalg.cholesky(K)
        L[t, :n, :n] = Lt
        alpha[t, :n] = np.linalg.solve(Lt.T, np.linalg.solve(Lt, inp["y"][t, :n]))
        Lp = np.eye(NB * 16)
        Lp[:n, :n] = Lt
        for b in range(NB):
            W[t, b] = np.linalg.inv(Lp[16 * b:16 * b + 16, 16 * b:16 * b + 16])
        Linv[t, :n, :n] = np.tril(np.linalg.inv(Lt))
    return dict(L=L, alpha=alpha, Linv_diag=W, Linv=Linv)


# ------------------------------------------------------------------------------------------------------------------
# reference and bound
def _kernel(d2, kind):
    """k(d2) and dk/dd2 without the outputscale, gpytorch's 1e-30 clamp before the Matern square root (any float type)."""
    one = d2.dtype.type(1)
    if kind == KIND_RBF:
        k = np.exp(-d2 / 2)
        return k, -k / 2
    s5 = np.sqrt(one * 5)
    r = np.sqrt(np.maximum(d2, one * 1e-30))
    e = np.exp(-s5 * r)
    lin = 1 + s5 * r
    return (lin + (one * 5 / 3) * r * r) * e, -(one * 5 / 6) * lin * e


_S = {KIND_RBF: (0.5, 0.25), KIND_MATERN52: (5.0 / 6.0, 25.0 / 12.0)}


def columns(Xn, l, kind, xq, grad):
    """Right-hand-side columns against the points Xn (n, D) and their bound E, both (n, ncols) long double.
    grad = False: xq (M, D), column c = os k(Xn, xq_c).  grad = True: xq (D,), 16 columns [os k, d os k / d x_0 .. x_{D-1}, 0 ..]."""
    n, D = Xn.shape
    a = LD(Xn) / LD(l)
    q = LD(np.atleast_2d(xq)) / LD(l)
    na, nq = np.sqrt((a * a).sum(-1)), np.sqrt((q * q).sum(-1))
    diff = q[None, :, :] - a[:, None, :]                        # (n, M, D): q' - a'
    d2 = (diff * diff).sum(-1)
    E_d2 = (D + 8) * U * (na[:, None] + nq[None, :]) ** 2
    k, dk = _kernel(d2, kind)
    S, S1 = _S[kind]
    E_K = OS * (S * E_d2 + 4 * U * np.abs(k))
    if not grad:
        return OS * k, E_K
    C, E = np.zeros((n, 16), dtype=LD), np.zeros((n, 16), dtype=LD)
    C[:, 0], E[:, 0] = OS * k[:, 0], E_K[:, 0]
    E_dk = OS * (S1 * E_d2[:, 0] + 4 * U * np.abs(dk[:, 0]))
    for d in range(D):
        df, il = diff[:, 0, d], 1 / LD(l[d])
        C[:, 1 + d] = 2 * OS * dk[:, 0] * df * il
        E[:, 1 + d] = 2 * il * (E_dk * np.abs(df) + OS * np.abs(dk[:, 0]) * (2 * U * (np.abs(q[0, d]) + np.abs(a[:, d])) + U * np.abs(df))) \
            + 5 * U * np.abs(C[:, 1 + d])
    return C, E


def forward_subst(L, B):
    """L^-1 B in long double, row by row."""
    n = L.shape[0]
    V = np.zeros(B.shape, dtype=LD)
    Ll = LD(L)
    for i in range(n):
        V[i] = (B[i] - np.dot(Ll[i, :i], V[:i])) / Ll[i, i]
    return V


def inverse_lower(L):
    """L^-1 in long double (forward substitution against the identity, one row at a time)."""
    return forward_subst(L, np.eye(L.shape[0], dtype=LD))


Quantity = namedtuple("Quantity", "ref bound scale")   # ref / bound: long-double arrays of the output's shape; scale: float


def _scale(x):
    x = np.abs(x[np.isfinite(x)])
    return float(x.max()) if x.size else 0.0


def task_reference(c: Case, arr: dict, t: int) -> dict:
    """Reference and bound of every output of case c's kernel for task t.  arr: the case's inputs plus the device's (or the host
    stand-in's) L, Linv_diag, Linv, alpha, and V / VA where the kernel takes them.  Shapes are those of the task's slice of the
    output; rows >= n_t of V have reference and bound 0 (they must be exactly zero)."""
    N, D, M = c.N, c.D, c.M
    n = N if arr["n_points"] is None else int(arr["n_points"][t])
    g = gamma(N + 4)
    if c.kern.startswith("linvmat"):
        ref, bound = np.eye(N, dtype=LD), np.zeros((N, N), dtype=LD)
        if n:
            Ln = arr["L"][t, :n, :n]
            ref[:n, :n] = inverse_lower(Ln)
            A = np.abs(ref[:n, :n].astype(np.float64))
            bound[:n, :n] = g * (1 + 1e-9) * (A @ np.abs(Ln) @ A)
        return dict(Linv=Quantity(ref, bound, _scale(ref)))
    th = arr["theta"][t]
    l = th[:D]
    ym = 0.0 if arr["y_mean"] is None else float(arr["y_mean"][t])
    ys = 1.0 if arr["y_std"] is None else float(arr["y_std"][t])
    ys2 = LD(ys) * LD(ys)
    Xn = arr["X"][t, :n]
    al = LD(arr["alpha"][t, :n])
    Xq = arr["Xq"][t] if c.per_task else arr["Xq"]
    grad = c.kern == "grad"
    out = {k: [] for k in ("mu", "var", "V", "cov")}
    with np.errstate(invalid="ignore"):
        if c.kern == "cov":        # V is an input here
            Vd = LD(arr["V"][t, :n])
            Kaq, E_Kaq = columns(Xq[:c.Ma], l, c.kind, Xq, False)
            dot = Vd[:, :c.Ma].T @ Vd
            cov = ys2 * (Kaq - dot)
            E = ys2 * (E_Kaq + g * (np.abs(Vd[:, :c.Ma]).T @ np.abs(Vd)) + U * (np.abs(Kaq) + np.abs(dot))) + 2 * U * np.abs(cov)
            return dict(cov=Quantity(cov, E, OS * float(ys2)))
        for xq in (Xq if grad else [Xq]):      # GRAD: one 16-column strip per query point
            C, EC = columns(Xn, l, c.kind, xq, grad)
            ncol = C.shape[1]
            dot = C.T @ al
            value_col = np.eye(16)[0] if grad else np.ones(ncol)      # the columns that carry y_mean
            mu = ys * dot + ym * value_col
            E_mu = ys * (EC.T @ np.abs(al) + g * (np.abs(C).T @ np.abs(al))) + 2 * U * (abs(ym) * value_col + np.abs(ys * dot))
            out["mu"].append((mu, E_mu))
            if c.kern == "subst_mean":
                continue
            V, EV = np.zeros((N, ncol), dtype=LD), np.zeros((N, ncol), dtype=LD)
            if c.kern == "subst":
                Ln = arr["L"][t, :n, :n]
                V[:n] = forward_subst(Ln, C)
                Li = np.abs(np.linalg.inv(Ln)) * (1 + 1e-9) if n else np.zeros((0, 0))
                EV[:n] = LD(Li) @ (EC + g * (LD(np.abs(Ln)) @ np.abs(V[:n])))
            else:
                Li = LD(np.tril(arr["Linv"][t, :n, :n]))     # (the lower-only variant leaves the rest unwritten: never read)
                V[:n] = Li @ C
                EV[:n] = np.abs(Li) @ EC + g * (np.abs(Li) @ np.abs(C))
            out["V"].append((V, EV))
            aV = np.abs(V)
            if grad:
                p = (V[:, :1] * V).sum(0)
                var = -2 * ys2 * p
                E_var = 2 * ys2 * ((aV[:, :1] * EV + aV * EV[:, :1] + EV[:, :1] * EV).sum(0) + g * (aV[:, :1] * aV).sum(0)) + 3 * U * np.abs(var)
                s0 = p[0]
                var[0] = ys2 * (OS - s0)
                E_var[0] = ys2 * ((2 * aV[:, 0] * EV[:, 0] + EV[:, 0] ** 2).sum() + g * s0 + 2 * U * OS) + 2 * U * np.abs(var[0])
            else:
                s = (V * V).sum(0)
                var = ys2 * (OS - s)
                E_var = ys2 * ((2 * aV * EV + EV * EV).sum(0) + g * s + 2 * U * OS) + 2 * U * np.abs(var)
            out["var"].append((var, E_var))
            if c.Ma and c.kern in ("linv_cov", "grad"):
                Xa = arr["Xa"] if grad else Xq[:c.Ma]
                A = LD(arr["VA"][t, :n, :c.Ma])
                Kaq, E_Kaq = columns(Xa, l, c.kind, xq, grad)
                dotAV = A.T @ V[:n]
                cov = ys2 * (Kaq - dotAV)
                E = ys2 * (E_Kaq + np.abs(A).T @ EV[:n] + g * (np.abs(A).T @ aV[:n]) + U * (np.abs(Kaq) + np.abs(dotAV))) + 2 * U * np.abs(cov)
                out["cov"].append((cov, E))
    res = {}
    for name, parts in out.items():
        if not parts:
            continue
        if grad:      # (Mq, 16) for mu / var, (Ma, Mq * 16) for cov, (N, Mq * 16) for V (never an output: kept for the stand-ins)
            cat = (lambda xs: np.stack(xs, 0)) if name in ("mu", "var") else (lambda xs: np.concatenate(xs, 1))
            ref, bound = cat([p[0] for p in parts]), cat([p[1] for p in parts])
        else:
            ref, bound = parts[0]
        res[name] = Quantity(ref, bound, 0.0)
    fin = {}
    for name, qn in res.items():
        if name in ("var", "cov") and not grad:
            fin[name] = qn._replace(scale=OS * float(ys2))
        elif grad and name != "V":
            # value columns and derivative columns are different quantities (the latter carry 1 / length): each gets its own scale
            val = np.zeros(qn.ref.shape, dtype=bool)
            val[..., 0::16] = True
            sv = OS * float(ys2) if name in ("var", "cov") else _scale(qn.ref[val])
            fin[name] = qn._replace(scale=np.where(val, sv, _scale(qn.ref[~val])))
        else:
            fin[name] = qn._replace(scale=_scale(qn.ref))
    return fin


# ------------------------------------------------------------------------------------------------------------------
# shared assertions
class Ratios(dict):
    """(kernel, output) -> [largest error / bound, largest bound / scale] seen, for profiles/posterior_bounds_notes.md."""

    def note(self, key, err_ratio, cap_ratio):
        cur = self.setdefault(key, [0.0, 0.0])
        cur[0], cur[1] = max(cur[0], err_ratio), max(cur[1], cap_ratio)


RATIOS = Ratios()


def assert_within(c: Case, t: int, name: str, got, q: Quantity, nan_mask=None):
    """|got - ref| <= bound elementwise, the bound itself at most CAP of the quantity's scale; entries under nan_mask must be NaN
    (and are NaN in the reference).  The first failing element is quoted."""
    got = np.asarray(got)
    ref, bound = np.broadcast_to(q.ref, got.shape), np.broadcast_to(q.bound, got.shape)
    assert got.shape == q.ref.shape, f"{case_id(c)} task {t} {name}: shape {got.shape} against {q.ref.shape}"
    live = np.ones(got.shape, dtype=bool) if nan_mask is None else ~np.broadcast_to(nan_mask, got.shape)
    if nan_mask is not None:
        assert np.isnan(got[~live]).all(), f"{case_id(c)} task {t} {name}: a non-finite query must give NaN, got {got[~live].ravel()[:4]}"
    scale = np.broadcast_to(q.scale, got.shape)
    over_cap = live & ~(bound <= CAP * scale)
    assert not over_cap.any(), (f"{case_id(c)} task {t} {name}: the bound {float(bound[over_cap].max()):.3e} exceeds {CAP} of the scale "
                                f"{float(scale[over_cap].max()):.3e} -- the input set is ill-chosen")
    err = np.abs(LD(got) - ref)
    bad = live & ~(err <= bound)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{case_id(c)} task {t} {name}{list(i)}: got {got[i]!r}, reference {float(ref[i])!r}, error {float(err[i]):.3e} "
                             f"> bound {float(bound[i]):.3e} ({int(bad.sum())} of {bad.size} elements)")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(live & (bound > 0), err / np.where(bound > 0, bound, 1), 0)
        cr = np.where(live & (scale > 0), bound / np.where(scale > 0, scale, 1), 0)
    RATIOS.note((c.kern, "rbf" if c.kind == KIND_RBF else "matern", name), float(r.max()) if r.size else 0.0, float(cr.max()) if cr.size else 0.0)


def nan_columns(c: Case, inp: dict, width: int):
    """Mask over an output's last axis (length `width`: M, or 16 Mq in GRAD layout) of the columns that belong to the NaN query."""
    if not c.nanq:
        return None
    m = np.zeros(width, dtype=bool)
    qn = c.M - 2
    if c.kern == "grad":
        m[16 * qn:16 * qn + 16] = True
    else:
        m[qn] = True
    return m


def check_task(c: Case, inp: dict, arr: dict, t: int, got: dict, v_nan=True):
    """Every output of the case's kernel for task t against its reference.  got: name -> the task's slice (numpy).  v_nan: whether
    the NaN query's column of V is NaN too (the substitution kernel) or unspecified (the explicit-inverse pass)."""
    refs = task_reference(c, arr, t)
    n = counts(c, inp)[t]
    for name, arr_got in got.items():
        if arr_got is None:
            continue
        q = refs[name]
        if name == "Linv":
            lower = c.kern == "linvmat_lower"
            blk = np.arange(c.N) // 16
            above = blk[:, None] < blk[None, :]
            if lower:      # block rows above a strip's diagonal block are not written
                assert (arr_got[above] == SENTINEL).all(), f"{case_id(c)} task {t}: the lower-only inverse wrote above its diagonal blocks"
                arr_got = np.where(above, 0.0, arr_got)
            assert (arr_got[np.triu_indices(c.N, 1)] == 0).all(), f"{case_id(c)} task {t}: Linv is not zero above the diagonal"
            assert (arr_got[n:] == np.eye(c.N)[n:]).all(), f"{case_id(c)} task {t}: rows past n_t of Linv are not identity rows"
            assert_within(c, t, name, arr_got, q)
            continue
        if c.kern == "grad" and name in ("mu", "var"):      # (Mq, 16) -> the strips side by side, as cov has them
            arr_got = arr_got.reshape(-1)
            q = Quantity(q.ref.reshape(-1), q.bound.reshape(-1), np.broadcast_to(q.scale, q.ref.shape).reshape(-1))
        mask = nan_columns(c, inp, arr_got.shape[-1])
        if name == "V":
            tail = arr_got[n:] if mask is None else arr_got[n:][:, ~mask]      # (0 * NaN: the NaN query's column is NaN throughout)
            assert (tail == 0).all(), f"{case_id(c)} task {t}: rows >= n_t of V are not exactly zero"
            if mask is not None:
                if v_nan:
                    assert np.isnan(arr_got[:n][:, mask]).all(), f"{case_id(c)} task {t}: V of a non-finite query must be NaN"
                keep = ~mask
                assert_within(c, t, name, arr_got[:, keep], Quantity(q.ref[:, keep], q.bound[:, keep], q.scale))
                continue
        if c.kern == "grad":
            dead = np.zeros(arr_got.shape[-1], dtype=bool)
            for col in range(1 + c.D, 16):
                dead[col::16] = True
            if mask is not None:
                dead &= ~mask
            assert (arr_got[..., dead] == 0).all(), f"{case_id(c)} task {t} {name}: GRAD columns 1 + D .. 15 are not exactly zero"
        if n == 0 and name in ("mu", "var") and c.kern != "grad" and mask is None:      # the posterior is the prior, exactly
            ym = 0.0 if inp["y_mean"] is None else inp["y_mean"][t]
            ys = 1.0 if inp["y_std"] is None else inp["y_std"][t]
            want = ym if name == "mu" else ys * ys * OS
            assert (arr_got == want).all(), f"{case_id(c)} task {t} {name}: n_t = 0 must give the prior {want!r} exactly, got {arr_got.ravel()[:3]}"
        assert_within(c, t, name, arr_got, q, mask)
