"""Long-double reference, a-priori forward error bound, input sets and shared assertions for the joint q-point acquisition kernels
scaml_target_qacqf_f64 (7p), scaml_target_qacqf_pending_f64 (7q) and scaml_target_qacqf_value_f64 (7r) of include/scaml_gp.h: one
body, qa_batch / qa_tail of csrc/gp_qacqf.h.

Same construction as tests/_fantasy_bounds.py and tests/_target_bounds.py (whose helpers are used here).  The reference is numpy long
double, fed exactly the arrays the entry point is handed, in that entry point's layout (GRAD: 16 columns per point of cov_g / mu_g /
var_g, batch b at columns b q ..; VALUE: one column per point, the packing of csrc/gp_qacqf_columns.h); one function serves the three
entry points (p >= 0 pending points, a switch between the layouts).  It follows the header's order: mu and Sigma (mixed block and
the given Sigma_pp included), the factor of Sigma + jitter I at the rung the reference's OWN ladder picks, f = mu + C eps, the
utility, the lowest-index arg-max and the sub-gradient rules, mubar, Cbar, Phi, Sigmabar, the gradient with its weights on training,
pending and mate rows.  The value is piecewise linear in (mu, C) once the winners are fixed, so the bound is first order through a
linear chain, every term from the reference's own quantities, every constant counted from the statements of csrc/gp_qacqf.h.  With
u = 2^-53, g_k = k u / (1 - k u), Q = q + p, R = n + p + q, chunk = ceil(S / 4):

  mu_j       n sequential fmas from mean_q, one fma with s and m:  E_mu = s g_n (|mean_q| + |Knq|^T |alpha|) + u |mu|;  mu_p is given
  d2         df = (x - x') / l (a subtraction, a division), D fmas:  E_d2 = g_{D+4} d2
  k, dk      sa_kernel_and_slope, os included:  E_k = os (S' E_d2 + c u |k|), E_dk = os (S'' E_d2 + c u |dk|), S' / S'' the suprema of
             tests/_posterior_bounds.py; c = 4 (RBF: exp within EXP_U = 2 ulp, the product with os, one to spare); Matern-5/2, counted
             from its statements with t = sqrt(5) r:  c = 3 t + 10  (r, the rounded sqrt(5) and their product reach exp's argument as
             3 u t; exp EXP_U, os 1; the polynomial 6, the last product 1)
  Sigma_jk   kz by n fmas:  E_kz = g_n |Knq_j|^T |Z_k|;  cg = cov / s^2 by s * s, 1 / s2 and a product: 3 u |cg|;  prior = cg + k:
             E_prior = 3 u |cg| + E_k + u |prior|  (exactly var_q on the diagonal);  v = s2 (prior - kz):
             E_Sigma = s^2 (E_prior + E_kz + u |prior - kz|) + 2 u |v|;  the mixed block the same statement with Zp;  Sigma_pp is given
  factor     on the diagonal + jitter is one more rounding, u |Sigma_jj + jitter|;  Cholesky's backward error:
             dSigma <= E_Sigma + g_{Q+1} |C| |C^T|;  to first order  E_C = |C| tril_half(|C^-1| dSigma |C^-T|)  (strict lower triangle
             and half the diagonal);  E_Cinv = |C^-1| E_C |C^-1| + g_Q |C^-1| |C| |C^-1|
  pivots     pivot k is the Schur complement Sigma_kk + jitter - c^T A^-1 c of the leading block A:  with w = A^-1 c,
             E_piv = dS_kk + 2 |w|^T dS_{:k,k} + |w|^T dS_{:k,:k} |w|, dS as above from the k + 1 rows factored so far
  z_j        j + 1 fmas:  E_z = |eps|^T E_C_j + g_{j+1} |C_j| |eps|
  utility    qEI  g = best_f - (mu + z):  E_g = E_mu + E_z + u |mu + z| + u |g|
             qUCB g = c |z| - mu, c = sqrt(beta pi / 2) (the rounded constant, the product, the root: 2 u c):
             E_g = c E_z + 3 u c |z| + E_mu + u |g|
  value      E = (sum_s E_a + g_{chunk+3} sum_s |a_s|) / S   (chunk - 1 additions, two levels of the four chunks, 1 / S and its
             product);  a clamped sample (qEI, best <= 0) adds exactly 0
  mubar      sums of -1 and 0 are exact:  E_mbar = 2 u |mubar|  (1 / S and its product)
  Cbar       E = g_{chunk+3+w} sum_s |wc eps| / S,  w = 3 under qUCB (wc = +-c carries 2 u, the product 1), 0 under qEI
  Phi        tril(C^T Cbar), at most 8 fmas:  E_Phi = tril(E_C^T |Cbar| + |C^T| E_Cbar + g_8 |C^T| |Cbar|), diagonal halved exactly
  Sigmabar   X = Phi C^-1:  E_X = E_Phi |C^-1| + |Phi| E_Cinv + g_8 |Phi| |C^-1|;   Y = C^-T X likewise;
             Sigmabar = (Y + Y^T) / 2:  E_Sbar = (E_Y + E_Y^T) / 2 + u |Sigmabar|
  weights    training row a:  sz = Sbar_j . (Z_a, Zp_a) by Q fmas, u_ja = s mbar_j alpha_a - 2 s^2 sz:
             E_u = s |alpha_a| E_mbar_j + 2 s^2 (E_Sbar_j . |Z_a| + g_Q |Sbar_j| . |Z_a|) + 2 u |s mbar_j alpha_a| + 2 u |2 s^2 sz| + u |u_ja|
             pending / mate row:  u = 2 s^2 Sbar_jk (0 for the point itself):  E_u = 2 s^2 E_Sbar_jk + 2 u |u|
             U = u / s^2:  E_U = E_u / s^2 + 3 u |U|;   SL = 2 u dk:  E_SL = 2 (E_u |dk| + |u| E_dk) + u |SL|
  grad       acc = fma(mbar, mu_g, Sbar_jj var_g), then 2 R fmas against cov_g and w_a = (x_j - x_a) / l^2 (a subtraction, l * l, 1 / .,
             a product: 4 u):  E = E_mbar |mu_g| + E_Sbar_jj |var_g| + sum_a (E_U |cov_g| + E_SL |w_a| + 4 u |SL w_a|)
             + g_{2R+2} (|mbar mu_g| + |Sbar_jj var_g| + sum_a (|U cov_g| + |SL w_a|))

Where the kernel was followed against the issue's reading: `df` is a division by theta[d] and the slope's coordinate factor a
product with 1 / (l * l) (counted as such); Matern's c grows with the distance (3 t + 10, not the 4 of the posterior kernels);
a rejected rung is not abandoned at its failing pivot -- the loop runs on over NaN and only `ok` records it, so one failing pivot per
rejected rung is all the ladder needs; qUCB's |z_b| condition is waived at beta = 0, where both slopes are the same +-0.

Second order: every bound is multiplied by 1 / (1 - 1e-6), and max | |C^-1| dSigma |C^-T| | <= 1e-6 is asserted on the inputs.

Conditions on the inputs, asserted with every comparison (conditions, not measurements; no sample is left out): for every sample
the winner's utility is at least MARGIN = 1e3 (E_winner + E_j) above every other entry j; under qEI |best| >= MARGIN E_best, under qUCB
|z_b| >= MARGIN E_z; every pivot of the chosen rung and the failing pivot of every rejected rung is at least MARGIN E_piv from 0 -- then
rung, winners and clamps of kernel and reference provably coincide; every bound at most CAP = 1e-8 of the output's largest reference
magnitude in the call (the ladder sets, whose condition number the rung sets: the north star 1e-4; a set whose reference is all
zero: against sqrt(max Sigma_jj)).

Input sets: planted arrays, no model fit -- cov_g / cov_s and var_q are free inputs, so Sigma is planted with a chosen spectrum under
a random rotation.  Listed at SETS_7P, SETS_7Q, SETS_7R, COND_SETS and the check_* drivers below.  Backend: be.run(a, info) ->
(rc, value (B), grad (Mq, D) or None, jitter (B), info_out (B)), every output through a guarded buffer of SENTINEL.
"""
from __future__ import annotations

import numpy as np

from tests import _target_bounds as B
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, SENTINEL, U, Quantity, _kernel, _S, gamma, inverse_lower
from tests._target_bounds import FAMILY, within

UCB, EI = 0, 1
ACQ = {UCB: "qucb", EI: "qei"}
SECOND_ORDER = 1e-6
GUARD = 1.0 / (1.0 - SECOND_ORDER)
MARGIN = 1e3
NORTH_STAR = 1e-4
LADDER = (0.0, 1e-8, 1e-7, 1e-6)
ISENTINEL = -77
PI = LD(4) * np.arctan(LD(1))
M_ALL, S_ALL, BETA = 0.3, 1.7, 4.0
_SQRT5 = np.sqrt(LD(5))


# ------------------------------------------------------------------------------------------------------------------
# reference and bound
def columns(a, b):
    """The columns of batch b's q points in the entry point's layout."""
    q = a["q"]
    if a["layout"] == "value":
        bps = 16 // q
        return 16 * (b // bps) + (b % bps) * q + np.arange(q)
    return b * q + np.arange(q)


def value_columns(Bn, q):
    bps = 16 // q
    return 16 * ((Bn + bps - 1) // bps)


def _kern(d2, kind, os_):
    """os k, os dk and their bounds at squared scaled distance d2 (E_d2 = g_{D+4} d2 is handed to the returned function)."""
    k, dk = _kernel(d2, kind)
    c = LD(4) if kind == KIND_RBF else 3 * _SQRT5 * np.sqrt(np.maximum(d2, LD(1e-30))) + 10
    S0, S1 = _S[kind]

    def bounds(E_d2):
        return os_ * (S0 * E_d2 + c * U * np.abs(k)), os_ * (S1 * E_d2 + c * U * np.abs(dk))
    return os_ * k, os_ * dk, bounds


def _d2(xa, xb, l):
    df = (xa[:, None, :] - xb[None, :, :]) / l
    return (df * df).sum(-1)


def _chol(M):
    """Lower factor in long double and the first failing pivot: (C, None) or (partial C, k) with pivot k <= 0 or not finite."""
    Q = M.shape[0]
    C = np.zeros((Q, Q), dtype=LD)
    for k in range(Q):
        piv = M[k, k] - (C[k, :k] * C[k, :k]).sum()
        if not (piv > 0 and np.isfinite(piv)):
            return C, k
        C[k, k] = np.sqrt(piv)
        for i in range(k + 1, Q):
            C[i, k] = (M[i, k] - (C[i, :k] * C[k, :k]).sum()) / C[k, k]
    return C, None


def _pivot_margin(M, E_S, C, k):
    """|pivot k| / E_piv of the factorisation of M (rows < k of C are its factor so far)."""
    g = gamma(M.shape[0] + 1)
    row = C[k, :k]                     # (column by column: row k is complete up to the pivot, on a failing attempt too)
    piv = M[k, k] - (row * row).sum()
    Cp = np.zeros((k + 1, k + 1), dtype=LD)
    Cp[:k, :k], Cp[k, :k], Cp[k, k] = np.abs(C[:k, :k]), np.abs(row), np.sqrt(np.abs(piv))
    dS = E_S[:k + 1, :k + 1] + g * (Cp @ Cp.T)
    if k == 0:
        E = dS[0, 0]
    else:
        Li = inverse_lower(C[:k, :k])
        w = np.abs(Li.T @ (Li @ M[:k, k]))
        E = dS[k, k] + 2 * (w * dS[:k, k]).sum() + w @ dS[:k, :k] @ w
    return float(np.abs(piv) / (GUARD * E)) if E > 0 else np.inf


def _tril_half(X):
    return np.tril(X, -1) + np.diag(np.diag(X)) / 2


def _batch(a, b):
    """Reference and bounds of batch b: dict(value, E_value, grad (q, D), E_grad, jitter, info, cond: the conditions' figures)."""
    n, q, p, S, D, kind, acqf = a["n"], a["q"], a["p"], a["S"], a["D"], a["kind"], a["acqf"]
    Q, R = q + p, n + p + q
    val = a["layout"] == "value"
    CS = 1 if val else 16
    cols = columns(a, b)
    s, m_all, par = LD(a["s"]), LD(a["m"]), LD(a["param"])
    s2 = s * s
    th = LD(a["theta"])
    l, os_ = th[:D], th[D]
    K, Z, al = LD(a["Knq"][:, cols]), LD(a["Z"][:, cols]), LD(a["alpha"])
    cov = LD(a["cov"])
    Xb = LD(a["Xq"][cols])
    Xp = LD(a["Xp"]).reshape(p, D)
    Zall = np.concatenate([Z, LD(a["Zp"]).reshape(n, p)], 1)                               # (n, Q)
    aK, aZ = np.abs(K), np.abs(Zall)
    gn, gd = gamma(n), gamma(D + 4)
    cond = dict(second=0.0, pivot=np.inf, gap=np.inf, kink=np.inf)

    # ---- mu, Sigma
    mu = np.zeros(Q, dtype=LD)
    E_mu = np.zeros(Q, dtype=LD)
    acc = LD(a["mean_q"][cols]) + K.T @ al
    mu[:q] = m_all + s * acc
    E_mu[:q] = s * gn * (np.abs(LD(a["mean_q"][cols])) + aK.T @ np.abs(al)) + U * np.abs(mu[:q])
    mu[q:] = LD(a["mu_p"]).reshape(p)
    Xj = np.concatenate([Xb, Xp], 0)                                                       # the joint vector's points
    d2 = _d2(Xj, Xb, l)                                                                    # (Q, q)
    k0, _, kb = _kern(d2, kind, os_)
    E_k0 = kb(gd * d2)[0]
    kz = Zall.T @ K                                                                        # (Q, q): row j (a point's Z), column k (Knq)
    E_kz = gn * (aZ.T @ aK)
    Sg = np.zeros((Q, Q), dtype=LD)
    E_S = np.zeros((Q, Q), dtype=LD)
    for j in range(Q):
        for k in range(min(j + 1, q)):
            # moving j >= k: Knq_j . Z_k; pending j: Knq_k . Zp_j -- kz[j, k] = Zall_j . K_k holds the second, the first is its transpose
            dot, E_dot = (kz[k, j], E_kz[k, j]) if j < q else (kz[j, k], E_kz[j, k])
            if j == k:
                prior, E_prior = LD(a["var_q"][cols[j]]), LD(0)
            else:
                row = n + (j - q) if j >= q else n + p + k
                col = cols[k] if j >= q else cols[j]
                cg = cov[row, col * CS] / s2
                prior = cg + k0[j, k]
                E_prior = 3 * U * np.abs(cg) + E_k0[j, k] + U * np.abs(prior)
            v = s2 * (prior - dot)
            Sg[j, k] = Sg[k, j] = v
            E_S[j, k] = E_S[k, j] = s2 * (E_prior + E_dot + U * np.abs(prior - dot)) + 2 * U * np.abs(v)
    Sg[q:, q:] = LD(a["Sigma_pp"]).reshape(p, p)
    out = dict(mu=mu, Sigma=Sg, cond=cond, sigma_max=float(np.sqrt(np.abs(np.diag(Sg)).max())))

    # ---- the ladder
    C = None
    for jit in LADDER:
        M = Sg + LD(jit) * np.eye(Q, dtype=LD)
        E_M = E_S + np.diag(U * np.abs(np.diag(M))) if jit else E_S
        Ct, fail = _chol(M)
        if fail is not None:
            cond["pivot"] = min(cond["pivot"], _pivot_margin(M, E_M, Ct, fail))
            continue
        C, E_SM = Ct, E_M
        for k in range(Q):
            cond["pivot"] = min(cond["pivot"], _pivot_margin(M, E_M, C, k))
        break
    nanq = np.full((q, D), np.nan, dtype=LD)
    if C is None:
        out.update(value=LD(np.nan), E_value=LD(0), grad=nanq, E_grad=nanq, jitter=np.nan, info=1)
        return out
    aC = np.abs(C)
    Ci = inverse_lower(C)
    aCi = np.abs(Ci)
    dS = E_SM + gamma(Q + 1) * (aC @ aC.T)
    W = aCi @ dS @ aCi.T
    cond["second"] = float(W.max())
    E_C = GUARD * (aC @ _tril_half(W))
    E_C = np.tril(E_C)
    E_Ci = GUARD * (aCi @ E_C @ aCi + gamma(Q) * (aCi @ aC @ aCi))
    E_Ci = np.tril(E_Ci)

    # ---- the samples
    eps = LD(a["eps"])                                                                     # (S, Q)
    ae = np.abs(eps)
    z = eps @ C.T
    gj = np.array([gamma(j + 1) for j in range(Q)])
    E_z = ae @ E_C.T + gj * (ae @ aC.T)
    if acqf == EI:
        f = mu + z
        g = par - f
        E_g = E_mu + E_z + U * np.abs(f) + U * np.abs(g)
        cu = LD(0)
    else:
        cu = np.sqrt(par * PI / 2)
        g = cu * np.abs(z) - mu
        E_g = cu * E_z + 3 * U * cu * np.abs(z) + E_mu + U * np.abs(g)
    E_g = GUARD * E_g
    jb = np.argmax(g, 1)                                                                   # (lowest index among equals)
    rows = np.arange(S)
    best, E_best, zb = g[rows, jb], E_g[rows, jb], z[rows, jb]
    if Q > 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = (best[:, None] - g) / (E_best[:, None] + E_g)
        gap[rows, jb] = np.inf
        cond["gap"] = float(gap.min())
    if acqf == EI:
        on = best > 0
        with np.errstate(divide="ignore"):
            cond["kink"] = float((np.abs(best) / E_best).min())
        av, E_a = np.where(on, best, 0), np.where(on, E_best, 0)
        wm = np.where(on, LD(-1), LD(0))
        wc = wm
    else:
        if cu > 0:
            with np.errstate(divide="ignore"):
                cond["kink"] = float((np.abs(zb) / (GUARD * E_z[rows, jb])).min())
        av, E_a = best, E_best
        wm = np.full(S, LD(-1))
        wc = np.sign(zb) * cu
    out["winners"], out["clamped"] = jb, (int((~on).sum()) if acqf == EI else 0)
    chunk = (S + 3) // 4
    value = av.sum() / S
    E_value = GUARD * (E_a.sum() + gamma(chunk + 3) * np.abs(av).sum()) / S
    out.update(value=value, E_value=E_value, jitter=float(jit), info=0)
    if val:
        return out

    # ---- the adjoint
    onehot = (jb[:, None] == np.arange(Q)[None, :])                                        # (S, Q)
    mb = (onehot * wm[:, None]).sum(0) / S
    E_mb = 2 * U * np.abs(mb)
    Cb = np.tril((onehot * wc[:, None]).T @ eps) / S
    E_Cb = gamma(chunk + 3 + (3 if acqf == UCB else 0)) * np.tril((onehot * np.abs(wc)[:, None]).T @ ae) / S
    Phi = _tril_half(np.tril(C.T @ Cb))
    E_Phi = _tril_half(np.tril(E_C.T @ np.abs(Cb) + aC.T @ E_Cb + gamma(8) * (aC.T @ np.abs(Cb))))
    X = Phi @ Ci
    E_X = E_Phi @ aCi + np.abs(Phi) @ E_Ci + gamma(8) * (np.abs(Phi) @ aCi)
    Y = Ci.T @ X
    E_Y = E_Ci.T @ np.abs(X) + aCi.T @ E_X + gamma(8) * (aCi.T @ np.abs(X))
    Sb = (Y + Y.T) / 2
    E_Sb = GUARD * ((E_Y + E_Y.T) / 2 + U * np.abs(Sb))
    out.update(mubar=mb, Sigmabar=Sb)

    # ---- the gradient of the q moving points
    Xall = np.concatenate([LD(a["Xt"]), Xp, Xb], 0)                                        # (R, D)
    d2g = _d2(Xb, Xall, l)                                                                 # (q, R)
    _, dk, kb = _kern(d2g, kind, os_)
    E_dk = kb(gd * d2g)[1]
    u = np.zeros((q, R), dtype=LD)
    E_u = np.zeros((q, R), dtype=LD)
    sz = Sb[:q] @ Zall.T                                                                   # (q, n)
    E_sz = E_Sb[:q] @ aZ.T + gamma(Q) * (np.abs(Sb[:q]) @ aZ.T)
    t1 = s * mb[:q, None] * al[None, :]
    t2 = 2 * s2 * sz
    u[:, :n] = t1 - t2
    E_u[:, :n] = s * E_mb[:q, None] * np.abs(al)[None, :] + 2 * s2 * E_sz + 2 * U * np.abs(t1) + 2 * U * np.abs(t2) + U * np.abs(u[:, :n])
    um = 2 * s2 * np.concatenate([Sb[:q, q:], Sb[:q, :q]], 1)                              # pending rows, then mate rows
    E_um = 2 * s2 * np.concatenate([E_Sb[:q, q:], E_Sb[:q, :q]], 1) + 2 * U * np.abs(um)
    for j in range(q):
        um[j, p + j] = E_um[j, p + j] = 0
    u[:, n:], E_u[:, n:] = um, E_um
    Uw = u / s2
    E_U = E_u / s2 + 3 * U * np.abs(Uw)
    SL = 2 * u * dk
    E_SL = 2 * (E_u * np.abs(dk) + np.abs(u) * E_dk) + U * np.abs(SL)
    mu_g = LD(a["mu_g"]).reshape(-1, 16)[cols][:, 1:1 + D]                                 # (q, D)
    var_g = LD(a["var_g"]).reshape(-1, 16)[cols][:, 1:1 + D]
    cg = cov.reshape(R, -1, 16)[:, cols][:, :, 1:1 + D]                                    # (R, q, D)
    w = (Xb[:, None, :] - Xall[None, :, :]) / (l * l)                                      # (q, R, D)
    dSb = np.diag(Sb)[:q, None]
    terms = np.abs(mb[:q, None] * mu_g) + np.abs(dSb * var_g) + np.einsum("ja,ajd->jd", np.abs(Uw), np.abs(cg)) \
        + np.einsum("ja,jad->jd", np.abs(SL), np.abs(w))
    grad = mb[:q, None] * mu_g + dSb * var_g + np.einsum("ja,ajd->jd", Uw, cg) + np.einsum("ja,jad->jd", SL, w)
    E_grad = E_mb[:q, None] * np.abs(mu_g) + np.diag(E_Sb)[:q, None] * np.abs(var_g) + np.einsum("ja,ajd->jd", E_U, np.abs(cg)) \
        + np.einsum("ja,jad->jd", E_SL + 4 * U * np.abs(SL), np.abs(w)) + gamma(2 * R + 2) * terms
    out.update(grad=grad, E_grad=GUARD * E_grad)
    return out


_REFS = {}


def reference(a: dict) -> dict:
    """a: the arguments of the entry point (numpy; a["layout"]: "grad" or "value") -> value / grad Quantities, the exact jitter and info,
    and the conditions' figures (the worst over the batches).  Computed once per set (a["name"]) and never changed."""
    if a.get("name") in _REFS:
        return _REFS[a["name"]]
    Bn, q, D = a["B"], a["q"], a["D"]
    bs = [_batch(a, b) for b in range(Bn)]
    value = np.array([x["value"] for x in bs], dtype=LD)
    E_value = np.array([x["E_value"] for x in bs], dtype=LD)
    sig = max(x["sigma_max"] for x in bs)
    vs = B._scale(value)
    ref = dict(value=Quantity(value, E_value, vs if vs > 0 else sig), jitter=np.array([x["jitter"] for x in bs]),
               info=np.array([x["info"] for x in bs], dtype=np.int32), failed=np.array([x["info"] == 1 for x in bs]), batches=bs, sigma=sig,
               cond={k: (max if k == "second" else min)(x["cond"][k] for x in bs) for k in ("second", "pivot", "gap", "kink")})
    if a["layout"] == "grad":
        grad = np.concatenate([x["grad"] for x in bs], 0)
        gs = B._scale(grad)
        ref["grad"] = Quantity(grad, np.concatenate([x["E_grad"] for x in bs], 0), gs if gs > 0 else sig)
    if a.get("name"):
        _REFS[a["name"]] = ref
    return ref


def conditions(label, ref):
    """The conditions on the inputs: first order is enough, and rung, winners and clamps of kernel and reference coincide."""
    c = ref["cond"]
    assert c["second"] <= SECOND_ORDER, f"{label}: | |C^-1| dSigma |C^-T| | = {c['second']:.3e} > {SECOND_ORDER} -- the input set is ill-chosen"
    assert c["pivot"] >= MARGIN, f"{label}: a pivot within {c['pivot']:.3e} of its bound from 0 -- the input set is ill-chosen"
    assert c["gap"] >= MARGIN, f"{label}: two utilities within {c['gap']:.3e} of their bounds -- the input set is ill-chosen"
    assert c["kink"] >= MARGIN, f"{label}: a sample within {c['kink']:.3e} of its bound from the kink -- the input set is ill-chosen"


def key(a, name):
    return ("qacqf", f"{a['entry']}/{FAMILY[a['kind']]}/{ACQ[a['acqf']]}", name)


def report():
    return B.report("qacqf") + B.report("qacqf_chain")


def _within(label, k, got, q, mask, up):
    """tests/_target_bounds.within with the cap at `up` CAP: the scale is handed over `up` times as large, and the table's bound / scale
    is put back into the output's own units."""
    old = B.RATIOS.get(k, [0.0, 0.0])[1]
    within(label, k, got, q._replace(scale=q.scale * up), mask)
    if up != 1:
        fin = np.isfinite(q.bound)
        B.RATIOS[k][1] = max(old, float(q.bound[fin].max() / q.scale) if fin.any() and q.scale > 0 else 0.0)


def hold(label, a, ref, got, cap=CAP, k=None):
    """The shared assertion: the conditions, then value and grad element by element within their bounds (each bound at most `cap` of the
    output's scale), jitter and info exactly.  got: (rc, value, grad, jitter, info_out).  A failed batch (no rung of the ladder) is NaN
    in value, jitter and its q rows of grad, info 1."""
    rc, value, grad, jitter, info = got
    assert rc == 0, f"{label}: return code {rc}"
    conditions(label, ref)
    k = k or (lambda name: key(a, name))
    failed = ref["failed"]
    up = cap / CAP                                                                         # (within() caps at CAP of the scale)
    qv = ref["value"]
    _within(label, k("value"), value, qv, failed if failed.any() else None, up)
    assert np.array_equal(jitter, ref["jitter"], equal_nan=True), f"{label}: jitter {jitter} against {ref['jitter']}"
    assert np.array_equal(info, ref["info"]), f"{label}: info {info} against {ref['info']}"
    if a["layout"] == "grad" and grad is not None:
        qg = ref["grad"]
        gmask = np.repeat(failed, a["q"])[:, None] if failed.any() else None
        _within(label, k("grad"), grad, qg, gmask, up)


# ------------------------------------------------------------------------------------------------------------------
# input sets
def _rng(*seed):
    return np.random.default_rng([20261021, *seed])


def _rotation(rng, k):
    Qm, Rm = np.linalg.qr(rng.normal(size=(k, k)))
    return Qm * np.sign(np.diag(Rm))


def _spectrum(rng, k, lo, hi):
    ev = np.geomspace(lo, hi, k) if k > 1 else np.array([0.7])
    Qm = _rotation(rng, k)
    M = (Qm * ev) @ Qm.T
    return 0.5 * (M + M.T)


def _k64(xa, xb, th, D, kind):
    d2 = _d2(xa, xb, th[:D])
    return th[D] * _kernel(d2, kind)[0]


def plant(a, b, Sigma):
    """Write var_q and the value columns of cov so that batch b's joint covariance is Sigma (Q, Q) to fp64 rounding (its pending block
    must be a["Sigma_pp"])."""
    n, q, p, D, kind = a["n"], a["q"], a["p"], a["D"], a["kind"]
    CS = 1 if a["layout"] == "value" else 16
    cols = columns(a, b)
    s2 = a["s"] * a["s"]
    K, Z = a["Knq"][:, cols], a["Z"][:, cols]
    Xb = a["Xq"][cols]
    kmm = _k64(Xb, Xb, a["theta"], D, kind)
    for j in range(q):
        a["var_q"][cols[j]] = Sigma[j, j] / s2 + K[:, j] @ Z[:, j]
        for k in range(j):
            a["cov"][n + p + k, cols[j] * CS] = s2 * (Sigma[j, k] / s2 + K[:, j] @ Z[:, k] - kmm[j, k])
    if p:
        kpm = _k64(a["Xp"], Xb, a["theta"], D, kind)
        for jp in range(p):
            for k in range(q):
                a["cov"][n + jp, cols[k] * CS] = s2 * (Sigma[q + jp, k] / s2 + K[:, k] @ a["Zp"][:, jp] - kpm[jp, k])


def joint_sigma(rng, q, p, Spp, lo, hi):
    """A (q + p)-point covariance with the given pending block: [[A, Bm], [Bm^T, Spp]], A = Bm Spp^-1 Bm^T + a Schur complement of
    spectrum lo .. hi."""
    if p == 0:
        return _spectrum(rng, q, lo, hi)
    Bm = 0.3 * rng.normal(size=(q, p))
    A = Bm @ np.linalg.solve(Spp, Bm.T) + _spectrum(rng, q, lo, hi)
    M = np.block([[A, Bm], [Bm.T, Spp]])
    return 0.5 * (M + M.T)


def utilities64(a):
    """fp64: the smallest f = mu + C eps over the points, per batch and sample (for placing best_f); needs PD Sigma."""
    outs = []
    for b in range(a["B"]):
        x = _batch(dict(a, acqf=UCB, param=0.0, layout=a["layout"]), b)
        C = np.linalg.cholesky(x["Sigma"].astype(np.float64))
        outs.append((x["mu"].astype(np.float64) + a["eps"] @ C.T).min(1))
    return np.array(outs)


def inputs(entry, n, q, p, S, D, Bn, kind, acqf, cond=100.0, best="bulk", beta=BETA, seed=0, name=None) -> dict:
    """Xt, Xq, Xp uniform in the unit cube, theta = (l in 0.3 .. 1.3 times sqrt(D) / 2 + 1 / 2, os 1.3, noise 1e-3), Knq = 0.3 randn,
    Z, Zp = 0.01 randn, alpha = randn / sqrt(n), mean_q, mu_p = randn, cov = 0.1 randn and mu_g, var_g = randn in ALL their columns (the
    kernel may read only the ones the header names), base samples randn; Sigma planted per batch with eigenvalues 5 / cond .. 5 under
    a random rotation.  qEI: best_f at the 40 % quantile of the samples' smallest f ("bulk": a good share of the samples is clamped)
    or 1 below every sample ("below"); qUCB: beta.  entry "7r": the VALUE layout, padding columns full of SENTINEL."""
    rng = _rng(seed, n, q, p, S, D, Bn, kind)
    Q, R = q + p, n + p + q
    val = entry == "7r"
    Mq = value_columns(Bn, q) if val else Bn * q
    W = Mq if val else Mq * 16
    th = np.concatenate([rng.uniform(0.3, 1.3, size=D) * (0.5 * np.sqrt(D) + 0.5), [1.3, 1e-3]])
    a = dict(entry=entry, layout="value" if val else "grad", n=n, q=q, p=p, S=S, D=D, B=Bn, kind=kind, acqf=acqf, m=M_ALL, s=S_ALL,
             name=name, Knq=0.3 * rng.normal(size=(n, Mq)), Z=0.01 * rng.normal(size=(n, Mq)), alpha=rng.normal(size=n) / np.sqrt(n),
             mean_q=rng.normal(size=Mq), var_q=np.zeros(Mq), cov=0.1 * rng.normal(size=(R, W)), Xt=rng.uniform(size=(n, D)),
             Xq=rng.uniform(size=(Mq, D)), theta=th, eps=rng.normal(size=(S, Q)), Xp=rng.uniform(size=(p, D)),
             Zp=0.01 * rng.normal(size=(n, p)), mu_p=rng.normal(size=p), Sigma_pp=np.zeros((p, p)),
             mu_g=None if val else rng.normal(size=Mq * 16), var_g=None if val else rng.normal(size=Mq * 16))
    if p:
        a["Sigma_pp"] = _spectrum(rng, p, 0.2, 2.0)
    for b in range(Bn):
        plant(a, b, joint_sigma(rng, q, p, a["Sigma_pp"], 5.0 / cond, 5.0))
    if val:                                                                                # padding columns: nothing may read them
        pad = np.ones(Mq, dtype=bool)
        for b in range(Bn):
            pad[columns(a, b)] = False
        for k in ("Knq", "Z", "cov"):
            a[k][:, pad] = SENTINEL
        for k in ("mean_q", "var_q", "Xq"):
            a[k][pad] = SENTINEL
    if acqf == UCB:
        a["param"] = float(beta)
    else:
        fmin = utilities64(a)
        a["param"] = float(np.round(np.quantile(fmin, 0.4), 3)) if best == "bulk" else float(np.floor(fmin.min()) - 1.0)
    return a


def to_value_layout(a) -> dict:
    """The same numbers as the GRAD-layout set `a` in the VALUE layout of (7r): column col(b, j) holds point j of batch b, cov_s the
    value columns of cov_g, padding columns SENTINEL."""
    n, q, p, Bn = a["n"], a["q"], a["p"], a["B"]
    Mp = value_columns(Bn, q)
    v = dict(a, entry="7r", layout="value", mu_g=None, var_g=None, name=None if a.get("name") is None else a["name"] + "/value")
    v["Knq"], v["Z"], v["cov"] = (np.full((r, Mp), SENTINEL) for r in (n, n, n + p + q))
    v["mean_q"], v["var_q"], v["Xq"] = np.full(Mp, SENTINEL), np.full(Mp, SENTINEL), np.full((Mp, a["D"]), SENTINEL)
    for b in range(Bn):
        src, dst = columns(a, b), columns(v, b)
        for k in ("Knq", "Z"):
            v[k][:, dst] = a[k][:, src]
        v["cov"][:, dst] = a["cov"][:, src * 16]
        for k in ("mean_q", "var_q", "Xq"):
            v[k][dst] = a[k][src]
    return v


def set_id(c):
    return "-".join(f"{k}{v}" for k, v in zip(("n", "q", "p", "S", "D", "B"), c))


#          n   q  p  S    D   B
SETS_7P = ((1, 1, 0, 1, 1, 1), (17, 3, 0, 5, 2, 5), (9, 5, 0, 257, 6, 2), (20, 4, 0, 2, 6, 3), (33, 7, 0, 3, 15, 2), (90, 6, 0, 509, 15, 2),
           (88, 8, 0, 512, 15, 1))
SETS_7Q = ((17, 2, 3, 300, 2, 5), (8, 1, 7, 511, 6, 3), (20, 7, 1, 64, 6, 3), (83, 5, 3, 257, 15, 2), (88, 3, 5, 512, 15, 1))
#          every q of the packing that is not dense, a last strip that is not full; (88, 2, 6, 512): n + p + q = 96 at S = 512
SETS_7R = ((9, 3, 0, 64, 6, 7), (20, 5, 3, 64, 6, 4), (17, 6, 1, 5, 2, 3), (20, 7, 1, 64, 6, 2), (9, 1, 0, 257, 6, 17), (20, 8, 0, 64, 6, 3),
           (88, 2, 6, 512, 15, 16))
LARGEST = {"7p": (88, 8, 0, 512, 15, 1), "7q": (88, 3, 5, 512, 15, 1), "7r": (88, 2, 6, 512, 15, 16)}
COND_SHAPE = (20, 8, 0, 64, 6, 2)
CONDS = (1e2, 1e4)
LADDER_EIGS = (1e-2, -5e-9, -5e-8, -5e-7, -1e-5)
KINDS = (KIND_RBF, KIND_MATERN52)
CODES = (UCB, EI)
_SETS = {}


def make(entry, shape, kind, acqf, **kw):
    """A set by its name, built once."""
    name = f"{entry}-{set_id(shape)}-{FAMILY[kind]}-{ACQ[acqf]}" + "".join(f"-{k}={v}" for k, v in sorted(kw.items()))
    if name not in _SETS:
        _SETS[name] = inputs(entry, *shape, kind, acqf, name=name, **kw)
    return _SETS[name]


def ladder_inputs(kind, acqf, with_last=True) -> dict:
    """One call of five batches with q = 3 (n = 5, S = 64, D = 2): the smallest eigenvalue of Sigma planted at LADDER_EIGS, the other
    two at 0.1 and 0.4 (with them | |C^-1| dSigma |C^-T| | stays under 1e-6 on the 1e-8 rung).  with_last = False: the first four batches alone, the same numbers."""
    name = f"ladder-{FAMILY[kind]}-{ACQ[acqf]}-{with_last}"
    if name in _SETS:
        return _SETS[name]
    a = inputs("7p", 5, 3, 0, 64, 2, 5, kind, UCB, name=None)
    a["theta"][2] = 1e-3           # os: the rounding of an off-diagonal entry then scales with Sigma, not with os k_t(x_j, x_k)
    rng = _rng(77, kind)
    for b, lam in enumerate(LADDER_EIGS):
        Qm = _rotation(rng, 3)
        M = (Qm * np.array([lam, 0.1, 0.4])) @ Qm.T
        plant(a, b, 0.5 * (M + M.T))
    a.update(acqf=acqf, param=BETA if acqf == UCB else float(a["m"]), name=name)
    if not with_last:
        for k in ("Knq", "Z"):
            a[k] = np.ascontiguousarray(a[k][:, :12])
        for k in ("mean_q", "var_q", "Xq"):
            a[k] = np.ascontiguousarray(a[k][:12])
        a["cov"] = np.ascontiguousarray(a["cov"][:, :12 * 16])
        a["mu_g"], a["var_g"] = a["mu_g"][:12 * 16].copy(), a["var_g"][:12 * 16].copy()
        a["B"] = 4
    _SETS[name] = a
    return a


# ------------------------------------------------------------------------------------------------------------------
# drivers
def check_set(be, a, label, infos=(None, 0, 2), cap=CAP):
    ref = reference(a)
    for info in infos:
        got = be.run(a, info)
        if info:
            rc, value, grad, jitter, info_out = got
            assert rc == 0, f"{label}: return code {rc}"
            assert np.isnan(value).all() and np.isnan(jitter).all() and (info_out == 1).all() and (grad is None or np.isnan(grad).all()), \
                f"{label}: info = {info} must give NaN everywhere and info_out 1"
        else:
            hold(f"{label}-info{info}", a, ref, got, cap)
    return ref


def check_shape(be, entry, shape, kind):
    """Both codes (qEI with best_f in the bulk), info NULL / 0 / 2.  be.run asserts that every entry of every output is written and
    nothing behind it."""
    for acqf in CODES:
        a = make(entry, shape, kind, acqf)
        ref = check_set(be, a, a["name"])
        if acqf == EI and a["S"] * a["B"] >= 64:
            cl = sum(x["clamped"] for x in ref["batches"])
            assert 0.1 * a["S"] * a["B"] <= cl <= 0.9 * a["S"] * a["B"], f"{a['name']}: {cl} samples clamped -- best_f is not in the bulk"


def check_value_layout(be, shape, kind):
    """(7r) within its bound, and value, jitter and info bit-equal to the gradient kernel's on the same numbers in the GRAD layout
    ((7q), or (7p) when nothing is pending)."""
    for acqf in CODES:
        g = make("7q" if shape[2] else "7p", shape, kind, acqf)
        v = to_value_layout(g)
        check_set(be, v, v["name"])
        rv, rg = be.run(v, None), be.run(g, None)
        for i, what in ((1, "value"), (3, "jitter"), (4, "info")):
            assert np.array_equal(rv[i], rg[i]), f"{v['name']}: {what} differs from the GRAD layout's: {rv[i]} against {rg[i]}"


def check_cond(be, cond, kind):
    for acqf in CODES:
        a = make("7p", COND_SHAPE, kind, acqf, cond=cond)
        check_set(be, a, a["name"], infos=(None,))


def check_below(be, kind):
    """best_f below every sample: value exactly 0, every gradient entry exactly 0, and not a bit of it moves with mu_g / var_g."""
    a = make("7p", (17, 3, 0, 5, 2, 5), kind, EI, best="below")
    ref = check_set(be, a, a["name"], infos=(None,))
    assert all(x["clamped"] == a["S"] for x in ref["batches"]), "the set does not clamp every sample"
    _, value, grad, _, _ = be.run(a, None)
    assert (value == 0).all() and (grad == 0).all(), f"{a['name']}: value and gradient must be exactly 0"
    g2 = be.run(dict(a, mu_g=3.0 * a["mu_g"] + 1.0, var_g=3.0 * a["var_g"] + 1.0), None)[2]
    assert np.array_equal(grad, g2), f"{a['name']}: a clamped sample's weight is live in the gradient"


def check_beta0(be, kind):
    a = make("7p", (17, 3, 0, 5, 2, 5), kind, UCB, beta=0.0)
    check_set(be, a, a["name"], infos=(None,))


def check_ladder(be, kind, acqf):
    a = ladder_inputs(kind, acqf)
    ref = reference(a)
    assert np.array_equal(ref["jitter"], np.array([0.0, 1e-8, 1e-7, 1e-6, np.nan]), equal_nan=True) and list(ref["info"]) == [0, 0, 0, 0, 1], \
        f"the reference's own ladder: jitter {ref['jitter']}, info {ref['info']}"
    got = be.run(a, None)
    hold(a["name"], a, ref, got, cap=NORTH_STAR, k=lambda name: ("qacqf", f"ladder/{FAMILY[kind]}/{ACQ[acqf]}", name))
    assert np.isnan(got[1][4]) and np.isnan(got[2][12:]).all() and np.isnan(got[3][4]) and got[4][4] == 1
    four = be.run(ladder_inputs(kind, acqf, with_last=False), None)
    assert np.array_equal(four[1], got[1][:4]) and np.array_equal(four[2], got[2][:12]) and np.array_equal(four[3], got[3][:4]) \
        and np.array_equal(four[4], got[4][:4]), "batches 0 .. 3 change with batch 4 in the call"


# what is made NaN in batch 1 -> what the kernel gives there, read from csrc/gp_qacqf.h:
#   fail: Sigma holds the NaN, no rung passes -- value, jitter and the batch's gradient NaN, info 1
#   value: the factor is fine (jitter, info as in the clean call), value NaN and with it the batch's gradient
#   row: value, jitter, info as in the clean call; EVERY entry of that point's gradient row NaN (the rule of (7p)), the other rows of
#        the batch bit for bit
NONFINITE = dict(knq="fail", z="fail", var_q="fail", mate_value="fail", mate_slope="row", mu_g="row", var_g="row", cov_slope="row",
                 eps="all")
NONFINITE_SHAPE = (9, 3, 2, 5, 6, 3)


def nonfinite_inputs(what, kind, acqf):
    a = dict(make("7q", NONFINITE_SHAPE, kind, acqf))
    n, q, p, D = a["n"], a["q"], a["p"], a["D"]
    for k in ("Knq", "Z", "var_q", "cov", "mu_g", "var_g", "eps"):
        a[k] = a[k].copy()
    a["name"] = None
    col = 1 * q + 1                                                                        # point 1 of batch 1
    nan = np.nan
    if what == "knq":
        a["Knq"][:, col] = nan
    elif what == "z":
        a["Z"][:, col] = nan
    elif what == "var_q":
        a["var_q"][col] = nan
    elif what == "mate_value":                                                             # Sigma_10 of the batch
        a["cov"][n + p + 0, col * 16] = nan
    elif what == "mate_slope":
        a["cov"][n + p + 2, col * 16 + 1 + 3] = nan
    elif what == "cov_slope":
        a["cov"][4, col * 16 + 1 + 3] = nan
    elif what in ("mu_g", "var_g"):
        a[what][col * 16 + 1 + 3] = nan
    elif what == "eps":
        a["eps"][3, 1] = nan
    return a, col


def check_nonfinite(be, what, kind, acqf):
    clean = make("7q", NONFINITE_SHAPE, kind, acqf)
    c = be.run(clean, None)
    hold(clean["name"], clean, reference(clean), c)
    a, col = nonfinite_inputs(what, kind, acqf)
    rc, value, grad, jitter, info = be.run(a, None)
    q, rule = a["q"], NONFINITE[what]
    label = f"{clean['name']}-bad={what}"
    assert rc == 0
    if rule == "all":                                                                      # the base samples are shared by every batch
        assert np.isnan(value).all() and np.isnan(grad).all(), f"{label}: every batch must be NaN"
        assert np.array_equal(jitter, c[3]) and np.array_equal(info, c[4]), f"{label}: the factor does not depend on the samples"
        return
    others = np.array([0, 2])
    rows = np.concatenate([np.arange(b * q, b * q + q) for b in others])
    assert np.array_equal(value[others], c[1][others]) and np.array_equal(grad[rows], c[2][rows]) and np.array_equal(jitter[others], c[3][others]) \
        and np.array_equal(info[others], c[4][others]), f"{label}: the other batches are not bit-equal to the clean call"
    if rule == "fail":
        assert np.isnan(value[1]) and np.isnan(jitter[1]) and info[1] == 1 and np.isnan(grad[q:2 * q]).all(), \
            f"{label}: value {value[1]}, jitter {jitter[1]}, info {info[1]}, grad {grad[q:2 * q]}"
    else:
        assert value[1] == c[1][1] and jitter[1] == c[3][1] and info[1] == c[4][1], f"{label}: value, jitter, info must be the clean call's"
        assert np.isnan(grad[col]).all(), f"{label}: a partly NaN gradient row {grad[col]}"
        keep = [r for r in range(q, 2 * q) if r != col]
        assert np.array_equal(grad[keep], c[2][keep]), f"{label}: the other points' rows are not bit-equal to the clean call"


def check_twice(be, entry, kind, acqf):
    """Two calls on the largest set of the entry point, bit for bit."""
    shape = LARGEST[entry]
    a = make("7q" if entry == "7r" else entry, shape, kind, acqf)
    if entry == "7r":
        a = to_value_layout(a)
    r1, r2 = be.run(a, None), be.run(a, None)
    for x, y in zip(r1[1:], r2[1:]):
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), f"{entry}: two calls differ"


def chain_set(kw, acqf, par, entry, name) -> dict:
    """The real pipeline's own upstream outputs (the keyword arguments of ops.target_qacqf / ops.target_qacqf_pending as numpy) as a set."""
    g = lambda k: np.ascontiguousarray(np.asarray(kw[k], dtype=np.float64))   # noqa: E731
    n, Mq = g("Knq").shape
    p = int(np.asarray(kw["Xp"]).shape[0]) if "Xp" in kw else 0
    S, Q = g("base_samples").shape
    q, D = Q - p, g("Xq").shape[1]
    a = dict(entry=entry, layout="grad", n=n, q=q, p=p, S=S, D=D, B=Mq // q, kind=int(kw["kind"]), acqf=acqf, param=float(par), m=float(kw["m_all"]),
             s=float(kw["s_all"]), name=name, Knq=g("Knq"), Z=g("Z"), alpha=g("alpha"), mean_q=g("mean_q"), var_q=g("var_q"),
             cov=g("cov_g").reshape(n + p + q, Mq * 16), mu_g=g("mu_g").reshape(-1), var_g=g("var_g").reshape(-1), Xt=g("Xt"), Xq=g("Xq"),
             theta=g("theta"), eps=g("base_samples"), Xp=g("Xp") if p else np.zeros((0, D)), Zp=g("Zp") if p else np.zeros((n, 0)),
             mu_p=g("mu_p") if p else np.zeros(0), Sigma_pp=g("Sigma_pp") if p else np.zeros((0, 0)))
    return a
