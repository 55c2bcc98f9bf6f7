"""Long-double reference, a-priori forward error bound, input sets and shared drivers for sa_block<R, Params> of csrc/gp_studies_acqf.h,
the one body behind scaml_target_acqf_batched_f64 (7g), scaml_target_score_batched_f64 (7i), scaml_target_fantasy_acqf_batched_f64 and
scaml_target_fantasy_score_batched_f64 (7k) of include/scaml_gp.h (and the evaluation inside the device optimisers (7h) / (7l)).

Same construction as tests/_target_bounds.py and tests/_fantasy_bounds.py, whose helpers are used here.  The reference is numpy long
double, fed exactly the arrays the entry point is handed, and works per right-hand side: a query point of the 16-column layout
(R = 1, columns 1 .. D its gradient columns) or one candidate of a strip (R = 16, value only) are the same statements on column 0.
Only value, grad, mu_out and var_out leave the kernel, so the bound is first order through the whole block; the conditioning of Knn
enters through z.  With u = 2^-53, g_k = k u / (1 - k u), every count read from the statements of sa_block:

  task sums      acc by T fmas (a chunk's unused slots are fma(0, 0, acc): exact), cf = w_t or w_t w_t (one rounding):
                 E_S = g_{T+1} sum_t |c_t| |in_t| over the active tasks.  A masked task contributes nothing whatever it holds; every
                 task masked gives exact zeros.  C = acc (1 / (s s)): three roundings,  E_C = E_S / s^2 + g_3 |C|
  target kernel  df = (x_q - x_a) / l (two roundings), d2 by D fmas of df df:  E_d2 = g_{D+4} d2
                 k:  E_k = os (S E_d2 + c_k u |k|),  S = 1/2 (RBF), 5/6 (Matern-5/2) as tests/_posterior_bounds.py;
                     RBF  c_k = EXP_U + 1 (-d2 / 2 is exact; exp; the product with os),  dk = -k / 2 exactly: c_dk = c_k
                     Matern  with x = sqrt 5 r:  r = sqrt d2 (1), the exponent sqrt 5 r (1, and r's own: 2 x u in the exponential),
                     exp (EXP_U), os (1), lin = 1 + sqrt 5 r (3), ((5/3) r) r (4), their sum (5), the product (1):
                     c_k = 7 + EXP_U + 2 x;   dk = ((-5/6) lin) ex:  c_dk = 6 + EXP_U + 2 x
                 Knq = C[0] + k:  E_Knq = E_C + E_k + u |Knq|
                 gradient column  c = 2 dk ((x_q - x_a) / (l l)): four roundings besides dk's own,  E_c = 2 E_dk |(x_q - x_a) / l^2|
                 + 4 u |c|,  E_dk = os (S1 E_d2 + c_dk u |dk|);   dKnq = C[1 + d] + c:  E_dKnq = E_C + E_c + u |dKnq|
  solve          the reference is the long-double inverse of L alone, never Linv_diag (a wrong W is an error).  A row of u meets at most
                 16 fmas per block to its left and 16 in its own block's product with W: 16 nb <= n + 15 fmas; W itself is a 16 x 16
                 inverse with residual g_16 |W| |L_kk|:  g_{n+31}, for the backward half alike
                 E_y = |L^-1| E_Knq + g_{n+31} |L^-1| |L| |y|,    E_z = |L^-T| (E_y + g_{n+31} |L^T| |z|)
                 (the diagonal blocks are applied as inverses: their forward error lies inside |L^-1| |L| |y| for the block itself,
                 and its way into the later blocks is taken at first order, as the solve bound of tests/_target_bounds.py has it)
  posterior      mean_q = (S_mu[0] - m) / s:  E_mean_q = E_S / s + g_2 |mean_q|;   Knq . alpha, Knq . z by n sequential fmas
                 mu = fma(s, mean_q + Knq . alpha, m):
                   E_mu = s (E_mean_q + |alpha|^T E_Knq + g_n |alpha|^T |Knq| + u |mean_q + Knq . alpha|) + u |mu|
                 var_q = S_var[0] (1 / s^2) + os:  E_var_q = E_S / s^2 + 3 u |S_var[0] / s^2| + u |var_q|
                 var = (s s) (var_q - Knq . z):
                   E_var = s^2 (E_var_q + |z|^T E_Knq + |Knq|^T E_z + g_n |Knq|^T |z|) + 3 u |var|
                 dmu = fma(s, sum_a alpha_a dKnq, S_mu[1 + d]):  E_dmu = E_S + s (|alpha|^T E_dKnq + g_n |alpha|^T |dKnq|) + u |dmu|
                 gv = sum_a z_a dKnq:  E_gv = |z|^T E_dKnq + E_z^T |dKnq| + g_n |z|^T |dKnq|
                 dvar = fma(-2 (s s), gv, S_var[1 + d]):  E_dvar = E_S + 2 s^2 (E_gv + u |gv|) + u |dvar|
  transform      UCB / EI: tests/_fantasy_bounds.transform(acqf, par, mu, var, E_mu, E_var);  LogEI (code 17):
                 tests/_logei_bounds.transform_e (g_ld with budgets; A = log sigma + g, Amu = -g' / sigma, Av = om / (2 sigma^2),
                 exactly 0 on the floor)
                 grad = fma(Av, dvar, Amu dmu):  E_grad = E_Amu |dmu| + |Amu| E_dmu + u |Amu dmu| + E_Av |dvar| + |Av| E_dvar + u |grad|
  fantasies      (F_g > 1; (7f)'s lines of tests/_fantasy_bounds.py with this kernel's own sums, all sequential)
                 r_f by n fmas: E_mu per fantasy as above with alpha_f[:, f];  var is shared
                 value = (sum_f A_f) / F:  (sum_f E_A + g_F sum_f |A_f|) / F + u |value|;   sAmu, sAv:  sum_f E + g_F sum_f |.|
                 abar_a by F fmas:  E_abar = sum_f E_Amu_f |alpha_f[a, f]| + g_F sum_f |Amu_f alpha_f[a, f]|
                 gm = sum_a abar_a dKnq by n fmas:  E_gm = |abar|^T E_dKnq + E_abar^T |dKnq| + g_n |abar|^T |dKnq|
                 gmu = fma(s, gm, sAmu S_mu[1 + d]):  E_gmu = E_sAmu |S_mu| + |sAmu| E_S + u |sAmu S_mu| + s E_gm + u |gmu|
                 grad = fma(sAv, dvar, gmu) / F:  (E_gmu + E_sAv |dvar| + |sAv| E_dvar + u |fma|) / F + u |grad|
                 LogEI: value = mx + log S - log F by tests/_logei_bounds.average, the weights w_f = e_f / S with
                 E_w_f = w_f (E_A_f + sum_j w_j E_A_j + u (2 EXP_U + F + 4)) + 2^-1074 / S, the weighted factors Amu_f w_f, Av_f w_f
                 with E = E_A. w_f + |A.| E_w_f + u |A. w_f|, then the lines above with the divisor 1

Every bound is multiplied by GUARD = 1 / (1 - 1e-6) (second order).  Corrections to the model the work started from:
  * E_mu carries E_S of the mean sum (through mean_q) and the rounding of the sum mean_q + Knq . alpha as s u |mean_q + Knq . alpha|
    in place of a second u |mu| (m may cancel); E_var_q carries E_S of the variance sum
  * d2: two roundings per df, so g_{D+4}; the gradient column's factor has four roundings (the difference, l l, the quotient, the product)
  * Matern-5/2: the 4 u |k| of the evaluation is c_k u |k| with c_k = 7 + EXP_U + 2 sqrt(5 d2) (the exponent's own rounding grows
    with the distance); RBF: c_k = EXP_U + 1
  * the solve's constant is g_{n+31}: 16 nb <= n + 15 fmas on a row's chain and the 16 of the block inverse's own residual
  * dvar: -2 (s s) carries the rounding of s s, u |2 s^2 gv|
  * fantasies: the value's division is one rounding (no reciprocal): u |value|, the sums over f carry g_F

Conditions on the inputs, asserted with every comparison: each bound at most CAP = 1e-8 of the output's largest reference magnitude
IN ITS GROUP (a clamped query with a source variance of -1e3 does not set the scale for the others); var at least MARGIN = 1e3 bounds
away from the clamp on whichever side it lies; the second-order measure eps of the transform at most 1e-6.  (The set with every
u <= -40 has an all-zero EI: its cap is taken against sigma.)

Input sets (the smallest shapes at which sa_block branches; both families; UCB, EI, LogEI; every call has one padding query; NaN
past n_g in Xt, L, alpha and cov, in the strict upper triangle of L, in the unused rows and columns of a partial last block of
Linv_diag and in its blocks past the group's own; columns c > D of mu / var / cov hold the finite JUNK):
  T1      T = 1, n_max = 1, n = (1), D = 1 (thread 0 writes value and grad[0])
  T8      T = 8, n_max = 33 (odd: ldl = n_max), n = (15, 16, 17, 32, 33), D = 2
  T9      T = 9, n_max = 96 (even: ldl = n_max + 1), n = (1, 17, 95, 96, 5), D = 15; the last task has 1e-4 of the others' weight; task 4
          masked in group 1 only, holding NaN values and a NaN weight; group 4 has every task masked; the last input dimension is an
          irrelevant one (lengthscale 1e5, source derivatives 1e-11): a gradient component eleven orders under the largest
  T17     T = 17, n_max = 33, n = (16, 33), D = 2, the last weight 1e-4 of the others
  GEO     T = 3, n_max = 33, n = (17, 33), D = 2: query 0 of a group ON its training point 0, query 1 1e-7 from training point 3, training
          rows 0 and 1 identical
  FAR     T = 3, n_max = 33, n = (17, 33), D = 2: the last training point of every group far from every query (its terms of the
          contractions are small against the sums, and large against the bounds);  FARF: the same with fantasies, (n, F) = (9, 7), (17, 2)
  CLAMP   T = 3, n_max = 17, n = (9, 17, 5), D = 15, noise 0.5 (so that E_var leaves the margin): queries 0 and 2 of group 0 with var = -0.01,
          of group 1 with var = 5e-10 (EI, LogEI; UCB: -0.01); group 2 has os = 0 and query 0 with zero columns: var == 0 exactly;
          beta = 0 in group 1 (UCB).  The clamped partial is exactly absent: grad is bit for bit the same when var's gradient columns change
  TAIL    T = 3, n_max = 17, n = (17), D = 2, seven queries: 'span' u = -9 .. +9; 'deep' every u = -45 (EI, LogEI)
  FA      fantasies, F_max = 64, n_max = 96, T = 3, D = 15: (n, F) = (7, 1), (8, 2), (9, 7), (96, 64), (8, 8), (7, 9), (9, 63): F = 1 next
          to F = 64 in one launch, (96, 64) in the strip layout (R F = 1024 exceeds the workgroup); NaN past F_g in alpha_f
  FB      fantasies, F_max = 9, n_max = 9, T = 9, D = 2: (n, F) = (9, 9), (7, 2), (8, 1)
  contracts  SENTINEL and one guard row in every output; a padding query / strip gives zeros; info != 0, n_points outside 1 .. n_max,
          n_fant outside 1 .. F_max: NaN for that group only, the others bit for bit and within their bounds; grad, mu_out, var_out
          NULL; a NaN query coordinate: NaN in all of its outputs, once per entry point
  chain   (GPU only, tests/test_studies_bounds_gpu.py) the ragged golden stack T = 4, N = 48 under studies of n = (1, 17, 40), the second
          with 3 pending points and F = 5: the grouped source passes (5e) / (5f), (7j) (train_block_reference below) and one POTRF, the
          solve for alpha_f, the four entry points, each reference fed the device's own upstream outputs

The drivers (`check_*`) run a set through a BACKEND: be.run(entry, a, grad=, post=) -> dict(value, grad, mu, var) (None where not
asked for), entry one of ENTRIES, every output through a buffer of SENTINEL with one guard row.
"""
from __future__ import annotations

import numpy as np

from tests import _fantasy_bounds as FB
from tests import _logei_bounds as LE
from tests import _target_bounds as B
from tests._fantasy_bounds import GUARD, MARGIN
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, SENTINEL, U, Quantity, _kernel, _S, gamma, inverse_lower
from tests._target_bounds import FAMILY, within

UCB, EI, LOGEI = 0, 1, 17
ACQS = (UCB, EI, LOGEI)
ACQ = {UCB: "ucb", EI: "ei", LOGEI: "logei"}
KINDS = (KIND_RBF, KIND_MATERN52)
ENTRIES = ("acqf", "score", "fantasy", "fantasy_score")      # (7g), (7i), (7k) query layout, (7k) strip layout
JUNK = 3.25e3
SOLVE_EXTRA = 31
_SQRT5 = np.sqrt(LD(5))
assert CAP == 1e-8 and MARGIN == 1e3 and SENTINEL < 0


def is_strips(a):
    return a["mu"].ndim == 2


def rhs_groups(a):
    """The group of every right-hand side: group[q] in the query layout, group[q // 16] in the strip layout."""
    return np.repeat(a["group"], 16) if is_strips(a) else a["group"]


# ------------------------------------------------------------------------------------------------------------------
# reference and bound
_LINV = {}


def _linv(L):
    key = L.tobytes()
    if key not in _LINV:
        if len(_LINV) > 64:
            _LINV.clear()
        _LINV[key] = inverse_lower(L)
    return _LINV[key]


def _group_reference(a, g, rows, want_grad):
    """The right-hand sides `rows` of group g -> dict of (ref, bound) pairs per output and the transform's conditions."""
    T, D, kind, acqf, n_max = a["T"], a["D"], a["kind"], a["acqf"], a["n_max"]
    strips = is_strips(a)
    n, Q = int(a["n_points"][g]), len(rows)
    nc = 1 + D if want_grad else 1
    s, m = LD(a["s_all"][g]), LD(a["m_all"][g])
    s2 = s * s
    th = a["theta"][g]
    l, os_ = LD(th[:D]), LD(th[D])
    if strips:
        mu_c, var_c = a["mu"][:, rows, None], a["var"][:, rows, None]                       # (T, Q, 1)
        cov_c = a["cov"][:, :n][:, :, rows, None]                                           # (T, n, Q, 1)
    else:
        mu_c, var_c = a["mu"][:, rows, :nc], a["var"][:, rows, :nc]
        cov_c = a["cov"].reshape(T, n_max, -1, 16)[:, :n][:, :, rows, :nc]
    Smu, Svar, Cs = np.zeros((Q, nc), dtype=LD), np.zeros((Q, nc), dtype=LD), np.zeros((n, Q, nc), dtype=LD)
    Mmu, Mvar, Mc = np.zeros((Q, nc), dtype=LD), np.zeros((Q, nc), dtype=LD), np.zeros((n, Q, nc), dtype=LD)
    for t in range(T):
        if not a["active"][g, t]:
            continue
        w1 = LD(a["w"][g, t])
        w2 = w1 * w1
        Smu, Mmu = Smu + w1 * LD(mu_c[t]), Mmu + np.abs(w1) * np.abs(LD(mu_c[t]))
        Svar, Mvar = Svar + w2 * LD(var_c[t]), Mvar + w2 * np.abs(LD(var_c[t]))
        Cs, Mc = Cs + w2 * LD(cov_c[t]), Mc + w2 * np.abs(LD(cov_c[t]))
    gT = gamma(T + 1)
    E_Smu, E_Svar = gT * Mmu, gT * Mvar
    C = Cs / s2
    E_C = gT * Mc / s2 + gamma(3) * np.abs(C)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        xq = LD(a["Xq"][rows])
        diff = xq[None, :, :] - LD(a["Xt"][g, :n])[:, None, :]                               # (n, Q, D)
        df = diff / l
        d2 = (df * df).sum(-1)
        E_d2 = gamma(D + 4) * d2
        k, dk = _kernel(d2, kind)
        S0, S1 = _S[kind]
        if kind == KIND_RBF:
            ck = cdk = FB.EXP_U + 1
        else:
            x = _SQRT5 * np.sqrt(np.maximum(d2, LD(1e-30)))
            ck, cdk = 7 + FB.EXP_U + 2 * x, 6 + FB.EXP_U + 2 * x
        E_k = os_ * (S0 * E_d2 + ck * U * np.abs(k))
        Knq = C[..., 0] + os_ * k                                                            # (n, Q)
        E_Knq = E_C[..., 0] + E_k + U * np.abs(Knq)
        # the solve against the long-double inverse of L alone
        Lg = np.tril(a["L"][g, :n, :n])
        Li = _linv(Lg)
        aLi, aL = np.abs(Li), np.abs(LD(Lg))
        gs = gamma(n + SOLVE_EXTRA)
        y = Li @ Knq
        z = Li.T @ y
        E_y = aLi @ E_Knq + gs * (aLi @ (aL @ np.abs(y)))
        E_z = aLi.T @ (E_y + gs * (aL.T @ np.abs(z)))
        aK, az = np.abs(Knq), np.abs(z)
        gn = gamma(n)
        mean_q = (Smu[:, 0] - m) / s
        E_mean_q = E_Smu[:, 0] / s + gamma(2) * np.abs(mean_q)
        sv = Svar[:, 0] / s2
        var_q = sv + os_
        E_var_q = E_Svar[:, 0] / s2 + 3 * U * np.abs(sv) + U * np.abs(var_q)
        v = s2 * (var_q - (Knq * z).sum(0))
        E_v = s2 * (E_var_q + (az * E_Knq).sum(0) + (aK * E_z).sum(0) + gn * (aK * az).sum(0)) + 3 * U * np.abs(v)
        fant = "alpha_f" in a
        F = int(a["n_fant"][g]) if fant else 1
        al = LD(a["alpha_f"][g, :n, :F]) if fant else LD(a["alpha"][g, :n, None])            # (n, F)
        aal = np.abs(al)
        kal = Knq.T @ al                                                                     # (Q, F)
        pre = mean_q[:, None] + kal
        mu = m + s * pre
        E_mu = s * (E_mean_q[:, None] + E_Knq.T @ aal + gn * (aK.T @ aal) + U * np.abs(pre)) + U * np.abs(mu)
        par = a["acqf_param"][g]
        if acqf == LOGEI:
            t = LE.transform_e(par, mu, v[:, None], E_mu, E_v[:, None])
        else:
            t = FB.transform(acqf, par, mu, v[:, None], E_mu, E_v[:, None])
        A, Amu, Av, E_A, E_Amu, E_Av = (t[k_] for k_ in ("A", "Amu", "Av", "E_A", "E_Amu", "E_Av"))
        gF = gamma(F)
        if F == 1:
            value, E_value = A[:, 0], E_A[:, 0]
        elif acqf == LOGEI:
            value, wts, E_avg = LE.average(A)
            E_value = (wts * E_A).sum(1) + E_avg
            Ssum = np.exp(A - A.max(1, keepdims=True)).sum(1, keepdims=True)
            E_w = GUARD * (wts * (E_A + (wts * E_A).sum(1, keepdims=True) + U * (2 * FB.EXP_U + F + 4)) + FB._TINY / Ssum)
            E_Amu = E_Amu * wts + np.abs(Amu) * E_w + U * np.abs(Amu * wts)
            E_Av = E_Av * wts + np.abs(Av) * E_w + U * np.abs(Av * wts)
            Amu, Av = Amu * wts, Av * wts
        else:
            value = A.sum(1) / F
            E_value = (E_A.sum(1) + gF * np.abs(A).sum(1)) / F + U * np.abs(value)
        out = dict(value=(value, GUARD * E_value), mu=(mu[:, 0], GUARD * E_mu[:, 0]), var=(v, GUARD * E_v), eps=t["eps"], margin=t["margin"],
                   u=t["u"], v=v, F=F)
        if not want_grad:
            return out
        e = diff / (l * l)
        E_dk = os_ * (S1 * E_d2 + cdk * U * np.abs(dk))
        c = 2 * os_ * dk[..., None] * e                                                      # (n, Q, D)
        E_c = 2 * E_dk[..., None] * np.abs(e) + 4 * U * np.abs(c)
        dK = C[..., 1:] + c
        E_dK = E_C[..., 1:] + E_c + U * np.abs(dK)
        adK = np.abs(dK)
        Smu_d, Svar_d, E_Smu_d, E_Svar_d = Smu[:, 1:], Svar[:, 1:], E_Smu[:, 1:], E_Svar[:, 1:]
        gv = np.einsum("aq,aqd->qd", z, dK)
        E_gv = np.einsum("aq,aqd->qd", az, E_dK) + np.einsum("aq,aqd->qd", E_z, adK) + gn * np.einsum("aq,aqd->qd", az, adK)
        dvar = Svar_d - 2 * s2 * gv
        E_dvar = E_Svar_d + 2 * s2 * (E_gv + U * np.abs(gv)) + U * np.abs(dvar)
        if F == 1:
            ga = np.einsum("a,aqd->qd", al[:, 0], dK)
            dmu = Smu_d + s * ga
            E_dmu = E_Smu_d + s * (np.einsum("a,aqd->qd", aal[:, 0], E_dK) + gn * np.einsum("a,aqd->qd", aal[:, 0], adK)) + U * np.abs(dmu)
            t1, t2 = Amu * dmu, Av * dvar
            grad = t1 + t2
            E_grad = E_Amu * np.abs(dmu) + np.abs(Amu) * E_dmu + U * np.abs(t1) + E_Av * np.abs(dvar) + np.abs(Av) * E_dvar + U * np.abs(grad)
        else:
            Fdiv = 1 if acqf == LOGEI else F
            sAmu, sAv = Amu.sum(1, keepdims=True), Av.sum(1, keepdims=True)
            E_sAmu = E_Amu.sum(1, keepdims=True) + gF * np.abs(Amu).sum(1, keepdims=True)
            E_sAv = E_Av.sum(1, keepdims=True) + gF * np.abs(Av).sum(1, keepdims=True)
            ab = Amu @ al.T                                                                  # (Q, n)
            E_ab = E_Amu @ aal.T + gF * (np.abs(Amu) @ aal.T)
            gm = np.einsum("qa,aqd->qd", ab, dK)
            E_gm = np.einsum("qa,aqd->qd", np.abs(ab), E_dK) + np.einsum("qa,aqd->qd", E_ab, adK) + gn * np.einsum("qa,aqd->qd", np.abs(ab), adK)
            t1 = sAmu * Smu_d
            gmu = t1 + s * gm
            E_gmu = E_sAmu * np.abs(Smu_d) + np.abs(sAmu) * E_Smu_d + U * np.abs(t1) + s * E_gm + U * np.abs(gmu)
            t2 = sAv * dvar
            grad = (gmu + t2) / Fdiv
            E_grad = (E_gmu + E_sAv * np.abs(dvar) + np.abs(sAv) * E_dvar + U * np.abs(gmu + t2)) / Fdiv + U * np.abs(grad)
        out["grad"] = (grad, GUARD * E_grad)
    return out


def reference(a: dict, want_grad=None) -> dict:
    """a: the arguments of one of the four entry points (numpy) -> per output the long-double reference and bound over all right-hand
    sides (padding: 0 +- 0; a refused group: NaN), the kind of every right-hand side ('pad', 'nan', 'live'), and per live group the
    transform's conditions."""
    strips = is_strips(a)
    want_grad = (not strips) if want_grad is None else want_grad
    Mq, D, G = a["Xq"].shape[0], a["D"], a["G"]
    rg = rhs_groups(a)
    fant = "alpha_f" in a
    names = ("value", "mu", "var") + (("grad",) if want_grad else ())
    ref = {k: np.zeros((Mq, D) if k == "grad" else Mq, dtype=LD) for k in names}
    bound = {k: np.zeros((Mq, D) if k == "grad" else Mq, dtype=LD) for k in names}
    state = np.full(Mq, "pad", dtype=object)
    cond = {}
    for g in sorted(set(int(x) for x in rg)):
        rows = np.nonzero(rg == g)[0]
        if g < 0 or g >= G:
            continue
        n = int(a["n_points"][g])
        refused = a["info"][g] != 0 or n < 1 or n > a["n_max"] or (fant and not 1 <= int(a["n_fant"][g]) <= a["F_max"])
        if refused:
            state[rows] = "nan"
            for k in names:
                ref[k][rows] = np.nan
            continue
        state[rows] = "live"
        r = _group_reference(a, g, rows, want_grad)
        for k in names:
            ref[k][rows], bound[k][rows] = r[k]
        cond[g] = dict(eps=r["eps"], margin=r["margin"], u=r["u"], v=r["v"], F=r["F"], rows=rows)
    with np.errstate(invalid="ignore"):
        bad_q = ~np.isfinite(a["Xq"]).all(1)
    return dict(ref=ref, bound=bound, state=state, cond=cond, groups=rg, bad_q=bad_q, names=names)


def key(entry, a, name):
    return (entry, f"{FAMILY[a['kind']]}/{ACQ[a['acqf']]}", name)


def report():
    return [line for e in ENTRIES + ("studies_chain",) for line in B.report(e)]


def train_block_reference(means, covs, X, y, m, s, w, active, theta, kind) -> dict:
    """(7j) for one study: Knn (lower triangle) and resid from the source terms means (T, n) and covs (T, n, n), as the composition of
    the weighted task sums and the target assemble, each under its bound of tests/_target_bounds.py: the assemble's reference is fed the
    sums' long-double reference rounded to fp64, and the sums' bound with that rounding reaches Knn through 1 / s^2, resid through 1 / s."""
    T, n = means.shape
    D = X.shape[1]
    ms = B.wsum_reference(means, w, active, 1)
    cs = B.wsum_reference(covs.reshape(T, -1), w, active, 2)
    a = dict(cov_s=cs.ref.astype(np.float64).reshape(n, n), mean_s=ms.ref.astype(np.float64), var_s=np.zeros(n), Xall=X, theta=theta, y=y, m=m, s=s,
             n=n, M=0, D=D, kind=kind)
    asm = B.assemble_reference(a)
    E_c = (cs.bound + U * np.abs(cs.ref)).reshape(n, n) / (LD(s) * LD(s))
    E_m = (ms.bound + U * np.abs(ms.ref)) / LD(s)
    low = np.tril(np.ones((n, n), dtype=bool))
    Knn = Quantity(np.where(low, asm["Knn"].ref, 0), np.where(low, asm["Knn"].bound + GUARD * E_c, 0), asm["Knn"].scale)
    return dict(Knn=Knn, resid=Quantity(asm["resid"].ref, asm["resid"].bound + GUARD * E_m, asm["resid"].scale))


def hold(label, entry, a, ref, got, scale=None, table=None):
    """Every output of one call against `ref`: the conditions on the inputs, padding zeros, refused groups NaN, every other element
    within its bound, the bound at most CAP of the output's largest reference magnitude in its group (`scale`: in its place).
    table: the row of the ratio table in place of the entry point's."""
    state, rg = ref["state"], ref["groups"]
    outs = [k for k in ref["names"] if got.get(k) is not None]
    assert "value" in outs
    for k in outs:
        x = got[k]
        assert x.shape == ref["ref"][k].shape, f"{label} {k}: shape {x.shape}"
        pad = state == "pad"
        assert (x[pad] == 0).all() and not np.signbit(x[pad]).any(), f"{label} {k}: a padding right-hand side must give zeros, got {x[pad].ravel()[:4]}"
        assert np.isnan(x[state == "nan"]).all(), f"{label} {k}: a refused group must give NaN, got {x[state == 'nan'].ravel()[:4]}"
    for g, c in ref["cond"].items():
        FB.conditions(f"{label} group {g}", c)
        rows = c["rows"]
        for k in outs:
            r, b = ref["ref"][k][rows], ref["bound"][k][rows]
            mask = ref["bad_q"][rows]
            mask = (mask[:, None] if k == "grad" else mask) if mask.any() else None
            sc = B._scale(r if mask is None else r[~ref["bad_q"][rows]]) if scale is None else scale
            within(f"{label} group {g}", key(table or entry, a, k if table is None else f"{entry}/{k}"), got[k][rows], Quantity(r, b, sc), mask)


# ------------------------------------------------------------------------------------------------------------------
# input sets
def _rng(*seed):
    return np.random.default_rng([20261021, *seed])


class Fields:
    """Smooth synthetic source-pass outputs of T tasks, as tests/test_studies_acqf_emul.py has them, in numpy: mu_t, var_t, cov_t with
    their analytic derivatives (kap: the inverse lengthscales of the covariance; an irrelevant dimension has a tiny one)."""

    def __init__(self, rng, T, D, irrelevant_last=False):
        self.T, self.D = T, D
        self.A, self.b, self.C = rng.uniform(-1, 1, size=(T, D)), rng.uniform(size=T), rng.uniform(size=(T, D))
        self.kap = np.ones(D)
        if irrelevant_last:
            self.A[:, -1] *= 1e-11
            self.C[:, -1] *= 1e-11
            self.kap[-1] = 1e-11

    def mu(self, t, x):
        ph = x @ self.A[t] + self.b[t]
        return 2.0 * np.sin(ph) + 0.3 * t, 2.0 * np.cos(ph)[:, None] * self.A[t]

    def var(self, t, x):
        ph = x @ self.C[t]
        return 2.0 + np.cos(ph), -np.sin(ph)[:, None] * self.C[t]

    def cov(self, t, xa, x):
        """(n, M) and its derivative in x (n, M, D)"""
        diff = (x[None, :, :] - xa[:, None, :]) * self.kap
        c = 0.3 * (1.0 + 0.1 * t) * np.exp(-0.5 * (diff * diff).sum(-1))
        return c, -(diff * self.kap) * c[..., None]


def _k64(Xa, Xb, th, kind):
    D = Xa.shape[1]
    d2 = (((Xa[:, None, :] - Xb[None, :, :]) / th[:D]) ** 2).sum(-1)
    return th[D] * _kernel(d2, kind)[0]


def make_set(name, ns, n_max, T, D, kind, acqf, counts, fs=None, F_max=None, small_last=False, masked=None, all_masked=None,
             geometry=False, noise=None, os_zero=None, irrelevant_last=False, far_last=None) -> dict:
    """One call in the query layout: G = len(ns) studies of n_g points under n_max, counts[g] query points each and one padding query."""
    import zlib
    rng = _rng(zlib.crc32(name.encode()), kind)
    G = len(ns)
    fld = Fields(rng, T, D, irrelevant_last)
    w = 0.2 + rng.uniform(size=(G, T))
    if small_last:
        w[:, T - 1] = 1e-4 * w[:, 0]
    active = np.ones((G, T), dtype=np.uint8)
    if masked is not None:
        active[masked] = 0
    if all_masked is not None:
        active[all_masked] = 0
    nan = np.nan
    nbm = (n_max + 15) // 16
    Xt, theta = np.full((G, n_max, D), nan), np.zeros((G, D + 2))
    L, W = np.full((G, n_max, n_max), nan), np.full((G, nbm, 16, 16), nan)
    m_all, s_all = rng.uniform(-0.5, 0.5, size=G), 0.7 + rng.uniform(size=G)
    group = np.array([g for g, c in enumerate(counts) for _ in range(c)] + [-1], dtype=np.int32)
    Mq = len(group)
    Xq = rng.uniform(size=(Mq, D))
    fant = fs is not None
    alpha = np.full((G, n_max, F_max), nan) if fant else np.full((G, n_max), nan)
    for g, n in enumerate(ns):
        X = rng.uniform(size=(n, D))
        if geometry and n >= 4:
            X[1] = X[0]
        if far_last is not None:
            X[n - 1] = 0.5 + far_last
        th = np.concatenate([0.4 + rng.uniform(size=D), 0.5 + rng.uniform(size=1), (1e-2 + 0.1 * rng.uniform(size=1)) if noise is None else [noise]])
        if irrelevant_last:
            th[D - 1] = 1e5
        if os_zero == g:
            th[D] = 0.0
        Xt[g, :n], theta[g] = X, th
        Knn = _k64(X, X, th, kind) + th[D + 1] * np.eye(n)
        for t in range(T):
            if active[g, t]:
                Knn += w[g, t] ** 2 * fld.cov(t, X, X)[0] / s_all[g] ** 2
        Lc = np.linalg.cholesky(0.5 * (Knn + Knn.T))
        L[g, :n, :n] = np.tril(Lc) + np.triu(np.full((n, n), nan), 1)
        for kb in range((n + 15) // 16):
            c = min(16, n - 16 * kb)
            W[g, kb, :c, :c] = np.linalg.inv(Lc[16 * kb:16 * kb + c, 16 * kb:16 * kb + c])
        F = fs[g] if fant else 1
        resid = np.repeat(rng.uniform(-0.5, 0.5, size=(n, 1)), max(F, 1), axis=1)
        p = max(1, n // 8)
        resid[-p:] += 0.5 * rng.uniform(-0.5, 0.5, size=(p, max(F, 1)))
        sol = np.linalg.solve(Lc.T, np.linalg.solve(Lc, resid))
        if fant:
            alpha[g, :n, :F] = sol[:, :F]
        else:
            alpha[g, :n] = sol[:, 0]
    if geometry:
        for g, n in enumerate(ns):
            q = np.nonzero(group == g)[0]
            if n >= 4 and len(q) >= 2:
                Xq[q[0]] = Xt[g, 0]
                Xq[q[1]] = Xt[g, 3] + 1e-7
    mu, var = np.full((T, Mq, 16), JUNK), np.full((T, Mq, 16), JUNK)
    cov = np.full((T, n_max, Mq, 16), nan)
    for t in range(T):
        f, df = fld.mu(t, Xq)
        mu[t, :, 0], mu[t, :, 1:1 + D] = f, df
        f, df = fld.var(t, Xq)
        var[t, :, 0], var[t, :, 1:1 + D] = f, df
        for q in range(Mq):
            g = int(group[q])
            if g < 0:
                continue
            n = ns[g]
            c, dc = fld.cov(t, Xt[g, :n], Xq[q:q + 1])
            cov[t, :n, q, :] = JUNK
            cov[t, :n, q, 0], cov[t, :n, q, 1:1 + D] = c[:, 0], dc[:, 0]
    if masked is not None:      # the masked task of that group holds NaN values and a NaN weight
        g, t = masked
        rows = group == g
        mu[t, rows], var[t, rows], cov[t, :, rows] = nan, nan, nan
        w[g, t] = nan
    param = {UCB: 4.0 + 5.0 * rng.uniform(size=G), EI: rng.uniform(-0.3, 0.7, size=G)}
    a = dict(name=name, mu=mu, var=var, cov=np.ascontiguousarray(cov.reshape(T, n_max, Mq * 16)), group=group, Xq=Xq, w=w, active=active, Xt=Xt,
             theta=theta, L=L, Linv_diag=W, n_points=np.array(ns, dtype=np.int32), m_all=m_all, s_all=s_all, info=np.zeros(G, dtype=np.int32),
             acqf_param=param[UCB if acqf == UCB else EI].copy(), Mq=Mq, G=G, n_max=n_max, T=T, D=D, kind=kind, acqf=acqf)
    if fant:
        a.update(alpha_f=alpha, n_fant=np.array(fs, dtype=np.int32), F_max=F_max)
    else:
        a["alpha"] = alpha
    if acqf != UCB:      # best_f next to the group's posterior means: u of order 1
        mu64 = posterior64(a)[0]
        for g in range(G):
            a["acqf_param"][g] = mu64[group == g].mean() + 0.1
    return a


def posterior64(a):
    """mu*, var* of every query of a query-layout set in plain fp64 (fantasy 0 of a fantasy set): what the clamp and tail sets are placed
    with.  NaN for padding."""
    T, D, n_max = a["T"], a["D"], a["n_max"]
    Mq = a["Xq"].shape[0]
    mu, v = np.full(Mq, np.nan), np.full(Mq, np.nan)
    cov = a["cov"].reshape(T, n_max, Mq, 16)
    for q in range(Mq):
        g = int(a["group"][q])
        if g < 0:
            continue
        n, s, th = int(a["n_points"][g]), a["s_all"][g], a["theta"][g]
        act = [t for t in range(T) if a["active"][g, t]]
        Smu = sum(a["w"][g, t] * a["mu"][t, q, 0] for t in act)
        Svar = sum(a["w"][g, t] ** 2 * a["var"][t, q, 0] for t in act)
        C = sum(a["w"][g, t] ** 2 * cov[t, :n, q, 0] for t in act) if act else np.zeros(n)
        Knq = C / s ** 2 + _k64(a["Xt"][g, :n], a["Xq"][q:q + 1], th, a["kind"])[:, 0]
        Lg = np.tril(a["L"][g, :n, :n])
        z = np.linalg.solve(Lg.T, np.linalg.solve(Lg, Knq))
        al = a["alpha_f"][g, :n, 0] if "alpha_f" in a else a["alpha"][g, :n]
        mu[q] = Smu + s * (Knq @ al)
        v[q] = Svar + s * s * (th[D] - Knq @ z)
    return mu, v


def _first_active(a, g):
    return int(np.nonzero(a["active"][g])[0][0])


def shift_var(a, q, target):
    """Move the source variance of query q (its first active task) so that var* becomes `target`."""
    g = int(a["group"][q])
    t = _first_active(a, g)
    a["var"][t, q, 0] += (target - posterior64(a)[1][q]) / a["w"][g, t] ** 2


def shift_mu(a, q, target):
    g = int(a["group"][q])
    t = _first_active(a, g)
    a["mu"][t, q, 0] += (target - posterior64(a)[0][q]) / a["w"][g, t]


def set_T1(kind, acqf):
    return make_set("T1", (1,), 1, 1, 1, kind, acqf, (3,))


def set_T8(kind, acqf):
    return make_set("T8", (15, 16, 17, 32, 33), 33, 8, 2, kind, acqf, (2, 2, 2, 2, 2))


T9_MASKED = (1, 4)
T9_ALL_MASKED = 4


def set_T9(kind, acqf):
    return make_set("T9", (1, 17, 95, 96, 5), 96, 9, 15, kind, acqf, (2, 3, 2, 2, 2), small_last=True, masked=T9_MASKED,
                    all_masked=T9_ALL_MASKED, irrelevant_last=True)


def set_T17(kind, acqf):
    return make_set("T17", (16, 33), 33, 17, 2, kind, acqf, (2, 3), small_last=True)


def set_GEO(kind, acqf):
    return make_set("GEO", (17, 33), 33, 3, 2, kind, acqf, (3, 3), geometry=True)


FAR, FAR_F = 3.3, 7.0      # the last training point of every group sits at 0.5 + FAR in every coordinate, the queries in the unit cube


def set_FAR(kind, acqf):
    return make_set("FAR", (17, 33), 33, 3, 2, kind, acqf, (3, 3), far_last=FAR)


ORDINARY_SETS = dict(T1=set_T1, T8=set_T8, T9=set_T9, T17=set_T17, GEO=set_GEO, FAR=set_FAR)
CLAMP_ZERO_GROUP = 2


def set_CLAMP(kind, acqf):
    """Queries 0 and 2 of groups 0 and 1 on the clamp (group 0: var = -0.01; group 1: 5e-10 for EI / LogEI, -0.01 and beta = 0 for UCB);
    group 2 has os = 0 and query 0 with zero value columns of var and cov: var == 0 exactly.  EI / LogEI: the clamped queries' mu
    within a fraction of sigma of best_f (or pdf underflows and Av is 0, clamp or no clamp).  -> (set, the clamped queries)"""
    a = make_set("CLAMP", (9, 17, 5), 17, 3, 15, kind, acqf, (3, 3, 2), noise=0.5, os_zero=CLAMP_ZERO_GROUP)
    T, n_max, Mq = a["T"], a["n_max"], a["Mq"]
    clamped = []
    for g, target in ((0, -0.01), (1, -0.01 if acqf == UCB else 5e-10)):
        q = np.nonzero(a["group"] == g)[0]
        for qq in (q[0], q[2]):
            shift_var(a, qq, target)
            clamped.append(int(qq))
    q0 = int(np.nonzero(a["group"] == CLAMP_ZERO_GROUP)[0][0])
    a["var"][:, q0, 0] = 0.0
    a["cov"].reshape(T, n_max, Mq, 16)[:, :, q0, 0] = 0.0
    clamped.append(q0)
    if acqf == UCB:
        a["acqf_param"][1] = 0.0
    else:
        for qq in clamped:
            shift_mu(a, qq, a["acqf_param"][a["group"][qq]] + 1e-5)
    return a, clamped


TAIL_U = {"span": np.linspace(-9.0, 9.0, 7), "deep": np.full(7, -45.0)}


def set_TAIL(mode, kind, acqf):
    a = make_set("TAIL", (17,), 17, 3, 2, kind, acqf, (7,), noise=0.5)
    _, v = posterior64(a)
    for q, u in enumerate(TAIL_U[mode]):
        shift_mu(a, q, a["acqf_param"][0] - u * np.sqrt(v[q]))
    return a


FA_GROUPS = ((7, 1), (8, 2), (9, 7), (96, 64), (8, 8), (7, 9), (9, 63))
FB_GROUPS = ((9, 9), (7, 2), (8, 1))


def set_FA(kind, acqf):
    return make_set("FA", [n for n, _ in FA_GROUPS], 96, 3, 15, kind, acqf, (2,) * 7, fs=[f for _, f in FA_GROUPS], F_max=64)


def set_FB(kind, acqf):
    return make_set("FB", [n for n, _ in FB_GROUPS], 9, 9, 2, kind, acqf, (2,) * 3, fs=[f for _, f in FB_GROUPS], F_max=9, small_last=True)


def set_FARF(kind, acqf):
    return make_set("FARF", (9, 17), 17, 3, 2, kind, acqf, (3, 3), fs=(7, 2), F_max=9, far_last=FAR_F)


FANTASY_SETS = dict(FA=set_FA, FB=set_FB, FARF=set_FARF)


def to_strips(a):
    """The value layout of the same call: one strip per group holding column 0 of the group's queries, the first one repeated up to 16,
    then a padding strip.  -> (arrays, the query of every candidate)"""
    T, n_max, G = a["T"], a["n_max"], a["G"]
    qs = []
    for g in list(range(G)) + [-1]:
        mine = [q for q in range(len(a["group"])) if a["group"][q] == g]
        qs += mine + [mine[0]] * (16 - len(mine))
    qs = np.array(qs)
    cov = a["cov"].reshape(T, n_max, -1, 16)
    b = dict(a)
    b.update(mu=np.ascontiguousarray(a["mu"][:, qs, 0]), var=np.ascontiguousarray(a["var"][:, qs, 0]), cov=np.ascontiguousarray(cov[:, :, qs, 0]),
             Xq=np.ascontiguousarray(a["Xq"][qs]), group=np.array(list(range(G)) + [-1], dtype=np.int32), Mq=len(qs))
    return b, qs


# ------------------------------------------------------------------------------------------------------------------
# drivers
def _entries(a):
    return ("fantasy", "fantasy_score") if "alpha_f" in a else ("acqf", "score")


_REFS = {}


def cached_reference(a, tag):
    """One reference per (set, family, acquisition function, layout) for all the backends and tests that use the unchanged set."""
    k = (tag, a["name"], a["kind"], a["acqf"], is_strips(a))
    if k not in _REFS:
        _REFS[k] = reference(a)
    return _REFS[k]


def check_set(be, a, label, tag=None, scale=None):
    """One set through both layouts of its kernel family: the query layout with every output, again with grad / mu_out / var_out NULL (the
    same value, bit for bit), and column 0 re-laid as strips.  -> the query layout's outputs and reference."""
    query, strip = _entries(a)
    post = query == "acqf"
    ref = reference(a) if tag is None else cached_reference(a, tag)
    got = be.run(query, a, grad=True, post=post)
    hold(label, query, a, ref, got, scale)
    bare = be.run(query, a, grad=False, post=False)
    assert bare["grad"] is None and bare["mu"] is None
    assert np.array_equal(bare["value"], got["value"], equal_nan=True), f"{label}: the value changes when grad / mu_out / var_out are NULL"
    b, qs = to_strips(a)
    sref = reference(b) if tag is None else cached_reference(b, tag)
    sgot = be.run(strip, b, grad=False, post=post)
    hold(label + " strips", strip, b, sref, sgot, scale)
    return got, ref


def check_junk_columns(be, a, label):
    """No output depends on the columns c > D of mu / var / cov."""
    query, _ = _entries(a)
    D = a["D"]
    if D == 15:
        return
    g1 = be.run(query, a, grad=True, post=query == "acqf")
    b = dict(a, mu=a["mu"].copy(), var=a["var"].copy(), cov=a["cov"].copy())
    b["mu"][..., 1 + D:], b["var"][..., 1 + D:] = -7.0 * JUNK, 0.5
    cv = b["cov"].reshape(a["T"], a["n_max"], -1, 16)
    cv[..., 1 + D:] = np.where(np.isnan(cv[..., 1 + D:]), np.nan, 11.0)
    g2 = be.run(query, b, grad=True, post=query == "acqf")
    for k, x in g1.items():
        assert x is None or np.array_equal(x, g2[k], equal_nan=True), f"{label} {k}: the output depends on the columns past D"


def check_clamp(be, kind, acqf):
    a, clamped = set_CLAMP(kind, acqf)
    label = f"studies-CLAMP-{FAMILY[kind]}-{ACQ[acqf]}"
    got, ref = check_set(be, a, label)
    thr = 0.0 if acqf == UCB else 1e-9
    v = ref["ref"]["var"]
    assert (v[clamped] <= thr).all(), f"{label}: the set does not clamp: var = {v[clamped]}"
    assert v[int(np.nonzero(a["group"] == CLAMP_ZERO_GROUP)[0][0])] == 0
    b = dict(a, var=a["var"].copy())
    b["var"][:, :, 1:] = 3.0 * b["var"][:, :, 1:] + 1.0
    g2 = be.run("acqf", b, grad=True, post=True)["grad"]
    dead = clamped + ([int(q) for q in np.nonzero(a["group"] == 1)[0]] if acqf == UCB else [])      # (beta = 0: every query of group 1)
    assert np.array_equal(got["grad"][dead], g2[dead]), f"{label}: the clamped partial d A / d var is live in the gradient"
    free = int(np.nonzero(a["group"] == 0)[0][1])
    assert (got["grad"][free] != g2[free]).all(), f"{label}: the unclamped query must depend on var's gradient columns"


def check_tail(be, mode, kind, acqf):
    a = set_TAIL(mode, kind, acqf)
    label = f"studies-TAIL-{mode}-{FAMILY[kind]}-{ACQ[acqf]}"
    pre = reference(a)
    u = pre["cond"][0]["u"]
    if mode == "span":
        assert float(u.min()) < -8.9 and float(u.max()) > 8.9, f"{label}: u spans {float(u.min())} .. {float(u.max())}"
        check_set(be, a, label)
        return
    assert float(u.max()) <= -40.0
    if acqf == EI:      # an exact zero within the absolute term: the cap against sigma
        assert float(np.abs(pre["ref"]["value"]).max()) < 1e-300 and float(np.abs(pre["ref"]["grad"]).max()) < 1e-300
        sigma = float(np.sqrt(pre["cond"][0]["v"].max()))
        query, strip = _entries(a)
        got = be.run(query, a, grad=True, post=False)
        hold(label, query, a, pre, got, scale=sigma)
        b, _ = to_strips(a)
        hold(label + " strips", strip, b, reference(b), be.run(strip, b, grad=False, post=False), scale=sigma)
    else:
        got, _ = check_set(be, a, label)
        assert np.isfinite(got["value"][:-1]).all(), f"{label}: LogEI must stay finite"


def _same_elsewhere(label, good, bad, keep):
    for k, x in good.items():
        if x is not None:
            assert np.array_equal(x[keep], bad[k][keep], equal_nan=True), f"{label} {k}: the other groups changed"


REFUSALS = (("info", 3), ("n_points", 0), ("n_points", "n_max + 1"), ("n_fant", 0), ("n_fant", "F_max + 1"))


def check_refusals(be, a, label, victim):
    """info != 0, n_points outside 1 .. n_max, n_fant outside 1 .. F_max: NaN for that group only, in both layouts; the others bit for bit
    those of the clean call and within their bounds."""
    query, strip = _entries(a)
    post = query == "acqf"
    good = be.run(query, a, grad=True, post=post)
    b0, qs = to_strips(a)
    sgood = be.run(strip, b0, grad=False, post=post)
    for field, val in REFUSALS:
        if field == "n_fant" and "alpha_f" not in a:
            continue
        val = {"n_max + 1": a["n_max"] + 1, "F_max + 1": a.get("F_max", 0) + 1}.get(val, val)
        b = dict(a)
        b[field] = a[field].copy()
        b[field][victim] = val
        ref = reference(b)
        assert (ref["state"][a["group"] == victim] == "nan").all()
        bad = be.run(query, b, grad=True, post=post)
        hold(f"{label} {field}={val}", query, b, ref, bad)
        _same_elsewhere(f"{label} {field}={val}", good, bad, a["group"] != victim)
        bs, _ = to_strips(b)
        sbad = be.run(strip, bs, grad=False, post=post)
        hold(f"{label} {field}={val} strips", strip, bs, reference(bs), sbad)
        _same_elsewhere(f"{label} {field}={val} strips", sgood, sbad, rhs_groups(bs) != victim)


def check_nonfinite(be, a, label, q):
    """A NaN coordinate in query q (source columns finite): NaN in all of its outputs, in both layouts; the others within their bounds."""
    query, strip = _entries(a)
    b = dict(a, Xq=a["Xq"].copy())
    b["Xq"][q, a["D"] - 1] = np.nan
    ref = reference(b)
    assert ref["bad_q"][q] and ref["bad_q"].sum() == 1
    hold(label, query, b, ref, be.run(query, b, grad=True, post=query == "acqf"))
    bs, _ = to_strips(b)
    sref = reference(bs)
    assert sref["bad_q"].any()
    hold(label + " strips", strip, bs, sref, be.run(strip, bs, grad=False, post=query == "acqf"))
