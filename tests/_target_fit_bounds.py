"""Long-double reference, a-priori error bound, input sets and shared assertions for the target GP's training objective and its
analytic gradient (csrc/gp_target_fit.hip behind scaml_target_mll_f64, scaml_target_fit_f64 and their batched forms).

Same construction as tests/_posterior_bounds.py, tests/_target_bounds.py and tests/_fit_bounds.py, whose helpers are used here.  The
reference (`reference`) is numpy long double fed exactly the arrays the entry point is handed -- means_t, covs_packed, X, y, m_all,
s_all, the spec block and z -- and writes the formulas on full symmetric matrices, independently of the kernel's packed / tiled
formulation:
  theta = lo + (hi - lo) sigmoid(z), w = z[D + 2:],  K = sum_t w_t^2 C_t / s^2 + os k(X, X; l) + (noise + jitter) I  (gpytorch's clamp
  of d2 at 1e-30 before the Matern root),  r = y - (M w - m_all) / s,  L, alpha, K^-1,  G = (alpha alpha^T - K^-1) / 2,
  value = (-(quad + logdet + n log 2pi) / 2 + log priors) / n,
  d / dw_i = (<G, 2 w_i C_i / s^2> + alpha . M_i / s + prior') / n,   d / dz_q = (<G, dK / dtheta_q> + prior') dtheta_q / dz_q / n.

The ABI hands out only value, grad, info and jitter: no intermediate can be fed back, so the conditioning of K enters the bound.  It
is a first-order componentwise perturbation bound, every term evaluated from the reference's own quantities, no constant fitted to
what a kernel returns.  u = 2^-53, g_k = k u / (1 - k u), |.| elementwise.

  theta    sigmoid: exp 2 u, the sum, the division: 4 u; (hi - lo), the product, the sum with lo > 0: dTH = 8 u relative on l, os, noise
           (tf_eval, "parameters").  It acts as a relative perturbation of those inputs: 2 dTH d2 on every scaled squared distance,
           dTH on os k and on the noise, dTH |x dlogp/dx| on each log prior; on a gradient entry dTH per factor os and 1 / l_d, and
           the chain factor dth = (hi - lo) s (1 - s), whose 1 - s cancels: (8 + 4 s / (1 - s)) u relative
  E        the perturbation of K that stands for everything up to and including the factorisation:
           task sum   g_{T+8} sum_t |w_t^2 C_t / s^2|: w2 = (w w) ((1 / s) (1 / s)) carries 5 roundings (the reciprocal, its square, w w,
                      the product; `inv_s2`, `c.w2[i]`), each product one, the split accumulators at most T additions, `acc + k` one more
                      (u |K| below)
           kernel     os (S E_d2 + c_k u |k|) + dTH os |k|, E_d2 = g_{D+28} d2: df = (x_a - x_b) invl carries 3 roundings, its square 7, the
                      sum over D at most D - 1 more, the Matern root 2 u on r = 4 u on d2, 2 dTH = 16 u from l.  S = 1/2, 5/6 as in
                      tests/_fit_bounds.py.  c_k = 4 (RBF: exp 2 u, os k), 10 + sqrt5 r (Matern: the constants, the polynomial's five
                      operations, exp 2 u, the products -- and the ROUNDED argument -s5 r of exp, which alone moves e5 by sqrt5 r u:
                      the polynomial's slope does not cancel it)
           diagonal   `k += noise + jit`, then `acc + k`: u (noise + jitter) + u (os + noise + jitter) + u |K_ii| + dTH noise
           factor     sum_k g_{min(i,j)+7} |L_ik| |L_jk| <= g_{min(i,j)+7} (|L| |L^T|)_ij on both paths: element (i, j) is a sum of min(i, j) + 1
                      products, Cholesky's g_{m+1} with m + 1 of them made m + 4 by what follows, 3 to spare.  Column path (square-root-free elimination, `v - f * inv * cb`): three roundings per
                      term and inv = tf_rcp(pivot), an f32 seed and two Newton steps (2^-22 -> 2^-44 -> 2^-88, then the last fma's
                      rounding: 1.01 u; the host build divides: u) against Cholesky's two.
                      Matrix-core path: a column is scaled by rsqrt_pos(pivot) (f32 seed + one Halley step: 1/2 u from the rounded
                      t = d y in e = 1 - t y, u from the last fma, 1e-19 truncation: 2 u) and L_cc = pv rsq: 3 u per column scaling, the
                      updates single fmas: the same count
           panel      matrix-core path only (term added): L_iK = A_iK W_K^T with the EXPLICIT inverse W_K of the diagonal tile is not a
                      triangular solve.  With M_K = |L_KK|^T |W_K|^T:  g_40 |L_iK| M_K (I + M_K) |L_KK|^T on block (i, K)
                      (g_16 of the tile product and g_20 |W| |L_KK| |W| of W, 4 to spare)
  E_r      g_{T+2} |w|^T |M| / s (the two accumulators take two products per trip) + 4 u |(m - m_all) / s| + u |r|
  maps     |d(quad + logdet)| <= |alpha|^T E |alpha| + sum (|K^-1| o E) + 2 |alpha|^T E_r,  |dK^-1| <= |K^-1| E |K^-1|,
           |dalpha| <= |K^-1| (E |alpha| + E_r),  E_G = (E_Kinv + |alpha| E_alpha^T + E_alpha |alpha|^T + 3 u |alpha alpha^T|) / 2
  inverses L^-1 is formed explicitly on both paths (identity rows riding along, scaled by 1 / sqrt(pivot); X by tile products with
           the W_i), then K^-1 = X^T X and alpha = X^T (X r):  E_Linv = g_{n+c} |L^-1| |L| |L^-1| (c = 6 column, 36 matrix core: W's g_20
           and the tile product's g_16), E_Kinv += 2 |L^-1|^T E_Linv + g_{n+4} |L^-1|^T |L^-1|,
           E_alpha += E_Linv^T |v| + |L^-1|^T E_Linv |r| + g_{n+4} |L^-1|^T |L^-1| |r|,  quad += 2 |v| (E_Linv |r| + g_{n+4} |L^-1| |r|)
  sums     g_m sum |terms|, m the longest chain of additions a term passes through, counted for the device (64 lanes, 512 threads,
           8 waves) and for the single-threaded host build / the numpy stand-in (1, 1, 1):
           quad      g_{n+16} (column path: n subtractions into the border element; matrix core: one term per thread, the wave's 6, 8 waves)
           logdet    ceil(n / threads) + 6 + waves, 2 u per logarithm, and 3 u on each L_ii the matrix-core path takes the logarithm of
           priors    ceil((D + 2) / threads) + ceil(T / threads) + 6 + waves (`lp`, tf_block_sum); a log prior itself 24 u of the magnitudes
                     of its terms (log 2 u, theta's dTH, the square)
           weights   ceil(E / (4 lanes)) + 2 (the 4-way split) + 6 (wave) + 12 (the products, 2 w inv_s2, the prior, 1 / n)
           theta     ceil(E / threads) + 6 + waves (c.part) + 12
           (6: the depth of the 64-lane reduction; on one lane it is 0)
  E_dK     os: E_k;  noise: 0;  l_d: dK = -2 os dk df_d^2 / l_d,  E = (2 os / l_d) (E_dk df^2 + |dk| E_df2 + E_dk E_df2) + (8 u + 2 dTH) |dK|,
           E_df2 = 24 u df^2 (7 roundings, 2 dTH), E_dk = S' E_d2 + c_k u |dk|
  second order   rho = || |K^-1| E ||_inf; every first-order term is multiplied by 1 / (1 - rho), and rho <= 1e-6 is asserted
One bound per path: they differ in the panel term and in c of E_Linv; the chains depend on who executes (device / one thread).

Caps (conditions on the INPUTS, asserted with every comparison): the value's bound at most CAP = 1e-8 of
(|quad| + sum |2 log L_ii| + n log 2pi + sum |log prior terms|) / (2 n); each gradient entry's bound at most CAP of S_p (g_p with every
term in magnitude) and at most GRAD_CAP_G = 1e-6 of the start point's largest |g_p|.

Input sets (`make_problem`, `starts`): X uniform in the unit cube, T smooth source means, source covariances 0.02-scale random PSD
matrices, y a smooth function + 0.3 unit noise; start points written through interval_inverse_transform from l = 0.5 sqrt(D) (0.8 .. 1.2),
os in 0.1 .. 0.15, noise in 7e-3 .. 9e-3 (s <= 0.9 keeps 1 - s from cancelling), weights 0.02 + 2 U / T with (T >= 3) task 1 at 1e-6 of
task 0 and task 2 exactly w_lower.  B = 3 start points per launch, the output buffers one guard row longer and full of SENTINEL.
The binding cap is GRAD_CAP_G: the chain factor of the raw noise, (hi - lo) s (1 - s) <= 2.5e-3, shrinks the largest gradient entry,
while S_p of the outputscale and the lengthscales grows with os n / noise.  With os up to 0.3 and noise down to 5e-3 the reference
alone broke it at n >= 97 for the smoothest sets (RBF, D <= 6: up to 1.1e-5 of max |g|), hence the lower halves of both ranges, RBF at
n >= 112 only with D = 1 (column path) or D >= 12, and the largest-n set at (T, D) = (4, 4) in the Matern family.
tests/test_target_fit_bounds.py asserts the caps for the device's chains and paths on every set, without any kernel.
Shapes: CASES below; the dispatch (target_fit_mfma_shape, csrc/gp_target_params.h) sends n <= 112 to the matrix cores, everything
larger and everything under scaml_debug_target_fit_path(1) to the columns.  E = n (n + 1) / 2 < 256 for n <= 21 (n = 1 .. 17 here);
E mod 256 != 0 for every n in the list (32: 528, 64: 2080, 128: 8256, ...).
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from tests import _fit_bounds as FB
from tests._dispatch import target_fit_plan
from tests._fit_bounds import GRAD_CAP_G, LOG_2PI, grad_within
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, SENTINEL, U, Quantity, Ratios, _kernel, _S, gamma, inverse_lower
from tests._target_bounds import FAMILY, within
from tests import _target_bounds as TB
from tests._target_problem import TARGET_SPEC

RHO_MAX = 1e-6
D_TH = 8 * U
OS_RANGE, NZ_RANGE = (0.1, 0.15), (7e-3, 9e-3)
GUARD = 1                                  # rows past B in every output buffer
Arith = namedtuple("Arith", "lanes nthr nwave")
DEVICE_ARITH, SERIAL_ARITH = Arith(64, 512, 8), Arith(1, 1, 1)
RATIOS = Ratios()      # (backend path, family, output) -> [largest error / bound, largest bound / scale]
NOTES = []             # the conditional comparisons that were not made, with their figures


def report():
    return [f"{k[0]} {k[1]} {k[2]}: largest error / bound {e:.3e}, largest bound / scale {c:.3e}" for k, (e, c) in sorted(RATIOS.items())] + NOTES


# ------------------------------------------------------------------------------------------------------------------
# input sets
Case = namedtuple("Case", "path n T D kind forced")      # path "mfma" / "col"; forced: through scaml_debug_target_fit_path(1); n None: the limit


def _cases():
    R, M = KIND_RBF, KIND_MATERN52
    mfma = [(1, 1, 1, R), (2, 3, 6, M), (15, 4, 16, R), (16, 5, 1, M), (17, 15, 6, R), (32, 16, 16, M), (33, 17, 1, R), (96, 20, 6, M), (97, 33, 6, R),
            (111, 70, 1, M), (112, 4, 6, M), (112, 33, 16, R)]
    col = [(113, 8, 6, M), (128, 9, 1, R), (128, 5, 6, M), (None, 4, 4, M)]
    forced = [(1, 1, 1, M), (2, 3, 6, R), (7, 9, 16, M), (31, 8, 1, R), (32, 16, 6, M), (33, 17, 1, R), (63, 4, 6, M), (64, 5, 16, R), (65, 20, 1, M),
              (80, 33, 6, R), (80, 70, 1, M)]
    return [Case("mfma", *c, False) for c in mfma] + [Case("col", *c, False) for c in col] + [Case("col", *c, True) for c in forced]


CASES = _cases()
COLUMN_CASES = [c for c in CASES if c.path == "col"]
FAULT_CASE = Case("mfma", 33, 17, 6, KIND_MATERN52, False)      # T mod 4 = 1, a partial last tile holding row n - 1 alone, three tiles, D >= 2
NAN_CASES = [Case("mfma", 33, 5, 3, KIND_MATERN52, False), Case("mfma", 17, 4, 2, KIND_RBF, False), Case("col", 20, 5, 3, KIND_MATERN52, True),
             Case("col", 20, 4, 2, KIND_RBF, True)]
RAGGED = dict(sizes=(1, 112, 113, 40), T=9, D=12)               # both sides of 112 and one n_s = 1: strides ldn, ldE of n_max = 113
# (the third: P = 74 > 64, the optimiser's bookkeeping by all waves instead of one)
REFIT_CASES = [Case("mfma", 20, 5, 3, KIND_MATERN52, False), Case("col", 20, 5, 3, KIND_RBF, True), Case("mfma", 16, 70, 2, KIND_RBF, False)]


def case_id(c: Case) -> str:
    return f"{c.path}{'-forced' if c.forced else ''}-n{'max' if c.n is None else c.n}-T{c.T}-D{c.D}-{FAMILY[c.kind]}"


def make_problem(n, T, D, kind, seed=0):
    """One training set in the layouts of (8): means_t (T, n), covs_p (T, n (n + 1) / 2), X, y, m_all, s_all, the spec block."""
    rng = np.random.default_rng([20261020, n, T, D, kind, seed])
    X = rng.uniform(size=(n, D))
    m_all, s_all = 0.7, 1.9
    dirs, ph = rng.normal(size=(T, D)) * 2.0 / np.sqrt(D), rng.uniform(size=T) * 6.28
    means_t = m_all + s_all * (0.8 * np.sin(X @ dirs.T + ph).T + 0.1 * np.arange(T)[:, None] / T)
    ia, ib = np.tril_indices(n)
    covs_p = np.empty((T, ia.size))
    for t in range(T):
        A = rng.normal(size=(n, min(n, 6) + 2))
        covs_p[t] = (s_all * s_all * 0.02 * (A @ A.T) / A.shape[1])[ia, ib]
    y = np.sin(3.0 * X.sum(-1) / np.sqrt(D)) + 0.3 * rng.normal(size=n)
    return dict(means_t=means_t, covs_p=covs_p, X=X, y=y, m_all=m_all, s_all=s_all, n=n, T=T, D=D, kind=kind, spec=np.array(TARGET_SPEC, dtype=np.float64))


def starts(prob, B=3, seed=0, os_range=OS_RANGE, nz_range=NZ_RANGE):
    """(B, P) start points of the recipe, the raw values through the oracle's interval_inverse_transform."""
    import torch

    from oracle import gp_oracle as O

    T, D, spec = prob["T"], prob["D"], prob["spec"]
    rng = np.random.default_rng([20261021, prob["n"], T, D, seed])
    th = np.concatenate([0.5 * np.sqrt(D) * rng.uniform(0.8, 1.2, size=(B, D)), rng.uniform(*os_range, size=(B, 1)), rng.uniform(*nz_range, size=(B, 1))], 1)
    lo = torch.tensor([spec[0]] * D + [spec[2], spec[4]], dtype=torch.float64)
    hi = torch.tensor([spec[1]] * D + [spec[3], spec[5]], dtype=torch.float64)
    raw = O.interval_inverse_transform(torch.from_numpy(th), lo, hi).numpy()
    w = 0.02 + rng.uniform(size=(B, T)) * 2.0 / T
    if T >= 3:
        w[:, 1] = 1e-6 * w[:, 0]
        w[:, 2] = spec[18]
    return np.ascontiguousarray(np.concatenate([raw, w], 1))


def jitter_problem():
    """The duplicated-points problem of tests/test_target_fit_gpu.py: a singular kernel part under 1e-8 noise minus 6e-8 from the source
    term fails without jitter and with 1e-8 and passes with 1e-7.  Returns (problem, z (1, P))."""
    prob = make_problem(12, 3, 2, KIND_RBF, seed=4)
    prob["X"][5] = prob["X"][4]
    prob["X"][7] = prob["X"][4]
    w = 0.1
    c = 6e-8 * prob["s_all"] ** 2 / (3 * w * w)
    ia, ib = np.tril_indices(12)
    prob["covs_p"] = np.ascontiguousarray(np.broadcast_to((-c * np.eye(12))[ia, ib], (3, ia.size)))
    z = starts(prob, B=1)
    z[:, 3], z[:, 2], z[:, 4:] = -40.0, 5.0, w      # raw noise -> 1e-8, outputscale ~ 99
    return prob, z


def pack_batch(probs, fill=np.nan):
    """The (S, ...) layouts of (8b); everything past a problem's n_s is `fill` (it is never read)."""
    S, T, D = len(probs), probs[0]["T"], probs[0]["D"]
    n_max = max(p["n"] for p in probs)
    e_max = n_max * (n_max + 1) // 2
    b = dict(means_t=np.full((S, T, n_max), fill), covs_p=np.full((S, T, e_max), fill), X=np.full((S, n_max, D), fill), y=np.full((S, n_max), fill),
             n_points=np.array([p["n"] for p in probs], dtype=np.int32), m_all=np.array([p["m_all"] for p in probs]),
             s_all=np.array([p["s_all"] for p in probs]), S=S, T=T, D=D, n_max=n_max, kind=probs[0]["kind"], spec=probs[0]["spec"])
    for s, p in enumerate(probs):
        n = p["n"]
        b["means_t"][s, :, :n], b["covs_p"][s, :, :n * (n + 1) // 2], b["X"][s, :n], b["y"][s, :n] = p["means_t"], p["covs_p"], p["X"], p["y"]
    return b


# ------------------------------------------------------------------------------------------------------------------
# reference and bound
def cholesky_ld(K):
    """Lower Cholesky factor in long double, column by column; None if a pivot is not positive."""
    n = K.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = K[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _prior(pr, x):
    """(log p, d log p / dx, magnitudes of the terms of log p, of its derivative, and the magnitude its evaluation error scales with)."""
    kind, p1, p2 = int(pr[0]), LD(pr[1]), LD(pr[2])
    x = LD(x)
    zero = np.zeros(x.shape, dtype=LD)
    if kind == 0:
        return zero, zero, zero, zero, zero
    lx = np.log(x)
    if kind == 1:
        c0 = p1 * np.log(p2) - LD(math.lgamma(float(p1)))
        mag = np.abs(c0) + np.abs((p1 - 1) * lx) + np.abs(p2 * x)
        return c0 + (p1 - 1) * lx - p2 * x, (p1 - 1) / x - p2, mag, np.abs((p1 - 1) / x) + p2, mag
    c0 = -np.log(p2) - LOG_2PI / 2
    uu = (lx - p1) / p2
    return (c0 - lx - uu * uu / 2, -(1 + (lx - p1) / (p2 * p2)) / x, np.abs(c0) + np.abs(lx) + uu * uu / 2, (1 + (np.abs(lx) + np.abs(p1)) / (p2 * p2)) / np.abs(x),
            np.abs(c0) + np.abs(lx) + ((np.abs(lx) + np.abs(p1)) / p2) ** 2)


def unpack(cp, n):
    """(T, >= n (n + 1) / 2) packed lower -> (T, n, n) symmetric long double."""
    ia, ib = np.tril_indices(n)
    C = np.zeros((cp.shape[0], n, n), dtype=LD)
    C[:, ia, ib] = cp[:, :ia.size]
    C[:, ib, ia] = cp[:, :ia.size]
    return C


Ref = namedtuple("Ref", "value E_value S_value grad E_grad S_grad rho parts")


def reference(prob, z, path, arith=DEVICE_ARITH, jit=0.0):
    """Value and gradient at one z (P,) in long double with their bounds and cap scales (the module docstring); None if K is not
    positive definite in long double."""
    n, T, D, kind, spec = prob["n"], prob["T"], prob["D"], prob["kind"], prob["spec"]
    lo, hi = LD([spec[0]] * D + [spec[2], spec[4]]), LD([spec[1]] * D + [spec[3], spec[5]])
    sg = 1 / (1 + np.exp(-LD(z[:D + 2])))
    th, dth = lo + (hi - lo) * sg, (hi - lo) * sg * (1 - sg)
    l, os_, nz = th[:D], th[D], th[D + 1]
    w, s, m_all = LD(z[D + 2:]), LD(prob["s_all"]), LD(prob["m_all"])
    C = unpack(prob["covs_p"], n)
    aC = np.abs(C)
    cw = w * w / (s * s)
    Ksrc, Asrc = np.einsum("t,tab->ab", cw, C), np.einsum("t,tab->ab", np.abs(cw), aC)
    a = LD(prob["X"][:n]) / l
    diff = a[:, None, :] - a[None, :, :]
    df2 = diff * diff
    d2 = df2.sum(-1)
    k, dk = _kernel(d2, kind)
    idx = np.arange(n)
    k[idx, idx], dk[idx, idx] = 1, 0
    K = Ksrc + os_ * k
    K[idx, idx] += nz + LD(jit)
    M = LD(prob["means_t"][:, :n])
    mw = w @ M
    qm = (mw - m_all) / s
    r = LD(prob["y"][:n]) - qm
    L = cholesky_ld(K)
    if L is None:
        return None
    Li = inverse_lower(L)
    Kinv = Li.T @ Li
    v = Li @ r
    alpha = Li.T @ v
    quad = v @ v
    logs = 2 * np.log(np.diagonal(L))
    pr = [_prior(spec[6:9], l), _prior(spec[9:12], th[D:D + 1]), _prior(spec[12:15], th[D + 1:]), _prior(spec[15:18], w)]
    lp, lpmag, lperr = (sum(p[i].sum() for p in pr) for i in (0, 2, 4))
    dp_th, dpmag_th = np.concatenate([p[1] for p in pr[:3]]), np.concatenate([p[3] for p in pr[:3]])
    dp_w, dpmag_w = pr[3][1], pr[3][3]
    c2pi = n * LOG_2PI
    value = (-(quad + logs.sum() + c2pi) / 2 + lp) / n
    S_value = (np.abs(quad) + np.abs(logs).sum() + c2pi + lpmag) / (2 * n)
    aa = np.outer(alpha, alpha)
    G = (aa - Kinv) / 2
    aG = np.abs(G)
    s2 = s * s
    GC, aGC = np.einsum("ab,tab->t", G, C), np.einsum("ab,tab->t", aG, aC)
    gw = (GC * 2 * w / s2 + (M @ alpha) / s + dp_w) / n
    S_w = (aGC * 2 * np.abs(w) / s2 + (np.abs(M) @ np.abs(alpha)) / s + dpmag_w) / n
    dK = [-2 * os_ * dk * df2[:, :, d] / l[d] for d in range(D)]
    gsum = np.array([(G * x).sum() for x in dK] + [(G * k).sum(), G[idx, idx].sum()], dtype=LD)
    Ssum = np.array([(aG * np.abs(x)).sum() for x in dK] + [(aG * np.abs(k)).sum(), aG[idx, idx].sum()], dtype=LD)
    gth = (gsum + dp_th) * dth / n
    S_th = (Ssum + dpmag_th) * dth / n
    grad, S_grad = np.concatenate([gth, gw]), np.concatenate([S_th, S_w])

    # ---- the bound ----
    mat = kind == KIND_MATERN52
    S0, S1 = _S[kind]
    E_d2 = gamma(D + 28) * d2
    ck = (10 + np.sqrt(LD(5)) * np.sqrt(np.maximum(d2, LD(1e-30)))) if mat else 4
    ak, adk = np.abs(k), np.abs(dk)
    E_k, E_dk = S0 * E_d2 + ck * U * ak, S1 * E_d2 + ck * U * adk
    E_k[idx, idx] = 0
    aL, aLi, aKinv, aal, av, ar = np.abs(L), np.abs(Li), np.abs(Kinv), np.abs(alpha), np.abs(v), np.abs(r)
    cinv = 6 if path == "col" else 36
    mn = np.minimum(idx[:, None], idx[None, :]) + 7                      # element (i, j) sums min(i, j) + 1 products
    gfac = mn * U / (1 - mn * U)
    E = gamma(T + 8) * Asrc + U * np.abs(K) + os_ * (E_k + D_TH * ak) + gfac * (aL @ aL.T)
    E[idx, idx] += U * (nz + jit) + U * (os_ + nz + jit) + D_TH * nz
    if path == "mfma":
        nb = (n + 15) // 16
        Lp = np.eye(16 * nb, dtype=LD)
        Lp[:n, :n] = aL
        Ep = np.zeros((16 * nb, 16 * nb), dtype=LD)
        for kb in range(nb - 1):
            sl = slice(16 * kb, 16 * kb + 16)
            Lkk = Lp[sl, sl]
            Mk = Lkk.T @ np.abs(inverse_lower(Lkk)).T
            Ep[16 * kb + 16:, sl] = gamma(40) * (Lp[16 * kb + 16:, sl] @ (Mk @ (np.eye(16, dtype=LD) + Mk) @ Lkk.T))
        E += Ep[:n, :n] + Ep[:n, :n].T
    E_m = gamma(T + 2) * (np.abs(w) @ np.abs(M))
    E_r = E_m / s + 4 * U * np.abs(qm) + U * ar
    rho = float((aKinv @ E).sum(1).max())
    amp = 1 / (1 - min(rho, 0.5))
    E_Linv = gamma(n + cinv) * (aLi @ aL @ aLi)
    gn4 = gamma(n + 4)
    E_Kinv = (aKinv @ E @ aKinv) * amp + 2 * (aLi.T @ E_Linv) + gn4 * (aLi.T @ aLi)
    E_alpha = (aKinv @ (E @ aal + E_r)) * amp + E_Linv.T @ av + aLi.T @ (E_Linv @ ar) + gn4 * (aLi.T @ (aLi @ ar))
    depth = 6 if arith.lanes > 1 else 0
    ceil = lambda x, y: -(-x // y)   # noqa: E731
    E_quad = (aal @ E @ aal + 2 * (aal @ E_r)) * amp + 2 * (av @ (E_Linv @ ar + gn4 * (aLi @ ar))) + gamma(n + 16) * quad
    m_ld = ceil(n, arith.nthr) + depth + arith.nwave
    E_logdet = (aKinv * E).sum() * amp + (gamma(m_ld) + 2 * U) * np.abs(logs).sum() + 6 * U * n
    m_lp = ceil(D + 2, arith.nthr) + ceil(T, arith.nthr) + depth + arith.nwave
    E_lp = 24 * U * lperr + D_TH * (np.abs(dp_th) * th).sum() + gamma(m_lp) * lpmag
    E_value = (E_quad + E_logdet + 2 * U * c2pi + 2 * U * np.abs(quad + logs.sum() + c2pi)) / (2 * n) + E_lp / n + 3 * U * np.abs(value)
    E_G = (E_Kinv + np.outer(aal, E_alpha) + np.outer(E_alpha, aal) + 3 * U * np.abs(aa)) / 2
    Epk = n * (n + 1) // 2
    m_w = ceil(Epk, 4 * arith.lanes) + 2 + depth + 12
    E_w = (np.einsum("ab,tab->t", E_G, aC) * 2 * np.abs(w) / s2 + (np.abs(M) @ E_alpha) / s + gamma(m_w) * (S_w * n - dpmag_w) + 24 * U * dpmag_w) / n + 4 * U * np.abs(gw)
    m_t = ceil(Epk, arith.nthr) + depth + arith.nwave + 12
    gm = gamma(m_t)
    E_sum = np.zeros(D + 2, dtype=LD)
    for d in range(D):
        adK = np.abs(dK[d])
        E_df2 = 24 * U * df2[:, :, d]
        E_dKd = (2 * os_ / l[d]) * (E_dk * df2[:, :, d] + adk * E_df2 + E_dk * E_df2) + (8 * U + 2 * D_TH) * adK
        E_sum[d] = (aG * E_dKd + E_G * adK + E_G * E_dKd).sum() + gm * (aG * adK).sum()
    E_sum[D] = (aG * E_k + E_G * ak + E_G * E_k).sum() + gm * (aG * ak).sum()
    E_sum[D + 1] = E_G[idx, idx].sum() + gm * aG[idx, idx].sum()
    rel = (12 + 4 * sg / (1 - sg)) * U
    E_th = (E_sum + 24 * U * dpmag_th) * dth / n + rel * np.abs(gth)
    parts = dict(theta=th, dth=dth, K=K, L=L, alpha=alpha, G=G, quad=quad, logdet=logs.sum(), E=E)
    return Ref(value, E_value, float(S_value), grad, np.concatenate([E_th, E_w]), S_grad, rho, parts)


# ------------------------------------------------------------------------------------------------------------------
# check drivers.  A backend has: name, arith, max_n(T, D), mll(prob, z, forced) / mll_batched(batch, z, forced) -> dict(value, grad, info,
# jitter) of B + GUARD rows handed over full of SENTINEL (info: -7), fit(prob, z0, forced, max_iter) / fit_batched(batch, z0, forced, max_iter)
# -> dict(z, value, info, jitter, stats), path_of(n, T, D, forced) -> "mfma" / "col".
def _guard(label, out, rows):
    for k in ("value", "grad", "jitter"):
        assert (out[k][rows:] == SENTINEL).all(), f"{label}: {k} was written past row {rows}"
    assert (out["info"][rows:] == -7).all(), f"{label}: info was written past row {rows}"


def hold_row(label, key, prob, z, value, grad, path, arith, jit=0.0, want_grad=True):
    """One row's value (and gradient) against the reference at z, rho and the caps asserted."""
    ref = reference(prob, z, path, arith, jit)
    assert ref is not None, f"{label}: the reference's K is not positive definite"
    assert ref.rho <= RHO_MAX, f"{label}: rho = {ref.rho:.3e} exceeds {RHO_MAX} -- the input set is ill-chosen"
    within(label, key + ("value",), np.asarray(value), Quantity(np.asarray(ref.value), np.asarray(ref.E_value), ref.S_value))
    RATIOS.note(key + ("value",), *TB.RATIOS[key + ("value",)])
    if want_grad:
        grad_within(label, key + ("grad",), grad, ref.grad, ref.E_grad, ref.S_grad)
        RATIOS.note(key + ("grad",), *FB.RATIOS[key + ("grad",)])
    return ref


def assert_caps(label, ref: Ref):
    """The conditions on the inputs alone (no kernel): rho and the three caps of one start point."""
    assert ref is not None and ref.rho <= RHO_MAX, f"{label}: rho"
    assert ref.E_value <= CAP * ref.S_value, f"{label}: the value's bound {float(ref.E_value):.3e} exceeds {CAP} of {ref.S_value:.3e}"
    gmax = np.abs(ref.grad).max()
    assert (ref.E_grad <= CAP * ref.S_grad).all() and (ref.E_grad <= GRAD_CAP_G * gmax).all(), (
        f"{label}: gradient caps, bound / S_p {float((ref.E_grad / ref.S_grad).max()):.3e}, bound / max |g| {float((ref.E_grad / gmax).max()):.3e}")


def device_path(n, T, D, forced=False):
    """The factorisation the launcher's plan takes (forced: through scaml_debug_target_fit_path(1)).  By shape every set here fits the
    matrix-core footprint up to n = 112, which tests/test_target_fit_bounds.py asserts."""
    return "mfma" if target_fit_plan(n, T, D, mode=1 if forced else 0).use_mfma else "col"


def resolve(be, c: Case) -> Case:
    return c._replace(n=be.max_n(c.T, c.D)) if c.n is None else c


def check_mll(be, c: Case, B=3):
    """One shape through the single-problem entry: info / jitter exact, the guard rows untouched, every start within its bounds."""
    c = resolve(be, c)
    assert be.path_of(c.n, c.T, c.D, c.forced) == c.path, f"{case_id(c)}: the dispatch takes the other path"
    prob = make_problem(c.n, c.T, c.D, c.kind)
    z = starts(prob, B)
    out = be.mll(prob, z, c.forced)
    label = case_id(c)
    _guard(label, out, B)
    assert (out["info"][:B] == 0).all() and (out["jitter"][:B] == 0.0).all(), f"{label}: info {out['info'][:B]}, jitter {out['jitter'][:B]}"
    key = (f"{be.name}[{c.path}]", FAMILY[c.kind])
    for b in range(B):
        hold_row(f"{label} start {b}", key, prob, z[b], out["value"][b], out["grad"][b], c.path, be.arith)
    return out


def check_jitter(be, forced):
    """The duplicated-points problem: info 0 and jitter 1e-7 exactly; the value within its bound with (noise + 1e-7) I in the reference
    if rho keeps the condition, otherwise its sign and finiteness only (noted)."""
    prob, z = jitter_problem()
    out = be.mll(prob, z, forced)
    _guard("jitter set", out, 1)
    assert out["info"][0] == 0 and out["jitter"][0] == 1e-7, f"jitter set: info {out['info'][0]}, jitter {out['jitter'][0]}"
    path = be.path_of(prob["n"], prob["T"], prob["D"], forced)
    ref = reference(prob, z[0], path, be.arith, jit=1e-7)
    assert ref is not None
    ok = ref.rho <= RHO_MAX and ref.E_value <= CAP * ref.S_value
    if ok:
        hold_row("jitter set", (f"{be.name}[{path}]", "rbf-jitter"), prob, z[0], out["value"][0], None, path, be.arith, jit=1e-7, want_grad=False)
    else:
        note = (f"jitter set ({be.name}, {path}): rho = {ref.rho:.3e}, bound / scale = {float(ref.E_value / ref.S_value):.3e}: the value is held to "
                f"info, jitter, sign and finiteness only")
        if note not in NOTES:
            NOTES.append(note)
        assert np.isfinite(out["value"][0]) and np.sign(out["value"][0]) == np.sign(float(ref.value)), f"jitter set: value {out['value'][0]!r}, reference {float(ref.value)!r}"
        assert np.isfinite(out["grad"][0]).all()
    return out, ref


def _failed(label, out, row):
    assert out["info"][row] > 0 and np.isnan(out["value"][row]) and not out["grad"][row].any(), (
        f"{label}: a non-finite input must give info > 0, a NaN value and a zero gradient, got info {out['info'][row]}, value {out['value'][row]!r}, "
        f"gradient {out['grad'][row]}")


def check_nan_start(be, c: Case, what):
    """what: "weight" / "ls" -- NaN in start point 1 of 3: that row fails as (8) states, the others stay within their bounds."""
    prob = make_problem(c.n, c.T, c.D, c.kind, seed=1)
    z = starts(prob, 3, seed=1)
    z[1, c.D + 2 + c.T - 1 if what == "weight" else c.D - 1] = np.nan
    out = be.mll(prob, z, c.forced)
    label = f"{case_id(c)} NaN {what}"
    _guard(label, out, 3)
    _failed(label, out, 1)
    key = (f"{be.name}[{c.path}]", FAMILY[c.kind])
    for b in (0, 2):
        assert out["info"][b] == 0 and out["jitter"][b] == 0.0
        hold_row(f"{label} start {b}", key, prob, z[b], out["value"][b], out["grad"][b], c.path, be.arith)


def check_nan_point(be, c: Case, bad):
    """A NaN / inf coordinate of X in problem 1 of a batch of 3: every row of that problem fails, the other problems stay within bounds."""
    probs = [make_problem(c.n - s, c.T, c.D, c.kind, seed=2 + s) for s in range(3)]
    probs[1]["X"][probs[1]["n"] - 1, c.D - 1] = bad
    z = np.stack([starts(p, 2, seed=2) for p in probs])
    out = be.mll_batched(pack_batch(probs), z, c.forced)
    label = f"{case_id(c)} X = {bad}"
    _guard(label, out, 6)
    key = (f"{be.name}[{c.path}]", FAMILY[c.kind])
    for s in range(3):
        for b in range(2):
            row = 2 * s + b
            if s == 1:
                _failed(f"{label} problem 1 start {b}", out, row)
                continue
            assert out["info"][row] == 0 and out["jitter"][row] == 0.0
            hold_row(f"{label} problem {s} start {b}", key, probs[s], z[s, b], out["value"][row], out["grad"][row], c.path, be.arith)


def check_ragged(be, kind, B=2):
    """One ragged batch through the bounds directly: every problem held to the single-problem bound of ITS path."""
    probs = [make_problem(n, RAGGED["T"], RAGGED["D"], kind, seed=5 + s) for s, n in enumerate(RAGGED["sizes"])]
    z = np.stack([starts(p, B, seed=5) for p in probs])
    out = be.mll_batched(pack_batch(probs), z, False)
    S = len(probs)
    _guard("ragged batch", out, S * B)
    assert (out["info"][:S * B] == 0).all() and (out["jitter"][:S * B] == 0.0).all()
    for s, p in enumerate(probs):
        path = be.path_of(p["n"], p["T"], p["D"], False)
        for b in range(B):
            hold_row(f"ragged batch n{p['n']}-{FAMILY[kind]} start {b}", (f"{be.name}[{path}]", FAMILY[kind]), p, z[s, b], out["value"][s * B + b],
                     out["grad"][s * B + b], path, be.arith)
    return out


def _hold_refit(be, label, prob, zr, value, path, key):
    ref = reference(prob, zr, path, be.arith)
    if ref is None or not (ref.rho <= RHO_MAX and ref.E_value <= CAP * ref.S_value):
        NOTES.append(f"{label}: the returned point breaks the caps (rho {None if ref is None else ref.rho}): not compared")
        return 0
    hold_row(label, key, prob, zr, value, None, path, be.arith, want_grad=False)
    return 1


def check_refit(be, c: Case, batched, max_iter=8, B=2):
    """The value reported at the returned z within the value bound of the reference evaluated at THAT z."""
    path = be.path_of(c.n, c.T, c.D, c.forced)
    key = (f"{be.name}[{path}]-refit", FAMILY[c.kind])
    done = 0
    if not batched:
        prob = make_problem(c.n, c.T, c.D, c.kind, seed=7)
        res = be.fit(prob, starts(prob, B, seed=7), c.forced, max_iter)
        assert (res["info"] == 0).all() and (res["stats"][:, 2] != 4).all() and (res["stats"][:, 0] >= 1).all()
        for b in range(B):
            done += _hold_refit(be, f"refit {case_id(c)} start {b}", prob, res["z"][b], res["value"][b], path, key)
    else:
        probs = [make_problem(c.n - 3 * s, c.T, c.D, c.kind, seed=8 + s) for s in range(2)]
        z0 = np.stack([starts(p, B, seed=8) for p in probs])
        res = be.fit_batched(pack_batch(probs), z0, c.forced, max_iter)
        assert (res["info"] == 0).all() and (res["stats"][..., 2] != 4).all()
        for s, p in enumerate(probs):
            for b in range(B):
                done += _hold_refit(be, f"batched refit {case_id(c)} problem {s} start {b}", p, res["z"][s, b], res["value"][s, b], path, key)
    assert done, f"refit {case_id(c)}: no returned point kept the caps"
