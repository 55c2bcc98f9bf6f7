"""Long-double reference, a-priori error bound, input sets and shared assertions for the fit family (scaml_gp_fit_fused_f64 in its five
variants, scaml_gp_fit_blocked_f64 on both paths, scaml_potrf_batched_f64 at T > 1, scaml_kernel_matrix_f64) and for the MLL
gradient (scaml_mll_backward_f64: the single-launch kernel in every (size class, kind, staging) combination, its two-workgroup
split, and the two-launch path).

Same construction as tests/_posterior_bounds.py and tests/_target_bounds.py, whose helpers are used here: the reference is numpy
long double fed exactly the arrays the kernel is handed -- a downstream quantity the DEVICE's own upstream output (L for Linv_diag,
alpha, quad and logdet; L and alpha for the gradient) --, so the conditioning of K enters only through a solve's own bound.  With
u = 2^-53, g_k = k u / (1 - k u), a' = x / l, |.| the Euclidean norm of a scaled point:

  K        fused / blocked fit: squared distances on the matrix core in the expanded form,  E_d2 = (D + 8) u (|a'| + |b'|)^2,
           E_K = os (S E_d2 + 4 u |k|), S = 1/2 (RBF), 5/6 (Matern-5/2); the diagonal at d2 = 0 exactly (`row == col ? 0.0 : d2`):
           E_ii = os 4 u + u |K_ii| (the noise's addition).  The several-CU kernel (csrc/gp_fit_coop.hip) takes coordinate differences,
           whose g_{D+5} d2 the expanded form's bound dominates: one bound for the family.  scaml_kernel_matrix_f64 takes them divided by l
           (csrc/gp_posterior.hip): E_d2 = g_{D+5} d2, the diagonal d2 = 0 exactly again
  factor   |L L^T - (K_ref + (noise + jitter) I)| <= g_{n+4} |L| |L^T| + E_K on the lower triangle, the product in long double from the
           device's L; POTRF: E_K = 0 and A is the input.  Exactly: the strict upper triangle inside n_t is zero with zero_upper and
           untouched without; rows and columns at or past n_t are never written (include/scaml_gp.h: "treated as an identity block and
           never written") -- the buffers are handed over full of a sentinel (the blocked fit: zeros, its later launches read them)
  W        block b of Linv_diag against the long-double inverse of the device's L_bb (identity-padded past n_t):
           |W_b - L_bb^-1| <= g_20 |L_bb^-1| |L_bb| |L_bb^-1|; a block wholly past n_t is the identity exactly
  alpha    solve_reference(L, y, n) of tests/_target_bounds.py, R = 1: the device's L alone; entries at or past n_t exactly zero
           (the buffer is handed over zeroed, as scamlgp_amd.ops does: they are never written)
  quad     every fit computes |L^-1 y|^2 (csrc/gp_fit_fused.hip: `q = fma(v, v, q)` over v = L^-1 y; the blocked fit adds the two
           blocks' sums, the several-CU kernel sums v_r^2 per thread):  v = L^-1 y, E_v = g_{N+4} |L^-1| |L| |v|,
           E = sum (2 |v| E_v + E_v^2) + g_{n+2} sum v^2
  logdet   2 sum log L_ii:  E = (g_{n+2} + 2 u) sum |2 log L_ii|   (one ulp = 2 u relative per logarithm)
  mll      `-0.5 * (q + ld + n * log2pi) / n`:  E = (E_q + E_ld + u |q + ld| + 2 u n log 2pi + u |q + ld + n log 2pi|) / (2 n) + u |mll|
           (the sum q + ld, the product n log2pi and its constant, the second sum, the division; -0.5 is exact); n_t = 0: 0.0 exactly
  info, jitter_used   0 and 0.0 exactly on these sets (the failure paths are tests/test_fit_failpath_gpu.py's)

  gradient g_p = (1 / 2n) sum_ij G_ij dK_ij / dtheta_p over ALL ordered pairs (the kernels visit the lower triangle of 16 x 16 tiles
           and weight an off-diagonal tile twice), G = alpha alpha^T - K^-1 from the device's L and alpha, theta = [l, os, noise]:
           dK/dos = k, dK/dnoise = I, dK/dl_d = -2 os dk delta'_d^2 / l_d  (dk = dk/dd2 < 0, delta' = a' - b')
           E_G    = E_Kinv + 3 u |alpha_i alpha_j|
           E_Kinv   single launch: the bound of solve_reference(L, I, n), forward and backward substitution by column strips
                    two launches:  E_Linv = g_{N+4} |L^-1| |L| |L^-1|,  E_Kinv = 2 |Linv|^T E_Linv + g_{n+4} |Linv|^T |Linv|
           E_d2     single launch: expanded form, (D + 8) u (|a'| + |b'|)^2; two launches: coordinate differences, g_{D+5} d2; the
                    diagonal d2 = 0 exactly in both
           E_k  = S E_d2 + 4 u |k|,  E_dk = S' E_d2 + 4 u |dk|,  S' = 1/4 (RBF), 25/12 (Matern-5/2)
           E_dK(l_d) = (2 os / l_d) (E_dk delta'^2 + |dk| E_delta2 + E_dk E_delta2) + 6 u |dK|
                    6 u: the constant os * hscale folded into the outputscale (its product and the constant 5/3), the two products
                    of `(G * hs) * h`, 1 / l_d and the final product with it
                    E_delta2, two launches: delta' = a'_d - b'_d of two coordinates that carry 2 u each,
                        E_delta = 2 u (|a'_d| + |b'_d|) + u |delta'|,  E_delta2 = 2 |delta'| E_delta + E_delta^2 + u delta'^2, 0 on the diagonal
                    E_delta2, single launch: 7 u (|a'_d| + |b'_d|)^2   (see "terms added")
           E_g  = (1 / 2n) (sum (|G| E_dK + E_G |dK| + E_G E_dK) + g_m sum |G| M) + 2 u |g|,  M = |dK| except as under "terms added"
           m, the longest chain of additions a term passes through, counted in the kernels:
             single launch  m = NP + 32, NP = 16 * (2, 4, 8, 16) the class's padded order: the matrix-core accumulation of Q / Q2 over the NP
                            rows of a strip (the os sum: 4 terms per block, at most NBT + 1 blocks per lane, is shorter), 3 to combine
                            Q2 - 2 x Q + x^2 CS, 2 strips per wave, 15 for the 16 columns of a lane group, 8 waves, 2 split halves in
                            the torch sum over the tile axis (every other slot is an exact zero), 2 to spare for the noise sum
             two launches   m = 16 + 63 + NT + 2: 16 elements of a super-tile per lane, the wave reduction, the torch sum over the NT =
                            nb (nb + 1) / 2 tile slots
           an empty task's gradient is exactly zero (every partial sum is a sum of masked zeros; the caller divides by max(2 n, 2))

Terms added to the issue's model, each read off the code and named:
  * fit, diagonal with jitter_in: `diag_add = noise + jitter + jit_in` is rounded before it is added: + u (noise + jitter_in) on K_ii.
  * gradient, single launch, lengthscales: the kernel never forms delta'^2 per element.  It accumulates Q = X_a^T GH, Q2 = (X_a^2)^T GH
    and the column sums CS on the matrix core and combines  sum_a GH_ac delta'^2 = Q2 - 2 x_c Q + x_c^2 CS  per column
    (csrc/gp_mll_grad_fused.hip, gf_epilogue): the three products carry the 2 u of each scaled coordinate twice, the square's and the
    factor 2 x_c's own rounding -- 7 u (|a'_d| + |b'_d|)^2 per element in place of the difference's E_delta2 --, and the additions
    cancel, so the g_m term carries M = (2 os / l_d) |dk| (|a'_d| + |b'_d|)^2 in place of |dK|.
  * gradient, E_dK: the cross term E_dk E_delta2 (second order).
No constant here is fitted to what a kernel returns.

Caps (conditions on the INPUTS, asserted with every comparison).  Fit: every bound at most CAP = 1e-8 of the quantity's largest
reference magnitude in the task; for the three scalar sums the scale is the sum of the magnitudes of its terms.  Gradient: each
bound at most CAP of S_p = (1 / 2n) sum |G| |dK / dtheta_p| AND at most 1e-6 of the task's largest |g_p|.

Input sets: the recipe of make_inputs (X uniform in the unit cube, l = c sqrt(D) (0.5 .. 1.5), os = 1.3, noise 1e-2 or 1e-3, a smooth
standardised y), ragged_counts(N) = N, N - 1, a multiple of 16, 1, 0 dealt to the tasks in turn (clamped at N for N < 16).  #CUs = 256.
Fit shapes, the smallest at which the kernels branch (fit_plan, fit_class_max_d, blocked_plan of csrc/gp_dispatch.h):
  N  1, 2, 15, 16, 17  one and two blocks in the nb = 2 variant;  32 | 33, 64 | 65, 128 | 129 the class edges (nb = 2 | 4 | 8 | 16);
     255, 256 close the fused classes;  272 the first blocked size;  320 | 336 either side of the 4 -> 2 waves-per-workgroup switch of
     the strip kernels that consume the factor (and of `parts == 2 && nbc <= 10` in the blocked dispatch);  512 the limit.  Every
     blocked size through both scaml_debug_blocked_fit_path values (1: the 2 x 2 sequence of launches, 2: several CUs per task)
  D  1, 8, 9 (the blocked solve switches kernels at D <= 8) and the largest each class admits: scaml_fit_max_d = 592, 296, 144, 44
     for N <= 32, 64, 128, 256, scaml_fit_blocked_max_d() = 17 (past the several-CU kernel's D <= 16: the launch sequence by shape)
  T  1;  9 (a second round over the 8 XCDs, every ragged count);  #CUs + 1 at N = 65 and 128: the narrow four-wave variant nb = 8, wu = 3
     that only a stack larger than the CU count selects (three tasks referenced: first, middle, last);  T <= #CUs: the wide nb = 8, wu = 7
  flags  store_L = False with alpha = NULL: the same quad / logdet / mll bit for bit;  zero_upper = False: a NaN-filled upper triangle
     stays NaN
  jitter_in  NULL, and 1e-4 on one blocked and one fused set (the `(noise + jitter) I` of the factor bound)
  neighbour rule  one full task with a NaN coordinate (its first point; N = 272: its last, in the second block) among finite ones: info > 0
     there, every other task within its bounds
Gradient shapes, every instance scaml_mll_backward_f64 can dispatch, in both families:
  single launch (forced)  class NBT = 2: N = 16 staged by LDS-DMA, N = 32 ragged without;  NBT = 4: N = 64 with, N = 33 without;  NBT = 8:
     N = 128 with, N = 65 ragged without;  NBT = 16: N = 256 with (T = #CUs / 2 + 1 = 129: one workgroup per task, mllgrad_fused[3][kind][1];
     T = 2: the two-workgroup split, mllgrad_split[1][kind][0]), N = 129 and N = 200 without;  D in {1, 8}.  The ragged single-launch
     sets leave out n_t = 1: a single point has S_p = 0 for the lengthscales while the expanded form's roundings are not zero
  two launches (forced)  D = 9: N = 129 ragged with every count (n_t = 1: the lengthscale entries are exactly zero, n_t = 0: all of
     them), 272, 512 (T = 1);  N = 48, D = 33: the staged points of four waves, 4 * 64 * 35 doubles = 70 KiB, pass the 64 KiB default
  by shape  N = 64 (single launch) and N = 128, T = 2 (a small stack: two launches): within the sum of the two forced paths' bounds of both
Unreachable (loaded, no dispatch selects them): mllgrad_split[0][kind][*] (the N <= 128 class split over 2 or 4 workgroups) and
mllgrad_split[1][kind][1] (four workgroups per task).

The drivers below (`check_*`) run a set through a BACKEND -- the C ABI on the device (tests/test_fit_bounds_gpu.py) or plain fp64
numpy stand-ins in the kernels' formulation (tests/test_fit_bounds.py) -- and hold every output to its bound.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import _dispatch as DP
from tests import _posterior_bounds as P
from tests import _target_bounds as TB
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, SENTINEL, U, Quantity, Ratios, _kernel, _S, gamma, inverse_lower, make_inputs, ragged_counts
from tests._target_bounds import FAMILY, _col, _up, potrf_reference, solve_reference, within

CUS = 256                                                   # compute units of the MI355X: the count the cases are chosen for
LOG_2PI = LD("1.8378770664093454835606594728112353")
GRAD_CAP_G = 1e-6                                           # second half of the gradient's cap: of the task's largest |g_p|
FIT_MAX_D = {32: 592, 64: 296, 128: 144, 256: 44}           # scaml_fit_max_d per class (the GPU file asserts them against the library)
BLOCKED_MAX_D = 17                                          # scaml_fit_blocked_max_d()
RATIOS = Ratios()      # (kernel instance, family, output) -> [largest error / bound, largest bound / scale]


def held(label, key, got, q: Quantity, nan_mask=None):
    """`within` of tests/_target_bounds.py, the ratios kept in this module's table."""
    within(label, key, got, q, nan_mask)
    RATIOS[key] = TB.RATIOS[key]


def report():
    """The ratio table so far, one line per (kernel instance, family, output)."""
    return [f"{k[0]} {k[1]} {k[2]}: largest error / bound {e:.3e}, largest bound / scale {c:.3e}" for k, (e, c) in sorted(RATIOS.items())]


def _sc(x):
    x = np.abs(np.asarray(x, dtype=LD))
    x = x[np.isfinite(x)]
    return float(x.max()) if x.size else 0.0


# ------------------------------------------------------------------------------------------------------------------
# fit family: input sets
FitCase = namedtuple("FitCase", "T N D kind ragged noise c jit path refs nan_task")


def _f(T, N, D, kind, ragged=None, noise=1e-2, c=0.5, jit=0.0, path=0, refs=None, nan_task=None):
    return FitCase(T, N, D, kind, ragged, noise, c, jit, path, refs, nan_task)


def fit_instance(c: FitCase) -> str:
    """The kernel instance fit_common / the blocked dispatch sends the case to: the launcher's own plan (tests/_dispatch.py) at CUS."""
    if c.N > 256:
        return "fit_blocked[launches]" if DP.blocked_plan(c.T, c.N, c.D, CUS, mode=c.path).path == 1 else "fit_blocked[coop]"
    p = DP.fit_plan(c.T, c.N, c.D, CUS)
    return f"fit_fused[nb{p.nb},wu{p.wu}]"


def _fit_shapes():
    s = [
        dict(T=1, N=1, D=1), dict(T=9, N=2, D=1, ragged=0), dict(T=9, N=15, D=8, ragged=1), dict(T=1, N=16, D=9, noise=1e-3),
        dict(T=9, N=17, D=1, ragged=0, c=0.3), dict(T=1, N=32, D=8), dict(T=1, N=32, D=FIT_MAX_D[32], noise=1e-3),
        dict(T=9, N=33, D=9, ragged=0), dict(T=1, N=64, D=1, c=0.3), dict(T=1, N=64, D=FIT_MAX_D[64]),
        dict(T=9, N=65, D=8, ragged=0, noise=1e-3), dict(T=CUS + 1, N=65, D=1, ragged=0, refs=(0, CUS // 2, CUS)),
        dict(T=1, N=128, D=9), dict(T=1, N=128, D=FIT_MAX_D[128], noise=1e-3), dict(T=CUS + 1, N=128, D=8, ragged=2, refs=(0, CUS // 2 + 1, CUS)),
        dict(T=9, N=129, D=1, ragged=0), dict(T=1, N=255, D=8, noise=1e-3), dict(T=9, N=256, D=9, ragged=0, jit=1e-4),
        dict(T=1, N=256, D=FIT_MAX_D[256]), dict(T=9, N=33, D=8, ragged=0, nan_task=5),
    ]
    for path in (1, 2):
        s += [dict(T=9, N=272, D=8, ragged=0, path=path, jit=1e-4), dict(T=1, N=320, D=1, path=path, noise=1e-3), dict(T=1, N=336, D=9, path=path),
              dict(T=2, N=512, D=8, ragged=1, path=path, noise=1e-3), dict(T=9, N=272, D=9, ragged=0, path=path, nan_task=5)]
    s.append(dict(T=1, N=512, D=BLOCKED_MAX_D, path=1))
    return s


FIT_CASES = [_f(kind=kind, **s) for s in _fit_shapes() for kind in (KIND_RBF, KIND_MATERN52)]
FLAG_CASES = [_f(T=9, N=N, D=D, kind=kind, ragged=0) for (N, D, kind) in ((17, 1, KIND_RBF), (64, 8, KIND_MATERN52), (128, 9, KIND_RBF), (129, 8, KIND_MATERN52))]


def fit_id(c: FitCase) -> str:
    s = f"{fit_instance(c)}-T{c.T}-N{c.N}-D{c.D}-{FAMILY[c.kind]}"
    s += "" if c.ragged is None else f"-ragged{c.ragged}"
    s += "-jit" if c.jit else ""
    return s + ("" if c.nan_task is None else "-nantask")


def fit_inputs(c: FitCase) -> dict:
    """X, y, theta, n_points (int32 or None), jitter_in (or None) of one case."""
    small = c.ragged is not None and c.N < 16      # (make_inputs deals a count of 16 whatever N is: below it the counts are clamped here)
    inp = make_inputs(P._c("linvmat", c.T, c.N, 0, c.D, c.kind, ragged=None if small else c.ragged, noise=c.noise, c=c.c))
    if small:
        inp["n_points"] = np.array([min(c.N, ragged_counts(c.N)[(t + c.ragged) % 5]) for t in range(c.T)], dtype=np.int32)
        for t, n in enumerate(inp["n_points"]):
            inp["y"][t, n:] = 0.0
    inp["jitter_in"] = np.full(c.T, c.jit) if c.jit else None
    if c.nan_task is not None:      # the first point; past 256 points the last one, which lies in the second block of the launch sequence
        inp["X"][c.nan_task, c.N - 1 if c.N > 256 else 0, c.D - 1] = np.nan
    return inp


def counts(c, inp):
    return [c.N] * c.T if inp["n_points"] is None else [int(v) for v in inp["n_points"]]


def referenced(c, inp):
    """The tasks held to the long-double reference: all of them, or the case's three."""
    return [t for t in (range(c.T) if c.refs is None else c.refs) if t != getattr(c, "nan_task", None)]


# ------------------------------------------------------------------------------------------------------------------
# fit family: references and bounds
def kmat_reference(X, th, kind, expanded, noise_add=0.0, jit=0.0, X2=None):
    """os k(X / l, X2 / l) (+ (noise + jit) I) and its bound, long double.  expanded: the fit's distance form; else coordinate
    differences (scaml_kernel_matrix_f64).  X2 None: the square matrix with d2 = 0 exactly on the diagonal."""
    D = X.shape[1]
    l, os_ = LD(th[:D]), LD(th[D])
    a = LD(X) / l
    b = a if X2 is None else LD(X2) / l
    diff = a[:, None, :] - b[None, :, :]
    d2 = (diff * diff).sum(-1)
    k = _kernel(d2, kind)[0]
    if expanded:
        na, nb = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1))
        E_d2 = (D + 8) * U * (na[:, None] + nb[None, :]) ** 2
    else:
        E_d2 = gamma(D + 5) * d2
    K = os_ * k
    if X2 is None:
        i = np.arange(X.shape[0])
        E_d2[i, i] = 0
        K[i, i] = os_
    E = os_ * (_S[kind][0] * E_d2 + 4 * U * np.abs(k))
    if X2 is None and (noise_add or jit):
        add = LD(noise_add) + LD(jit)
        K[i, i] += add
        E[i, i] += U * np.abs(K[i, i]) + (U * add if jit else 0)
    return Quantity(K, E, _sc(K))


def wblock_reference(L, n, NB):
    """Linv_diag (NB, 16, 16): the long-double inverses of the identity-padded diagonal blocks of the device's L."""
    Lp = np.eye(NB * 16)
    Lp[:n, :n] = np.tril(L[:n, :n])
    ref, bound = np.zeros((NB, 16, 16), dtype=LD), np.zeros((NB, 16, 16), dtype=LD)
    for b in range(NB):
        blk = Lp[16 * b:16 * b + 16, 16 * b:16 * b + 16]
        ref[b] = inverse_lower(blk)
        if 16 * b < n:
            A = np.abs(ref[b].astype(np.float64))
            bound[b] = _up(gamma(20) * (A @ np.abs(blk) @ A))
    return Quantity(ref, bound, _sc(ref))


def scalars_reference(L, y, n, N, Li):
    """quad, logdet, mll (name -> Quantity of shape ()) from the device's L (Li: its long-double inverse)."""
    if n == 0:
        z = Quantity(np.zeros((), dtype=LD), np.zeros((), dtype=LD), 0.0)
        return dict(quad=z, logdet=z, mll=z)
    Ln = np.tril(L[:n, :n])
    v = Li @ LD(y[:n])
    av = np.abs(v.astype(np.float64))
    E_v = _up(gamma(N + 4) * (np.abs(Li.astype(np.float64)) @ (np.abs(Ln) @ av)))
    q = (v * v).sum()
    E_q = LD((2 * av * E_v + E_v * E_v).sum()) + gamma(n + 2) * q
    logs = 2 * np.log(LD(np.diagonal(Ln)))
    ld, ld_mag = logs.sum(), np.abs(logs).sum()
    E_ld = (gamma(n + 2) + 2 * U) * ld_mag
    c = n * LOG_2PI
    mll = -(q + ld + c) / (2 * n)
    E_mll = (E_q + E_ld + U * np.abs(q + ld) + 2 * U * c + U * np.abs(q + ld + c)) / (2 * n) + U * np.abs(mll)
    return dict(quad=Quantity(q, E_q, float(q)), logdet=Quantity(ld, E_ld, float(ld_mag)),
                mll=Quantity(mll, E_mll, float((q + ld_mag + c) / (2 * n))))


def _same(x, fill):
    return np.isnan(x) if np.isnan(fill) else x == fill


def check_padding(label, Lt, n, fill, zero_upper):
    """Exact: rows / columns at or past n_t untouched, the strict upper triangle inside n_t zero (zero_upper) or untouched."""
    assert _same(Lt[n:, :], fill).all() and _same(Lt[:, n:], fill).all(), f"{label}: L was written at or past n_t = {n}"
    up = Lt[:n, :n][np.triu_indices(n, 1)]
    if zero_upper:
        assert (up == 0).all(), f"{label}: L is not zero above the diagonal"
    else:
        assert _same(up, fill).all(), f"{label}: zero_upper = False wrote above the diagonal"


def check_factor_task(label, key, out, t, n, N, y, A_ref: Quantity, zero_upper=True, cache_key=None):
    """Everything one task's factorisation returns: L L^T, the padding, Linv_diag, alpha, quad, logdet, mll (where given).
    A_ref: the matrix that was factored (with the diagonal additions) and ITS error bound (0 for the POTRF)."""
    inst, fam = key
    Lt = out["L"][t]
    check_padding(label, Lt, n, out["fill"], zero_upper)
    NB = (N + 15) // 16
    Ln = np.zeros((N, N))
    Ln[:n, :n] = np.tril(np.nan_to_num(Lt[:n, :n]))
    if n:
        LLt, q = potrf_reference(Ln[:n, :n], A_ref.ref, 0.0)
        low = np.tril_indices(n)
        held(label, (inst, fam, "L L^T"), LLt[low], Quantity(q.ref[low], (q.bound + A_ref.bound)[low], q.scale))
    if out.get("Linv_diag") is not None:
        held(label, (inst, fam, "Linv_diag"), out["Linv_diag"][t], wblock_reference(Ln, n, NB))
    Li = None
    if out.get("alpha") is not None:
        assert (out["alpha"][t, n:] == 0).all(), f"{label}: alpha is not exactly zero at or past n_t = {n}"
        held(label, (inst, fam, "alpha"), out["alpha"][t], _col(solve_reference(Ln, np.nan_to_num(y)[:, None], n, cache_key=cache_key)))
        Li = TB._LINV.pop(cache_key, None)      # (the task's long-double inverse: shared with the scalars below, then dropped)
    if out.get("quad") is not None:
        if Li is None and n:
            Li = inverse_lower(Ln[:n, :n])
        for name, q in scalars_reference(Ln, y, n, N, Li).items():
            if out.get(name) is None:
                continue
            if n == 0:
                assert out[name][t] == 0.0, f"{label}: an empty task must give {name} = 0.0 exactly, got {out[name][t]!r}"
            held(label, (inst, fam, name), np.asarray(out[name][t]), q)


def check_fit(be, c: FitCase):
    """One fit case through the backend: info / jitter exact, every referenced task's outputs within their bounds, the neighbour rule."""
    inp = fit_inputs(c)
    out = be.fit(c, inp)
    ns = counts(c, inp)
    key = (fit_instance(c), FAMILY[c.kind])
    for t in range(c.T):
        if t == c.nan_task:
            assert out["info"][t] > 0, f"{fit_id(c)} task {t}: a NaN coordinate must give info > 0, got {out['info'][t]}"
            continue
        assert out["info"][t] == 0 and out["jitter"][t] == 0.0, f"{fit_id(c)} task {t}: info {out['info'][t]}, jitter {out['jitter'][t]} on a well-conditioned set"
    D = c.D
    for t in referenced(c, inp):
        n = ns[t]
        label = f"{fit_id(c)} task {t}"
        th = inp["theta"][t]
        A = kmat_reference(inp["X"][t, :n], th, c.kind, True, noise_add=th[D + 1], jit=c.jit) if n else None
        check_factor_task(label, key, out, t, n, c.N, inp["y"][t], A, cache_key=(be.name, c, t))
    return out


def check_flags(be, c: FitCase):
    """store_L = False with alpha = NULL: the same scalars bit for bit; zero_upper = False: a NaN-filled upper triangle stays NaN, and
    the lower triangle and the scalars are those of the plain call bit for bit (alpha is not compared bit for bit: its
    back-substitution meets in LDS floating-point atomics, whose order is not fixed; it is held to its bound instead)."""
    inp = fit_inputs(c)
    full = be.fit(c, inp)
    lite = be.fit(c, inp, store_L=False, want_alpha=False)
    assert lite["L"] is None and lite["alpha"] is None
    for name in ("quad", "logdet", "mll"):
        assert np.array_equal(full[name], lite[name]), f"{fit_id(c)}: {name} differs without L and alpha: {full[name]} against {lite[name]}"
    assert np.array_equal(full["info"], lite["info"])
    raw = be.fit(c, inp, zero_upper=False)
    for t, n in enumerate(counts(c, inp)):
        check_padding(f"{fit_id(c)} task {t} zero_upper=False", raw["L"][t], n, raw["fill"], False)
        low = np.tril_indices(n)
        assert np.array_equal(raw["L"][t][low], full["L"][t][low]), f"{fit_id(c)} task {t}: zero_upper changes the factor"
        held(f"{fit_id(c)} task {t} zero_upper=False", (fit_instance(c), FAMILY[c.kind], "alpha"), raw["alpha"][t],
             _col(solve_reference(np.tril(np.nan_to_num(raw["L"][t])), inp["y"][t][:, None], n)))
    for name in ("quad", "logdet", "mll"):
        assert np.array_equal(raw[name], full[name]), f"{fit_id(c)}: zero_upper changes {name}"


# scaml_potrf_batched_f64 at T > 1: A = the fp64 kernel matrix of a fit case plus its noise, given
POTRF_CASES = [_f(T=9, N=N, D=4, kind=kind, ragged=r) for (N, kind, r) in ((2, KIND_RBF, 0), (17, KIND_MATERN52, 0), (64, KIND_RBF, 1), (100, KIND_MATERN52, 0),
                                                                          (200, KIND_RBF, 2))] + [_f(T=CUS + 1, N=100, D=4, kind=KIND_RBF, ragged=0, refs=(0, 77, CUS))]


def potrf_instance(c):
    return fit_instance(c).replace("fit_fused", "potrf")


def potrf_id(c):
    return fit_id(c).replace("fit_fused", "potrf")


def potrf_inputs(c: FitCase):
    inp = fit_inputs(c)
    A = np.zeros((c.T, c.N, c.N))
    for t in range(c.T):
        a = inp["X"][t] / inp["theta"][t, :c.D]
        d2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)
        A[t] = inp["theta"][t, c.D] * _kernel(d2, c.kind)[0] + inp["theta"][t, c.D + 1] * np.eye(c.N)
    inp["A"] = A
    return inp


def check_potrf(be, c: FitCase, inp=None):
    inp = potrf_inputs(c) if inp is None else inp
    out = be.potrf(c, inp)
    ns = counts(c, inp)
    assert (out["info"] == 0).all() and (out["jitter"] == 0.0).all(), f"{potrf_id(c)}: info {out['info']}, jitter {out['jitter']}"
    for t in referenced(c, inp):
        n = ns[t]
        A = LD(inp["A"][t, :n, :n])
        check_factor_task(f"{potrf_id(c)} task {t}", (potrf_instance(c), "-"), out, t, n, c.N, inp["y"][t], Quantity(A, np.zeros((n, n), dtype=LD), _sc(A)),
                          cache_key=(be.name, "potrf", c, t))
    return out


KMAT_CASES = [(T, N1, N2, D, kind, mode) for (T, N1, N2, D, mode) in ((2, 17, 17, 1, "noise"), (2, 33, 33, 9, "plain"), (3, 5, 129, 8, "shared"), (2, 16, 130, 3, "per_task"))
              for kind in (KIND_RBF, KIND_MATERN52)]


def kmat_id(c):
    return f"T{c[0]}-N{c[1]}x{c[2]}-D{c[3]}-{FAMILY[c[4]]}-{c[5]}"


def check_kmat(be, c):
    T, N1, N2, D, kind, mode = c
    inp = make_inputs(P._c("linvmat", T, N1, 0, D, kind))
    rng = np.random.default_rng([7, T, N1, N2, D])
    X2 = None if mode in ("noise", "plain") else rng.uniform(size=(N2, D) if mode == "shared" else (T, N2, D))
    if X2 is not None:
        (X2 if mode == "shared" else X2[0])[1] = inp["X"][0, 2]      # a query ON a training point of task 0
    got = be.kmat(inp["X"], X2, inp["theta"], kind, mode == "noise")
    for t in range(T):
        x2 = None if X2 is None else (X2 if mode == "shared" else X2[t])
        q = kmat_reference(inp["X"][t], inp["theta"][t], kind, False, noise_add=inp["theta"][t, D + 1] if mode == "noise" else 0.0, X2=x2)
        held(f"kmat-{kmat_id(c)} task {t}", ("kernel_matrix", FAMILY[kind], "K"), got[t], q)


# ------------------------------------------------------------------------------------------------------------------
# MLL gradient
GradCase = namedtuple("GradCase", "path T N D kind ragged noise refs")


def _g(path, T, N, D, kind, ragged=None, noise=1e-2, refs=None):
    return GradCase(path, T, N, D, kind, ragged, noise, refs)


GRAD_MODE = {"default": 0, "two": 1, "single": 2}      # a case's path as scaml_debug_force_two_launch_grad's mode


def grad_instance(c: GradCase, path=None) -> str:
    """The kernel instance scaml_mll_backward_f64 sends the case to: the launcher's own plan (grad_plan, csrc/gp_dispatch.h) at CUS."""
    path = path or c.path
    fam = FAMILY[c.kind]
    p = DP.grad_plan(c.T, c.N, c.D, CUS, mode=GRAD_MODE[path], ragged=c.ragged is not None)      # (the backends' buffers are 16-byte aligned)
    pre = "default->" if path == "default" else ""
    if not p.single:
        return f"{pre}mllgrad[{fam}]"
    if p.split > 1:
        return f"{pre}mllgrad_split[{p.sc - 2}][{fam}][{0 if p.split == 2 else 1}]"
    return f"{pre}mllgrad_fused[{p.sc}][{fam}][{p.dma}]"


# single-launch ragged sets: T = 4, ragged = 4 -> counts 0, N, N - 1, a multiple of 16 (no single point, see the header)
_GRAD_SHAPES = [
    dict(path="single", T=3, N=16, D=1), dict(path="single", T=4, N=32, D=8, ragged=4),
    dict(path="single", T=2, N=33, D=8, noise=1e-3), dict(path="single", T=2, N=64, D=1),
    dict(path="single", T=4, N=65, D=1, ragged=4), dict(path="single", T=2, N=128, D=8),
    dict(path="single", T=2, N=129, D=8), dict(path="single", T=2, N=200, D=1, noise=1e-3),
    dict(path="single", T=CUS // 2 + 1, N=256, D=8, refs=(0, CUS // 4, CUS // 2)), dict(path="single", T=2, N=256, D=8),
    dict(path="two", T=9, N=129, D=9, ragged=0), dict(path="two", T=2, N=272, D=9), dict(path="two", T=1, N=512, D=9),
    dict(path="two", T=2, N=48, D=33, noise=1e-3),
    dict(path="default", T=2, N=64, D=8), dict(path="default", T=2, N=128, D=8),
]
GRAD_CASES = [_g(kind=kind, **s) for s in _GRAD_SHAPES for kind in (KIND_RBF, KIND_MATERN52)]


def grad_id(c: GradCase) -> str:
    return f"{grad_instance(c)}-T{c.T}-N{c.N}-D{c.D}" + ("" if c.ragged is None else f"-ragged{c.ragged}")


def grad_fit_case(c: GradCase) -> FitCase:
    return _f(c.T, c.N, c.D, c.kind, ragged=c.ragged, noise=c.noise)


def grad_reference(c: GradCase, inp, fit, t, form):
    """(g, E_g, S) of task t, each (D + 2) long double, from the fit's L and alpha.  form: "single" / "two" (the header)."""
    N, D, kind = c.N, c.D, c.kind
    n = counts(c, inp)[t]
    g, E, S = (np.zeros(D + 2, dtype=LD) for _ in range(3))
    if n == 0:
        return g, E, S
    th = inp["theta"][t]
    l, os_ = LD(th[:D]), LD(th[D])
    Ln = np.tril(fit["L"][t, :n, :n])
    al = LD(fit["alpha"][t, :n])
    if form == "single":
        Lfull = np.zeros((N, N))
        Lfull[:n, :n] = Ln
        q = solve_reference(Lfull, np.eye(N), n)
        Kinv, E_Kinv = q.ref[:n, :n], q.bound[:n, :n]
        NP = 16 * (2 << DP.fit_class(N))
        m = NP + 32
    else:
        Li = inverse_lower(Ln)
        Kinv = Li.T @ Li
        aLi = np.abs(Li.astype(np.float64))
        E_Linv = _up(gamma(N + 4) * (aLi @ np.abs(Ln) @ aLi))
        E_Kinv = _up(2 * (aLi.T @ E_Linv) + gamma(n + 4) * (aLi.T @ aLi))
        nb = (N + 15) // 16
        m = 16 + 63 + nb * (nb + 1) // 2 + 2
    gm = gamma(m)
    aa = np.outer(al, al)
    G = aa - Kinv
    E_G = E_Kinv + 3 * U * np.abs(aa)
    aG = np.abs(G)
    a = LD(inp["X"][t, :n]) / l
    diff = a[:, None, :] - a[None, :, :]
    d2 = (diff * diff).sum(-1)
    k, dk = _kernel(d2, kind)
    i = np.arange(n)
    k[i, i] = 1
    if form == "single":
        na = np.sqrt((a * a).sum(-1))
        E_d2 = (D + 8) * U * (na[:, None] + na[None, :]) ** 2
    else:
        E_d2 = gamma(D + 5) * d2
    E_d2[i, i] = 0
    S0, S1 = _S[kind]
    ak, adk = np.abs(k), np.abs(dk)
    E_k, E_dk = S0 * E_d2 + 4 * U * ak, S1 * E_d2 + 4 * U * adk
    g[D], S[D] = (G * k).sum(), (aG * ak).sum()
    E[D] = (aG * E_k + E_G * ak + E_G * E_k).sum() + gm * S[D]
    g[D + 1], S[D + 1] = G[i, i].sum(), aG[i, i].sum()
    E[D + 1] = E_G[i, i].sum() + gm * S[D + 1]
    absa = np.abs(a)
    for d in range(D):
        df = diff[:, :, d]
        df2 = df * df
        cd = 2 * os_ / l[d]
        dKd = -cd * dk * df2
        both = absa[:, None, d] + absa[None, :, d]
        if form == "single":
            E_df2 = 7 * U * both ** 2
            M = cd * adk * both ** 2
        else:
            E_df = 2 * U * both + U * np.abs(df)
            E_df2 = 2 * np.abs(df) * E_df + E_df * E_df + U * df2
            E_df2[i, i] = 0
            M = np.abs(dKd)
        E_dK = cd * (E_dk * df2 + adk * E_df2 + E_dk * E_df2) + 6 * U * np.abs(dKd)
        g[d], S[d] = (G * dKd).sum(), (aG * np.abs(dKd)).sum()
        E[d] = (aG * E_dK + E_G * np.abs(dKd) + E_G * E_dK).sum() + gm * (aG * M).sum()
    g, S = g / (2 * n), S / (2 * n)
    E = E / (2 * n) + 2 * U * np.abs(g)
    return g, E, S


def grad_within(label, key, got, ref, bound, S):
    """|got - ref| <= bound per entry of theta; the bound at most CAP of S_p and at most GRAD_CAP_G of the task's largest |g_p|."""
    got = np.asarray(got)
    gmax = float(np.abs(ref).max())
    over = ~(bound <= CAP * S)
    assert not over.any(), (f"{label}: the bound {bound[over].astype(float)} exceeds {CAP} of S_p {S[over].astype(float)} at theta{list(np.flatnonzero(over))} -- the "
                            f"input set is ill-chosen")
    over = ~(bound <= GRAD_CAP_G * gmax)
    assert not over.any(), (f"{label}: the bound {bound[over].astype(float)} exceeds {GRAD_CAP_G} of the largest |g_p| {gmax:.3e} at theta{list(np.flatnonzero(over))} -- "
                            f"the input set is ill-chosen")
    err = np.abs(LD(got) - ref)
    bad = ~(err <= bound)
    if bad.any():
        p = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{label} g[{p}]: got {float(got[p])!r}, reference {float(ref[p])!r}, error {float(err[p]):.3e} > bound {float(bound[p]):.3e} "
                             f"({int(bad.sum())} of {bad.size} entries)")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
        cr = np.where(S > 0, bound / np.where(S > 0, S, 1), 0)
    RATIOS.note(key, float(r.max()), float(cr.max()))


def check_grad(be, c: GradCase, fit=None):
    """One gradient case: the backend's fit of the set (or the one given), then the gradient on ITS L / Linv_diag / alpha on the forced
    path(s), each referenced task within its bound; an empty task exactly zero; `default`: the by-shape call within the sum of the two
    forced paths' bounds of both."""
    fc = grad_fit_case(c)
    inp = fit_inputs(fc)
    fit = be.fit_for_grad(fc, inp) if fit is None else fit
    ns = counts(c, inp)
    fam = FAMILY[c.kind]
    forms = ("single", "two") if c.path == "default" else (c.path,)
    got = {f: be.grad(c, inp, fit, f) for f in forms}
    by_shape = be.grad(c, inp, fit, "default") if c.path == "default" else None
    for t in referenced(c, inp):
        n = ns[t]
        refs = {}
        for f in forms:
            label = f"{grad_id(c)} [{f}] task {t}"
            ref, E, S = grad_reference(c, inp, fit, t, f)
            refs[f] = (ref, E)
            if n == 0:
                assert (got[f][t] == 0).all(), f"{label}: an empty task's gradient must be exactly zero, got {got[f][t]}"
            if n == 1 and f == "two":
                assert (got[f][t, :c.D] == 0).all(), f"{label}: one point has no lengthscale gradient, got {got[f][t, :c.D]}"
            grad_within(label, (grad_instance(c, f), fam, "g"), got[f][t], ref, E, S)
        if by_shape is not None:
            tol = refs["single"][1] + refs["two"][1]
            for f in forms:
                err = np.abs(LD(by_shape[t]) - LD(got[f][t]))
                assert (err <= tol).all(), (f"{grad_id(c)} task {t}: the by-shape call is {err.astype(float)} from the forced {f} path, the sum of the bounds "
                                            f"is {tol.astype(float)}")
    return got
