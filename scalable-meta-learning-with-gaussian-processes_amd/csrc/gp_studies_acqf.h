// gp_studies_acqf.h -- the batched target acquisition of many BO studies (include/scaml_gp.h (7g)): argument block, LDS footprint and
// the arithmetic of one block of right-hand sides, sa_block<R>.  One source for both device kernels (csrc/gp_studies_acqf.hip: a
// workgroup per query point, R = 1; csrc/gp_studies_score.hip: a workgroup per strip of 16 candidates, R = 16, value only (7i)), the
// host launcher and the single-threaded host build the CPU tests check against torch (any compiler but hipcc: tests/host_emul).
//
// Per query point q of group g (a study: its weights, target kernel, training inputs, cached factor of Knn, alpha, standardiser):
//   S_mu[c]  = sum_t w_t   mu[t][q][c],   S_var[c] = sum_t w_t^2 var[t][q][c],   C[a][c] = sum_t w_t^2 cov[t][a][16 q + c]
//              over the active tasks, t = 0 .. T-1 in order, for the 16 columns c of the GRAD pass and the n_g training points a
//   Knq[a]   = C[a][0] / s^2 + os k_t(x_a, x_q),      dKnq[a][d] = C[a][1 + d] / s^2 + d/dx_d os k_t(x_a, x_q)
//   z        = Knn^-1 Knq from the cached factor (blocked substitution with the 16 x 16 inverses of L's diagonal blocks)
//   mu*      = m + s ((S_mu[0] - m) / s + Knq . alpha),   var* = s^2 (S_var[0] / s^2 + os - Knq . z)
//   dmu*[d]  = S_mu[1 + d] + s sum_a alpha_a dKnq[a][d],   dvar*[d] = S_var[1 + d] - 2 s^2 sum_a z_a dKnq[a][d]
//   UCB / EI and their chain rule with the clamps of scamlgp_amd/utils.py (sa_acquisition, which csrc/gp_fantasy.hip calls for F fantasies).
// Every sum runs in a fixed order (tasks ascending, training points ascending) by ONE thread per output: no atomics, no wave
// reductions, so the result is a pure function of the inputs and the host build computes what the device computes.
#pragma once
#include "gp_studies_formulas.h"   // SA_DEV / SA_SYNC, sa_kernel_and_slope, sa_acquisition

namespace scaml {

constexpr int STUDIES_ACQF_MAX_N = 96;   // training points per study (the GRAD pass's covariance block)
constexpr int STUDIES_ACQF_MAX_D = 15;   // (its 16 columns per query point)
constexpr int STUDIES_ACQF_THREADS = 256;

struct StudiesAcqfParams {
  const double* mu;           // (T, Mq, 16)          GRAD-pass outputs of the source stack, all tasks
  const double* var;          // (T, Mq, 16)
  const double* cov;          // (T, n_max, Mq * 16)  rows a < n_g of query q's strip are read
  const int32_t* group;       // (Mq) study of a query point; negative: padding (zeros come out)
  const double* Xq;           // (Mq, D)
  const double* w;            // (G, T) weights, zero where pruned
  const uint8_t* active;      // (G, T) a masked task is skipped, not multiplied by zero
  const double* Xt;           // (G, n_max, D) training inputs
  const double* theta;        // (G, D + 2) target kernel: lengthscales, outputscale, noise
  const double* L;            // (G, n_max, n_max) factor of Knn, row stride n_max, the leading n_g x n_g block
  const double* Linv_diag;    // (G, ceil(n_max / 16), 16, 16) inverses of its diagonal blocks
  const double* alpha;        // (G, n_max) Knn^-1 resid
  const int32_t* n_points;    // (G) 1 <= n_g <= n_max
  const double* m_all;        // (G)
  const double* s_all;        // (G) > 0
  const int32_t* info;        // (G) != 0: the study's factorisation failed, its outputs are NaN
  const double* acqf_param;   // (G) UCB: beta; EI: best_f
  double* value;              // (Mq)
  double* grad;               // (Mq, D) or NULL
  double* mu_out;             // (Mq) or NULL: the target posterior mean (original units)
  double* var_out;            // (Mq) or NULL: its variance
  int Mq, G, n_max, T, D, kind, acqf, pad_;
};

// LDS of one block of R right-hand sides, in doubles:
//   C [n_max][16] | S_mu, S_var [32] | u, v [2][np * R] | alpha [np] | W [nb][256] | L [n_max][n_max | 1] | red [R == 1 ? 48 : 32]
template <int R>
constexpr size_t sa_lds_doubles(int n_max) {
  const size_t nb = (size_t)(n_max + 15) / 16, np = nb * 16;
  return (size_t)n_max * 16 + 32 + 2 * np * R + np + nb * 256 + (size_t)n_max * (size_t)(n_max | 1) + (R == 1 ? 48 : 32);
}
constexpr size_t studies_acqf_lds_doubles(int n_max) { return sa_lds_doubles<1>(n_max); }

// One block `blk` of R right-hand sides of one study by `nthr` cooperating threads (thread `tid`; SA_SYNC between the phases).
// `lds`: sa_lds_doubles<R>(n_max).  The two instantiations are the two layouts of the grouped source pass:
//   R = 1   a query point in the 16-column GRAD layout: mu, var (T, Mq, 16), cov (T, n_max, Mq * 16), group (Mq) per query.  Column 0
//           is the right-hand side, columns 1 .. 15 of C are the gradient columns that ride along; `grad` is written where given.
//   R = 16  a strip of 16 candidates in the value layout: mu, var (T, Mq), cov (T, n_max, Mq), group (Mq / 16) per strip, Mq a
//           multiple of 16.  The 16 columns of C are 16 right-hand sides against ONE copy of the factor; `grad` is not used.
// Either way a block owns 16 consecutive columns of a source row and C is [a][16]; element e of an [.][R] array is (e / R, e % R).
template <int R>
SA_DEV void sa_block(const StudiesAcqfParams& p, double* lds, int blk, int tid, int nthr) {
  static_assert(R == 1 || R == 16, "a query point with its gradient columns, or a strip of 16 candidates");
  const int D = p.D, T = p.T, n_max = p.n_max;
  const int g = p.group[blk];
  const size_t q0 = (size_t)blk * R;   // the block's first output
  const double nan = NAN;
  // (every branch up to the first barrier is uniform over the workgroup)
  if (g < 0 || g >= p.G) {   // padding
    for (int c = tid; c < R; c += nthr) {
      p.value[q0 + c] = 0.0;
      if (p.mu_out) p.mu_out[q0 + c] = 0.0;
      if (p.var_out) p.var_out[q0 + c] = 0.0;
    }
    if constexpr (R == 1)
      if (p.grad) for (int d = tid; d < D; d += nthr) p.grad[q0 * D + d] = 0.0;
    return;
  }
  const int n = p.n_points[g];
  if (p.info[g] != 0 || n < 1 || n > n_max) {
    for (int c = tid; c < R; c += nthr) {
      p.value[q0 + c] = nan;
      if (p.mu_out) p.mu_out[q0 + c] = nan;
      if (p.var_out) p.var_out[q0 + c] = nan;
    }
    if constexpr (R == 1)
      if (p.grad) for (int d = tid; d < D; d += nthr) p.grad[q0 * D + d] = nan;
    return;
  }
  const int nbm = (n_max + 15) / 16, np = nbm * 16, nb = (n + 15) / 16, ldl = n_max | 1;
  double* C = lds;                          // [a][16]: Knq in columns c < R, then (R = 1) dKnq in columns 1 + d
  double* Ssum = C + (size_t)n_max * 16;    // S_mu [16] | S_var [16]
  double* u = Ssum + 32;                    // [a][R]
  double* v = u + (size_t)np * R;
  double* al = v + (size_t)np * R;
  double* Wd = al + np;
  double* Ls = Wd + (size_t)nbm * 256;
  double* red = Ls + (size_t)n_max * ldl;   // Knq . alpha [R] | Knq . z [R]; R = 1: then sum_a alpha_a dKnq [2 + d], sum_a z_a dKnq [18 + d]

  const double s = p.s_all[g], m = p.m_all[g], s2 = s * s, inv_s2 = 1.0 / s2;
  const double* th = p.theta + (size_t)g * (D + 2);
  const double os = th[D];
  const double* wg = p.w + (size_t)g * T;
  const uint8_t* ag = p.active + (size_t)g * T;
  const size_t W = (size_t)p.Mq * (R == 1 ? 16 : 1), col0 = (size_t)blk * 16;   // a source row, the block's 16 columns in it

  // ---- phase 1: the weighted task sums (eight tasks' loads in flight; a row's 16 columns are 128 consecutive bytes), the factor,
  // its block inverses and alpha into LDS
  for (int e = tid; e < n * 16 + 32; e += nthr) {
    const bool is_cov = e < n * 16;
    const int a = e >> 4, c = e & 15;
    const int which = (e - n * 16) >> 4;   // 0: mu, 1: var
    const double* src = is_cov ? p.cov + (size_t)a * W + col0 + c : (which == 0 ? p.mu : p.var) + col0 + c;
    const size_t tstride = is_cov ? (size_t)n_max * W : W;
    const bool lin = !is_cov && which == 0;
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += 8) {
      double val[8], cf[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = t0 + k;
        const bool ok = t < T && ag[t];   // (a masked task is skipped, not multiplied by zero: its values may be NaN)
        val[k] = ok ? src[(size_t)t * tstride] : 0.0;
        const double wt = ok ? wg[t] : 0.0;
        cf[k] = lin ? wt : wt * wt;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(cf[k], val[k], acc);
    }
    if (is_cov) C[e] = acc * inv_s2;
    else Ssum[e - n * 16] = acc;
  }
  {
    const double* Lg = p.L + (size_t)g * n_max * n_max;
    for (int e = tid; e < n * n; e += nthr) {
      const int i = e / n, j = e - i * n;
      if (j <= i) Ls[(size_t)i * ldl + j] = Lg[(size_t)i * n_max + j];
    }
    const double* Wg = p.Linv_diag + (size_t)g * nbm * 256;
    for (int e = tid; e < nb * 256; e += nthr) Wd[e] = Wg[e];
    for (int a = tid; a < n; a += nthr) al[a] = p.alpha[(size_t)g * n_max + a];
  }
  SA_SYNC();
  // ---- phase 1b: the target kernel's part of Knq and (R = 1) of its input gradient, one slope evaluation per (training point, rhs)
  for (int e = tid; e < n * R; e += nthr) {
    const int a = e / R, c = e % R;
    const double* xa = p.Xt + ((size_t)g * n_max + a) * D;
    const double* xq = p.Xq + (q0 + c) * D;
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (xq[d] - xa[d]) / th[d];
      d2 = fma(df, df, d2);
    }
    double k0, dk;
    sa_kernel_and_slope(p.kind, d2, os, k0, dk);
    double* Ca = C + (size_t)a * 16;
    Ca[c] += k0;
    if constexpr (R == 1)
      for (int d = 0; d < D; ++d) Ca[1 + d] += 2.0 * dk * ((xq[d] - xa[d]) / (th[d] * th[d]));
    u[e] = Ca[c];
  }
  SA_SYNC();
  // ---- phase 2: z = Knn^-1 Knq, R right-hand sides.  Forward L y = Knq by block rows: y_kb = W_kb u_kb, then
  // u_i -= L[i, kb] y_kb below the block
  for (int kb = 0; kb < nb; ++kb) {
    const int r0 = 16 * kb, cnt = n - r0 < 16 ? n - r0 : 16;
    for (int e = tid; e < cnt * R; e += nthr) {
      const int r = e / R, c = e % R;
      double acc = 0.0;
      for (int k = 0; k <= r; ++k) acc = fma(Wd[kb * 256 + r * 16 + k], u[(r0 + k) * R + c], acc);
      v[(r0 + r) * R + c] = acc;
    }
    SA_SYNC();
    for (int e = (r0 + 16) * R + tid; e < n * R; e += nthr) {
      const int i = e / R, c = e % R;
      double acc = u[e];
      for (int k = 0; k < 16; ++k) acc = fma(-Ls[(size_t)i * ldl + r0 + k], v[(r0 + k) * R + c], acc);
      u[e] = acc;
    }
    SA_SYNC();
  }
  // backward L^T z = y (y in v, z into u): z_kb = W_kb^T v_kb, then v_i -= L[kb, i]^T z_kb above the block
  for (int kb = nb - 1; kb >= 0; --kb) {
    const int r0 = 16 * kb, cnt = n - r0 < 16 ? n - r0 : 16;
    for (int e = tid; e < cnt * R; e += nthr) {
      const int r = e / R, c = e % R;
      double acc = 0.0;
      for (int k = r; k < cnt; ++k) acc = fma(Wd[kb * 256 + k * 16 + r], v[(r0 + k) * R + c], acc);
      u[(r0 + r) * R + c] = acc;
    }
    SA_SYNC();
    for (int e = tid; e < r0 * R; e += nthr) {
      const int i = e / R, c = e % R;
      double acc = v[e];
      for (int k = 0; k < cnt; ++k) acc = fma(-Ls[(size_t)(r0 + k) * ldl + i], u[(r0 + k) * R + c], acc);
      v[e] = acc;
    }
    SA_SYNC();
  }
  // ---- phase 3: the contractions over the training points, one thread per output, a = 0 .. n-1 in order
  //   red[c] = Knq . alpha, red[R + c] = Knq . z; R = 1: red[2 + d] = sum_a alpha_a dKnq[a][d], red[18 + d] = sum_a z_a dKnq[a][d]
  for (int o = tid; o < 2 * R + (R == 1 ? 2 * D : 0); o += nthr) {
    const bool grad_col = R == 1 && o >= 2;
    const int og = o - 2;
    const bool with_alpha = grad_col ? og < D : o < R;
    const int c = grad_col ? 0 : o % R, col = grad_col ? 1 + (og < D ? og : og - D) : c;
    double acc = 0.0;
    for (int a = 0; a < n; ++a) acc = fma(with_alpha ? al[a] : u[a * R + c], C[(size_t)a * 16 + col], acc);
    red[grad_col ? (og < D ? 2 + og : 18 + (og - D)) : o] = acc;
  }
  SA_SYNC();
  // ---- phase 4: the posterior, the acquisition value and (R = 1) its chain rule: one thread per right-hand side, or per input
  // dimension of the one (every writing thread restates the scalars)
  for (int e = tid; e < (R == 1 ? (D > 1 ? D : 1) : R); e += nthr) {
    const int c = R == 1 ? 0 : e, o = R == 1 ? e : 0;
    const double mean_q = (Ssum[c] - m) / s, var_q = Ssum[16 + c] * inv_s2 + os;
    const double mu = fma(s, mean_q + red[c], m);
    const double vr = s2 * (var_q - red[R + c]);
    const double par = p.acqf_param[g];
    double A, Amu, Av;
    sa_acquisition(p.acqf, par, mu, vr, A, Amu, Av);
    // a query point with a NaN / inf coordinate: fmax in the Matern branch drops a NaN operand, so only that coordinate's slope
    // would carry it (and nothing at all with source sums that happen to be finite).  sum_d (x_d - x_d) is 0, or NaN for such a
    // point: every output of THAT point is NaN, as (5d)'s target gradient has it (a select: finite inputs are untouched)
    double bad = 0.0;
    for (int d = 0; d < D; ++d) {
      const double x = p.Xq[(q0 + c) * D + d];
      bad += x - x;
    }
    if (o == 0) {
      p.value[q0 + c] = bad == 0.0 ? A : bad;
      if (p.mu_out) p.mu_out[q0 + c] = bad == 0.0 ? mu : bad;
      if (p.var_out) p.var_out[q0 + c] = bad == 0.0 ? vr : bad;
    }
    if constexpr (R == 1)
      if (p.grad && o < D) {
        const double dmu = fma(s, red[2 + o], Ssum[1 + o]);
        const double dvar = fma(-2.0 * s2, red[18 + o], Ssum[17 + o]);
        p.grad[q0 * D + o] = bad == 0.0 ? fma(Av, dvar, Amu * dmu) : bad;
      }
  }
}

// One query point (7g): the R = 1 instantiation.
SA_DEV void sa_query(const StudiesAcqfParams& p, double* lds, int q, int tid, int nthr) { sa_block<1>(p, lds, q, tid, nthr); }

}  // namespace scaml
