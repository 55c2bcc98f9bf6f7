// gp_studies_score.h -- scoring a TABLE of candidates for many BO studies (include/scaml_gp.h (7i)): stage 1 of the studies'
// acquisition optimiser, 1,024 raw candidates per study, value only.  One source for the device kernel (csrc/gp_studies_score.hip: a
// workgroup per strip of 16 candidates of one study), the host launcher and the single-threaded host build the CPU tests run
// (tests/host_emul/studies_score_emul.cpp).
//
// Inputs are the VALUE layout of the grouped source pass (5f): mu, var (T, Mq), cov (T, n_max, Mq), 16 different candidates per strip,
// all of one study, group[strip] names it.  What csrc/gp_studies_acqf.h (7g) does for one query point with its 16 gradient columns
// -- a workgroup that stages the study's factor in LDS for a single right-hand side -- is done here for 16 candidates against ONE
// copy of the factor: thread <-> (row, candidate), the 16 columns are the parallelism.
//
// Arithmetic contract: per candidate exactly sa_query's operations in sa_query's order on column 0 of its layout -- the task sums
// ascending in chunks of eight, the target-kernel term, the blocked forward and backward substitution with the 16 x 16 block inverses,
// Knq . alpha and Knq . z ascending over the training points, UCB / EI with the clamps, the non-finite-coordinate rule.  Every output
// comes from one thread, no atomics: value, mu_out and var_out are a pure function of the inputs and equal (7g)'s bit for bit.
#pragma once
#include "gp_studies_acqf.h"   // StudiesAcqfParams, the limits, and through it csrc/gp_studies_formulas.h

namespace scaml {

constexpr int STUDIES_SCORE_THREADS = 256;   // 16 rows x 16 candidates

// The argument block is (7g)'s, read in the value layout: mu, var (T, Mq), cov (T, n_max, Mq), group (Mq / 16) per STRIP, Xq (Mq, D),
// value / mu_out / var_out (Mq); Mq is a multiple of 16 and `grad` is not used.
using StudiesScoreParams = StudiesAcqfParams;

// LDS of one strip, in doubles: Knq [n_max][16] | S_mu, S_var [2][16] | u, v [2][np][16] | alpha [np] | W [nb][256] |
// L [n_max][n_max | 1] | red [2][16]
constexpr size_t studies_score_lds_doubles(int n_max) {
  const size_t nb = (size_t)(n_max + 15) / 16, np = nb * 16;
  return (size_t)n_max * 16 + 32 + 2 * np * 16 + np + nb * 256 + (size_t)n_max * (size_t)(n_max | 1) + 32;
}

// One strip of 16 candidates by `nthr` cooperating threads (thread `tid`; SA_SYNC between the phases).
// `lds`: studies_score_lds_doubles(n_max).
SA_DEV void sa_score_strip(const StudiesScoreParams& p, double* lds, int strip, int tid, int nthr) {
  const int D = p.D, T = p.T, n_max = p.n_max;
  const int g = p.group[strip];
  const size_t q0 = (size_t)strip * 16;
  const double nan = NAN;
  // (every branch up to the first barrier is uniform over the workgroup)
  if (g < 0 || g >= p.G) {   // a padding strip
    for (int c = tid; c < 16; c += nthr) {
      p.value[q0 + c] = 0.0;
      if (p.mu_out) p.mu_out[q0 + c] = 0.0;
      if (p.var_out) p.var_out[q0 + c] = 0.0;
    }
    return;
  }
  const int n = p.n_points[g];
  if (p.info[g] != 0 || n < 1 || n > n_max) {
    for (int c = tid; c < 16; c += nthr) {
      p.value[q0 + c] = nan;
      if (p.mu_out) p.mu_out[q0 + c] = nan;
      if (p.var_out) p.var_out[q0 + c] = nan;
    }
    return;
  }
  const int nbm = (n_max + 15) / 16, np = nbm * 16, nb = (n + 15) / 16, ldl = n_max | 1;
  double* K = lds;                          // Knq [a][c]
  double* Ssum = K + (size_t)n_max * 16;    // S_mu [16] | S_var [16]
  double* u = Ssum + 32;                    // [a][c]
  double* v = u + (size_t)np * 16;
  double* al = v + (size_t)np * 16;
  double* Wd = al + np;
  double* Ls = Wd + (size_t)nbm * 256;
  double* red = Ls + (size_t)n_max * ldl;   // Knq . alpha [16] | Knq . z [16]

  const double s = p.s_all[g], m = p.m_all[g], s2 = s * s, inv_s2 = 1.0 / s2;
  const double* th = p.theta + (size_t)g * (D + 2);
  const double os = th[D];
  const double* wg = p.w + (size_t)g * T;
  const uint8_t* ag = p.active + (size_t)g * T;
  const size_t W = (size_t)p.Mq;

  // ---- phase 1: the weighted task sums (eight tasks' loads in flight; a row's 16 candidates are 128 consecutive bytes), the factor,
  // its block inverses and alpha into LDS
  for (int e = tid; e < n * 16 + 32; e += nthr) {
    const bool is_cov = e < n * 16;
    const int a = e >> 4, c = e & 15;
    const int which = (e - n * 16) >> 4;   // 0: mu, 1: var
    const double* src = is_cov ? p.cov + (size_t)a * W + q0 + c : (which == 0 ? p.mu : p.var) + q0 + c;
    const size_t tstride = is_cov ? (size_t)n_max * W : W;
    const bool lin = !is_cov && which == 0;
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += 8) {
      double val[8], cf[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = t0 + k;
        const bool ok = t < T && ag[t];
        val[k] = ok ? src[(size_t)t * tstride] : 0.0;
        const double wt = ok ? wg[t] : 0.0;
        cf[k] = lin ? wt : wt * wt;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(cf[k], val[k], acc);
    }
    if (is_cov) K[e] = acc * inv_s2;
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
  // ---- phase 1b: the target kernel's part of Knq
  for (int e = tid; e < n * 16; e += nthr) {
    const int a = e >> 4, c = e & 15;
    const double* xa = p.Xt + ((size_t)g * n_max + a) * D;
    const double* xq = p.Xq + (q0 + c) * D;
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (xq[d] - xa[d]) / th[d];
      d2 = fma(df, df, d2);
    }
    double k0, dk;
    sa_kernel_and_slope(p.kind, d2, os, k0, dk);
    K[e] += k0;
    u[e] = K[e];
  }
  SA_SYNC();
  // ---- phase 2: z = Knn^-1 Knq, 16 right-hand sides.  Forward L y = Knq by block rows: y_kb = W_kb u_kb, then
  // u_i -= L[i, kb] y_kb below the block
  for (int kb = 0; kb < nb; ++kb) {
    const int r0 = 16 * kb, cnt = n - r0 < 16 ? n - r0 : 16;
    for (int e = tid; e < cnt * 16; e += nthr) {
      const int r = e >> 4, c = e & 15;
      double acc = 0.0;
      for (int k = 0; k <= r; ++k) acc = fma(Wd[kb * 256 + r * 16 + k], u[(r0 + k) * 16 + c], acc);
      v[(r0 + r) * 16 + c] = acc;
    }
    SA_SYNC();
    for (int e = (r0 + 16) * 16 + tid; e < n * 16; e += nthr) {
      const int i = e >> 4, c = e & 15;
      double acc = u[e];
      for (int k = 0; k < 16; ++k) acc = fma(-Ls[(size_t)i * ldl + r0 + k], v[(r0 + k) * 16 + c], acc);
      u[e] = acc;
    }
    SA_SYNC();
  }
  // backward L^T z = y (y in v, z into u): z_kb = W_kb^T v_kb, then v_i -= L[kb, i]^T z_kb above the block
  for (int kb = nb - 1; kb >= 0; --kb) {
    const int r0 = 16 * kb, cnt = n - r0 < 16 ? n - r0 : 16;
    for (int e = tid; e < cnt * 16; e += nthr) {
      const int r = e >> 4, c = e & 15;
      double acc = 0.0;
      for (int k = r; k < cnt; ++k) acc = fma(Wd[kb * 256 + k * 16 + r], v[(r0 + k) * 16 + c], acc);
      u[(r0 + r) * 16 + c] = acc;
    }
    SA_SYNC();
    for (int e = tid; e < r0 * 16; e += nthr) {
      const int i = e >> 4, c = e & 15;
      double acc = v[e];
      for (int k = 0; k < cnt; ++k) acc = fma(-Ls[(size_t)(r0 + k) * ldl + i], u[(r0 + k) * 16 + c], acc);
      v[e] = acc;
    }
    SA_SYNC();
  }
  // ---- phase 3: the contractions over the training points, one thread per (output, candidate), a = 0 .. n-1 in order
  for (int e = tid; e < 32; e += nthr) {
    const int c = e & 15;
    const bool with_alpha = e < 16;
    double acc = 0.0;
    for (int a = 0; a < n; ++a) acc = fma(with_alpha ? al[a] : u[a * 16 + c], K[a * 16 + c], acc);
    red[e] = acc;
  }
  SA_SYNC();
  // ---- phase 4: the posterior and the acquisition value, one thread per candidate
  for (int c = tid; c < 16; c += nthr) {
    const double mean_q = (Ssum[c] - m) / s, var_q = Ssum[16 + c] * inv_s2 + os;
    const double mu = fma(s, mean_q + red[c], m);
    const double vr = s2 * (var_q - red[16 + c]);
    const double par = p.acqf_param[g];
    double A, Amu, Av;
    sa_acquisition(p.acqf, par, mu, vr, A, Amu, Av);
    // a candidate with a NaN / inf coordinate: every output of THAT candidate is NaN (the rule of sa_query: a select, finite inputs
    // are untouched)
    double bad = 0.0;
    for (int d = 0; d < D; ++d) {
      const double x = p.Xq[(q0 + c) * D + d];
      bad += x - x;
    }
    p.value[q0 + c] = bad == 0.0 ? A : bad;
    if (p.mu_out) p.mu_out[q0 + c] = bad == 0.0 ? mu : bad;
    if (p.var_out) p.var_out[q0 + c] = bad == 0.0 ? vr : bad;
  }
}

// ---- the studies' training blocks, all at once (include/scaml_gp.h (7j)): Knn and resid of G studies from the padded per-study
// source terms the batched refit (8b) already holds, as (7)'s assemble forms them for one study behind (6')'s weighted sums.
struct TrainBlockParams {
  const double* means_t;      // (G, T, n_max) source means at the training inputs
  const double* covs_p;       // (G, T, n_max (n_max + 1) / 2) source covariances, lower triangle packed row by row
  const double* X;            // (G, n_max, D)
  const double* y;            // (G, n_max) standardised targets
  const int32_t* n_points;    // (G)
  const double* m_all;        // (G)
  const double* s_all;        // (G)
  const double* w;            // (G, T) pruned weights
  const uint8_t* active;      // (G, T)
  const double* theta;        // (G, D + 2)
  double* Knn;                // (G, n_max, n_max): the leading n_g x n_g block is written, both triangles
  double* resid;              // (G, n_max): the leading n_g entries
  int G, n_max, T, D;
};

}  // namespace scaml
