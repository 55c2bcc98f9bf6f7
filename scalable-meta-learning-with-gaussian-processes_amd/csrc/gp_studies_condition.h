// gp_studies_condition.h -- the fantasy set-up of many BO studies with pending evaluations in a constant number of launches
// (include/scaml_gp.h (7m), (7n)): argument blocks, LDS footprints and the arithmetic of one study.  One source for the device kernels
// (csrc/gp_studies_condition.hip: a workgroup of 256 threads per study), the host launcher and the single-threaded host build the CPU
// tests check against torch and against a long-double reference (any compiler but hipcc: tests/host_emul/studies_condition_emul.cpp).
//
// Everything a fantasy model needs follows from ONE Cholesky factor of the joint block.  With X' = cat(train_X, X_pend), n' = n + p,
//   K'    = sum_t w_t^2 Sigma_t(X', X') / s^2 + os k(X', X') + sigma^2 I   (standardised units; what the conditioned model factors),
//   mean' = (sum_t w_t mu_t(X') - m) / s,          L' = chol(K') = [[L_nn, 0], [L_pn, L_pp]]:
//   L_nn is the parent's factor and L_pp L_pp^T the posterior covariance at the pending points WITH observation noise;
//   v = L_nn^-1 (y~_n - mean'_n);   posterior mean at the pending points  mu~_p = mean'_p + L_pn v;
//   fantasy targets  y~_p^f = mu~_p + L_pp eps_f  (eps_f: row f of the standard-normal draw), in original units m + s y~;
//   the residual of fantasy f is L' [v ; eps_f], hence  alpha_f[:, f] = K'^-1 resid_f = L'^-T [v ; eps_f].
// (7m) sc_condition_block forms K', the observed rows' residual and mean'_p from the value-mode grouped source pass (5f) called with the
// study's own X' as query strips; (2) factors all blocks; (7n) sc_fantasy_condition does the one forward and the F backward substitutions.
//
// Every sum is formed by ONE thread in a fixed ascending order (tasks in (6)'s order, then rows / columns ascending), no atomics, no
// cross-wave reductions: the outputs are a pure function of the inputs and the host build computes what the device computes.
#pragma once
#include "gp_studies_acqf.h"   // the limits (n_max <= 96, D <= 15, F_max <= 64) and, through it, SA_DEV / SA_SYNC and the target kernel

namespace scaml {

constexpr int STUDIES_CONDITION_THREADS = 256;

// ---- (7m) the training block of the CONDITIONED models ---------------------------------------------------------------------------
struct StudiesConditionBlockParams {
  const double* mu;            // (T, Mq)          value-mode grouped pass (5f) at the studies' own X' strips
  const double* cov;           // (T, n_max, Mq)   row a: the study's leading point a, column: a point of its strips
  const int32_t* strip_base;   // (G) the first strip of study g: point i of X'_g is column 16 strip_base[g] + i
  const double* w;             // (G, T) weights, zero where pruned
  const uint8_t* active;       // (G, T) a masked task is skipped, not multiplied by zero
  const double* Xt;            // (G, n_max, D) X'_g: the observed inputs, then the pending ones
  const double* theta;         // (G, D + 2) target kernel: lengthscales, outputscale, noise
  const double* y;             // (G, n_max) standardised targets; rows >= n_obs are not read
  const int32_t* n_points;     // (G) n'_g
  const int32_t* n_obs;        // (G) n_g, 1 <= n_g <= n'_g
  const double* m_all;         // (G)
  const double* s_all;         // (G) > 0
  double* Knn;                 // (G, n_max, n_max) the leading n'_g block, both triangles, noise on the diagonal
  double* resid;               // (G, n_max) y_i - mean'_i for i < n_obs, zero for the pending rows
  double* mean_p;              // (G, n_max) mean'_i at the pending rows i = n_obs .. n' - 1 (the observed rows are not written)
  int Mq, G, n_max, T, D, kind;
};

// LDS in doubles:  X' [n_max][D] | bad [n_max]
constexpr size_t sc_block_lds_doubles(int n_max, int D) { return (size_t)n_max * (size_t)D + (size_t)n_max; }

// Study g by `nthr` cooperating threads.  Element (i, c), c <= i, of K' is fed by cov[t][a = i][column of point c]: the row of the LATER
// point, the column of the earlier one (consecutive threads, consecutive columns); (c, i) is its mirror image.
//   n'_g outside 1 .. n_max: nothing is known about the study's extent and nothing is written ((7n) answers NaN for it).
//   n_obs outside 1 .. n', strips outside the pass's Mq columns, or a NaN / infinite coordinate in X'_g: the study's outputs are NaN.
SA_DEV void sc_condition_block(const StudiesConditionBlockParams& p, double* lds, int g, int tid, int nthr) {
  const int n_max = p.n_max, T = p.T, D = p.D;
  const int n = p.n_points[g], no = p.n_obs[g], base = p.strip_base[g];
  if (n < 1 || n > n_max) return;   // (uniform over the workgroup, as every branch up to the first barrier)
  const bool refused = no < 1 || no > n || base < 0 || (long long)16 * base + n > (long long)p.Mq;
  double* Xs = lds;                      // [i][D]
  double* bad = Xs + (size_t)n_max * D;  // [i]: sum_d (x_d - x_d), 0 or NaN
  const double* Xg = p.Xt + (size_t)g * n_max * D;
  for (int e = tid; e < n * D; e += nthr) Xs[e] = Xg[e];
  SA_SYNC();
  for (int i = tid; i < n; i += nthr) {
    double b = 0.0;
    for (int d = 0; d < D; ++d) b += Xs[i * D + d] - Xs[i * D + d];
    bad[i] = b;
  }
  SA_SYNC();
  double bd = refused ? (double)NAN : 0.0;
  for (int i = 0; i < n; ++i) bd += bad[i];
  const bool ok = bd == 0.0;
  const double nan = NAN;
  double* Kg = p.Knn + (size_t)g * n_max * n_max;
  double* rg = p.resid + (size_t)g * n_max;
  double* mg = p.mean_p + (size_t)g * n_max;
  if (!ok) {
    for (int e = tid; e < n * n; e += nthr) Kg[(size_t)(e / n) * n_max + e % n] = nan;
    for (int i = tid; i < n; i += nthr) {
      rg[i] = nan;
      if (i >= no) mg[i] = nan;
    }
    return;
  }
  const double s = p.s_all[g], m = p.m_all[g], s2 = s * s;
  const double* th = p.theta + (size_t)g * (D + 2);
  const double os = th[D], noise = th[D + 1];
  const double* wg = p.w + (size_t)g * T;
  const uint8_t* ag = p.active + (size_t)g * T;
  const size_t W = (size_t)p.Mq, col0 = (size_t)16 * base;
  for (int e = tid; e < n * n; e += nthr) {
    const int i = e / n, c = e - i * n;
    if (c > i) continue;
    const double cov_s = sa_weighted_sum(p.cov + (size_t)i * W + col0 + c, (size_t)n_max * W, wg, ag, T, 2);
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (Xs[i * D + d] - Xs[c * D + d]) / th[d];
      d2 = fma(df, df, d2);
    }
    double k0, dk;
    sa_kernel_and_slope(p.kind, d2, os, k0, dk);
    const double v = cov_s / s2 + k0;
    Kg[(size_t)i * n_max + c] = v + (i == c ? noise : 0.0);
    if (i != c) Kg[(size_t)c * n_max + i] = v;
  }
  for (int i = tid; i < n; i += nthr) {
    const double mean_s = sa_weighted_sum(p.mu + col0 + i, W, wg, ag, T, 1);
    const double mean = (mean_s - m) / s;
    if (i < no) {
      rg[i] = p.y[(size_t)g * n_max + i] - mean;
    } else {
      rg[i] = 0.0;
      mg[i] = mean;
    }
  }
}

// ---- (7n) the fantasies and alpha_f from the factor of K' ------------------------------------------------------------------------
struct StudiesFantasyConditionParams {
  const double* L;             // (G, n_max, n_max) factor of K', row stride n_max: (2)'s output
  const double* resid;         // (G, n_max) (7m)'s
  const double* mean_p;        // (G, n_max) (7m)'s
  const int32_t* n_points;     // (G) n'_g
  const int32_t* n_obs;        // (G) n_g
  const int32_t* info;         // (G) (2)'s status: != 0, the study's outputs are NaN
  const double* eps;           // (G, p_max, F_max) standard-normal draws: row i holds the F_g values of pending point i contiguously
  const int32_t* n_fant;       // (G) 1 <= F_g <= F_max
  const double* m_all;         // (G)
  const double* s_all;         // (G)
  double* alpha_f;             // (G, n_max, F_max) K'^-1 [resid_0 .. resid_{F_g - 1}]: (7k)'s layout
  double* y_fant;              // (G, p_max, F_max) fantasy targets, original units
  double* mu_p;                // (G, p_max) posterior mean at the pending points, original units
  int G, n_max, p_max, F_max;
};

// LDS in doubles:  L [n_max][n_max | 1] | r, v, mu~_p [3][n_max] | x [n_max][F_max]
constexpr size_t sc_fantasy_lds_doubles(int n_max, int F_max) {
  return (size_t)n_max * (size_t)(n_max | 1) + 3 * (size_t)n_max + (size_t)n_max * (size_t)F_max;
}

// Study g by `nthr` cooperating threads.  info[g] != 0, n'_g outside 1 .. n_max, n_g outside 1 .. n'_g, F_g outside 1 .. F_max,
// n'_g - n_g > p_max, or a study with nothing pending (n_g == n'_g) whose F_g is not 1: the study's outputs are NaN, over the part of
// its extent that the valid counts describe.  Nothing past n'_g, p_g or F_g is read or written.
SA_DEV void sc_fantasy_condition(const StudiesFantasyConditionParams& p, double* lds, int g, int tid, int nthr) {
  const int n_max = p.n_max, p_max = p.p_max, Fm = p.F_max;
  const int n = p.n_points[g], no = p.n_obs[g], F = p.n_fant[g];
  const double nan = NAN;
  double* ag = p.alpha_f + (size_t)g * n_max * Fm;
  double* yg = p.y_fant + (size_t)g * p_max * Fm;
  double* mg = p.mu_p + (size_t)g * p_max;
  const bool n_ok = n >= 1 && n <= n_max, no_ok = n_ok && no >= 1 && no <= n, f_ok = F >= 1 && F <= Fm;
  if (p.info[g] != 0 || !no_ok || !f_ok || n - no > p_max || (no == n && F != 1)) {
    const int nn = n < 0 ? 0 : (n > n_max ? n_max : n), ff = F < 0 ? 0 : (F > Fm ? Fm : F);
    const int pp = no_ok ? (n - no > p_max ? p_max : n - no) : 0;
    for (int e = tid; e < nn * ff; e += nthr) ag[(size_t)(e / ff) * Fm + e % ff] = nan;
    for (int e = tid; e < pp * ff; e += nthr) yg[(size_t)(e / ff) * Fm + e % ff] = nan;
    for (int i = tid; i < pp; i += nthr) mg[i] = nan;
    return;
  }
  const int np = n - no, ldl = n_max | 1;
  double* Ls = lds;                          // the lower triangle of L'
  double* r = Ls + (size_t)n_max * ldl;      // [n_obs]: the running right-hand side of the forward substitution
  double* v = r + n_max;                     // [n_obs]: v = L_nn^-1 resid
  double* mt = v + n_max;                    // [p]: mu~_p
  double* xs = mt + n_max;                   // [a][F_max]: the right-hand sides [v ; eps_f], then alpha_f
  const double* Lg = p.L + (size_t)g * n_max * n_max;
  for (int e = tid; e < n * n; e += nthr) {
    const int i = e / n, j = e - i * n;
    if (j <= i) Ls[(size_t)i * ldl + j] = Lg[(size_t)i * n_max + j];
  }
  for (int i = tid; i < no; i += nthr) r[i] = p.resid[(size_t)g * n_max + i];
  SA_SYNC();
  // forward L_nn v = resid, column by column: v_i = (r_i - sum_{k < i} L[i][k] v_k) / L[i][i], row i's running sum kept in r[i] by the
  // one thread that owns the row, k ascending.  Every thread divides r[k] itself (the same operands, the same quotient); the owner of
  // row k keeps the quotient in v[k], which nobody reads before the substitution is over.
  for (int k = 0; k < no; ++k) {
    const double vk = r[k] / Ls[(size_t)k * ldl + k];
    for (int i = tid; i < no; i += nthr) {
      if (i == k) v[k] = vk;
      else if (i > k) r[i] = fma(-Ls[(size_t)i * ldl + k], vk, r[i]);
    }
    SA_SYNC();
  }
  // mu~_p[i] = mean'_p[i] + sum_{k < n_obs} L[n_obs + i][k] v_k, one thread per pending point, k ascending
  const double s = p.s_all[g], m = p.m_all[g];
  for (int i = tid; i < np; i += nthr) {
    double acc = 0.0;
    for (int k = 0; k < no; ++k) acc = fma(Ls[(size_t)(no + i) * ldl + k], v[k], acc);
    const double mu = p.mean_p[(size_t)g * n_max + no + i] + acc;
    mt[i] = mu;
    mg[i] = fma(s, mu, m);
  }
  // the right-hand sides [v ; eps_f], one thread per element
  const double* eg = p.eps + (size_t)g * p_max * Fm;
  for (int e = tid; e < n * F; e += nthr) {
    const int a = e / F, f = e - a * F;
    xs[(size_t)a * Fm + f] = a < no ? v[a] : eg[(size_t)(a - no) * Fm + f];
  }
  SA_SYNC();
  // y~_p^f[i] = mu~_p[i] + sum_{j <= i} L_pp[i][j] eps_f[j], one thread per (pending point, fantasy), j ascending
  for (int e = tid; e < np * F; e += nthr) {
    const int i = e / F, f = e - i * F;
    double acc = 0.0;
    for (int j = 0; j <= i; ++j) acc = fma(Ls[(size_t)(no + i) * ldl + no + j], xs[(size_t)(no + j) * Fm + f], acc);
    yg[(size_t)i * Fm + f] = fma(s, mt[i] + acc, m);
  }
  SA_SYNC();   // (the samples have read eps out of xs before the substitution overwrites it)
  // backward L'^T x = [v ; eps_f], one thread per fantasy column: x_i = (b_i - sum_{k > i} L[k][i] x_k) / L[i][i], k ascending
  for (int f = tid; f < F; f += nthr) {
    for (int i = n - 1; i >= 0; --i) {
      double acc = xs[(size_t)i * Fm + f];
      for (int k = i + 1; k < n; ++k) acc = fma(-Ls[(size_t)k * ldl + i], xs[(size_t)k * Fm + f], acc);
      const double x = acc / Ls[(size_t)i * ldl + i];
      xs[(size_t)i * Fm + f] = x;
      ag[(size_t)i * Fm + f] = x;
    }
  }
}

}  // namespace scaml
