// Kernel-argument block of the target-GP fit kernel (csrc/gp_target_fit.hip), shared by device source and host launcher.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gp_hyper_spec.h"   // TargetSpec

namespace scaml {

struct TargetFitParams {
  const double* means_t;   // (T, n)            source posterior means at the target inputs, original units
  const double* covs_p;    // (T, n (n + 1) / 2) source posterior covariances, packed lower triangle (a >= b at a (a + 1) / 2 + b)
  const double* X;         // (n, D) target inputs
  const double* y;         // (n)    target observations standardised with (m_all, s_all)
  double m_all, s_all;
  TargetSpec spec;
  double* z;               // (B, P) P = D + 2 + T: [raw lengthscales, raw outputscale, raw noise, weights]; optimiser: start points in, optima out
  double* value;           // (B) objective mll = [log N(y | mean, cov) + log priors] / n at z (optimiser: at the optimum)
  double* grad;            // (B, P) d mll / d z (evaluation mode; may be NULL in optimiser mode)
  int32_t* info;           // (B) 0 ok, k > 0: pivot k not positive even with the largest jitter
  double* jitter;          // (B) jitter that succeeded (NULL ok)
  double* workspace;       // optimiser: B * (6 + 2 history) * P doubles
  int32_t* stats;          // optimiser: (B, 4) iterations, evaluations, status, reserved (NULL ok)
  int B, n, T, D;
  int kind;
  int mode;                // 0: value + gradient at z, 1: L-BFGS from z
  int max_iter, history, max_ls;
  int use_mfma;            // 1: factorisation on the matrix cores (16 x 16 tiles in LDS; n <= 112), 0: column-by-column elimination
  double gtol, ftol;
};

// scaml_target_fit_batched_kernel: S problems x B start points.  `base` describes the batch: means_t / covs_p / X / y point at
// problem 0 of (S, T, n_max), (S, T, n_max (n_max + 1) / 2), (S, n_max, D), (S, n_max); n = n_max; B = start points PER PROBLEM;
// z, value, grad, info, jitter, workspace, stats hold S * B rows, problem-major; m_all / s_all are not read (the arrays below are);
// use_mfma = 1: every problem whose own n takes the matrix-core factorisation (target_fit_mfma_shape) uses it.
struct TargetFitBatchParams {
  TargetFitParams base;
  const int32_t* n_points;   // (S) 1 <= n_s <= n_max
  const double* m_all;       // (S)
  const double* s_all;       // (S) > 0
  int S;
};

constexpr int TARGET_FIT_DMAX = 16;
constexpr int TARGET_FIT_HMAX = 16;
constexpr int TARGET_FIT_MFMA_MAX_N = 112;            // the matrix-core factorisation: two block triangles of 16 x 17 tiles in LDS
constexpr size_t TARGET_FIT_LDS_LIMIT = 160 * 1024;   // bytes of LDS a workgroup may ask for on gfx950

// Dynamic LDS footprint of scaml_target_fit_kernel in doubles: what tf_carve (csrc/gp_target_fit.hip) hands out for a workgroup
// of `waves` waves -- the one definition the host launcher and scaml_target_fit_max_n use (see csrc/gp_fit_params.h).
constexpr size_t target_fit_lds_doubles(int n, int T, int D, bool mfma, int waves) {
  const size_t nw = (size_t)waves, nb = (size_t)(n + 15) / 16;
  const size_t mats = mfma ? 2 * (nb * (nb + 1) / 2) * 16 * 17 : (size_t)(n + 1) * (n + 2) / 2 + (size_t)n * (n + 1) / 2;
  return mats + (size_t)n * D + 2 * (size_t)(n + 1) + 4 * (size_t)n + 16 + 2 * (size_t)T +
         2 * (size_t)(D + 2) + D + nw * (TARGET_FIT_DMAX + 2) + nw + 8 + 2 * TARGET_FIT_HMAX;
}

// Which problems take the matrix-core factorisation: decided per problem from its own n, by the single-problem launcher on the
// host and by each workgroup of the batched kernel on the device -- one rule, so a problem is factorised the same way in both.
constexpr bool target_fit_mfma_shape(int n, int T, int D, int waves) {
  return n <= TARGET_FIT_MFMA_MAX_N && target_fit_lds_doubles(n, T, D, true, waves) * sizeof(double) <= TARGET_FIT_LDS_LIMIT;
}

// LDS of a batched launch: the largest footprint any 1 <= n <= n_max can ask for (the counts live in device memory)
constexpr size_t target_fit_batched_lds_doubles(int n_max, int T, int D, bool may_mfma, int waves) {
  size_t m = 0;
  for (int n = 1; n <= n_max; ++n) {
    const size_t d = target_fit_lds_doubles(n, T, D, may_mfma && target_fit_mfma_shape(n, T, D, waves), waves);
    m = d > m ? d : m;
  }
  return m;
}

}  // namespace scaml
