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

constexpr int TARGET_FIT_DMAX = 16;
constexpr int TARGET_FIT_HMAX = 16;

// Dynamic LDS footprint of scaml_target_fit_kernel in doubles: what tf_carve (csrc/gp_target_fit.hip) hands out for a workgroup
// of `waves` waves -- the one definition the host launcher and scaml_target_fit_max_n use (see csrc/gp_fit_params.h).
constexpr size_t target_fit_lds_doubles(int n, int T, int D, bool mfma, int waves) {
  const size_t nw = (size_t)waves, nb = (size_t)(n + 15) / 16;
  const size_t mats = mfma ? 2 * (nb * (nb + 1) / 2) * 16 * 17 : (size_t)(n + 1) * (n + 2) / 2 + (size_t)n * (n + 1) / 2;
  return mats + (size_t)n * D + 2 * (size_t)(n + 1) + 4 * (size_t)n + 16 + 2 * (size_t)T +
         2 * (size_t)(D + 2) + D + nw * (TARGET_FIT_DMAX + 2) + nw + 8 + 2 * TARGET_FIT_HMAX;
}

}  // namespace scaml
