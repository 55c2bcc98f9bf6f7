// Kernel-argument block of the fantasy acquisition kernel (csrc/gp_fantasy.hip), shared by device source and host launcher.
#pragma once
#include <stdint.h>

namespace scaml {

constexpr int FANTASY_MAX_F = 64;      // fantasies: one lane each
constexpr int FANTASY_MAX_N = 256;     // training points of the value path (scaml_fit_max_n)
constexpr int FANTASY_GRAD_MAX_N = 96; // training points of the gradient path (the GRAD pass's covariance block)
constexpr int FANTASY_GRAD_MAX_D = 15; // (the GRAD pass's 16 columns per query point)

struct FantasyAcqfParams {
  const double* Knq;      // (n, M)  cross block of the target GP (scaml_target_assemble_f64)
  const double* Z;        // (n, M)  Knn^-1 Knq
  const double* alpha;    // (n, F)  Knn^-1 r_f, one column per fantasy (row-major: a row is contiguous)
  const double* mean_q;   // (M)     standardised prior mean at the queries
  const double* var_q;    // (M)     standardised prior variance at the queries
  double m_all, s_all, noise_add;
  const int32_t* info;    // (1) or NULL: a failed factorisation turns every output into NaN
  double acqf_param;      // UCB: beta; EI: best_f (original units)
  // gradient inputs (grad != NULL): the weighted sums of the GRAD pass and the target kernel
  const double* cov_g;    // (n, M * 16)
  const double* mu_g;     // (M * 16)
  const double* var_g;    // (M * 16)
  const double* Xt;       // (n, D)
  const double* Xq;       // (M, D)
  const double* theta;    // (D + 2)
  double* value;          // (M)
  double* grad;           // (M, D) or NULL
  int n, M, F, D;
  int acqf;               // 0 UCB, 1 EI
  int pad_;
};

}  // namespace scaml
