// TEST INFRASTRUCTURE, not product code: the BATCHED entry of csrc/gp_target_fit.hip (tf_main_batched: the body of
// scaml_target_fit_batched_kernel) compiled as single-threaded host code, next to the single-problem entry (tf_main) for the
// problem-by-problem comparison.  Same conventions as tests/host_emul/target_fit_emul.cpp; only
// tests/test_target_fit_batched_emul.py builds and loads it.
#include "target_fit_emul_common.h"

// S problems x B start points in the layouts of scaml_target_mll_batched_f64 / scaml_target_fit_batched_f64 (mode 0 / 1): one
// "workgroup" per row of z, in launch order.
extern "C" int emul_target_fit_batched(const double* means_t, const double* covs_p, const double* X, const double* y, const int32_t* n_points,
                                       const double* m_all, const double* s_all, const double* spec, double* z, int S, int B, int n_max, int T,
                                       int D, int kind, int mode, int max_iter, int history, double gtol, double ftol, double* value,
                                       double* grad, int32_t* info, double* jitter, int32_t* stats) {
  using namespace scaml;
  TargetFitBatchParams bp;
  memset(&bp, 0, sizeof(bp));
  std::vector<double> ws;
  if (!emul::fill_params(bp.base, ws, (size_t)S * B, means_t, covs_p, X, y, spec, z, B, n_max, T, D, kind, mode, max_iter, history, gtol, ftol,
                         value, grad, info, jitter, stats))
    return -2;
  bp.n_points = n_points; bp.m_all = m_all; bp.s_all = s_all; bp.S = S;
  std::vector<double> lds(target_fit_batched_lds_doubles(n_max, T, D, false, 1));
  for (int row = 0; row < S * B; ++row) {
    TfCtx c;
    emul::one_thread(c);
    tf_main_batched(c, bp, lds.data(), row, 0);
  }
  return 0;
}

// One problem through the single-problem entry (what tests/host_emul/target_fit_emul.cpp runs), from the same shared object.
extern "C" int emul_target_fit_single(const double* means_t, const double* covs_p, const double* X, const double* y, double m_all, double s_all,
                                      const double* spec, double* z, int B, int n, int T, int D, int kind, int mode, int max_iter, int history,
                                      double gtol, double ftol, double* value, double* grad, int32_t* info, double* jitter, int32_t* stats) {
  return emul::target_fit(means_t, covs_p, X, y, m_all, s_all, spec, z, B, n, T, D, kind, mode, max_iter, history, gtol, ftol, value, grad, info,
                          jitter, stats);
}

// the LDS a batched launch asks for, and the largest single-problem footprint it has to hold
extern "C" long long emul_target_fit_batched_lds_doubles(int n_max, int T, int D, int waves, int may_mfma) {
  return (long long)scaml::target_fit_batched_lds_doubles(n_max, T, D, may_mfma != 0, waves);
}
extern "C" long long emul_target_fit_problem_lds_doubles(int n, int T, int D, int waves, int may_mfma) {
  return (long long)scaml::target_fit_lds_doubles(n, T, D, may_mfma != 0 && scaml::target_fit_mfma_shape(n, T, D, waves), waves);
}
