// TEST INFRASTRUCTURE, not product code: the BATCHED entry of csrc/gp_target_fit.hip (tf_main_batched: the body of
// scaml_target_fit_batched_kernel) compiled as single-threaded host code, next to the single-problem entry (tf_main) for the
// problem-by-problem comparison.  Same conventions as tests/host_emul/target_fit_emul.cpp; only
// tests/test_target_fit_batched_emul.py builds and loads it.
#define SCAML_HOST_EMUL 1
#include <math.h>
#include <string.h>
#include <vector>
#include "gp_target_fit.hip"

namespace {
void one_thread(scaml::TfCtx& c) {
  c.tid = 0; c.nthr = 1; c.lane = 0; c.wave = 0; c.nwave = 1; c.solo = 0;
}
}  // namespace

// S problems x B start points in the layouts of scaml_target_mll_batched_f64 / scaml_target_fit_batched_f64 (mode 0 / 1): one
// "workgroup" per row of z, in launch order.
extern "C" int emul_target_fit_batched(const double* means_t, const double* covs_p, const double* X, const double* y, const int32_t* n_points,
                                       const double* m_all, const double* s_all, const double* spec, double* z, int S, int B, int n_max, int T,
                                       int D, int kind, int mode, int max_iter, int history, double gtol, double ftol, double* value,
                                       double* grad, int32_t* info, double* jitter, int32_t* stats) {
  using namespace scaml;
  TargetFitBatchParams bp;
  memset(&bp, 0, sizeof(bp));
  TargetFitParams& p = bp.base;
  p.means_t = means_t; p.covs_p = covs_p; p.X = X; p.y = y;
  bp.n_points = n_points; bp.m_all = m_all; bp.s_all = s_all; bp.S = S;
  if (!target_spec_from_host(spec, p.spec)) return -2;
  const int P = D + 2 + T;
  std::vector<double> ws((size_t)S * B * (6 + 2 * history) * P + 1);
  p.z = z; p.value = value; p.grad = grad; p.info = info; p.jitter = jitter; p.workspace = ws.data(); p.stats = stats;
  p.B = B; p.n = n_max; p.T = T; p.D = D; p.kind = kind; p.mode = mode; p.max_iter = max_iter; p.history = history; p.max_ls = 20;
  p.gtol = gtol; p.ftol = ftol;
  std::vector<double> lds(target_fit_batched_lds_doubles(n_max, T, D, false, 1));
  for (int row = 0; row < S * B; ++row) {
    TfCtx c;
    one_thread(c);
    tf_main_batched(c, bp, lds.data(), row, 0);
  }
  return 0;
}

// One problem through the single-problem entry (what tests/host_emul/target_fit_emul.cpp runs), from the same shared object.
extern "C" int emul_target_fit_single(const double* means_t, const double* covs_p, const double* X, const double* y, double m_all, double s_all,
                                      const double* spec, double* z, int B, int n, int T, int D, int kind, int mode, int max_iter, int history,
                                      double gtol, double ftol, double* value, double* grad, int32_t* info, double* jitter, int32_t* stats) {
  using namespace scaml;
  TargetFitParams p;
  memset(&p, 0, sizeof(p));
  p.means_t = means_t; p.covs_p = covs_p; p.X = X; p.y = y; p.m_all = m_all; p.s_all = s_all;
  if (!target_spec_from_host(spec, p.spec)) return -2;
  const int P = D + 2 + T;
  std::vector<double> ws((size_t)B * (6 + 2 * history) * P + 1);
  p.z = z; p.value = value; p.grad = grad; p.info = info; p.jitter = jitter; p.workspace = ws.data(); p.stats = stats;
  p.B = B; p.n = n; p.T = T; p.D = D; p.kind = kind; p.mode = mode; p.max_iter = max_iter; p.history = history; p.max_ls = 20;
  p.gtol = gtol; p.ftol = ftol;
  std::vector<double> lds(target_fit_lds_doubles(n, T, D, false, 1));
  for (int b = 0; b < B; ++b) {
    TfCtx c;
    one_thread(c);
    c.n = n; c.T = T; c.D = D; c.P = P; c.E = n * (n + 1) / 2; c.kind = kind;
    if (tf_carve(c, lds.data(), n, T, D, 1, 0) != lds.data() + lds.size()) return -1;
    tf_main(c, p, b);
  }
  return 0;
}

// the LDS a batched launch asks for, and the largest single-problem footprint it has to hold
extern "C" long long emul_target_fit_batched_lds_doubles(int n_max, int T, int D, int waves, int may_mfma) {
  return (long long)scaml::target_fit_batched_lds_doubles(n_max, T, D, may_mfma != 0, waves);
}
extern "C" long long emul_target_fit_problem_lds_doubles(int n, int T, int D, int waves, int may_mfma) {
  return (long long)scaml::target_fit_lds_doubles(n, T, D, may_mfma != 0 && scaml::target_fit_mfma_shape(n, T, D, waves), waves);
}
