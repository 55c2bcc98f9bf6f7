// TEST INFRASTRUCTURE, not product code: what tests/host_emul/target_fit_emul.cpp and target_fit_batched_emul.cpp share --
// csrc/gp_target_fit.hip compiled as single-threaded host code (SCAML_HOST_EMUL: one "thread", barriers are no-ops, every
// cooperative loop runs sequentially), the fill of its kernel arguments and one problem through the single-problem entry.
#pragma once
#define SCAML_HOST_EMUL 1
#include <math.h>
#include <string.h>
#include <vector>
#include "gp_target_fit.hip"

namespace emul {
inline void one_thread(scaml::TfCtx& c) {
  c.tid = 0; c.nthr = 1; c.lane = 0; c.wave = 0; c.nwave = 1; c.solo = 0;
}

// `p` zeroed, then everything but the standardiser (single: m_all / s_all; batch: its arrays); `ws` becomes the workspace of `rows`
// start points.  False: the constraint / prior block is not valid.
inline bool fill_params(scaml::TargetFitParams& p, std::vector<double>& ws, size_t rows, const double* means_t, const double* covs_p,
                        const double* X, const double* y, const double* spec, double* z, int B, int n, int T, int D, int kind, int mode,
                        int max_iter, int history, double gtol, double ftol, double* value, double* grad, int32_t* info, double* jitter,
                        int32_t* stats) {
  memset(&p, 0, sizeof(p));
  p.means_t = means_t; p.covs_p = covs_p; p.X = X; p.y = y;
  if (!scaml::target_spec_from_host(spec, p.spec)) return false;
  ws.resize(rows * (6 + 2 * history) * (D + 2 + T) + 1);
  p.z = z; p.value = value; p.grad = grad; p.info = info; p.jitter = jitter; p.workspace = ws.data(); p.stats = stats;
  p.B = B; p.n = n; p.T = T; p.D = D; p.kind = kind; p.mode = mode; p.max_iter = max_iter; p.history = history; p.max_ls = 20;
  p.gtol = gtol; p.ftol = ftol;
  return true;
}

// One problem, B start points, through tf_carve / tf_main: one "workgroup" per start, in launch order.
inline int target_fit(const double* means_t, const double* covs_p, const double* X, const double* y, double m_all, double s_all,
                      const double* spec, double* z, int B, int n, int T, int D, int kind, int mode, int max_iter, int history, double gtol,
                      double ftol, double* value, double* grad, int32_t* info, double* jitter, int32_t* stats) {
  using namespace scaml;
  TargetFitParams p;
  std::vector<double> ws;
  if (!fill_params(p, ws, (size_t)B, means_t, covs_p, X, y, spec, z, B, n, T, D, kind, mode, max_iter, history, gtol, ftol, value, grad, info,
                   jitter, stats))
    return -2;
  p.m_all = m_all; p.s_all = s_all;
  std::vector<double> lds(target_fit_lds_doubles(n, T, D, false, 1));
  for (int b = 0; b < B; ++b) {
    TfCtx c;
    one_thread(c);
    c.n = n; c.T = T; c.D = D; c.P = D + 2 + T; c.E = n * (n + 1) / 2; c.kind = kind;
    if (tf_carve(c, lds.data(), n, T, D, 1, 0) != lds.data() + lds.size()) return -1;
    tf_main(c, p, b);
  }
  return 0;
}
}  // namespace emul
