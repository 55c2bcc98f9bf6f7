// TEST INFRASTRUCTURE, not product code: the arithmetic of the value-only joint q-point acquisition kernel (csrc/gp_qacqf.h:
// qa_batch<true, true>, the body of scaml_target_qacqf_value_kernel, include/scaml_gp.h (7r)) compiled as host code, one batch after
// the other with a single emulated thread, and the column map of the value layout (csrc/gp_qacqf_columns.h).
// tests/test_qacqf_value_emul.py builds and loads it.
#include <limits>
#include <vector>
#include "gp_qacqf.h"
#include "gp_dispatch.h"   // the launch plans

extern "C" int emul_qav_column(int b, int j, int q) { return scaml::qav_column(b, j, q); }
extern "C" int emul_qav_columns(int B, int q) { return scaml::qav_columns(B, q); }
extern "C" int emul_qav_batch_of(int strip, int c, int q, int B) { return scaml::qav_batch_of(strip, c, q, B); }

extern "C" long long emul_qacqf_value_lds_doubles(int n, int q, int p, int S) { return (long long)scaml::qa_value_lds_doubles(n, q, p, S); }
extern "C" long long emul_posterior_linv_lds_doubles(int N, int D) { return (long long)scaml::posterior_linv_lds_doubles(N, D); }

// qacqf_value_plan(B, n, q, p, S) -> grid, block, LDS doubles
extern "C" void emul_qacqf_value_plan(int B, int n, int q, int p, int S, long long* out) {
  const scaml::QAcqfPlan pl = scaml::qacqf_value_plan(B, n, q, p, S);
  out[0] = pl.grid, out[1] = pl.block, out[2] = (long long)pl.lds_doubles;
}

// posterior_jointv_plan(T, N, D, Mp) -> grid, block, LDS doubles
extern "C" void emul_posterior_jointv_plan(int T, int N, int D, int Mp, long long* out) {
  const scaml::PosteriorJointValuePlan pl = scaml::posterior_jointv_plan(T, N, D, Mp);
  out[0] = pl.grid, out[1] = pl.block, out[2] = (long long)pl.lds_doubles;
}

// All B batches of a call of (7r), its argument list
extern "C" int emul_qacqf_value(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                double m_all, double s_all, const int32_t* info, const double* cov_s, const double* Xq, const double* theta,
                                const double* base_samples, const double* Xp, const double* Zp, const double* mu_p, const double* Sigma_pp,
                                int acqf, double acqf_param, int n, int Mp, int B, int q, int p, int S, int D, int kind, double* value,
                                double* jitter_used, int32_t* info_out) {
  using namespace scaml;
  if (n < 1 || q < 1 || p < 0 || S < 1 || D < 1 || Mp < 0 || B < 0 || !qa_acqf_valid(acqf)) return -1;
  if (p > 0 && (!Xp || !Zp || !mu_p || !Sigma_pp)) return -1;
  if (q <= QACQF_MAX_Q && Mp != qav_columns(B, q)) return -1;
  if (q + p > QACQF_MAX_Q || S > QACQF_MAX_SAMPLES || n + p + q > QACQF_MAX_ROWS || D > QACQF_MAX_D) return -2;
  QAcqfPendingParams pp{{Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_s, nullptr, nullptr, nullptr, Xq, theta, base_samples, acqf_param,
                         value, nullptr, jitter_used, info_out, n, Mp, q, S, D, kind, acqf, 0},
                        {Xp, Zp, mu_p, Sigma_pp, p, 0}};
  const size_t doubles = qa_value_lds_doubles(n, q, p, S);
  std::vector<double> lds(doubles);
  for (int b = 0; b < B; ++b) {
    lds.assign(doubles, std::numeric_limits<double>::quiet_NaN());   // what the batch reads of it, it has written
    qa_batch_value(pp, lds.data(), b, 0, 1);
  }
  return 0;
}
