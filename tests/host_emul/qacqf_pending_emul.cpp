// TEST INFRASTRUCTURE, not product code: the arithmetic of the joint q-point acquisition kernel with evaluations pending
// (csrc/gp_qacqf.h: qa_batch<true>, the body of scaml_target_qacqf_pending_kernel, include/scaml_gp.h (7q)) compiled as host code,
// one batch after the other with a single emulated thread.  tests/test_qacqf_pending_emul.py builds and loads it.
#include <limits>
#include <vector>
#include "gp_qacqf.h"
#include "gp_dispatch.h"   // the launch plan

extern "C" long long emul_qacqf_pending_lds_doubles(int n, int q, int p, int S) { return (long long)scaml::qa_pending_lds_doubles(n, q, p, S); }

// qacqf_pending_plan(B, n, q, p, S) -> grid, block, LDS doubles
extern "C" void emul_qacqf_pending_plan(int B, int n, int q, int p, int S, long long* out) {
  const scaml::QAcqfPlan pl = scaml::qacqf_pending_plan(B, n, q, p, S);
  out[0] = pl.grid, out[1] = pl.block, out[2] = (long long)pl.lds_doubles;
}

// All B = Mq / q batches of a call of (7q), its argument list
extern "C" int emul_qacqf_pending(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                  double m_all, double s_all, const int32_t* info, const double* cov_g, const double* mu_g,
                                  const double* var_g, const double* Xt, const double* Xq, const double* theta, const double* base_samples,
                                  const double* Xp, const double* Zp, const double* mu_p, const double* Sigma_pp, int acqf,
                                  double acqf_param, int n, int Mq, int q, int p, int S, int D, int kind, double* value, double* grad,
                                  double* jitter_used, int32_t* info_out) {
  using namespace scaml;
  if (n < 1 || q < 1 || p < 0 || S < 1 || D < 1 || Mq < 0 || Mq % q || !qa_acqf_valid(acqf)) return -1;
  if (p > 0 && (!Xp || !Zp || !mu_p || !Sigma_pp)) return -1;
  if (q + p > QACQF_MAX_Q || S > QACQF_MAX_SAMPLES || n + p + q > QACQF_MAX_ROWS || D > QACQF_MAX_D) return -2;
  QAcqfPendingParams pp{{Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_g, mu_g, var_g, Xt, Xq, theta, base_samples, acqf_param,
                         value, grad, jitter_used, info_out, n, Mq, q, S, D, kind, acqf, 0},
                        {Xp, Zp, mu_p, Sigma_pp, p, 0}};
  const size_t doubles = qa_pending_lds_doubles(n, q, p, S);
  std::vector<double> lds(doubles);
  for (int b = 0; b < Mq / q; ++b) {
    lds.assign(doubles, std::numeric_limits<double>::quiet_NaN());   // what the batch reads of it, it has written
    qa_batch_pending(pp, lds.data(), b, 0, 1);
  }
  return 0;
}
