// TEST INFRASTRUCTURE, not product code: the arithmetic of the joint q-point acquisition kernel (csrc/gp_qacqf.h: qa_tail and qa_batch,
// the body of csrc/gp_qacqf.hip) compiled as host code, one batch after the other with a single emulated thread.
// tests/test_qacqf_emul.py builds and loads it.
#include <limits>
#include <vector>
#include "gp_qacqf.h"
#include "gp_dispatch.h"   // the launch plan

extern "C" long long emul_qacqf_lds_doubles(int n, int q, int S) { return (long long)scaml::qa_lds_doubles(n, q, S); }

// qacqf_plan(B, n, q, S) -> grid, block, LDS doubles
extern "C" void emul_qacqf_plan(int B, int n, int q, int S, long long* out) {
  const scaml::QAcqfPlan p = scaml::qacqf_plan(B, n, q, S);
  out[0] = p.grid, out[1] = p.block, out[2] = (long long)p.lds_doubles;
}

// The tail alone: Sigma (q, q), mu (q), base samples (S, q) -> value, mubar (q), Sigmabar (q, q), jitter, info.
// The LDS is filled with NaN first: what the tail reads of it, the caller or the tail itself has written.
extern "C" int emul_qacqf_tail(const double* Sigma, const double* mu, const double* base_samples, int q, int S, int acqf, double par,
                               double* value, double* mubar, double* Sigmabar, double* jitter, int32_t* info) {
  using namespace scaml;
  if (q < 1 || S < 1 || !qa_acqf_valid(acqf)) return -1;
  if (q > QACQF_MAX_Q || S > QACQF_MAX_SAMPLES) return -2;
  std::vector<double> lds(qa_tail_lds_doubles(q, S), std::numeric_limits<double>::quiet_NaN());
  for (int e = 0; e < 64; ++e) lds[QA_SG + e] = ((e >> 3) < q && (e & 7) < q) ? Sigma[(e >> 3) * q + (e & 7)] : 0.0;
  for (int j = 0; j < 8; ++j) lds[QA_MU + j] = j < q ? mu[j] : 0.0;
  qa_tail(lds.data(), q, S, acqf, par, base_samples, 0, 1);
  *value = lds[QA_OUT + QA_OUT_VALUE];
  *jitter = lds[QA_OUT + QA_OUT_JITTER];
  *info = lds[QA_OUT + QA_OUT_INFO] != 0.0 ? 1 : 0;
  for (int j = 0; j < q; ++j) {
    mubar[j] = lds[QA_MB + j];
    for (int k = 0; k < q; ++k) Sigmabar[j * q + k] = lds[QA_SB + j * 8 + k];
  }
  return 0;
}

// All B = Mq / q batches of a call of (7p), its argument list
extern "C" int emul_qacqf(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q, double m_all,
                          double s_all, const int32_t* info, const double* cov_g, const double* mu_g, const double* var_g, const double* Xt,
                          const double* Xq, const double* theta, const double* base_samples, int acqf, double acqf_param, int n, int Mq, int q,
                          int S, int D, int kind, double* value, double* grad, double* jitter_used, int32_t* info_out) {
  using namespace scaml;
  if (n < 1 || q < 1 || S < 1 || D < 1 || Mq < 0 || Mq % q || !qa_acqf_valid(acqf)) return -1;
  if (q > QACQF_MAX_Q || S > QACQF_MAX_SAMPLES || n + q > QACQF_MAX_ROWS || D > QACQF_MAX_D) return -2;
  QAcqfParams p{Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_g, mu_g, var_g, Xt, Xq, theta, base_samples, acqf_param,
                value, grad, jitter_used, info_out, n, Mq, q, S, D, kind, acqf, 0};
  const size_t doubles = qa_lds_doubles(n, q, S);
  std::vector<double> lds(doubles);
  for (int b = 0; b < Mq / q; ++b) {
    lds.assign(doubles, std::numeric_limits<double>::quiet_NaN());
    qa_batch(p, lds.data(), b, 0, 1);
  }
  return 0;
}
