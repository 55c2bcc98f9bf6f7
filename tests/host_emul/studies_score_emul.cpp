// TEST INFRASTRUCTURE, not product code: the arithmetic of the strip scoring kernel (csrc/gp_studies_score.h: sa_score_strip, the body
// of scaml_target_score_batched_kernel) and of the batched target acquisition (csrc/gp_studies_acqf.h: sa_query) compiled as host code
// side by side, one strip / one query point after the other with a single emulated thread.  Only tests/test_studies_score_emul.py
// builds and loads it.
#include <vector>
#include "gp_studies_score.h"

extern "C" long long emul_studies_score_lds_doubles(int n_max) { return (long long)scaml::studies_score_lds_doubles(n_max); }

// the value layout: mu, var (T, Mq), cov (T, n_max, Mq), group (Mq / 16)
extern "C" int emul_studies_score(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq, const double* w,
                                  const uint8_t* active, const double* Xt, const double* theta, const double* L, const double* Linv_diag,
                                  const double* alpha, const int32_t* n_points, const double* m_all, const double* s_all, const int32_t* info,
                                  const double* acqf_param, int Mq, int G, int n_max, int T, int D, int kind, int acqf, double* value,
                                  double* mu_out, double* var_out) {
  using namespace scaml;
  if (n_max < 1 || n_max > STUDIES_ACQF_MAX_N || D < 1 || D > STUDIES_ACQF_MAX_D || Mq < 0 || (Mq & 15)) return -2;
  StudiesScoreParams p{mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info, acqf_param,
                       value, nullptr, mu_out, var_out, Mq, G, n_max, T, D, kind, acqf, 0};
  std::vector<double> lds(studies_score_lds_doubles(n_max));
  for (int s = 0; s < Mq / 16; ++s) sa_score_strip(p, lds.data(), s, 0, 1);
  return 0;
}

// the 16-column layout of (7g): mu, var (T, Mq, 16), cov (T, n_max, Mq * 16), group (Mq) -- no gradient asked for
extern "C" int emul_studies_acqf_value(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                       const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                       const double* Linv_diag, const double* alpha, const int32_t* n_points, const double* m_all,
                                       const double* s_all, const int32_t* info, const double* acqf_param, int Mq, int G, int n_max, int T,
                                       int D, int kind, int acqf, double* value, double* mu_out, double* var_out) {
  using namespace scaml;
  if (n_max < 1 || n_max > STUDIES_ACQF_MAX_N || D < 1 || D > STUDIES_ACQF_MAX_D) return -2;
  StudiesAcqfParams p{mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info, acqf_param,
                      value, nullptr, mu_out, var_out, Mq, G, n_max, T, D, kind, acqf, 0};
  std::vector<double> lds(studies_acqf_lds_doubles(n_max));
  for (int q = 0; q < Mq; ++q) sa_query(p, lds.data(), q, 0, 1);
  return 0;
}
