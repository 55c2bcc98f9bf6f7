// TEST INFRASTRUCTURE, not product code: the arithmetic of the batched target acquisition for studies with pending evaluations
// (csrc/gp_studies_acqf.h: sa_fantasy_query and sa_fantasy_strip, the bodies of the two kernels of csrc/gp_studies_fantasy.hip)
// compiled as host code, one query point / one strip after the other with a single emulated thread.  Only
// tests/test_studies_fantasy_emul.py builds and loads it.
#include <limits>
#include <vector>
#include "gp_studies_acqf.h"

extern "C" long long emul_studies_fantasy_lds_doubles(int strips, int n_max, int F_max) {
  return (long long)(strips ? scaml::sa_fantasy_lds_doubles<16>(n_max, F_max) : scaml::sa_fantasy_lds_doubles<1>(n_max, F_max));
}
extern "C" long long emul_studies_fantasy_params_bytes(int fantasy) {
  return (long long)(fantasy ? sizeof(scaml::StudiesFantasyParams) : sizeof(scaml::StudiesAcqfParams));
}

// strips == 0: the 16-column layout of (7g), mu, var (T, Mq, 16), cov (T, n_max, Mq * 16), group (Mq), grad (Mq, D) or NULL;
// strips != 0: the value layout of (7i), mu, var (T, Mq), cov (T, n_max, Mq), group (Mq / 16), no gradient.
// The LDS is filled with NaN before every block: what a block reads of it, it has written.
extern "C" int emul_studies_fantasy(int strips, const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                    const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                    const double* Linv_diag, const double* alpha_f, const int32_t* n_fant, const int32_t* n_points,
                                    const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int Mq, int G,
                                    int n_max, int F_max, int T, int D, int kind, int acqf, double* value, double* grad) {
  using namespace scaml;
  if (n_max < 1 || n_max > STUDIES_ACQF_MAX_N || D < 1 || D > STUDIES_ACQF_MAX_D || F_max < 1 || F_max > STUDIES_FANTASY_MAX_F) return -2;
  if (strips && (Mq & 15)) return -1;
  StudiesFantasyParams p{{mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, nullptr, n_points, m_all, s_all, info, acqf_param,
                          value, strips ? nullptr : grad, nullptr, nullptr, Mq, G, n_max, T, D, kind, acqf, 0},
                         alpha_f, n_fant, F_max, 0};
  const size_t doubles = strips ? sa_fantasy_lds_doubles<16>(n_max, F_max) : sa_fantasy_lds_doubles<1>(n_max, F_max);
  std::vector<double> lds(doubles);
  const int blocks = strips ? Mq / 16 : Mq;
  for (int b = 0; b < blocks; ++b) {
    lds.assign(doubles, std::numeric_limits<double>::quiet_NaN());
    if (strips) sa_fantasy_strip(p, lds.data(), b, 0, 1);
    else sa_fantasy_query(p, lds.data(), b, 0, 1);
  }
  return 0;
}
