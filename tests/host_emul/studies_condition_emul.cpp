// TEST INFRASTRUCTURE, not product code: the arithmetic of the studies' batched fantasy set-up (csrc/gp_studies_condition.h:
// sc_condition_block and sc_fantasy_condition, the bodies of the two kernels of csrc/gp_studies_condition.hip) compiled as host code, one
// study after the other with a single emulated thread.  tests/test_studies_condition_emul.py and tests/_condition_bounds.py build and
// load it.
#include <limits>
#include <vector>
#include "gp_studies_condition.h"
#include "gp_dispatch.h"   // the two launch plans

extern "C" long long emul_condition_block_lds_doubles(int n_max, int D) { return (long long)scaml::sc_block_lds_doubles(n_max, D); }
extern "C" long long emul_fantasy_condition_lds_doubles(int n_max, int F_max) { return (long long)scaml::sc_fantasy_lds_doubles(n_max, F_max); }

// which == 0: studies_condition_block_plan(G, n_max, D = third), else studies_fantasy_condition_plan(G, n_max, F_max = third) -> grid, block, LDS doubles
extern "C" void emul_condition_plan(int which, int G, int n_max, int third, long long* out) {
  const scaml::StudiesConditionPlan p = which == 0 ? scaml::studies_condition_block_plan(G, n_max, third) : scaml::studies_fantasy_condition_plan(G, n_max, third);
  out[0] = p.grid, out[1] = p.block, out[2] = (long long)p.lds_doubles;
}

// The LDS is filled with NaN before every study: what a study reads of it, it has written.
extern "C" int emul_studies_condition_block(const double* mu, const double* cov, const int32_t* strip_base, const double* w, const uint8_t* active,
                                            const double* Xt, const double* theta, const double* y, const int32_t* n_points, const int32_t* n_obs,
                                            const double* m_all, const double* s_all, int Mq, int G, int n_max, int T, int D, int kind, double* Knn,
                                            double* resid, double* mean_p) {
  using namespace scaml;
  if (n_max < 1 || n_max > STUDIES_ACQF_MAX_N || D < 1 || D > STUDIES_ACQF_MAX_D) return -2;
  if (Mq & 15) return -1;
  StudiesConditionBlockParams p{mu, cov, strip_base, w, active, Xt, theta, y, n_points, n_obs, m_all, s_all, Knn, resid, mean_p, Mq, G, n_max, T, D, kind};
  const size_t doubles = sc_block_lds_doubles(n_max, D);
  std::vector<double> lds(doubles);
  for (int g = 0; g < G; ++g) {
    lds.assign(doubles, std::numeric_limits<double>::quiet_NaN());
    sc_condition_block(p, lds.data(), g, 0, 1);
  }
  return 0;
}

extern "C" int emul_studies_fantasy_condition(const double* L, const double* resid, const double* mean_p, const int32_t* n_points,
                                              const int32_t* n_obs, const int32_t* info, const double* eps, const int32_t* n_fant,
                                              const double* m_all, const double* s_all, int G, int n_max, int p_max, int F_max, double* alpha_f,
                                              double* y_fant, double* mu_p) {
  using namespace scaml;
  if (n_max < 1 || n_max > STUDIES_ACQF_MAX_N || p_max < 1 || F_max < 1 || F_max > STUDIES_FANTASY_MAX_F) return -2;
  StudiesFantasyConditionParams p{L, resid, mean_p, n_points, n_obs, info, eps, n_fant, m_all, s_all, alpha_f, y_fant, mu_p, G, n_max, p_max, F_max};
  const size_t doubles = sc_fantasy_lds_doubles(n_max, F_max);
  std::vector<double> lds(doubles);
  for (int g = 0; g < G; ++g) {
    lds.assign(doubles, std::numeric_limits<double>::quiet_NaN());
    sc_fantasy_condition(p, lds.data(), g, 0, 1);
  }
  return 0;
}
