// TEST INFRASTRUCTURE, not product code: the scalar acquisition formulas of csrc/gp_studies_formulas.h (sa_log_ei_core, sa_acquisition
// and the test of an acquisition code the host launcher applies) compiled as host code, elementwise over arrays.  Only
// tests/test_logei_bounds.py builds and loads it.
#include "gp_studies_formulas.h"

extern "C" void emul_log_ei_core(const double* u, int M, double* g, double* gp, double* om) {
  for (int i = 0; i < M; ++i) {
    const scaml::SaLogEi r = scaml::sa_log_ei_terms(u[i]);
    g[i] = r.g, gp[i] = r.gp, om[i] = r.om;
  }
}
// the three-output form: g and g' only
extern "C" void emul_log_ei_core3(const double* u, int M, double* g, double* gp) {
  for (int i = 0; i < M; ++i) scaml::sa_log_ei_core(u[i], g[i], gp[i]);
}
extern "C" void emul_acquisition(int acqf, double par, const double* mu, const double* var, int M, double* A, double* Amu, double* Av) {
  for (int i = 0; i < M; ++i) scaml::sa_acquisition(acqf, par, mu[i], var[i], A[i], Amu[i], Av[i]);
}
extern "C" int emul_acqf_valid(int acqf) { return scaml::sa_acqf_valid(acqf) ? 1 : 0; }
