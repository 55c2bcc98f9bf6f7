// Host build of the rule that sends a fused fit to its full-tile instance (fit_full_instance, csrc/gp_dispatch.h) for
// tests/_fit_full.py: the header is plain C++, so the answer a test asks for is computed by the very function
// csrc/scaml_host.cpp launches from.  Test infrastructure, never part of the library.
#define __device__   // (csrc/gp_posterior_params.h marks one member function for the device)
#include "gp_dispatch.h"

extern "C" {

// the rule itself, on the instance <nb, wu> a plan names
int emul_fit_full_instance(int nb, int wu, int N, int ragged, int from_matrix, int blocked, int stores_l, unsigned long long l_addr, int mode) {
  return scaml::fit_full_instance(nb, wu, N, ragged != 0, from_matrix != 0, blocked != 0, stores_l != 0, (size_t)l_addr, mode) ? 1 : 0;
}

// ... as fit_common asks it: on the instance of fit_plan(T, N, D, cus)
int emul_fit_full_of_call(int T, int N, int D, int cus, int ragged, int from_matrix, int blocked, int stores_l, unsigned long long l_addr, int mode) {
  const scaml::FitPlan p = scaml::fit_plan(T, N, D, cus);
  return scaml::fit_full_instance(p.nb, p.wu, N, ragged != 0, from_matrix != 0, blocked != 0, stores_l != 0, (size_t)l_addr, mode) ? 1 : 0;
}

}  // extern "C"
