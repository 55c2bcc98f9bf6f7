// TEST INFRASTRUCTURE, not product code: csrc/gp_stack_fit.hip compiled as single-threaded host code (SCAML_HOST_EMUL: one "lane"
// loops over all variables, wave reductions are the identity), so that the arithmetic of the source-stack objective and the
// per-problem L-BFGS state machine can be checked on a machine without a GPU.  Never linked into libscaml_hip.so; only
// tests/test_stack_fit_emul.py builds and loads it.
#define SCAML_HOST_EMUL 1
#include <math.h>
#include <string.h>

#include "gp_stack_fit.hip"

extern "C" {

long long emul_stack_fit_state_doubles(int P, int H) { return (long long)scaml::stack_fit_state_doubles(P, H); }

// sf_objective for B problems: partials (B, tiles, D+2), theta / raw (B, D+2), n (B) -> f (B), g (B, D+2)
void emul_stack_objective(const double* spec15, const double* mll, const int32_t* info, const double* partials, int tiles,
                          const double* theta, const double* raw, const int32_t* n, int B, int D, double* f, double* g) {
  scaml::HyperSpec sp{};
  if (!scaml::hyper_spec_from_host(spec15, sp)) {   // a bad fixture fails loudly
    for (int b = 0; b < B; ++b) f[b] = NAN;
    return;
  }
  const int P = D + 2;
  for (int b = 0; b < B; ++b) {
    double gl[scaml::SF_NV];
    f[b] = scaml::sf_objective(sp, mll[b], info[b], partials + (size_t)b * tiles * P, tiles, theta + (size_t)b * P, raw + (size_t)b * P,
                               n[b], D, 0, gl);
    for (int i = 0; i < P; ++i) g[(size_t)b * P + i] = gl[i];
  }
}

// state (B, state_doubles): start every problem at z (B, P); xt_out (B, P) = the points to evaluate first
void emul_stack_reset(double* state, const double* z, int B, int P, int H, double* xt_out) {
  const size_t stride = scaml::stack_fit_state_doubles(P, H);
  for (int b = 0; b < B; ++b) {
    scaml::sf_reset(state + b * stride, z + (size_t)b * P, P, H, 0);
    memcpy(xt_out + (size_t)b * P, state + b * stride + 3 * (size_t)P, sizeof(double) * P);
  }
}

// one round of sf_advance: (f, g) evaluated at the trial points -> next trial points, accepted points, objective, stats (B, 3)
void emul_stack_advance(double* state, const double* f, const double* g, int B, int P, int H, int max_iter, int max_ls, double gtol,
                        double ftol, double c1, double* xt_out, double* x_out, double* f_out, int32_t* stats) {
  const size_t stride = scaml::stack_fit_state_doubles(P, H);
  for (int b = 0; b < B; ++b) {
    double gl[scaml::SF_NV];
    for (int i = 0; i < P; ++i) gl[i] = g[(size_t)b * P + i];
    double* st = state + b * stride;
    const scaml::SfResult r = scaml::sf_advance(st, P, H, max_iter, max_ls, gtol, ftol, c1, 0, f[b], gl);
    memcpy(xt_out + (size_t)b * P, st + 3 * (size_t)P, sizeof(double) * P);
    memcpy(x_out + (size_t)b * P, st, sizeof(double) * P);
    f_out[b] = r.f;
    stats[3 * b + 0] = r.it; stats[3 * b + 1] = r.n_eval; stats[3 * b + 2] = r.status;
  }
}

}  // extern "C"
