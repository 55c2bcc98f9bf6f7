// TEST INFRASTRUCTURE, not product code: csrc/gp_acqf_opt.h compiled as single-threaded host code (one "lane" loops over all
// coordinates, a lane broadcast is the identity), so that the per-start state machine of the device-side acquisition optimiser can be
// driven against hyper.batched_lbfgs(bounds=...) on a machine without a GPU.  Never linked into libscaml_hip.so; only
// tests/test_acqf_opt_emul.py builds and loads it.
#define SCAML_HOST_EMUL 1
#include <math.h>
#include <string.h>

#include "gp_acqf_opt.h"

extern "C" {

long long emul_acqf_opt_state_doubles(int D, int H) { return (long long)scaml::acqf_opt_state_doubles(D, H); }
int emul_acqf_opt_max_d(void) { return scaml::ACQF_OPT_MAX_D; }

// One launch of scaml_acqf_opt_step_kernel over B starts: mode 0 resets from x0, mode 1 consumes (value, grad) -- the MAXIMISED
// function's, as the device kernel is handed them.
void emul_acqf_opt_step(const double* value, const double* grad, const int32_t* group, const double* x0, const double* lo, const double* hi,
                        double* state, double* Xq, int32_t* group_live, double* x, double* f, int32_t* stats, int B, int G, int D, int mode,
                        int max_iter, int history, int max_ls, double gtol, double ftol, double c1) {
  scaml::AcqfOptParams p{value, grad, group, x0, lo, hi, state, Xq, group_live, x, f, stats, B, G, D, mode, max_iter, history, max_ls, 0,
                         gtol, ftol, c1};
  for (int b = 0; b < B; ++b) scaml::ao_step(p, b, 0);
}

// The round loop of scaml_studies_acqf_opt_f64: without the continue flag (1) a reset launch, then n_evals rounds of
// { evaluation: `eval` fills value / grad from Xq and group_live, one step launch }.
typedef void (*emul_eval_fn)(void);
void emul_acqf_opt_call(double* value, double* grad, const int32_t* group, const double* x0, const double* lo, const double* hi, double* state,
                        double* Xq, int32_t* group_live, double* x, double* f, int32_t* stats, int B, int G, int D, int max_iter, int history,
                        int max_ls, double gtol, double ftol, double c1, int n_evals, unsigned flags, emul_eval_fn eval) {
  if (!(flags & 1u))
    emul_acqf_opt_step(value, grad, group, x0, lo, hi, state, Xq, group_live, x, f, stats, B, G, D, 0, max_iter, history, max_ls, gtol, ftol, c1);
  for (int r = 0; r < n_evals; ++r) {
    eval();
    emul_acqf_opt_step(value, grad, group, x0, lo, hi, state, Xq, group_live, x, f, stats, B, G, D, 1, max_iter, history, max_ls, gtol, ftol, c1);
  }
}

}  // extern "C"
