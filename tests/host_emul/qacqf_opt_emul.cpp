// TEST INFRASTRUCTURE, not product code: csrc/gp_qacqf_opt.h compiled as single-threaded host code (one "lane" loops over all
// P variables, a lane broadcast is the identity), so that the per-start state machine of the device-side optimiser of the joint
// acquisition, its slot table and its gather can be driven against hyper.batched_lbfgs(bounds=...) and torch.cat on a machine without
// a GPU.  Never linked into libscaml_hip.so; only tests/test_qacqf_opt_emul.py and tests/test_qacqf_opt_step_gpu.py build and load it.
#define SCAML_HOST_EMUL 1
#include <math.h>
#include <string.h>

#include "gp_qacqf_opt.h"

extern "C" {

long long emul_qacqf_opt_state_doubles(int P, int H) { return (long long)scaml::qacqf_opt_state_doubles(P, H); }
int emul_qacqf_opt_max_p(void) { return scaml::QACQF_OPT_MAX_P; }

// One launch of scaml_qacqf_opt_step_kernel over Bs slots: mode 0 resets from x0, mode 1 consumes (value, grad) -- the MAXIMISED
// function's, as the device kernel is handed them.  slots NULL: the identity.
void emul_qacqf_opt_step(const double* value, const double* grad, const int32_t* slots, const double* x0, const double* lo, const double* hi,
                         double* state, double* Xq, double* x, double* f, int32_t* stats, int B, int Bs, int P, int mode, int max_iter,
                         int history, int max_ls, double gtol, double ftol, double c1) {
  scaml::QAcqfOptParams p{value, grad, slots, x0, lo, hi, state, Xq, x, f, stats, B, Bs, P, mode, max_iter, history, max_ls, 0, gtol, ftol, c1};
  for (int s = 0; s < Bs; ++s) scaml::qo_step(p, s, 0);
}

// The round loop of scaml_qacqf_opt_f64: a reset launch -- with the continue flag (1) a launch in mode 2 --, then n_evals rounds of
// { evaluation: `eval` fills value / grad from Xq, one step launch }.
typedef void (*emul_eval_fn)(void);
void emul_qacqf_opt_call(double* value, double* grad, const int32_t* slots, const double* x0, const double* lo, const double* hi, double* state,
                         double* Xq, double* x, double* f, int32_t* stats, int B, int Bs, int P, int max_iter, int history, int max_ls,
                         double gtol, double ftol, double c1, int n_evals, unsigned flags, emul_eval_fn eval) {
  // (a continued call: the trial points again, in the order of a slot table that may have changed)
  emul_qacqf_opt_step(value, grad, slots, x0, lo, hi, state, Xq, x, f, stats, B, Bs, P, (flags & 1u) ? 2 : 0, max_iter, history, max_ls, gtol, ftol, c1);
  for (int r = 0; r < n_evals; ++r) {
    eval();
    emul_qacqf_opt_step(value, grad, slots, x0, lo, hi, state, Xq, x, f, stats, B, Bs, P, 1, max_iter, history, max_ls, gtol, ftol, c1);
  }
}

// One launch of scaml_qacqf_opt_gather_kernel
void emul_qacqf_opt_gather(const double* mu_g, const double* var_g, const double* cov_g, const double* Xq, const double* mu_t, const double* var_t,
                           const double* cov_tt, const double* Xt, double* mean_s, double* var_s, double* cov_s, double* xall, int n, int Mq,
                           int D, int left) {
  scaml::QAcqfOptGatherParams p{mu_g, var_g, cov_g, Xq, mu_t, var_t, cov_tt, Xt, mean_s, var_s, cov_s, xall, n, Mq, D, left};
  const long long elems = scaml::qo_gather_elems(p);
  for (long long e = 0; e < elems; ++e) scaml::qo_gather_elem(p, e);
}

}  // extern "C"
