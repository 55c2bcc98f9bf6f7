// Kernel-argument block of the source-stack fit's step kernel (csrc/gp_stack_fit.hip), shared by device source and host launcher.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gp_hyper_spec.h"   // HyperSpec

namespace scaml {

constexpr int STACK_FIT_HMAX = 16;   // curvature pairs kept at most
constexpr int STACK_FIT_PMAX = 64;   // one lane per variable: D + 2 <= 64
constexpr int STACK_FIT_SCALARS = 16;

// Per-problem optimiser state in the caller's workspace, in doubles (P = D + 2, H = history):
//   x[P] accepted point (raw)   g[P] gradient there   d[P] search direction   xt[P] trial point (raw)
//   S[H][P], Y[H][P] curvature pairs (ring: the newest in slot head - 1)   rho[H]
//   sc[16]: f, step t, g.d, iteration, evaluations, status, failed trials of this line search, pairs held, head, phase
constexpr size_t stack_fit_state_doubles(int P, int H) { return (size_t)(4 + 2 * H) * P + H + STACK_FIT_SCALARS; }
enum { SF_F = 0, SF_T = 1, SF_GD = 2, SF_IT = 3, SF_NEVAL = 4, SF_STATUS = 5, SF_LS = 6, SF_HIST = 7, SF_HEAD = 8, SF_PHASE = 9 };

struct StackFitParams {
  const double* mll;         // (B)  marginal log-likelihood / n of the fit at `theta`
  const int32_t* info;       // (B)  status of that fit (anything but 0: the evaluation failed)
  const double* partials;    // (B, tiles, D+2) of scaml_mll_backward_f64
  const int32_t* n_points;   // (B) or NULL
  HyperSpec spec;
  double* z;                 // (B, D+2) raw: start points in (mode 0), accepted points out
  double* theta;             // (B, D+2) constrained: the point the next fit launch evaluates
  double* value;             // (B)  mll + prior term at the accepted point
  int32_t* stats;            // (B, 4) iterations, evaluations, status, 0
  double* state;             // (B, stack_fit_state_doubles(D + 2, history))
  int B, N, D, tiles;
  int mode;                  // 0: take z as the start point, reset the state; 1: consume one evaluation
  int max_iter, history, max_ls;
  double gtol, ftol, c1;
};

}  // namespace scaml
