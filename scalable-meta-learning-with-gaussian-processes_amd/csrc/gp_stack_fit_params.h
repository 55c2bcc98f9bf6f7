// Kernel-argument block of the source-stack fit's step kernel (csrc/gp_stack_fit.hip), shared by device source and host launcher.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gp_hyper_spec.h"   // HyperSpec
#include "gp_lbfgs_core.h"   // state layout and machine; taken with no contraction pragma set (csrc/gp_stack_fit.hip)

namespace scaml {

constexpr int STACK_FIT_HMAX = LBFGS_HMAX;
constexpr int STACK_FIT_PMAX = 64;   // one lane per variable: D + 2 <= 64
constexpr int STACK_FIT_SCALARS = LBFGS_SCALARS;
// per-problem optimiser state in the caller's workspace, in doubles (P = D + 2 raw variables): the layout of csrc/gp_lbfgs_core.h
constexpr size_t stack_fit_state_doubles(int P, int H) { return lbfgs_state_doubles(P, H); }

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
