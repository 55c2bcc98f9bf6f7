// gp_acqf_opt.h -- the optimiser step of the device-side acquisition optimiser (scaml_studies_acqf_opt_f64, include/scaml_gp.h (7h)):
// argument block, state stride and the per-start advance function.  One source for the device kernel (csrc/gp_acqf_opt.hip: one wave
// per start point, one lane per coordinate), the host launcher and the single-threaded host build the CPU tests drive against
// hyper.batched_lbfgs(bounds=...) (any compiler but hipcc: tests/host_emul).
//
// ao_advance is hyper._batched_lbfgs_box for ONE start as a state machine that consumes one evaluation per call: the box instance of
// csrc/gp_lbfgs_core.h (projection onto the box, held coordinates, two-loop recursion, projected steepest descent where there is no pair
// or no descent, projected trial points, Armijo on g . (trial - x) with halving, curvature pair kept when s . y > 0, scipy L-BFGS-B's
// stopping rules).  The state lives in the caller's workspace; no LDS; a lane reads back only what it wrote in this launch or what an
// earlier launch left.
//
// Rounding: every dot product accumulates coordinate by coordinate in ascending order (hyper._rowdot; on the device one lane
// broadcast per coordinate, no butterfly) and no product is contracted into the sum that follows it, so that, fed the same (f, g),
// the iterates are those of the host optimiser bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

// a * b + c stays two roundings in the arithmetic below (the device source and the host emulation include this header last; the
// launcher takes only the argument block and compiles as it always did)
#if defined(__HIPCC__) || defined(SCAML_HOST_EMUL)
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#endif
// (after the pragma, which is lexical: the core sets none of its own and its a * b + c must stay uncontracted in this instance)
#include "gp_lbfgs_core.h"

namespace scaml {

constexpr int ACQF_OPT_MAX_D = 15;     // one lane per coordinate; the limit of (5e) / (7g)
constexpr int ACQF_OPT_HMAX = LBFGS_HMAX;
constexpr int ACQF_OPT_SCALARS = LBFGS_SCALARS;
constexpr int AO_NV = LBFGS_LANES > 1 ? 1 : 16;   // a lane's coordinates: one on the device, all of them in the host build
// per-start optimiser state in the caller's workspace, in doubles: the layout of csrc/gp_lbfgs_core.h with P = D
constexpr size_t acqf_opt_state_doubles(int D, int H) { return lbfgs_state_doubles(D, H); }

struct AcqfOptParams {
  const double* value;     // (B)     acquisition value of (7g) at Xq (maximised: negated on the way in)
  const double* grad;      // (B, D)  its input gradient
  const int32_t* group;    // (B)     the caller's: study of a start; negative (or >= G): a padding row
  const double* x0;        // (B, D)  start points (mode 0)
  const double* lo;        // (D)
  const double* hi;        // (D)
  double* state;           // (B, acqf_opt_state_doubles(D, history))
  double* Xq;              // (B, D)  out: the point the next round evaluates
  int32_t* group_live;     // (B)     out: group[b] while the start is running, -1 once it has stopped
  double* x;               // (B, D)  out: accepted point
  double* f;               // (B)     out: the acquisition value there
  int32_t* stats;          // (B, 4)  out: iterations, evaluations, status, pairs held
  int B, G, D;
  int mode;                // 0: project x0 onto the box, reset the state; 1: consume one evaluation
  int max_iter, history, max_ls, pad_;
  double gtol, ftol, c1;
};

// lane j's value in every lane
LBFGS_DEV double ao_bcast(double v, int j) {
#if LBFGS_LANES > 1
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
#else
  (void)j;
  return v;
#endif
}
// sum / maximum of the coordinates' terms, coordinate 0 first, the same bits in every lane
LBFGS_DEV double ao_sum(const double* term, int D) {
#if LBFGS_LANES > 1
  double acc = ao_bcast(term[0], 0);
  for (int j = 1; j < D; ++j) acc = acc + ao_bcast(term[0], j);
#else
  double acc = term[0];
  for (int j = 1; j < D; ++j) acc = acc + term[j];
#endif
  return acc;
}
LBFGS_DEV double ao_max(const double* term, int D) {
#if LBFGS_LANES > 1
  double acc = ao_bcast(term[0], 0);
  for (int j = 1; j < D; ++j) acc = fmax(acc, ao_bcast(term[0], j));
#else
  double acc = term[0];
  for (int j = 1; j < D; ++j) acc = fmax(acc, term[j]);
#endif
  return acc;
}

struct AoReduce {
  static constexpr int NV = AO_NV;
  static LBFGS_INLINE double sum(const double* term, int D) { return ao_sum(term, D); }
  static LBFGS_INLINE double max(const double* term, int D) { return ao_max(term, D); }
};
using AoResult = LbfgsResult;

// Start of an optimisation: the projected start is the accepted point and the first trial; nothing has been evaluated.
LBFGS_DEV AoResult ao_reset(double* st, const double* x0, const double* lo, const double* hi, int D, int H, bool padding, int lane) {
  return lbfgs_reset<true>(st, x0, lo, hi, D, H, padding, lane);
}

// One evaluation (ft, gt) of the MINIMISED function at the trial point st.xt arrives: hyper._batched_lbfgs_box for this start alone.
// Leaves the next point to evaluate in st.xt -- the accepted point once the start has stopped (status != 0).
LBFGS_DEV AoResult ao_advance(double* st, const double* lo, const double* hi, int D, int H, int max_iter, int max_ls, double gtol, double ftol,
                              double c1, int lane, double ft, const double* gt) {
  return lbfgs_advance<true, AoReduce>(st, lo, hi, D, H, max_iter, max_ls, gtol, ftol, c1, lane, ft, gt);
}

// The whole step of start `b`: reset or consume (value, grad) of the round's evaluation, then hand the next trial point and the
// start's live group to the evaluation kernels and the accepted point, its value and the counters to the caller.
LBFGS_DEV void ao_step(const AcqfOptParams& p, int b, int lane) {
  const int D = p.D, H = p.history;
  if (b >= p.B) return;
  double* st = p.state + (size_t)b * acqf_opt_state_doubles(D, H);
  const double *x = st, *xt = st + 3 * (size_t)D;
  const int grp = p.group[b];
  const bool padding = grp < 0 || grp >= p.G;
  AoResult r;
  if (p.mode == 0) {
    r = ao_reset(st, p.x0 + (size_t)b * D, p.lo, p.hi, D, H, padding, lane);
  } else {
    double gt[AO_NV] = {0.0};
    LBFGS_FOR(i, D) gt[LBFGS_AT(i)] = -p.grad[(size_t)b * D + i];
    r = ao_advance(st, p.lo, p.hi, D, H, p.max_iter, p.max_ls, p.gtol, p.ftol, p.c1, lane, -p.value[b], gt);
  }
  LBFGS_FOR(i, D) {
    p.Xq[(size_t)b * D + i] = xt[i];
    p.x[(size_t)b * D + i] = x[i];
  }
  if (lane == 0) {
    p.group_live[b] = r.status == LBFGS_RUNNING ? grp : -1;
    p.f[b] = r.status == LBFGS_PADDING ? 0.0 : -r.f;
    p.stats[4 * b + 0] = r.it;
    p.stats[4 * b + 1] = r.n_eval;
    p.stats[4 * b + 2] = r.status;
    p.stats[4 * b + 3] = r.hist;
  }
}

}  // namespace scaml
