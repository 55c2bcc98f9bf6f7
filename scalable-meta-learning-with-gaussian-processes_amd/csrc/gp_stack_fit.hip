// gp_stack_fit.hip — the optimiser step of the source-stack hyper-parameter fit (scaml_stack_fit_f64, include/scaml_gp.h).
//
// scamlgp/utils.py:139-212 trains every source GP by L-BFGS on its marginal likelihood + hyper-priors.  The host enqueues, per
// evaluation, the fused fit at the trial hyper-parameters, the MLL gradient kernel and ONE launch of the kernel below, which turns
// the outputs of that evaluation into the next trial point of ALL B = tasks x starts problems: one wave per problem, one lane per
// variable (P = D + 2 <= 64), dot products by wave reductions, the optimiser state in the caller's workspace.  No LDS, no
// hand-off between workgroups: the stream orders the rounds.
//
//   sf_objective   f = -(mll + sum log p(theta) / n) and df / d raw from the fit's mll / info, the gradient kernel's per-tile
//                  partial sums (added up here in a fixed order), the sigmoid-Interval chain rule and the prior derivatives
//                  (the arithmetic of SourceGPStack.objective / hyper.HyperSpec)
//   sf_advance     hyper.batched_lbfgs as a per-problem state machine, one evaluation per call: the unconstrained instance of
//                  csrc/gp_lbfgs_core.h (Armijo test of the trial with halving, curvature pair, stopping rules, two-loop
//                  recursion, steepest-descent fallback) with the wave butterfly as its reduction
//
// SCAML_HOST_EMUL: the same source compiles as single-threaded host code (tests/host_emul: checked against the oracle and
// hyper.batched_lbfgs on CPU; never part of libscaml_hip.so).  A "lane" then loops over all variables and a wave reduction is
// the identity.
#ifndef SCAML_HOST_EMUL
#include <hip/hip_runtime.h>
#endif
// (brings csrc/gp_lbfgs_core.h with no contraction pragma set: this file is compiled with hipcc's default contraction, and the
// core's a * b + c contract here as they always did)
#include "gp_stack_fit_params.h"

namespace scaml {

// a lane's variables: i = lane, lane + LBFGS_LANES, ... < P; their per-lane values live in arrays of SF_NV entries (one register
// on the device, all P of them in the host build)
constexpr int SF_NV = STACK_FIT_PMAX / LBFGS_LANES;

// sum / maximum over the wave, the same bits in every lane (butterfly: both partners add the same two numbers)
LBFGS_DEV double sf_sum(double x) {
#ifndef SCAML_HOST_EMUL
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
#endif
  return x;
}
LBFGS_DEV double sf_max(double x) {
#ifndef SCAML_HOST_EMUL
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off));
#endif
  return x;
}
// the core's reduction: the lane's terms folded into zero in ascending order (device: its one term, as `acc = 0; acc += a * b`
// always was; host build: all P), then the butterfly
struct SfReduce {
  static constexpr int NV = SF_NV;
  static LBFGS_INLINE double sum(const double* term, int P) {
    double acc = 0.0;
    for (int i = 0; i < P && i < NV; ++i) acc += term[i];
    return sf_sum(acc);
  }
  static LBFGS_INLINE double max(const double* term, int P) {
    double acc = 0.0;
    for (int i = 0; i < P && i < NV; ++i) acc = fmax(acc, term[i]);
    return sf_max(acc);
  }
};

// sum over the tile axis of part (tiles, P), variable by variable.  Device: the wave's 64 lanes are 64 / PP streams of PP >= P
// lanes (PP a power of two); stream j adds tiles j, j + 64 / PP, ... and the streams are folded by a butterfly -- a fixed order.
LBFGS_DEV void sf_tile_sums(const double* part, int tiles, int P, int lane, double* ts) {
#ifndef SCAML_HOST_EMUL
  int PP = 1;
  while (PP < P) PP <<= 1;
  const int i = lane & (PP - 1), j = lane / PP, ns = LBFGS_LANES / PP;
  double s = 0.0;
  if (i < P) {
    for (int t = j; t < tiles; t += ns) s += part[(size_t)t * P + i];
  }
  for (int off = PP; off < LBFGS_LANES; off <<= 1) s += __shfl_xor(s, off);
  ts[0] = s;
#else
  LBFGS_FOR(i, P) {
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += part[(size_t)t * P + i];
    ts[LBFGS_AT(i)] = s;
  }
#endif
}

// Objective of one problem at the point (theta, raw) the fit was run at; returns f, the lane's components of df / d raw in g.
// A fit that did not succeed (info != 0) has no value: f is NaN and the gradient zero.
LBFGS_DEV double sf_objective(const HyperSpec& sp, double mll, int info, const double* part, int tiles, const double* theta,
                              const double* raw, int n, int D, int lane, double* g) {
  const int P = D + 2;
  const double nf = n < 1 ? 1.0 : (double)n;
  double ts[SF_NV];
  sf_tile_sums(part, tiles, P, lane, ts);
  double lp = 0.0;
  LBFGS_FOR(i, P) {
    const HyperVar v = hyper_var(sp, i, D);
    const double th = theta[i], s = interval_sigmoid(raw[i]);
    lp += prior_logp(v.prior, th);
    const double dmll = ts[LBFGS_AT(i)] / (2.0 * nf);
    g[LBFGS_AT(i)] = -(dmll + prior_dlogp(v.prior, th) / nf) * interval_slope(v, s);
  }
  lp = sf_sum(lp);
  if (info != 0) {
    LBFGS_FOR(i, P) g[LBFGS_AT(i)] = 0.0;
    return NAN;
  }
  return -(mll + lp / nf);
}

using SfResult = LbfgsResult;

// Start of a fit: the caller's point is the accepted point and the first trial; nothing has been evaluated.
LBFGS_DEV SfResult sf_reset(double* st, const double* z, int P, int H, int lane) {
  return lbfgs_reset<false>(st, z, nullptr, nullptr, P, H, false, lane);
}

// One evaluation (ft, gt) at the trial point st.xt arrives: hyper.batched_lbfgs for this problem alone.  Leaves the next point to
// evaluate in st.xt -- the accepted point once the problem has finished (status != 0).
LBFGS_DEV SfResult sf_advance(double* st, int P, int H, int max_iter, int max_ls, double gtol, double ftol, double c1, int lane, double ft,
                              const double* gt) {
  return lbfgs_advance<false, SfReduce>(st, nullptr, nullptr, P, H, max_iter, max_ls, gtol, ftol, c1, lane, ft, gt);
}

// The whole step of problem `b`.  (A lane reads back only what it wrote itself in this launch -- its components of x, xt -- or what
// an earlier launch left in the state.)
LBFGS_DEV void sf_step(const StackFitParams& p, int b, int lane) {
  const int P = p.D + 2, H = p.history;
  double* st = p.state + (size_t)b * stack_fit_state_doubles(P, H);
  double* z = p.z + (size_t)b * P;
  double* theta = p.theta + (size_t)b * P;
  const double *x = st, *xt = st + 3 * (size_t)P;
  SfResult r;
  if (p.mode == 0) {
    r = sf_reset(st, z, P, H, lane);
  } else {
    double gt[SF_NV];
    const int n = p.n_points ? p.n_points[b] : p.N;
    const double ft = sf_objective(p.spec, p.mll[b], p.info[b], p.partials + (size_t)b * p.tiles * P, p.tiles, theta, xt, n, p.D, lane, gt);
    r = sf_advance(st, P, H, p.max_iter, p.max_ls, p.gtol, p.ftol, p.c1, lane, ft, gt);
  }
  LBFGS_FOR(i, P) {
    // (spelled out, not hyper_var(p.spec, ...): through a reference to p.spec the compiler orders this loop differently)
    const double lo = i < p.D ? p.spec.ls_lo : (i == p.D ? p.spec.os_lo : p.spec.nz_lo);
    const double hi = i < p.D ? p.spec.ls_hi : (i == p.D ? p.spec.os_hi : p.spec.nz_hi);
    theta[i] = lo + (hi - lo) * interval_sigmoid(xt[i]);
    z[i] = x[i];
  }
  if (lane == 0) {
    p.value[b] = -r.f;
    p.stats[4 * b + 0] = r.it;
    p.stats[4 * b + 1] = r.n_eval;
    p.stats[4 * b + 2] = r.status;
    p.stats[4 * b + 3] = 0;
  }
}

#ifndef SCAML_HOST_EMUL
extern "C" __global__ __launch_bounds__(64) void scaml_stack_fit_step_kernel(StackFitParams p) {
  sf_step(p, (int)blockIdx.x, (int)threadIdx.x);
}
#endif

}  // namespace scaml
