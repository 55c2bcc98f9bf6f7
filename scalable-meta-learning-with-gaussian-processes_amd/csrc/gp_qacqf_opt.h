// gp_qacqf_opt.h -- the optimiser step of the device-side optimiser of the JOINT q-point acquisition (scaml_qacqf_opt_f64,
// include/scaml_gp.h (7s); the step alone: scaml_qacqf_opt_step_f64, (7t)): argument blocks, state stride, the per-start advance
// function and the gather that stands where ScaMLGP.joint_acqf_inputs concatenates.  One source for the device kernels
// (csrc/gp_qacqf_opt.hip: one wave per slot, two variables per lane), the host launcher and the single-threaded host build the CPU
// tests drive against hyper.batched_lbfgs(bounds=...) (any compiler but hipcc: tests/host_emul).
//
// A start is one batch of q points, P = q * D <= 128 variables.  qo_step is csrc/gp_acqf_opt.h's ao_step for P variables with a SLOT
// TABLE: slot s of a launch works on start slots[s] (NULL: the identity), reads the evaluation of row s and leaves the next trial
// point in row s, so that the evaluation kernels in front of it see only the starts the caller still lists.  The state, the accepted
// point, its value and the counters stay addressed by the start.  Starts not in the table are not touched.
//
// Rounding: every dot product accumulates variable 0 first, ascending to P - 1 (hyper._rowdot; on the device one lane broadcast per
// variable -- lanes 0 .. 63 of a lane's first variable, then of its second --, no butterfly) and no product is contracted into the sum
// that follows it, so that, fed the same (f, g), the iterates are those of the host optimiser bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

// a * b + c stays two roundings in the arithmetic below (csrc/gp_acqf_opt.h's rule: the device source and the host emulation include
// this header last; the launcher takes only the argument blocks and compiles as it always did)
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

constexpr int QACQF_OPT_MAX_P = 128;   // two variables per lane: q * D up to 8 * 15 = 120
constexpr int QACQF_OPT_HMAX = LBFGS_HMAX;
constexpr int QO_NV = LBFGS_LANES > 1 ? 2 : QACQF_OPT_MAX_P;   // a lane's variables: i % 64 is the lane, i / 64 the entry; all of them in the host build
// per-start optimiser state in the caller's workspace, in doubles: the layout of csrc/gp_lbfgs_core.h with P = q * D
constexpr size_t qacqf_opt_state_doubles(int P, int H) { return lbfgs_state_doubles(P, H); }

struct QAcqfOptParams {
  const double* value;     // (Bs)     acquisition value of (7p) / (7q) at Xq's row s (maximised: negated on the way in)
  const double* grad;      // (Bs, P)  its input gradient
  const int32_t* slots;    // (Bs)     the start of slot s, distinct entries within [0, B); NULL: s
  const double* x0;        // (B, P)   start points (mode 0)
  const double* lo;        // (P)
  const double* hi;        // (P)
  double* state;           // (B, qacqf_opt_state_doubles(P, history))
  double* Xq;              // (Bs, P)  out: the point the next round evaluates for slot s = the (Bs * q, D) array of the evaluation kernels
  double* x;               // (B, P)   out: accepted point
  double* f;               // (B)      out: the acquisition value there
  int32_t* stats;          // (B, 4)   out: iterations, evaluations, status, pairs held
  int B, Bs, P;
  int mode;                // 0: project x0 onto the box, reset the state; 1: consume one evaluation; 2: neither -- the outputs again
                           //    from the state as it is, for a slot table that has changed since the state's trial points were written
  int max_iter, history, max_ls, pad_;
  double gtol, ftol, c1;
};

// lane j's value in every lane
LBFGS_DEV double qo_bcast(double v, int j) {
#if LBFGS_LANES > 1
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
#else
  (void)j;
  return v;
#endif
}
// sum / maximum of the variables' terms, variable 0 first, the same bits in every lane
LBFGS_DEV double qo_sum(const double* term, int P) {
#if LBFGS_LANES > 1
  const int P0 = P < LBFGS_LANES ? P : LBFGS_LANES;
  double acc = qo_bcast(term[0], 0);
  for (int j = 1; j < P0; ++j) acc = acc + qo_bcast(term[0], j);
  for (int j = LBFGS_LANES; j < P; ++j) acc = acc + qo_bcast(term[1], j - LBFGS_LANES);
#else
  double acc = term[0];
  for (int j = 1; j < P; ++j) acc = acc + term[j];
#endif
  return acc;
}
LBFGS_DEV double qo_max(const double* term, int P) {
#if LBFGS_LANES > 1
  const int P0 = P < LBFGS_LANES ? P : LBFGS_LANES;
  double acc = qo_bcast(term[0], 0);
  for (int j = 1; j < P0; ++j) acc = fmax(acc, qo_bcast(term[0], j));
  for (int j = LBFGS_LANES; j < P; ++j) acc = fmax(acc, qo_bcast(term[1], j - LBFGS_LANES));
#else
  double acc = term[0];
  for (int j = 1; j < P; ++j) acc = fmax(acc, term[j]);
#endif
  return acc;
}

struct QoReduce {
  static constexpr int NV = QO_NV;
  static LBFGS_INLINE double sum(const double* term, int P) { return qo_sum(term, P); }
  static LBFGS_INLINE double max(const double* term, int P) { return qo_max(term, P); }
};

// The whole step of slot `s`: reset or consume (value, grad) of the round's evaluation, then hand the next trial point to the
// evaluation kernels (row s) and the accepted point, its value and the counters to the caller (row slots[s]).  A start that has
// stopped keeps its slot until the caller drops it: its row of Xq is its accepted point and what comes back for it is ignored.
LBFGS_DEV void qo_step(const QAcqfOptParams& p, int s, int lane) {
  const int P = p.P, H = p.history;
  if (s >= p.Bs) return;
  const int b = p.slots ? p.slots[s] : s;
  if (b < 0 || b >= p.B) return;   // (no start: nothing to address)
  double* st = p.state + (size_t)b * qacqf_opt_state_doubles(P, H);
  const double *x = st, *xt = st + 3 * (size_t)P;
  LbfgsResult r;
  if (p.mode == 0) {
    r = lbfgs_reset<true>(st, p.x0 + (size_t)b * P, p.lo, p.hi, P, H, false, lane);
  } else if (p.mode == 2) {
    const double* sc = st + (size_t)(4 + 2 * H) * P + H;
    r = LbfgsResult{sc[LBFGS_F], (int)sc[LBFGS_IT], (int)sc[LBFGS_NEVAL], (int)sc[LBFGS_STATUS], (int)sc[LBFGS_HIST]};
  } else {
    double gt[QO_NV] = {0.0};
    LBFGS_FOR(i, P) gt[LBFGS_AT(i)] = -p.grad[(size_t)s * P + i];
    r = lbfgs_advance<true, QoReduce>(st, p.lo, p.hi, P, H, p.max_iter, p.max_ls, p.gtol, p.ftol, p.c1, lane, -p.value[s], gt);
  }
  LBFGS_FOR(i, P) {
    p.Xq[(size_t)s * P + i] = xt[i];
    p.x[(size_t)b * P + i] = x[i];
  }
  if (lane == 0) {
    p.f[b] = -r.f;
    p.stats[4 * b + 0] = r.it;
    p.stats[4 * b + 1] = r.n_eval;
    p.stats[4 * b + 2] = r.status;
    p.stats[4 * b + 3] = r.hist;
  }
}

// ---- the gather: the joint prior of the target GP's value path from the weighted GRAD-pass sums --------------------------------------
// What ScaMLGP.joint_acqf_inputs concatenates, per element: the value column (column 0 of a query point's 16) of mu_g, var_g and of
// the training rows of cov_g goes behind the training block.  left != 0 writes the training block itself (it does not depend on the
// round; the row width n + Mq does, so it is written whenever Mq may have changed).
struct QAcqfOptGatherParams {
  const double* mu_g;      // (Mq * 16)
  const double* var_g;     // (Mq * 16)
  const double* cov_g;     // (>= n, Mq * 16): rows a < n are read
  const double* Xq;        // (Mq, D)
  const double* mu_t;      // (n)       left: the weighted source sums at the training inputs
  const double* var_t;     // (n)
  const double* cov_tt;    // (n, n)
  const double* Xt;        // (n, D)
  double* mean_s;          // (n + Mq)
  double* var_s;           // (n + Mq)
  double* cov_s;           // (n, n + Mq)
  double* xall;            // (n + Mq, D)
  int n, Mq, D, left;
};
// elements of one launch: a column of (n rows of cov, mean, var, D coordinates) per query point -- or per training point (left)
LBFGS_DEV long long qo_gather_elems(const QAcqfOptGatherParams& p) { return (long long)(p.left ? p.n : p.Mq) * (p.n + 2 + p.D); }
LBFGS_DEV void qo_gather_elem(const QAcqfOptGatherParams& p, long long e) {
  const int n = p.n, W = p.left ? p.n : p.Mq;
  const size_t ld = (size_t)n + p.Mq;
  const int j = (int)(e % W), r = (int)(e / W);
  if (p.left) {
    if (r < n) p.cov_s[(size_t)r * ld + j] = p.cov_tt[(size_t)r * n + j];
    else if (r == n) p.mean_s[j] = p.mu_t[j];
    else if (r == n + 1) p.var_s[j] = p.var_t[j];
    else p.xall[(size_t)j * p.D + (r - n - 2)] = p.Xt[(size_t)j * p.D + (r - n - 2)];
  } else {
    if (r < n) p.cov_s[(size_t)r * ld + n + j] = p.cov_g[((size_t)r * p.Mq + j) * 16];
    else if (r == n) p.mean_s[n + j] = p.mu_g[(size_t)j * 16];
    else if (r == n + 1) p.var_s[n + j] = p.var_g[(size_t)j * 16];
    else p.xall[(size_t)(n + j) * p.D + (r - n - 2)] = p.Xq[(size_t)j * p.D + (r - n - 2)];
  }
}

}  // namespace scaml
