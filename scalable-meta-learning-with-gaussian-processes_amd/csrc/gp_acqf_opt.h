// gp_acqf_opt.h -- the optimiser step of the device-side acquisition optimiser (scaml_studies_acqf_opt_f64, include/scaml_gp.h (7h)):
// argument block, state stride and the per-start advance function.  One source for the device kernel (csrc/gp_acqf_opt.hip: one wave
// per start point, one lane per coordinate), the host launcher and the single-threaded host build the CPU tests drive against
// hyper.batched_lbfgs(bounds=...) (any compiler but hipcc: tests/host_emul).
//
// ao_advance is hyper._batched_lbfgs_box for ONE start as a state machine that consumes one evaluation per call (csrc/gp_stack_fit.hip
// does the same for the unconstrained optimiser): projection onto the box, held coordinates (at a bound, gradient pointing outward),
// two-loop recursion, projected steepest descent where there is no pair or no descent, projected trial points, Armijo on
// g . (trial - x) with halving, curvature pair kept when s . y > 0, scipy L-BFGS-B's stopping rules.  The state lives in the caller's
// workspace; no LDS; a lane reads back only what it wrote in this launch or what an earlier launch left.
//
// Rounding: every dot product accumulates coordinate by coordinate in ascending order (hyper._rowdot; on the device one lane
// broadcast per coordinate, no butterfly) and no product is contracted into the sum that follows it, so that, fed the same (f, g),
// the iterates are those of the host optimiser bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define AO_DEV __device__ __forceinline__
#define AO_LANES 64
#define AO_NV 1
#else
#define AO_DEV static inline
#define AO_LANES 1
#define AO_NV 16
#endif

// a * b + c stays two roundings in the arithmetic below (the device source and the host emulation include this header last; the
// launcher takes only the argument block and compiles as it always did)
#if defined(__HIPCC__) || defined(SCAML_HOST_EMUL)
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#endif

namespace scaml {

constexpr int ACQF_OPT_MAX_D = 15;     // one lane per coordinate; the limit of (5e) / (7g)
constexpr int ACQF_OPT_HMAX = 16;      // curvature pairs kept at most
constexpr int ACQF_OPT_SCALARS = 16;

// Per-start optimiser state in the caller's workspace, in doubles (H = history):
//   x[D] accepted point   g[D] gradient of -acquisition there   d[D] search direction   xt[D] trial point
//   S[H][D], Y[H][D] curvature pairs (ring: the newest in slot head - 1)   rho[H]
//   sc[16]: f, step t, slope g . (xt - x), iteration, evaluations, status, failed trials of this line search, pairs held, head, phase
constexpr size_t acqf_opt_state_doubles(int D, int H) { return (size_t)(4 + 2 * H) * D + H + ACQF_OPT_SCALARS; }
enum { AO_F = 0, AO_T = 1, AO_SLOPE = 2, AO_IT = 3, AO_NEVAL = 4, AO_STATUS = 5, AO_LS = 6, AO_HIST = 7, AO_HEAD = 8, AO_PHASE = 9 };
// status: the stack fit's codes, and one for a padding row
enum { AO_RUNNING = 0, AO_CONVERGED = 1, AO_FTOL = 2, AO_STALLED = 3, AO_FAILED = 4, AO_MAXITER = 5, AO_PADDING = 6 };

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

#define AO_FOR(i) for (int i = lane; i < D; i += AO_LANES)
#define AO_AT(i) ((i) / AO_LANES)

AO_DEV bool ao_finite(double x) { return x - x == 0.0; }
// min(max(v, lo), hi) that keeps a NaN
AO_DEV double ao_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// lane j's value in every lane
AO_DEV double ao_bcast(double v, int j) {
#ifdef __HIPCC__
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
#else
  (void)j;
  return v;
#endif
}
// sum / maximum of the coordinates' terms, coordinate 0 first, the same bits in every lane
AO_DEV double ao_sum(const double* term, int D) {
#ifdef __HIPCC__
  double acc = ao_bcast(term[0], 0);
  for (int j = 1; j < D; ++j) acc = acc + ao_bcast(term[0], j);
#else
  double acc = term[0];
  for (int j = 1; j < D; ++j) acc = acc + term[j];
#endif
  return acc;
}
AO_DEV double ao_max(const double* term, int D) {
#ifdef __HIPCC__
  double acc = ao_bcast(term[0], 0);
  for (int j = 1; j < D; ++j) acc = fmax(acc, ao_bcast(term[0], j));
#else
  double acc = term[0];
  for (int j = 1; j < D; ++j) acc = fmax(acc, term[j]);
#endif
  return acc;
}

struct AoResult {
  double f;
  int it, n_eval, status, hist;
};

// Start of an optimisation: the projected start is the accepted point and the first trial; nothing has been evaluated.
AO_DEV AoResult ao_reset(double* st, const double* x0, const double* lo, const double* hi, int D, int H, bool padding, int lane) {
  double *x = st, *xt = st + 3 * (size_t)D, *sc = st + (size_t)(4 + 2 * H) * D + H;
  AO_FOR(i) {
    const double v = ao_clamp(x0[i], lo[i], hi[i]);
    x[i] = v;
    xt[i] = v;
  }
  if (lane == 0) {
    for (int k = 0; k < ACQF_OPT_SCALARS; ++k) sc[k] = 0.0;
    if (padding) sc[AO_STATUS] = (double)AO_PADDING;
  }
  return AoResult{0.0, 0, 0, padding ? AO_PADDING : AO_RUNNING, 0};
}

// max_i |P(x - g) - x|_i: scipy L-BFGS-B's stopping quantity (hyper.projected_gradient)
AO_DEV double ao_projected_gradient(const double* x, const double* g, const double* lo, const double* hi, int D, int lane) {
  double tm[AO_NV] = {0.0};
  AO_FOR(i) tm[AO_AT(i)] = fabs(ao_clamp(x[i] - g[i], lo[i], hi[i]) - x[i]);
  return ao_max(tm, D);
}

// One evaluation (ft, gt) of the MINIMISED function at the trial point st.xt arrives: hyper._batched_lbfgs_box for this start alone.
// Leaves the next point to evaluate in st.xt -- the accepted point once the start has stopped (status != 0).
AO_DEV AoResult ao_advance(double* st, const double* lo, const double* hi, int D, int H, int max_iter, int max_ls, double gtol, double ftol,
                           double c1, int lane, double ft, const double* gt) {
  double *x = st, *g = st + D, *d = st + 2 * (size_t)D, *xt = st + 3 * (size_t)D;
  double *S = st + 4 * (size_t)D, *Y = S + (size_t)H * D, *rho = Y + (size_t)H * D, *sc = rho + H;
  double f = sc[AO_F], t = sc[AO_T], slope = sc[AO_SLOPE];
  int it = (int)sc[AO_IT], n_eval = (int)sc[AO_NEVAL], status = (int)sc[AO_STATUS], ls = (int)sc[AO_LS], hist = (int)sc[AO_HIST],
      head = (int)sc[AO_HEAD];
  const int phase = (int)sc[AO_PHASE];
  if (status != AO_RUNNING) return AoResult{f, it, n_eval, status, hist};   // stopped: xt already is the accepted point
  ++n_eval;
  double tm[AO_NV] = {0.0};
  AO_FOR(i) tm[AO_AT(i)] = ao_finite(gt[AO_AT(i)]) ? 0.0 : 1.0;
  const bool finite = ao_finite(ft) && ao_sum(tm, D) == 0.0;
  bool new_dir = false;
  int new_slot = -1;     // (a pair pushed in this call: its rho is not read back from memory, another lane wrote it)
  double new_rho = 0.0;
  if (phase == 0) {
    if (!finite) {
      f = INFINITY;
      AO_FOR(i) g[i] = 0.0;
      status = AO_FAILED;
    } else {
      f = ft;
      AO_FOR(i) g[i] = gt[AO_AT(i)];
      if (ao_projected_gradient(x, g, lo, hi, D, lane) <= gtol) status = AO_CONVERGED;
      else if (max_iter < 1) status = AO_MAXITER;
      else new_dir = true;
    }
  } else if (finite && slope < 0.0 && ft <= f + c1 * slope) {
    double sy, ss, yy;
    AO_FOR(i) tm[AO_AT(i)] = (xt[i] - x[i]) * (gt[AO_AT(i)] - g[i]);
    sy = ao_sum(tm, D);
    AO_FOR(i) tm[AO_AT(i)] = (gt[AO_AT(i)] - g[i]) * (gt[AO_AT(i)] - g[i]);
    yy = ao_sum(tm, D);
    AO_FOR(i) tm[AO_AT(i)] = (xt[i] - x[i]) * (xt[i] - x[i]);
    ss = ao_sum(tm, D);
    const bool push = sy > 0.0 && sy > 1e-10 * sqrt(yy) * sqrt(ss);
    AO_FOR(i) {
      if (push) {
        S[(size_t)head * D + i] = xt[i] - x[i];
        Y[(size_t)head * D + i] = gt[AO_AT(i)] - g[i];
      }
      x[i] = xt[i];
      g[i] = gt[AO_AT(i)];
    }
    if (push) {
      new_slot = head;
      new_rho = 1.0 / fmax(sy, 1e-300);
      if (lane == 0) rho[head] = new_rho;
      head = (head + 1) % H;
      if (hist < H) ++hist;
    }
    const double rel = (f - ft) / fmax(fmax(fabs(f), fabs(ft)), 1.0);
    f = ft;
    if (ao_projected_gradient(x, g, lo, hi, D, lane) <= gtol) status = AO_CONVERGED;
    else if (rel <= ftol && it > 1) status = AO_FTOL;
    else if (it >= max_iter) status = AO_MAXITER;
    else new_dir = true;
  } else {
    if (++ls >= max_ls) status = AO_STALLED;   // line search exhausted: the start stops where it is
    else t = 0.5 * t;
  }
  if (new_dir) {
    ++it;
    ls = 0;
    // coordinates held by a bound: at it, and -g points out of the box
    double q[AO_NV] = {0.0}, gfree[AO_NV] = {0.0}, al[ACQF_OPT_HMAX];
    bool held[AO_NV] = {false};
    AO_FOR(i) {
      held[AO_AT(i)] = (x[i] <= lo[i] && g[i] > 0.0) || (x[i] >= hi[i] && g[i] < 0.0);
      gfree[AO_AT(i)] = held[AO_AT(i)] ? 0.0 : g[i];
      q[AO_AT(i)] = gfree[AO_AT(i)];
    }
    // two-loop recursion, newest pair first (pair h lives in slot (head - 1 - h) mod H)
#pragma unroll
    for (int h = 0; h < ACQF_OPT_HMAX; ++h) {
      if (h < hist) {
        const int slot = (head - 1 - h + 2 * H) % H;
        const double r = slot == new_slot ? new_rho : rho[slot];
        AO_FOR(i) tm[AO_AT(i)] = S[(size_t)slot * D + i] * q[AO_AT(i)];
        al[h] = r * ao_sum(tm, D);
        AO_FOR(i) q[AO_AT(i)] = q[AO_AT(i)] - al[h] * Y[(size_t)slot * D + i];
      }
    }
    double gamma = 1.0;
    if (hist > 0) {
      const int slot = (head - 1 + H) % H;
      AO_FOR(i) tm[AO_AT(i)] = S[(size_t)slot * D + i] * Y[(size_t)slot * D + i];
      const double ys = ao_sum(tm, D);
      AO_FOR(i) tm[AO_AT(i)] = Y[(size_t)slot * D + i] * Y[(size_t)slot * D + i];
      const double yy = ao_sum(tm, D);
      if (yy > 0.0) gamma = ys / fmax(yy, 1e-300);
    }
    AO_FOR(i) q[AO_AT(i)] = gamma * q[AO_AT(i)];
#pragma unroll
    for (int h = ACQF_OPT_HMAX - 1; h >= 0; --h) {
      if (h < hist) {
        const int slot = (head - 1 - h + 2 * H) % H;
        const double r = slot == new_slot ? new_rho : rho[slot];
        AO_FOR(i) tm[AO_AT(i)] = Y[(size_t)slot * D + i] * q[AO_AT(i)];
        const double b = r * ao_sum(tm, D);
        AO_FOR(i) q[AO_AT(i)] = q[AO_AT(i)] + (al[h] - b) * S[(size_t)slot * D + i];
      }
    }
    AO_FOR(i) {
      q[AO_AT(i)] = held[AO_AT(i)] ? 0.0 : -q[AO_AT(i)];
      tm[AO_AT(i)] = g[i] * q[AO_AT(i)];
    }
    const double gd = ao_sum(tm, D);
    // not a descent direction (or no pair yet): projected steepest descent, the first step scaled like scipy's
    const bool bad_dir = !(gd < 0.0);
    AO_FOR(i) {
      d[i] = bad_dir ? -gfree[AO_AT(i)] : q[AO_AT(i)];
      tm[AO_AT(i)] = gfree[AO_AT(i)] * gfree[AO_AT(i)];
    }
    const double gnorm = sqrt(ao_sum(tm, D));
    t = (hist > 0 && !bad_dir) ? 1.0 : fmin(1.0 / fmax(gnorm, 1e-12), 1.0);
  }
  if (status == AO_RUNNING) {
    AO_FOR(i) {
      xt[i] = ao_clamp(x[i] + t * d[i], lo[i], hi[i]);
      tm[AO_AT(i)] = g[i] * (xt[i] - x[i]);
    }
    slope = ao_sum(tm, D);
  } else {
    AO_FOR(i) xt[i] = x[i];
  }
  if (lane == 0) {
    sc[AO_F] = f; sc[AO_T] = t; sc[AO_SLOPE] = slope; sc[AO_IT] = it; sc[AO_NEVAL] = n_eval; sc[AO_STATUS] = status;
    sc[AO_LS] = ls; sc[AO_HIST] = hist; sc[AO_HEAD] = head; sc[AO_PHASE] = 1.0;
  }
  return AoResult{f, it, n_eval, status, hist};
}

// The whole step of start `b`: reset or consume (value, grad) of the round's evaluation, then hand the next trial point and the
// start's live group to the evaluation kernels and the accepted point, its value and the counters to the caller.
AO_DEV void ao_step(const AcqfOptParams& p, int b, int lane) {
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
    AO_FOR(i) gt[AO_AT(i)] = -p.grad[(size_t)b * D + i];
    r = ao_advance(st, p.lo, p.hi, D, H, p.max_iter, p.max_ls, p.gtol, p.ftol, p.c1, lane, -p.value[b], gt);
  }
  AO_FOR(i) {
    p.Xq[(size_t)b * D + i] = xt[i];
    p.x[(size_t)b * D + i] = x[i];
  }
  if (lane == 0) {
    p.group_live[b] = r.status == AO_RUNNING ? grp : -1;
    p.f[b] = r.status == AO_PADDING ? 0.0 : -r.f;
    p.stats[4 * b + 0] = r.it;
    p.stats[4 * b + 1] = r.n_eval;
    p.stats[4 * b + 2] = r.status;
    p.stats[4 * b + 3] = r.hist;
  }
}

}  // namespace scaml
