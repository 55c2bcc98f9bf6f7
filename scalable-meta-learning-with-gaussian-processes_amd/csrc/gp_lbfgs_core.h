// gp_lbfgs_core.h -- the L-BFGS state machine of the two device-side optimisers: one wave per problem, one lane per variable, the
// state in the caller's workspace, one evaluation consumed per call, no LDS.  Three instances:
//   BOX = false   csrc/gp_stack_fit.hip: hyper.batched_lbfgs, the unconstrained fit of the source stack's hyper-parameters
//   BOX = true    csrc/gp_acqf_opt.h:    hyper._batched_lbfgs_box, the projected optimiser of the acquisition function
//   BOX = true    csrc/gp_qacqf_opt.h:   the same for the joint q-point acquisition, q D <= 128 variables, two per lane
// What differs between them (the eight rows of DESIGN.md 4h's table) is an `if constexpr (BOX)` below or the reduction `R` the
// instance hands in:
//   R::NV                a lane's variables (i = lane, lane + LBFGS_LANES, ... < P live in arrays of NV entries)
//   R::sum(term, P)      sum / maximum over the P variables of the per-lane terms, the same bits in every lane.  A lane without
//   R::max(term, P)      a variable leaves its term at zero.
// Every dot product below is "fill term[LBFGS_AT(i)], reduce".
//
// Floating-point contraction belongs to the instance, not to this header, and the pragma is lexical: this file neither sets nor
// resets it and a * b + c is written as one expression wherever the instance may (stack fit: hipcc's default) or may not
// (acquisition: off) contract it.  A translation unit takes this header once, under the setting of its first include.
//
// Host form (one "lane" loops over all variables): SCAML_HOST_EMUL, or any compiler but hipcc.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(SCAML_HOST_EMUL)
#define LBFGS_INLINE __device__ __forceinline__
#define LBFGS_DEV LBFGS_INLINE
#define LBFGS_LANES 64
#else
#define LBFGS_INLINE inline
#define LBFGS_DEV static inline
#define LBFGS_LANES 1
#endif
#define LBFGS_FOR(i, n) for (int i = lane; i < (n); i += LBFGS_LANES)
#define LBFGS_AT(i) ((i) / LBFGS_LANES)

namespace scaml {

constexpr int LBFGS_HMAX = 16;      // curvature pairs kept at most
constexpr int LBFGS_SCALARS = 16;

// Per-problem optimiser state in the caller's workspace, in doubles (P variables, H = history):
//   x[P] accepted point   g[P] gradient there   d[P] search direction   xt[P] trial point
//   S[H][P], Y[H][P] curvature pairs (ring: the newest in slot head - 1)   rho[H]
//   sc[16]: f, step t, g . d (BOX: the slope g . (xt - x)), iteration, evaluations, status, failed trials of this line search,
//           pairs held, head, phase
constexpr size_t lbfgs_state_doubles(int P, int H) { return (size_t)(4 + 2 * H) * P + H + LBFGS_SCALARS; }
enum { LBFGS_F = 0, LBFGS_T = 1, LBFGS_GD = 2, LBFGS_IT = 3, LBFGS_NEVAL = 4, LBFGS_STATUS = 5, LBFGS_LS = 6, LBFGS_HIST = 7,
       LBFGS_HEAD = 8, LBFGS_PHASE = 9 };
enum { LBFGS_RUNNING = 0, LBFGS_CONVERGED = 1, LBFGS_FTOL = 2, LBFGS_STALLED = 3, LBFGS_FAILED = 4, LBFGS_MAXITER = 5,
       LBFGS_PADDING = 6 };   // (padding: a row of the box instance that belongs to no study)

struct LbfgsResult {
  double f;
  int it, n_eval, status, hist;
};

// A flag per variable of a lane: a bool where a lane has one variable; an int where it has several -- an array of bools indexed by
// the loop variable is kept in scratch memory, an array of ints in registers.
template <int NV> struct LbfgsFlag { typedef int type; };
template <> struct LbfgsFlag<1> { typedef bool type; };

LBFGS_DEV bool lbfgs_finite(double x) { return x - x == 0.0; }
// min(max(v, lo), hi) that keeps a NaN
LBFGS_DEV double lbfgs_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Start: the caller's point (BOX: projected onto the box) is the accepted point and the first trial; nothing has been evaluated.
template <bool BOX>
LBFGS_DEV LbfgsResult lbfgs_reset(double* st, const double* x0, const double* lo, const double* hi, int P, int H, bool padding, int lane) {
  double *x = st, *xt = st + 3 * (size_t)P, *sc = st + (size_t)(4 + 2 * H) * P + H;
  LBFGS_FOR(i, P) {
    double v = x0[i];
    if constexpr (BOX) v = lbfgs_clamp(v, lo[i], hi[i]);
    x[i] = v;
    xt[i] = v;
  }
  if (lane == 0) {
    for (int k = 0; k < LBFGS_SCALARS; ++k) sc[k] = 0.0;
    if constexpr (BOX) {
      if (padding) sc[LBFGS_STATUS] = (double)LBFGS_PADDING;
    }
  }
  return LbfgsResult{0.0, 0, 0, BOX && padding ? LBFGS_PADDING : LBFGS_RUNNING, 0};
}

// The stopping quantity at (x, g): max |g|; BOX: max_i |P(x - g) - x|_i, scipy L-BFGS-B's (hyper.projected_gradient)
template <bool BOX, class R>
LBFGS_DEV double lbfgs_stop_quantity(const double* x, const double* g, const double* lo, const double* hi, int P, int lane) {
  double term[R::NV] = {0.0};
  LBFGS_FOR(i, P) {
    if constexpr (BOX) term[LBFGS_AT(i)] = fabs(lbfgs_clamp(x[i] - g[i], lo[i], hi[i]) - x[i]);
    else term[LBFGS_AT(i)] = fabs(g[i]);
  }
  return R::max(term, P);
}

// Armijo test of a trial value ft; gd is slot LBFGS_GD
template <bool BOX>
LBFGS_DEV bool lbfgs_armijo(double f, double ft, double c1, double t, double gd) {
  if constexpr (BOX) return gd < 0.0 && ft <= f + c1 * gd;
  else return ft <= f + c1 * t * gd;
}

// One evaluation (ft, gt) of the minimised function at the trial point st.xt arrives.  Leaves the next point to evaluate in st.xt --
// the accepted point once the problem has stopped (status != 0).  lo / hi are read by the BOX instance only.
template <bool BOX, class R>
LBFGS_DEV LbfgsResult lbfgs_advance(double* st, const double* lo, const double* hi, int P, int H, int max_iter, int max_ls, double gtol,
                                    double ftol, double c1, int lane, double ft, const double* gt) {
  double *x = st, *g = st + P, *d = st + 2 * (size_t)P, *xt = st + 3 * (size_t)P;
  double *S = st + 4 * (size_t)P, *Y = S + (size_t)H * P, *rho = Y + (size_t)H * P, *sc = rho + H;
  double f = sc[LBFGS_F], t = sc[LBFGS_T], gd = sc[LBFGS_GD];
  int it = (int)sc[LBFGS_IT], n_eval = (int)sc[LBFGS_NEVAL], status = (int)sc[LBFGS_STATUS], ls = (int)sc[LBFGS_LS],
      hist = (int)sc[LBFGS_HIST], head = (int)sc[LBFGS_HEAD];
  const int phase = (int)sc[LBFGS_PHASE];
  if (status != LBFGS_RUNNING) return LbfgsResult{f, it, n_eval, status, hist};   // stopped: xt already is the accepted point
  ++n_eval;
  double term[R::NV] = {0.0};
  LBFGS_FOR(i, P) term[LBFGS_AT(i)] = lbfgs_finite(gt[LBFGS_AT(i)]) ? 0.0 : 1.0;
  const bool finite = lbfgs_finite(ft) && R::sum(term, P) == 0.0;
  bool new_dir = false;
  int new_slot = -1;     // (a pair pushed in this call: its rho is not read back from memory, another lane wrote it)
  double new_rho = 0.0;
  if (phase == 0) {
    if (!finite) {
      f = INFINITY;
      LBFGS_FOR(i, P) g[i] = 0.0;
      status = LBFGS_FAILED;
    } else {
      f = ft;
      LBFGS_FOR(i, P) g[i] = gt[LBFGS_AT(i)];
      bool converged = false;   // (the unconstrained optimiser does not test its start point)
      if constexpr (BOX) converged = lbfgs_stop_quantity<BOX, R>(x, g, lo, hi, P, lane) <= gtol;
      if (converged) status = LBFGS_CONVERGED;
      else if (max_iter < 1) status = LBFGS_MAXITER;
      else new_dir = true;
    }
  } else if (finite && lbfgs_armijo<BOX>(f, ft, c1, t, gd)) {
    LBFGS_FOR(i, P) term[LBFGS_AT(i)] = (xt[i] - x[i]) * (gt[LBFGS_AT(i)] - g[i]);
    const double sy = R::sum(term, P);
    LBFGS_FOR(i, P) term[LBFGS_AT(i)] = (gt[LBFGS_AT(i)] - g[i]) * (gt[LBFGS_AT(i)] - g[i]);
    const double yy = R::sum(term, P);
    LBFGS_FOR(i, P) term[LBFGS_AT(i)] = (xt[i] - x[i]) * (xt[i] - x[i]);
    const double ss = R::sum(term, P);
    bool push = sy > 1e-10 * sqrt(yy) * sqrt(ss);
    if constexpr (BOX) push = sy > 0.0 && push;
    LBFGS_FOR(i, P) {
      if (push) {
        S[(size_t)head * P + i] = xt[i] - x[i];
        Y[(size_t)head * P + i] = gt[LBFGS_AT(i)] - g[i];
      }
      x[i] = xt[i];
      g[i] = gt[LBFGS_AT(i)];
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
    if (lbfgs_stop_quantity<BOX, R>(x, g, lo, hi, P, lane) <= gtol) status = LBFGS_CONVERGED;
    else if (rel <= ftol && it > 1) status = LBFGS_FTOL;
    else if (it >= max_iter) status = LBFGS_MAXITER;
    else new_dir = true;
  } else {
    if (++ls >= max_ls) status = LBFGS_STALLED;   // line search exhausted: the problem stops where it is
    else t = 0.5 * t;
  }
  if (new_dir) {
    ++it;
    ls = 0;
    // BOX: coordinates held by a bound (at it, and -g points out of the box) take no part in the direction
    double q[R::NV] = {0.0}, gfree[R::NV] = {0.0}, al[LBFGS_HMAX];
    typename LbfgsFlag<R::NV>::type held[R::NV] = {};
    LBFGS_FOR(i, P) {
      if constexpr (BOX) held[LBFGS_AT(i)] = (x[i] <= lo[i] && g[i] > 0.0) || (x[i] >= hi[i] && g[i] < 0.0);
      gfree[LBFGS_AT(i)] = held[LBFGS_AT(i)] ? 0.0 : g[i];
      q[LBFGS_AT(i)] = gfree[LBFGS_AT(i)];
    }
    // two-loop recursion, newest pair first (pair h lives in slot (head - 1 - h) mod H)
#pragma unroll
    for (int h = 0; h < LBFGS_HMAX; ++h) {
      if (h < hist) {
        const int slot = (head - 1 - h + 2 * H) % H;
        const double r = slot == new_slot ? new_rho : rho[slot];
        LBFGS_FOR(i, P) term[LBFGS_AT(i)] = S[(size_t)slot * P + i] * q[LBFGS_AT(i)];
        al[h] = r * R::sum(term, P);
        LBFGS_FOR(i, P) q[LBFGS_AT(i)] = q[LBFGS_AT(i)] - al[h] * Y[(size_t)slot * P + i];
      }
    }
    double gamma = 1.0;
    if (hist > 0) {
      const int slot = (head - 1 + H) % H;
      LBFGS_FOR(i, P) term[LBFGS_AT(i)] = S[(size_t)slot * P + i] * Y[(size_t)slot * P + i];
      const double ys = R::sum(term, P);
      LBFGS_FOR(i, P) term[LBFGS_AT(i)] = Y[(size_t)slot * P + i] * Y[(size_t)slot * P + i];
      const double yy = R::sum(term, P);
      if (yy > 0.0) gamma = ys / fmax(yy, 1e-300);
    }
    LBFGS_FOR(i, P) q[LBFGS_AT(i)] = gamma * q[LBFGS_AT(i)];
#pragma unroll
    for (int h = LBFGS_HMAX - 1; h >= 0; --h) {
      if (h < hist) {
        const int slot = (head - 1 - h + 2 * H) % H;
        const double r = slot == new_slot ? new_rho : rho[slot];
        LBFGS_FOR(i, P) term[LBFGS_AT(i)] = Y[(size_t)slot * P + i] * q[LBFGS_AT(i)];
        const double b = r * R::sum(term, P);
        LBFGS_FOR(i, P) q[LBFGS_AT(i)] = q[LBFGS_AT(i)] + (al[h] - b) * S[(size_t)slot * P + i];
      }
    }
    LBFGS_FOR(i, P) {
      q[LBFGS_AT(i)] = held[LBFGS_AT(i)] ? 0.0 : -q[LBFGS_AT(i)];
      term[LBFGS_AT(i)] = g[i] * q[LBFGS_AT(i)];
    }
    const double gq = R::sum(term, P);
    // not a descent direction (or no pair yet): (projected) steepest descent, the first step scaled like scipy's
    const bool bad_dir = !(gq < 0.0);
    LBFGS_FOR(i, P) {
      d[i] = bad_dir ? -gfree[LBFGS_AT(i)] : q[LBFGS_AT(i)];
      term[LBFGS_AT(i)] = gfree[LBFGS_AT(i)] * gfree[LBFGS_AT(i)];
    }
    const double gg = R::sum(term, P);
    if constexpr (!BOX) gd = bad_dir ? -gg : gq;
    t = (hist > 0 && !bad_dir) ? 1.0 : fmin(1.0 / fmax(sqrt(gg), 1e-12), 1.0);
  }
  if (status == LBFGS_RUNNING) {
    LBFGS_FOR(i, P) {
      if constexpr (BOX) {
        xt[i] = lbfgs_clamp(x[i] + t * d[i], lo[i], hi[i]);
        term[LBFGS_AT(i)] = g[i] * (xt[i] - x[i]);
      } else {
        xt[i] = x[i] + t * d[i];
      }
    }
    if constexpr (BOX) gd = R::sum(term, P);
  } else {
    LBFGS_FOR(i, P) xt[i] = x[i];
  }
  if (lane == 0) {
    sc[LBFGS_F] = f; sc[LBFGS_T] = t; sc[LBFGS_GD] = gd; sc[LBFGS_IT] = it; sc[LBFGS_NEVAL] = n_eval; sc[LBFGS_STATUS] = status;
    sc[LBFGS_LS] = ls; sc[LBFGS_HIST] = hist; sc[LBFGS_HEAD] = head; sc[LBFGS_PHASE] = 1.0;
  }
  return LbfgsResult{f, it, n_eval, status, hist};
}

}  // namespace scaml
