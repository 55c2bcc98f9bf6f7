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
//   sf_advance     hyper.batched_lbfgs as a per-problem state machine, one evaluation per call: Armijo test of the trial with
//                  halving, curvature pair, stopping rules, two-loop recursion, steepest-descent fallback
//
// SCAML_HOST_EMUL: the same source compiles as single-threaded host code (tests/host_emul: checked against the oracle and
// hyper.batched_lbfgs on CPU; never part of libscaml_hip.so).  A "lane" then loops over all variables and a wave reduction is
// the identity.
#ifndef SCAML_HOST_EMUL
#include <hip/hip_runtime.h>
#define SF_DEV __device__ __forceinline__
#define SF_LANES 64
#else
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#define SF_DEV static inline
#define SF_LANES 1
#endif
#include "gp_stack_fit_params.h"

namespace scaml {

// a lane's variables: i = lane, lane + SF_LANES, ... < P; their per-lane values live in arrays of SF_NV entries (one register on
// the device, all P of them in the host build)
constexpr int SF_NV = STACK_FIT_PMAX / SF_LANES;
#define SF_FOR(i) for (int i = lane; i < P; i += SF_LANES)
#define SF_AT(i) ((i) / SF_LANES)

// sum / maximum over the wave, the same bits in every lane (butterfly: both partners add the same two numbers)
SF_DEV double sf_sum(double x) {
#ifndef SCAML_HOST_EMUL
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
#endif
  return x;
}
SF_DEV double sf_max(double x) {
#ifndef SCAML_HOST_EMUL
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off));
#endif
  return x;
}
SF_DEV bool sf_finite(double x) { return x - x == 0.0; }

// sum over the tile axis of part (tiles, P), variable by variable.  Device: the wave's 64 lanes are 64 / PP streams of PP >= P
// lanes (PP a power of two); stream j adds tiles j, j + 64 / PP, ... and the streams are folded by a butterfly -- a fixed order.
SF_DEV void sf_tile_sums(const double* part, int tiles, int P, int lane, double* ts) {
#ifndef SCAML_HOST_EMUL
  int PP = 1;
  while (PP < P) PP <<= 1;
  const int i = lane & (PP - 1), j = lane / PP, ns = SF_LANES / PP;
  double s = 0.0;
  if (i < P) {
    for (int t = j; t < tiles; t += ns) s += part[(size_t)t * P + i];
  }
  for (int off = PP; off < SF_LANES; off <<= 1) s += __shfl_xor(s, off);
  ts[0] = s;
#else
  SF_FOR(i) {
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += part[(size_t)t * P + i];
    ts[SF_AT(i)] = s;
  }
#endif
}

// Objective of one problem at the point (theta, raw) the fit was run at; returns f, the lane's components of df / d raw in g.
// A fit that did not succeed (info != 0) has no value: f is NaN and the gradient zero.
SF_DEV double sf_objective(const HyperSpec& sp, double mll, int info, const double* part, int tiles, const double* theta,
                           const double* raw, int n, int D, int lane, double* g) {
  const int P = D + 2;
  const double nf = n < 1 ? 1.0 : (double)n;
  double ts[SF_NV];
  sf_tile_sums(part, tiles, P, lane, ts);
  double lp = 0.0;
  SF_FOR(i) {
    const HyperVar v = hyper_var(sp, i, D);
    const double th = theta[i], s = interval_sigmoid(raw[i]);
    lp += prior_logp(v.prior, th);
    const double dmll = ts[SF_AT(i)] / (2.0 * nf);
    g[SF_AT(i)] = -(dmll + prior_dlogp(v.prior, th) / nf) * interval_slope(v, s);
  }
  lp = sf_sum(lp);
  if (info != 0) {
    SF_FOR(i) g[SF_AT(i)] = 0.0;
    return NAN;
  }
  return -(mll + lp / nf);
}

struct SfResult {
  double f;
  int it, n_eval, status;
};

// Start of a fit: the caller's point is the accepted point and the first trial; nothing has been evaluated.
SF_DEV SfResult sf_reset(double* st, const double* z, int P, int H, int lane) {
  double *x = st, *xt = st + 3 * (size_t)P, *sc = st + (size_t)(4 + 2 * H) * P + H;
  SF_FOR(i) {
    x[i] = z[i];
    xt[i] = z[i];
  }
  if (lane == 0) {
    for (int k = 0; k < STACK_FIT_SCALARS; ++k) sc[k] = 0.0;
  }
  return SfResult{0.0, 0, 0, 0};
}

// One evaluation (ft, gt) at the trial point st.xt arrives: hyper.batched_lbfgs for this problem alone.  Leaves the next point to
// evaluate in st.xt -- the accepted point once the problem has finished (status != 0).
SF_DEV SfResult sf_advance(double* st, int P, int H, int max_iter, int max_ls, double gtol, double ftol, double c1, int lane, double ft,
                           const double* gt) {
  double *x = st, *g = st + P, *d = st + 2 * (size_t)P, *xt = st + 3 * (size_t)P;
  double *S = st + 4 * (size_t)P, *Y = S + (size_t)H * P, *rho = Y + (size_t)H * P, *sc = rho + H;
  double f = sc[SF_F], t = sc[SF_T], gd = sc[SF_GD];
  int it = (int)sc[SF_IT], n_eval = (int)sc[SF_NEVAL], status = (int)sc[SF_STATUS], ls = (int)sc[SF_LS], hist = (int)sc[SF_HIST],
      head = (int)sc[SF_HEAD];
  const int phase = (int)sc[SF_PHASE];
  if (status != 0) return SfResult{f, it, n_eval, status};   // finished: xt already is the accepted point
  ++n_eval;
  double nbad = 0.0;
  SF_FOR(i) nbad += sf_finite(gt[SF_AT(i)]) ? 0.0 : 1.0;
  const bool finite = sf_finite(ft) && sf_sum(nbad) == 0.0;
  bool new_dir = false;
  int new_slot = -1;     // (a pair pushed in this call: its rho is not read back from memory, another lane wrote it)
  double new_rho = 0.0;
  if (phase == 0) {
    if (!finite) {
      f = INFINITY;
      SF_FOR(i) g[i] = 0.0;
      status = 4;
    } else {
      f = ft;
      SF_FOR(i) g[i] = gt[SF_AT(i)];
      if (max_iter < 1) status = 5;
      else new_dir = true;
    }
  } else if (finite && ft <= f + c1 * t * gd) {
    double sy = 0.0, ss = 0.0, yy = 0.0, gmax = 0.0;
    SF_FOR(i) {
      const double sv = xt[i] - x[i], yv = gt[SF_AT(i)] - g[i];
      sy += sv * yv;
      ss += sv * sv;
      yy += yv * yv;
      gmax = fmax(gmax, fabs(gt[SF_AT(i)]));
    }
    sy = sf_sum(sy);
    ss = sf_sum(ss);
    yy = sf_sum(yy);
    gmax = sf_max(gmax);
    const bool push = sy > 1e-10 * sqrt(yy) * sqrt(ss);
    SF_FOR(i) {
      if (push) {
        S[(size_t)head * P + i] = xt[i] - x[i];
        Y[(size_t)head * P + i] = gt[SF_AT(i)] - g[i];
      }
      x[i] = xt[i];
      g[i] = gt[SF_AT(i)];
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
    if (gmax <= gtol) status = 1;
    else if (rel <= ftol && it > 1) status = 2;
    else if (it >= max_iter) status = 5;
    else new_dir = true;
  } else {
    if (++ls >= max_ls) status = 3;   // line search exhausted: the problem stops where it is
    else t *= 0.5;
  }
  if (new_dir) {
    ++it;
    ls = 0;
    // two-loop recursion, newest pair first (pair h lives in slot (head - 1 - h) mod H)
    double q[SF_NV], al[STACK_FIT_HMAX];
    SF_FOR(i) q[SF_AT(i)] = g[i];
#pragma unroll
    for (int h = 0; h < STACK_FIT_HMAX; ++h) {
      if (h < hist) {
        const int slot = (head - 1 - h + 2 * H) % H;
        const double r = slot == new_slot ? new_rho : rho[slot];
        double sq = 0.0;
        SF_FOR(i) sq += S[(size_t)slot * P + i] * q[SF_AT(i)];
        al[h] = r * sf_sum(sq);
        SF_FOR(i) q[SF_AT(i)] -= al[h] * Y[(size_t)slot * P + i];
      }
    }
    double gamma = 1.0;
    if (hist > 0) {
      const int slot = (head - 1 + H) % H;
      double ys = 0.0, yy = 0.0;
      SF_FOR(i) {
        const double yv = Y[(size_t)slot * P + i];
        ys += S[(size_t)slot * P + i] * yv;
        yy += yv * yv;
      }
      ys = sf_sum(ys);
      yy = sf_sum(yy);
      if (yy > 0.0) gamma = ys / fmax(yy, 1e-300);
    }
    SF_FOR(i) q[SF_AT(i)] *= gamma;
#pragma unroll
    for (int h = STACK_FIT_HMAX - 1; h >= 0; --h) {
      if (h < hist) {
        const int slot = (head - 1 - h + 2 * H) % H;
        const double r = slot == new_slot ? new_rho : rho[slot];
        double yr = 0.0;
        SF_FOR(i) yr += Y[(size_t)slot * P + i] * q[SF_AT(i)];
        const double b = r * sf_sum(yr);
        SF_FOR(i) q[SF_AT(i)] += (al[h] - b) * S[(size_t)slot * P + i];
      }
    }
    double gq = 0.0, gg = 0.0;
    SF_FOR(i) {
      gq += g[i] * q[SF_AT(i)];
      gg += g[i] * g[i];
    }
    gd = -sf_sum(gq);
    gg = sf_sum(gg);
    // not a descent direction (or no pair yet): steepest descent, the first step scaled like scipy's
    const bool bad_dir = !(gd < 0.0);
    if (bad_dir) gd = -gg;
    SF_FOR(i) d[i] = bad_dir ? -g[i] : -q[SF_AT(i)];
    t = (hist > 0 && !bad_dir) ? 1.0 : fmin(1.0, 1.0 / fmax(sqrt(gg), 1e-12));
  }
  SF_FOR(i) xt[i] = status == 0 ? x[i] + t * d[i] : x[i];
  if (lane == 0) {
    sc[SF_F] = f; sc[SF_T] = t; sc[SF_GD] = gd; sc[SF_IT] = it; sc[SF_NEVAL] = n_eval; sc[SF_STATUS] = status;
    sc[SF_LS] = ls; sc[SF_HIST] = hist; sc[SF_HEAD] = head; sc[SF_PHASE] = 1.0;
  }
  return SfResult{f, it, n_eval, status};
}

// The whole step of problem `b`.  (A lane reads back only what it wrote itself in this launch -- its components of x, xt -- or what
// an earlier launch left in the state.)
SF_DEV void sf_step(const StackFitParams& p, int b, int lane) {
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
  SF_FOR(i) {
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
