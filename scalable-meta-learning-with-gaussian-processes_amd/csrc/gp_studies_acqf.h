// gp_studies_acqf.h -- the batched target acquisition of many BO studies (include/scaml_gp.h (7g)): argument block, LDS footprint and
// the arithmetic of one block of right-hand sides, sa_block<R>.  One source for both device kernels (csrc/gp_studies_acqf.hip: a
// workgroup per query point, R = 1; csrc/gp_studies_score.hip: a workgroup per strip of 16 candidates, R = 16, value only (7i)), the
// host launcher and the single-threaded host build the CPU tests check against torch (any compiler but hipcc: tests/host_emul).
//
// Per query point q of group g (a study: its weights, target kernel, training inputs, cached factor of Knn, alpha, standardiser):
//   S_mu[c]  = sum_t w_t   mu[t][q][c],   S_var[c] = sum_t w_t^2 var[t][q][c],   C[a][c] = sum_t w_t^2 cov[t][a][16 q + c]
//              over the active tasks, t = 0 .. T-1 in order, for the 16 columns c of the GRAD pass and the n_g training points a
//   Knq[a]   = C[a][0] / s^2 + os k_t(x_a, x_q),      dKnq[a][d] = C[a][1 + d] / s^2 + d/dx_d os k_t(x_a, x_q)
//   z        = Knn^-1 Knq from the cached factor (blocked substitution with the 16 x 16 inverses of L's diagonal blocks)
//   mu*      = m + s ((S_mu[0] - m) / s + Knq . alpha),   var* = s^2 (S_var[0] / s^2 + os - Knq . z)
//   dmu*[d]  = S_mu[1 + d] + s sum_a alpha_a dKnq[a][d],   dvar*[d] = S_var[1 + d] - 2 s^2 sum_a z_a dKnq[a][d]
//   UCB / EI and their chain rule with the clamps of scamlgp_amd/utils.py (sa_acquisition, which csrc/gp_fantasy.hip calls for F fantasies).
// Every sum runs in a fixed order (tasks ascending, training points ascending) by ONE thread per output: no atomics, no wave
// reductions, so the result is a pure function of the inputs and the host build computes what the device computes.
//
// Studies with pending evaluations (include/scaml_gp.h (7k)): the block's argument type is the second template parameter.  With
// StudiesFantasyParams a group is a fantasy model (ScaMLGP.fantasize) of F_g fantasies: phases 1 and 2 are the text above, the alpha
// load, phase 3 and phase 4 differ at `if constexpr (FANT)`, where UCB / EI are averaged over the group's columns of alpha_f with
// (7f)'s formula (sa_fantasy_tail).  A group with F_g == 1 takes the statements of the ordinary block.
#pragma once
#include <type_traits>
#include "gp_studies_formulas.h"   // SA_DEV / SA_SYNC, sa_kernel_and_slope, sa_acquisition

namespace scaml {

constexpr int STUDIES_ACQF_MAX_N = 96;   // training points per study (the GRAD pass's covariance block)
constexpr int STUDIES_ACQF_MAX_D = 15;   // (its 16 columns per query point)
constexpr int STUDIES_ACQF_THREADS = 256;

struct StudiesAcqfParams {
  const double* mu;           // (T, Mq, 16)          GRAD-pass outputs of the source stack, all tasks
  const double* var;          // (T, Mq, 16)
  const double* cov;          // (T, n_max, Mq * 16)  rows a < n_g of query q's strip are read
  const int32_t* group;       // (Mq) study of a query point; negative: padding (zeros come out)
  const double* Xq;           // (Mq, D)
  const double* w;            // (G, T) weights, zero where pruned
  const uint8_t* active;      // (G, T) a masked task is skipped, not multiplied by zero
  const double* Xt;           // (G, n_max, D) training inputs
  const double* theta;        // (G, D + 2) target kernel: lengthscales, outputscale, noise
  const double* L;            // (G, n_max, n_max) factor of Knn, row stride n_max, the leading n_g x n_g block
  const double* Linv_diag;    // (G, ceil(n_max / 16), 16, 16) inverses of its diagonal blocks
  const double* alpha;        // (G, n_max) Knn^-1 resid
  const int32_t* n_points;    // (G) 1 <= n_g <= n_max
  const double* m_all;        // (G)
  const double* s_all;        // (G) > 0
  const int32_t* info;        // (G) != 0: the study's factorisation failed, its outputs are NaN
  const double* acqf_param;   // (G) UCB: beta; EI: best_f
  double* value;              // (Mq)
  double* grad;               // (Mq, D) or NULL
  double* mu_out;             // (Mq) or NULL: the target posterior mean (original units)
  double* var_out;            // (Mq) or NULL: its variance
  int Mq, G, n_max, T, D, kind, acqf, pad_;
};

// The block of a launch in which studies hold pending evaluations: (7g)'s block and, per group, the F_g columns of alpha that its
// fantasies differ in.  `alpha` of the base block is not read.
constexpr int STUDIES_FANTASY_MAX_F = 64;   // fantasies per study (csrc/gp_fantasy_params.h has the same limit for (7f))
struct StudiesFantasyParams : StudiesAcqfParams {
  const double* alpha_f;      // (G, n_max, F_max) Knn^-1 [resid_0 .. resid_{F_g - 1}]: row a of group g holds its F_g values contiguously
  const int32_t* n_fant;      // (G) 1 <= F_g <= F_max; 1: an ordinary model, alpha_f[g, :, 0] is its alpha
  int F_max, pad2_;
};

// LDS of one block of R right-hand sides, in doubles:
//   C [n_max][16] | S_mu, S_var [32] | u, v [2][np * R] | alpha [np] | W [nb][256] | L [n_max][n_max | 1] | red [R == 1 ? 48 : 32]
template <int R>
constexpr size_t sa_lds_doubles(int n_max) {
  const size_t nb = (size_t)(n_max + 15) / 16, np = nb * 16;
  return (size_t)n_max * 16 + 32 + 2 * np * R + np + nb * 256 + (size_t)n_max * (size_t)(n_max | 1) + (R == 1 ? 48 : 32);
}
constexpr size_t studies_acqf_lds_doubles(int n_max) { return sa_lds_doubles<1>(n_max); }
// ... and of a block with fantasies: the above, then (alpha_f stays in global memory: at n_max = 96, F_max = 64 it alone is 6,144 doubles)
//   R == 1:  A, Amu, Av [3][F_max] | abar [np] | sum_f A, Amu, Av [4]        R == 16:  r_f, then A_f [16][F_max]
template <int R>
constexpr size_t sa_fantasy_lds_doubles(int n_max, int F_max) {
  const size_t np = ((size_t)(n_max + 15) / 16) * 16;
  return sa_lds_doubles<R>(n_max) + (R == 1 ? 3 * (size_t)F_max + np + 4 : 16 * (size_t)F_max);
}

// a count of fantasies outside 1 .. F_max turns the group's outputs into NaN; the ordinary block has none to refuse
SA_DEV bool sa_fantasies_refused(const StudiesAcqfParams&, int) { return false; }
SA_DEV bool sa_fantasies_refused(const StudiesFantasyParams& p, int F) { return F < 1 || F > p.F_max; }

// One block `blk` of R right-hand sides of one study by `nthr` cooperating threads (thread `tid`; SA_SYNC between the phases).
// `lds`: sa_lds_doubles<R>(n_max).  The two instantiations are the two layouts of the grouped source pass:
//   R = 1   a query point in the 16-column GRAD layout: mu, var (T, Mq, 16), cov (T, n_max, Mq * 16), group (Mq) per query.  Column 0
//           is the right-hand side, columns 1 .. 15 of C are the gradient columns that ride along; `grad` is written where given.
//   R = 16  a strip of 16 candidates in the value layout: mu, var (T, Mq), cov (T, n_max, Mq), group (Mq / 16) per strip, Mq a
//           multiple of 16.  The 16 columns of C are 16 right-hand sides against ONE copy of the factor; `grad` is not used.
// Either way a block owns 16 consecutive columns of a source row and C is [a][16]; element e of an [.][R] array is (e / R, e % R).
// `Params`: StudiesAcqfParams, or StudiesFantasyParams (`lds`: sa_fantasy_lds_doubles<R>(n_max, F_max)) -- the sites that differ are
// the refusal of a bad F_g, the alpha load and, for a group with F_g > 1, phases 3 and 4.
template <int R, class Params>
SA_DEV void sa_block(const Params& p, double* lds, int blk, int tid, int nthr) {
  static_assert(R == 1 || R == 16, "a query point with its gradient columns, or a strip of 16 candidates");
  constexpr bool FANT = std::is_same<Params, StudiesFantasyParams>::value;
  static_assert(FANT || std::is_same<Params, StudiesAcqfParams>::value, "one of the two argument blocks");
  const int D = p.D, T = p.T, n_max = p.n_max;
  const int g = p.group[blk];
  const size_t q0 = (size_t)blk * R;   // the block's first output
  const double nan = NAN;
  // (every branch up to the first barrier is uniform over the workgroup)
  if (g < 0 || g >= p.G) {   // padding
    for (int c = tid; c < R; c += nthr) {
      p.value[q0 + c] = 0.0;
      if (p.mu_out) p.mu_out[q0 + c] = 0.0;
      if (p.var_out) p.var_out[q0 + c] = 0.0;
    }
    if constexpr (R == 1)
      if (p.grad) for (int d = tid; d < D; d += nthr) p.grad[q0 * D + d] = 0.0;
    return;
  }
  const int n = p.n_points[g];
  [[maybe_unused]] int F = 1;   // the group's fantasies, 1 .. F_max
  if constexpr (FANT) F = p.n_fant[g];
  if (p.info[g] != 0 || n < 1 || n > n_max || sa_fantasies_refused(p, F)) {
    for (int c = tid; c < R; c += nthr) {
      p.value[q0 + c] = nan;
      if (p.mu_out) p.mu_out[q0 + c] = nan;
      if (p.var_out) p.var_out[q0 + c] = nan;
    }
    if constexpr (R == 1)
      if (p.grad) for (int d = tid; d < D; d += nthr) p.grad[q0 * D + d] = nan;
    return;
  }
  const int nbm = (n_max + 15) / 16, np = nbm * 16, nb = (n + 15) / 16, ldl = n_max | 1;
  double* C = lds;                          // [a][16]: Knq in columns c < R, then (R = 1) dKnq in columns 1 + d
  double* Ssum = C + (size_t)n_max * 16;    // S_mu [16] | S_var [16]
  double* u = Ssum + 32;                    // [a][R]
  double* v = u + (size_t)np * R;
  double* al = v + (size_t)np * R;
  double* Wd = al + np;
  double* Ls = Wd + (size_t)nbm * 256;
  double* red = Ls + (size_t)n_max * ldl;   // Knq . alpha [R] | Knq . z [R]; R = 1: then sum_a alpha_a dKnq [2 + d], sum_a z_a dKnq [18 + d]

  const double s = p.s_all[g], m = p.m_all[g], s2 = s * s, inv_s2 = 1.0 / s2;
  const double* th = p.theta + (size_t)g * (D + 2);
  const double os = th[D];
  const double* wg = p.w + (size_t)g * T;
  const uint8_t* ag = p.active + (size_t)g * T;
  const size_t W = (size_t)p.Mq * (R == 1 ? 16 : 1), col0 = (size_t)blk * 16;   // a source row, the block's 16 columns in it

  // ---- phase 1: the weighted task sums (eight tasks' loads in flight; a row's 16 columns are 128 consecutive bytes), the factor,
  // its block inverses and alpha into LDS
  for (int e = tid; e < n * 16 + 32; e += nthr) {
    const bool is_cov = e < n * 16;
    const int a = e >> 4, c = e & 15;
    const int which = (e - n * 16) >> 4;   // 0: mu, 1: var
    const double* src = is_cov ? p.cov + (size_t)a * W + col0 + c : (which == 0 ? p.mu : p.var) + col0 + c;
    const size_t tstride = is_cov ? (size_t)n_max * W : W;
    const bool lin = !is_cov && which == 0;
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += 8) {
      double val[8], cf[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = t0 + k;
        const bool ok = t < T && ag[t];   // (a masked task is skipped, not multiplied by zero: its values may be NaN)
        val[k] = ok ? src[(size_t)t * tstride] : 0.0;
        const double wt = ok ? wg[t] : 0.0;
        cf[k] = lin ? wt : wt * wt;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(cf[k], val[k], acc);
    }
    if (is_cov) C[e] = acc * inv_s2;
    else Ssum[e - n * 16] = acc;
  }
  {
    const double* Lg = p.L + (size_t)g * n_max * n_max;
    for (int e = tid; e < n * n; e += nthr) {
      const int i = e / n, j = e - i * n;
      if (j <= i) Ls[(size_t)i * ldl + j] = Lg[(size_t)i * n_max + j];
    }
    const double* Wg = p.Linv_diag + (size_t)g * nbm * 256;
    for (int e = tid; e < nb * 256; e += nthr) Wd[e] = Wg[e];
    if constexpr (FANT) {   // column 0: all there is of a group with F_g == 1 (a group with more reads alpha_f where it is, not `al`)
      if (F == 1)
        for (int a = tid; a < n; a += nthr) al[a] = p.alpha_f[((size_t)g * n_max + a) * p.F_max];
    } else {
      for (int a = tid; a < n; a += nthr) al[a] = p.alpha[(size_t)g * n_max + a];
    }
  }
  SA_SYNC();
  // ---- phase 1b: the target kernel's part of Knq and (R = 1) of its input gradient, one slope evaluation per (training point, rhs)
  for (int e = tid; e < n * R; e += nthr) {
    const int a = e / R, c = e % R;
    const double* xa = p.Xt + ((size_t)g * n_max + a) * D;
    const double* xq = p.Xq + (q0 + c) * D;
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (xq[d] - xa[d]) / th[d];
      d2 = fma(df, df, d2);
    }
    double k0, dk;
    sa_kernel_and_slope(p.kind, d2, os, k0, dk);
    double* Ca = C + (size_t)a * 16;
    Ca[c] += k0;
    if constexpr (R == 1)
      for (int d = 0; d < D; ++d) Ca[1 + d] += 2.0 * dk * ((xq[d] - xa[d]) / (th[d] * th[d]));
    u[e] = Ca[c];
  }
  SA_SYNC();
  // ---- phase 2: z = Knn^-1 Knq, R right-hand sides.  Forward L y = Knq by block rows: y_kb = W_kb u_kb, then
  // u_i -= L[i, kb] y_kb below the block
  for (int kb = 0; kb < nb; ++kb) {
    const int r0 = 16 * kb, cnt = n - r0 < 16 ? n - r0 : 16;
    for (int e = tid; e < cnt * R; e += nthr) {
      const int r = e / R, c = e % R;
      double acc = 0.0;
      for (int k = 0; k <= r; ++k) acc = fma(Wd[kb * 256 + r * 16 + k], u[(r0 + k) * R + c], acc);
      v[(r0 + r) * R + c] = acc;
    }
    SA_SYNC();
    for (int e = (r0 + 16) * R + tid; e < n * R; e += nthr) {
      const int i = e / R, c = e % R;
      double acc = u[e];
      for (int k = 0; k < 16; ++k) acc = fma(-Ls[(size_t)i * ldl + r0 + k], v[(r0 + k) * R + c], acc);
      u[e] = acc;
    }
    SA_SYNC();
  }
  // backward L^T z = y (y in v, z into u): z_kb = W_kb^T v_kb, then v_i -= L[kb, i]^T z_kb above the block
  for (int kb = nb - 1; kb >= 0; --kb) {
    const int r0 = 16 * kb, cnt = n - r0 < 16 ? n - r0 : 16;
    for (int e = tid; e < cnt * R; e += nthr) {
      const int r = e / R, c = e % R;
      double acc = 0.0;
      for (int k = r; k < cnt; ++k) acc = fma(Wd[kb * 256 + k * 16 + r], v[(r0 + k) * R + c], acc);
      u[(r0 + r) * R + c] = acc;
    }
    SA_SYNC();
    for (int e = tid; e < r0 * R; e += nthr) {
      const int i = e / R, c = e % R;
      double acc = v[e];
      for (int k = 0; k < cnt; ++k) acc = fma(-Ls[(size_t)(r0 + k) * ldl + i], u[(r0 + k) * R + c], acc);
      v[e] = acc;
    }
    SA_SYNC();
  }
  // ---- phases 3 and 4 of a fantasy model with F > 1 fantasies (uniform over the workgroup): (7f)'s formula on this block's Knq, dKnq
  // and z.  Every sum by one thread, a ascending, f ascending:
  //   r_f = sum_a alpha_f[a][f] Knq[a],  mu_f = fma(s, mean_q + r_f, m),  vr = s^2 (var_q - Knq . z),  (A_f, Amu_f, Av_f) = sa_acquisition
  //   value = (sum_f A_f) / F;  R = 1: sAmu = sum_f Amu_f, sAv = sum_f Av_f, abar[a] = sum_f Amu_f alpha_f[a][f],
  //   gm[d] = sum_a abar[a] dKnq[a][d], gv[d] = sum_a z[a] dKnq[a][d],
  //   grad[d] = fma(sAv, fma(-2 s^2, gv[d], S_var[1 + d]), fma(s, gm[d], sAmu S_mu[1 + d])) / F
  // LogEI (acqf & SA_ACQF_LOG): value = log((sum_f exp A_f) / F) and Amu_f, Av_f weighted by exp A_f / sum_f' exp A_f' in place of the 1 / F.
  if constexpr (FANT) {
    if (F > 1) {
      const int Fm = p.F_max, nr = R * F;
      const double* af = p.alpha_f + (size_t)g * n_max * Fm;   // row a at af + a * Fm, read where it is: columns f < F of rows a < n
      double* fA = red + (R == 1 ? 48 : 32);   // [c][F]: r_f, then A_f
      double* fAmu = fA + Fm;                  // (R = 1) [F]
      double* fAv = fAmu + Fm;                 //         [F]
      double* abar = fAv + Fm;                 //         [np]
      double* fsum = abar + np;                //         sum_f A_f | Amu_f | Av_f
      // phase 3: fA[c][f] = r_f of right-hand side c, eight rows of alpha_f in flight (consecutive threads, consecutive f);
      // red[R + c] = Knq . z; R = 1: red[18 + d] = sum_a z_a dKnq[a][d]
      for (int o = tid; o < nr + R + (R == 1 ? D : 0); o += nthr) {
        if (o < nr) {
          const int c = o / F, f = o - c * F;
          double acc = 0.0;
          for (int a0 = 0; a0 < n; a0 += 8) {
            double av[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) av[k] = a0 + k < n ? af[(size_t)(a0 + k) * Fm + f] : 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (a0 + k < n) acc = fma(av[k], C[(size_t)(a0 + k) * 16 + c], acc);
          }
          fA[o] = acc;
        } else {
          const int og = o - nr;   // R = 16: the right-hand side; R = 1: 0 for Knq . z, 1 + d for the gradient column d
          const int c = R == 1 ? 0 : og, col = og;
          double acc = 0.0;
          for (int a = 0; a < n; ++a) acc = fma(u[a * R + c], C[(size_t)a * 16 + col], acc);
          red[R == 1 ? (og == 0 ? 1 : 17 + og) : R + c] = acc;
        }
      }
      SA_SYNC();
      // phase 4a: one thread per (right-hand side, fantasy)
      const double par = p.acqf_param[g];
      for (int e = tid; e < nr; e += nthr) {
        const int c = e / F;
        const double mean_q = (Ssum[c] - m) / s, var_q = Ssum[16 + c] * inv_s2 + os;
        const double mu = fma(s, mean_q + fA[e], m);
        const double vr = s2 * (var_q - red[R + c]);
        double A, Amu, Av;
        sa_acquisition(p.acqf, par, mu, vr, A, Amu, Av);
        fA[e] = A;
        if constexpr (R == 1) {
          fAmu[e] = Amu;
          fAv[e] = Av;
        }
      }
      SA_SYNC();
      // LogEI: the average in the log domain, log((sum_f exp l_f) / F) of the l_f = A_f:
      //   mx = max_f l_f,  e_f = exp(l_f - mx),  S = sum_f e_f (f ascending),  value = mx + log S - log F,  w_f = e_f / S;
      //   R = 1: Amu_f, Av_f *= w_f
      // mx by one thread per right-hand side into red[c] (free in this branch); e_f by one thread per (right-hand side, fantasy), in
      // place of l_f; then, R = 1, every thread f sums S for itself (the same F additions in the same order: the same bits) and
      // weights its own factors, and thread f = 0 leaves the value in red[c].  Phase 4b sums the weighted factors and divides by 1.
      const bool logdom = (p.acqf & SA_ACQF_LOG) != 0;   // (uniform over the launch)
      if (logdom) {
        for (int c = tid; c < R; c += nthr) {
          const double* l = fA + c * F;
          double mx = l[0], any = 0.0;   // (the comparisons drop a NaN l_f: l - l puts it back, and with it NaN into every output)
          for (int f = 1; f < F; ++f) mx = l[f] > mx ? l[f] : mx;
          for (int f = 0; f < F; ++f) any += l[f] - l[f];
          red[c] = mx + any;
        }
        SA_SYNC();
        for (int e = tid; e < nr; e += nthr) fA[e] = exp(fA[e] - red[e / F]);
        SA_SYNC();
        for (int e = tid; e < nr; e += nthr) {
          const int c = e / F, f = e - c * F;
          if (R == 16 && f != 0) continue;
          const double* ex = fA + c * F;
          double S = 0.0;
          for (int k = 0; k < F; ++k) S += ex[k];
          if constexpr (R == 1) {
            const double wf = ex[f] / S;
            fAmu[f] *= wf;
            fAv[f] *= wf;
          }
          if (f == 0) red[c] = red[c] + log(S) - log((double)F);
        }
        SA_SYNC();
      }
      const double Fdiv = logdom ? 1.0 : (double)F;
      // phase 4b: the averages, one thread per right-hand side; R = 1 with a gradient: and one per training point for abar
      for (int e = tid; e < (R == 1 ? 1 + (p.grad ? n : 0) : R); e += nthr) {
        if (R == 16 || e == 0) {
          const int c = R == 1 ? 0 : e;
          double sA = 0.0;
          if (logdom) sA = red[c];
          else for (int f = 0; f < F; ++f) sA += fA[c * F + f];
          if constexpr (R == 1) {
            double sAmu = 0.0, sAv = 0.0;
            for (int f = 0; f < F; ++f) sAmu += fAmu[f];
            for (int f = 0; f < F; ++f) sAv += fAv[f];
            fsum[0] = sA;
            fsum[1] = sAmu;
            fsum[2] = sAv;
          }
          double bad = 0.0;   // (the rule of phase 4 below: a NaN / inf coordinate makes every output of THAT point NaN)
          for (int d = 0; d < D; ++d) {
            const double x = p.Xq[(q0 + c) * D + d];
            bad += x - x;
          }
          p.value[q0 + c] = bad == 0.0 ? sA / Fdiv : bad;
        } else {
          const int a = e - 1;
          double acc = 0.0;
          for (int f = 0; f < F; ++f) acc = fma(fAmu[f], af[(size_t)a * Fm + f], acc);
          abar[a] = acc;
        }
      }
      if constexpr (R == 1) {
        if (p.grad) {
          SA_SYNC();
          // phase 4c: one thread per input dimension
          for (int o = tid; o < D; o += nthr) {
            double gm = 0.0;
            for (int a = 0; a < n; ++a) gm = fma(abar[a], C[(size_t)a * 16 + 1 + o], gm);
            double bad = 0.0;
            for (int d = 0; d < D; ++d) {
              const double x = p.Xq[q0 * D + d];
              bad += x - x;
            }
            const double dmu = fma(s, gm, fsum[1] * Ssum[1 + o]);
            const double dvar = fma(-2.0 * s2, red[18 + o], Ssum[17 + o]);
            p.grad[q0 * D + o] = bad == 0.0 ? fma(fsum[2], dvar, dmu) / Fdiv : bad;
          }
        }
      }
      return;
    }
  }
  // ---- phase 3: the contractions over the training points, one thread per output, a = 0 .. n-1 in order
  //   red[c] = Knq . alpha, red[R + c] = Knq . z; R = 1: red[2 + d] = sum_a alpha_a dKnq[a][d], red[18 + d] = sum_a z_a dKnq[a][d]
  for (int o = tid; o < 2 * R + (R == 1 ? 2 * D : 0); o += nthr) {
    const bool grad_col = R == 1 && o >= 2;
    const int og = o - 2;
    const bool with_alpha = grad_col ? og < D : o < R;
    const int c = grad_col ? 0 : o % R, col = grad_col ? 1 + (og < D ? og : og - D) : c;
    double acc = 0.0;
    for (int a = 0; a < n; ++a) acc = fma(with_alpha ? al[a] : u[a * R + c], C[(size_t)a * 16 + col], acc);
    red[grad_col ? (og < D ? 2 + og : 18 + (og - D)) : o] = acc;
  }
  SA_SYNC();
  // ---- phase 4: the posterior, the acquisition value and (R = 1) its chain rule: one thread per right-hand side, or per input
  // dimension of the one (every writing thread restates the scalars)
  for (int e = tid; e < (R == 1 ? (D > 1 ? D : 1) : R); e += nthr) {
    const int c = R == 1 ? 0 : e, o = R == 1 ? e : 0;
    const double mean_q = (Ssum[c] - m) / s, var_q = Ssum[16 + c] * inv_s2 + os;
    const double mu = fma(s, mean_q + red[c], m);
    const double vr = s2 * (var_q - red[R + c]);
    const double par = p.acqf_param[g];
    double A, Amu, Av;
    sa_acquisition(p.acqf, par, mu, vr, A, Amu, Av);
    // a query point with a NaN / inf coordinate: fmax in the Matern branch drops a NaN operand, so only that coordinate's slope
    // would carry it (and nothing at all with source sums that happen to be finite).  sum_d (x_d - x_d) is 0, or NaN for such a
    // point: every output of THAT point is NaN, as (5d)'s target gradient has it (a select: finite inputs are untouched)
    double bad = 0.0;
    for (int d = 0; d < D; ++d) {
      const double x = p.Xq[(q0 + c) * D + d];
      bad += x - x;
    }
    if (o == 0) {
      p.value[q0 + c] = bad == 0.0 ? A : bad;
      if (p.mu_out) p.mu_out[q0 + c] = bad == 0.0 ? mu : bad;
      if (p.var_out) p.var_out[q0 + c] = bad == 0.0 ? vr : bad;
    }
    if constexpr (R == 1)
      if (p.grad && o < D) {
        const double dmu = fma(s, red[2 + o], Ssum[1 + o]);
        const double dvar = fma(-2.0 * s2, red[18 + o], Ssum[17 + o]);
        p.grad[q0 * D + o] = bad == 0.0 ? fma(Av, dvar, Amu * dmu) : bad;
      }
  }
}

// One query point (7g): the R = 1 instantiation.
SA_DEV void sa_query(const StudiesAcqfParams& p, double* lds, int q, int tid, int nthr) { sa_block<1>(p, lds, q, tid, nthr); }

// The same two layouts for studies with pending evaluations (7k): a query point, a strip of 16 candidates.
SA_DEV void sa_fantasy_query(const StudiesFantasyParams& p, double* lds, int q, int tid, int nthr) { sa_block<1>(p, lds, q, tid, nthr); }
SA_DEV void sa_fantasy_strip(const StudiesFantasyParams& p, double* lds, int strip, int tid, int nthr) { sa_block<16>(p, lds, strip, tid, nthr); }

}  // namespace scaml
