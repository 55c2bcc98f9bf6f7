// gp_fantasy.hip — the acquisition function of a fantasy model (ScaMLGP.fantasize), averaged over its F fantasies, and its exact
// input gradient, in one launch (gfx950).
//
// A fantasy model is the target GP conditioned on p pending points with F sampled outcomes each (the "integrated acquisition"
// over pending evaluations of Snoek et al., 2012).  All F models share the training block Knn, its factor, the cross block Knq and
// Z = Knn^-1 Knq; only alpha_f = Knn^-1 r_f differs.  So per query point q:
//   mu_f(q)  = m + s (mean_q[q] + Knq[:, q] . alpha[:, f])
//   v(q)     = s^2 (var_q[q] - Knq[:, q] . Z[:, q] + noise_add)        (the same for every f)
//   value(q) = (1/F) sum_f A(mu_f(q), v(q))        LogEI: log((1/F) sum_f exp A(mu_f(q), v(q))), A = log EI
// with A the UCB (-mu + sqrt(beta v)) or EI (sigma (phi(u) + u Phi(u)), sigma = sqrt(max(v, 1e-9)), u = -(mu - best_f) / sigma) of
// scamlgp_amd/utils.py, same clamps.  The gradient uses
//   sum_f A_mu,f grad mu_f = (sum_f A_mu,f) grad mu_prior + s sum_a (sum_f A_mu,f alpha[a, f]) grad k_a
// so the contraction over the training points runs once per query with the weighted column abar = sum_f A_mu,f alpha[:, f], as in
// scaml_target_grad_kernel (csrc/gp_posterior.hip), never once per fantasy; no (F, M) or (F, M, D) tensor reaches memory.
//
// One wave per query point.  Lanes = training points to stage Knq[:, q] in LDS and reduce Knq . Z; lanes = fantasies for mu_f (every
// lane reads the same Knq element from LDS, its own element of a contiguous row of alpha) and A; three wave reductions; the A_mu,f go
// to LDS; lanes = training points again for abar and the kernel slopes (one slope evaluation serves all D dimensions).
#include "scaml_common.hpp"
#include "gp_fantasy_params.h"
#include "gp_studies_formulas.h"   // sa_acquisition: the one statement of UCB / EI and their chain-rule factors

namespace {

__device__ __forceinline__ double wave_sum_all(double x) {
  return __shfl(scaml::wave_sum_to_lane15(x), 63);   // (the total lands in lanes 15, 31, 47, 63)
}

__device__ __forceinline__ double wave_max_all(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

template <int KIND, bool GRAD>
__device__ __forceinline__ void fantasy_acqf_body(const scaml::FantasyAcqfParams& p) {
  constexpr int DM = 16;
  __shared__ double exptab[64];
  __shared__ double kq[scaml::FANTASY_MAX_N];
  __shared__ double am[scaml::FANTASY_MAX_F];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int n = p.n, M = p.M, F = p.F, D = p.D;
  if (p.info && p.info[0] > 0) {   // not positive definite even with jitter: NaN, like scaml_target_finish_kernel
    if (lane == 0) p.value[q] = __builtin_nan("");
    if (GRAD && lane < D) p.grad[(size_t)q * D + lane] = __builtin_nan("");
    return;
  }
  if (GRAD) scaml::exp2_table_init(exptab, lane);
  // (1) lanes = training points: Knq[:, q] into LDS, Knq[:, q] . Z[:, q]
  double kz = 0.0;
  for (int a = lane; a < n; a += 64) {
    const double k = p.Knq[(size_t)a * M + q];
    kq[a] = k;
    kz = __builtin_fma(k, p.Z[(size_t)a * M + q], kz);
  }
  kz = wave_sum_all(kz);
  __syncthreads();
  const double s = p.s_all, s2 = s * s;
  const double v = s2 * (p.var_q[q] - kz + p.noise_add);
  // (2) lanes = fantasies: mu_f, eight rows of alpha in flight
  const int f = lane;
  const bool live = f < F;
  double mu = p.mean_q[q];
  for (int a0 = 0; a0 < n; a0 += 8) {
    double al[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) al[u] = (live && a0 + u < n) ? p.alpha[(size_t)(a0 + u) * F + f] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) mu = __builtin_fma(a0 + u < n ? kq[a0 + u] : 0.0, al[u], mu);
  }
  mu = __builtin_fma(s, mu, p.m_all);
  double A, Amu, Av;
  scaml::sa_acquisition(p.acqf, p.acqf_param, mu, v, A, Amu, Av);   // UCB / EI with the clamps: csrc/gp_studies_formulas.h
  if (!live) A = Amu = Av = 0.0;
  double invF = 1.0 / F;
  double val;
  if (p.acqf & scaml::SA_ACQF_LOG) {
    // LogEI: the average in the log domain, log((sum_f exp l_f) / F) of the l_f = A.  With mx = max_f l_f and S = sum_f exp(l_f - mx):
    // value = mx + log S - log F, and the chain-rule factors carry the weights w_f = exp(l_f - mx) / S in place of the 1 / F.
    // (F = 1: exp 0 = 1, S = 1, log 1 = 0, w = 1 -- l_0 and its factors bit for bit.  fmax drops a NaN l_f: A - A puts it back.)
    const double mx = wave_max_all(live ? A : -__builtin_inf());
    const double e = live ? exp(A - mx) : 0.0;
    const double S = wave_sum_all(e);
    const double w = e / S;
    Amu *= w;
    Av *= w;
    val = (mx + log(S) - log((double)F)) + wave_sum_all(A - A);
    invF = 1.0;
  } else {
    val = wave_sum_all(A);
  }
  if (lane == 0) p.value[q] = val * invF;
  if (!GRAD) return;
  const double sAmu = wave_sum_all(Amu), sAv = wave_sum_all(Av);
  am[lane] = Amu;
  __syncthreads();
  // a query point with a NaN / inf coordinate: the clamps of kernel_and_slope_scaled are bare v_max / v_min, which drop a NaN operand --
  // only that coordinate's df[d] would carry it, the other D - 1 entries would be the gradient at a nonsense distance; and a NaN value
  // (a NaN column of Knq / Z) leaves UCB's A_mu = -1, A_v = 0 and with them a finite gradient.  val - val and sum_d (x_d - x_d) are 0,
  // or NaN for such a query: every entry of its gradient is NaN where the results are stored, as in scaml_target_grad_kernel (a
  // select: finite inputs stay bit for bit what they were)
  double bad = val - val;
  for (int d = 0; d < D; ++d) {
    const double x = p.Xq[(size_t)q * D + d];
    bad += x - x;
  }
  // (3) lanes = training points: abar_a = sum_f A_mu,f alpha[a, f]; the kernel slopes at (x_a, x_q), once for all D dimensions
  const double os = p.theta[D], inv_s2 = 1.0 / s2;
  const size_t W = (size_t)M * 16, col0 = (size_t)q * 16 + 1;
  double gm[DM], gv[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) gm[d] = gv[d] = 0.0;
  for (int a = lane; a < n; a += 64) {
    double ab = 0.0;
    const double* ar = p.alpha + (size_t)a * F;
    for (int g = 0; g < F; ++g) ab = __builtin_fma(am[g], ar[g], ab);
    double df[DM];
    double d2 = 0.0;
#pragma unroll
    for (int d = 0; d < DM; ++d) {
      df[d] = 0.0;
      if (d < D) {
        const double il = 1.0 / p.theta[d];
        df[d] = (p.Xq[(size_t)q * D + d] - p.Xt[(size_t)a * D + d]) * il;
        d2 = __builtin_fma(df[d], df[d], d2);
        df[d] *= il;   // (x_q - x_a)_d / l_d^2
      }
    }
    double k0, dk;
    scaml::kernel_and_slope_scaled<KIND>(d2, os, exptab, k0, dk);
    const double z = p.Z[(size_t)a * M + q];
    const double* cg = p.cov_g + (size_t)a * W + col0;
#pragma unroll
    for (int d = 0; d < DM; ++d) {
      if (d < D) {
        const double dkn = __builtin_fma(cg[d], inv_s2, 2.0 * dk * df[d]);
        gm[d] = __builtin_fma(ab, dkn, gm[d]);
        gv[d] = __builtin_fma(z, dkn, gv[d]);
      }
    }
  }
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    if (d < D) {
      const double sm = scaml::wave_sum_to_lane15(gm[d]), sv = scaml::wave_sum_to_lane15(gv[d]);
      if (lane == 63) {
        const double gmu = __builtin_fma(sAmu, p.mu_g[col0 + d], s * sm);
        const double gvar = p.var_g[col0 + d] - 2.0 * s2 * sv;
        p.grad[(size_t)q * D + d] = bad == 0.0 ? __builtin_fma(sAv, gvar, gmu) * invF : bad;
      }
    }
  }
}

}  // namespace

// value only (any kernel family: the value path reads no kernel), and value + gradient per kernel family
extern "C" __global__ __launch_bounds__(64) void scaml_target_fantasy_acqf_kernel(scaml::FantasyAcqfParams p) {
  fantasy_acqf_body<0, false>(p);
}
extern "C" __global__ __launch_bounds__(64) void scaml_target_fantasy_acqf_grad_rbf_kernel(scaml::FantasyAcqfParams p) {
  fantasy_acqf_body<0, true>(p);
}
extern "C" __global__ __launch_bounds__(64) void scaml_target_fantasy_acqf_grad_matern_kernel(scaml::FantasyAcqfParams p) {
  fantasy_acqf_body<1, true>(p);
}
