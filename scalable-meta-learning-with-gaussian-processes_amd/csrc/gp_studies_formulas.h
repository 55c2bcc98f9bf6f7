// gp_studies_formulas.h -- the scalar formulas the studies' target kernels share: the target kernel with its slope, and the UCB / EI
// value with its chain-rule factors.  Included by csrc/gp_studies_acqf.h (sa_block<R>: a workgroup per query point, value + gradient,
// or per strip of 16 candidates, value only) and by csrc/gp_fantasy.hip (UCB / EI averaged over F fantasies): one text, so that all of
// them evaluate the same expressions.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SA_DEV __device__ __forceinline__
#define SA_DEV_CALL static __device__ __noinline__   // a real call: a large body that must not add to its callers' register count
#define SA_SYNC() __syncthreads()
#else
#define SA_DEV static inline
#define SA_DEV_CALL static inline
#define SA_SYNC() ((void)0)
#endif

namespace scaml {

// os k(d2) and os dk / d(d2) of the scaled squared distance (the formulas of kernel_and_slope_scaled, libm instead of the table)
SA_DEV void sa_kernel_and_slope(int kind, double d2, double os, double& k, double& dk) {
  if (kind == 0) {
    k = os * exp(-0.5 * d2);
    dk = -0.5 * k;
  } else {
    const double s5 = 2.2360679774997896964;
    const double r = sqrt(fmax(d2, 1e-30));   // gpytorch clamps the squared distance before the root
    const double ex = os * exp(-s5 * r);
    const double lin = 1.0 + s5 * r;
    k = (lin + (5.0 / 3.0) * r * r) * ex;
    dk = (-5.0 / 6.0) * lin * ex;
  }
}

// sum_t c_t in[t tstride], c_t = w_t (power 1) or w_t^2 (power 2), in (6)'s order: four quarters of the task axis, each ascending in
// chunks of eight, met as (q0 + q1) + (q2 + q3).  The training blocks of (7j) and (7m) are built from it.
SA_DEV double sa_weighted_sum(const double* __restrict__ in, size_t tstride, const double* __restrict__ w, const uint8_t* __restrict__ active,
                              int T, int power) {
  const int chunk = (T + 3) / 4;
  double part[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t_lo = q * chunk, t_hi = t_lo + chunk < T ? t_lo + chunk : T;
    double s = 0.0;
    for (int t0 = t_lo; t0 < t_hi; t0 += 8) {
      double v[8], c[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = t0 + k;
        const bool ok = t < t_hi && active[t];   // (a masked task is skipped, not multiplied by zero: its values may be NaN)
        v[k] = ok ? in[(size_t)t * tstride] : 0.0;
        const double wt = ok ? w[t] : 0.0;
        c[k] = power == 2 ? wt * wt : wt;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) s = fma(c[k], v[k], s);
    }
    part[q] = s;
  }
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// The acquisition codes of include/scaml_gp.h (SCAML_ACQF_*): UCB, EI, and EI in the log domain (EI | LOG).
constexpr int SA_ACQF_UCB = 0, SA_ACQF_EI = 1, SA_ACQF_LOG = 0x10, SA_ACQF_LOGEI = SA_ACQF_EI | SA_ACQF_LOG;
SA_DEV bool sa_acqf_valid(int acqf) { return acqf == SA_ACQF_UCB || acqf == SA_ACQF_EI || acqf == SA_ACQF_LOGEI; }

// g(u) = log(phi(u) + u Phi(u)), its derivative gp = Phi / (phi + u Phi) > 0 and om = 1 - u gp = phi / (phi + u Phi), each without
// cancellation, for u in [-1e8, 40] (phi, Phi: the standard normal density and distribution).
//   u >= -2:  the direct formula with Phi = erfc(-u / sqrt 2) / 2; phi + u Phi loses at most a factor (phi + |u| Phi) / (phi + u Phi)
//             (1 for u >= 0, 11.8 at u = -2) in relative accuracy.
//   u <  -2:  with t = -u and K(t) = 1 / (t + 2 / (t + 3 / (t + ...))) the Mills ratio is 1 / (t + K) and
//             phi + u Phi = phi(t) K / (t + K),  g = -t t / 2 - log sqrt(2 pi) + log(K / (t + K)),  gp = 1 / K,  om = (t + K) / K.
//             K by the backward recurrence x_k = k / (t + x_{k+1}), K = x_1, from the fixed point of x = (N + 1) / (t + x) as the tail
//             x_{N+1}: every operand is positive, and an error of x_{k+1} reaches x_k damped by x_{k+1} / (t + x_{k+1}) < 1.  The
//             term count N is fixed per range of t (tests/_logei_bounds.py states the truncation error they leave: below 2^-57 K).
struct SaLogEi {
  double g, gp, om;
};
SA_DEV_CALL SaLogEi sa_log_ei_terms(double u) {   // (returned by value: the three results travel in registers)
  SaLogEi r;
  if (u < -2.0) {
    const double t = -u;
    const int N = t < 3.0 ? 112 : t < 5.0 ? 72 : t < 8.0 ? 36 : t < 16.0 ? 20 : 12;
    double x = 0.5 * (sqrt(fma(t, t, 4.0 * (N + 1))) - t);
    for (int k = N; k >= 1; --k) x = (double)k / (t + x);
    const double tk = t + x;
    r.g = (-0.5 * t * t - 0.91893853320467274178) + log(x / tk);   // log sqrt(2 pi)
    r.gp = 1.0 / x;
    r.om = tk / x;
  } else {   // (a NaN u comes here and leaves NaN)
    const double pdf = exp(-0.5 * u * u) * 0.39894228040143267794;   // 1 / sqrt(2 pi)
    const double cdf = 0.5 * erfc(-u * 0.70710678118654752440);
    const double h = fma(u, cdf, pdf);
    r.g = log(h);
    r.gp = cdf / h;
    r.om = pdf / h;
  }
  return r;
}
SA_DEV void sa_log_ei_core(double u, double& g, double& gp) {
  const SaLogEi r = sa_log_ei_terms(u);
  g = r.g;
  gp = r.gp;
}

// The acquisition value A of a posterior (mu, vr) with its partial derivatives Amu = dA / dmu, Av = dA / dvr; `par`: UCB's beta, best_f
// of EI and LogEI.  The clamps are those of scamlgp_amd/utils.py.  (A code that is none of the three leaves NaN: the host refuses it.)
SA_DEV void sa_acquisition(int acqf, double par, double mu, double vr, double& A, double& Amu, double& Av) {
  if (acqf == SA_ACQF_UCB) {   // UCB: -mu + sqrt(beta max(v, 0)); d/dv = beta / (2 sqrt(beta v)), zero where v is clamped
    const double sd = sqrt(par * (vr > 0.0 ? vr : 0.0));
    A = sd - mu;
    Amu = -1.0;
    Av = vr > 0.0 ? 0.5 * par / (sd > 1e-300 ? sd : 1e-300) : 0.0;
  } else if (acqf == SA_ACQF_EI) {   // EI (minimisation): d/dmu = -Phi(u), d/dv = phi(u) / (2 sigma), zero on the 1e-9 floor
    const double sigma = sqrt(vr > 1e-9 ? vr : 1e-9);
    const double uu = -(mu - par) / sigma;
    const double pdf = exp(-0.5 * uu * uu) * 0.39894228040143267794;   // 1 / sqrt(2 pi)
    const double cdf = 0.5 * (1.0 + erf(uu * 0.70710678118654752440));
    A = sigma * (pdf + uu * cdf);
    Amu = -cdf;
    Av = vr > 1e-9 ? 0.5 * pdf / sigma : 0.0;
  } else if (acqf == SA_ACQF_LOGEI) {   // log EI = log sigma + g(u): d/dmu = -g'(u) / sigma, d/dv = (1 - u g'(u)) / (2 sigma^2), zero on the floor
    const double sigma = sqrt(vr > 1e-9 ? vr : 1e-9);
    const double uu = -(mu - par) / sigma;
    const SaLogEi r = sa_log_ei_terms(uu);
    A = log(sigma) + r.g;
    Amu = -r.gp / sigma;
    Av = vr > 1e-9 ? 0.5 * r.om / (sigma * sigma) : 0.0;
  } else {
    A = Amu = Av = NAN;
  }
}

}  // namespace scaml
