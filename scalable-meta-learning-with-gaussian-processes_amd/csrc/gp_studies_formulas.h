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
#define SA_SYNC() __syncthreads()
#else
#define SA_DEV static inline
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

// The acquisition value A of a posterior (mu, vr) with its partial derivatives Amu = dA / dmu, Av = dA / dvr; `par`: UCB's beta, EI's
// best_f.  The clamps are those of scamlgp_amd/utils.py.
SA_DEV void sa_acquisition(int acqf, double par, double mu, double vr, double& A, double& Amu, double& Av) {
  if (acqf == 0) {   // UCB: -mu + sqrt(beta max(v, 0)); d/dv = beta / (2 sqrt(beta v)), zero where v is clamped
    const double sd = sqrt(par * (vr > 0.0 ? vr : 0.0));
    A = sd - mu;
    Amu = -1.0;
    Av = vr > 0.0 ? 0.5 * par / (sd > 1e-300 ? sd : 1e-300) : 0.0;
  } else {             // EI (minimisation): d/dmu = -Phi(u), d/dv = phi(u) / (2 sigma), zero on the 1e-9 floor
    const double sigma = sqrt(vr > 1e-9 ? vr : 1e-9);
    const double uu = -(mu - par) / sigma;
    const double pdf = exp(-0.5 * uu * uu) * 0.39894228040143267794;   // 1 / sqrt(2 pi)
    const double cdf = 0.5 * (1.0 + erf(uu * 0.70710678118654752440));
    A = sigma * (pdf + uu * cdf);
    Amu = -cdf;
    Av = vr > 1e-9 ? 0.5 * pdf / sigma : 0.0;
  }
}

}  // namespace scaml
