// Constraints and hyper-priors of a GP's hyper-parameters: the structs inside the kernel-argument blocks of the two optimiser
// kernels (csrc/gp_target_fit.hip, csrc/gp_stack_fit.hip), the arithmetic on them, and the parse of the caller's host block
// (include/scaml_gp.h (8), (9)).  One source for device code, the host launcher and the SCAML_HOST_EMUL builds (tests/host_emul).
#pragma once
#include <math.h>
#include <stddef.h>

#ifdef __HIPCC__
#define SCAML_HD __device__ __forceinline__
#else
#define SCAML_HD static inline
#endif

namespace scaml {

// One hyper-prior: log-density on the CONSTRAINED value, evaluated as gpytorch does.
//   kind 0: none;  1: Gamma(concentration = p1, rate = p2);  2: LogNormal(loc = p1, scale = p2)
// c0 is the additive constant of the log-density (hyper_prior_from_host).
struct HyperPrior {
  int kind;
  int pad_;
  double p1, p2, c0;
};

// Lengthscales, outputscale and noise (scamlgp/model.py:25-33, 36-70): a sigmoid Interval and a hyper-prior per group.
struct HyperSpec {
  double ls_lo, ls_hi, os_lo, os_hi, nz_lo, nz_hi;
  HyperPrior ls_prior, os_prior, nz_prior;
};

// The target GP (scamlgp/model.py:73-105, 318-338) adds the weights: a prior and a plain box bound.
struct TargetSpec : HyperSpec {
  HyperPrior w_prior;
  double w_lower;   // optimiser only: w >= w_lower (GreaterThan(1e-10, transform=None), model.py:334)
};
// The names these had before the header was shared.  Nothing in the tree uses them; they keep the previous revision's
// tests/host_emul sources compiling against this header, and can go once nobody builds those.
using TargetPrior = HyperPrior;
using StackFitSpec = HyperSpec;
// kernel arguments: the bytes the launcher has always passed (a base class comes first; offsetof says so, with a warning about the base)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(HyperPrior) == 32 && sizeof(HyperSpec) == 144 && offsetof(HyperSpec, ls_prior) == 48, "HyperSpec layout");
static_assert(sizeof(TargetSpec) == 184 && offsetof(TargetSpec, w_prior) == 144 && offsetof(TargetSpec, w_lower) == 176, "TargetSpec layout");
#pragma GCC diagnostic pop

SCAML_HD double prior_logp(const HyperPrior& p, double x) {
  if (p.kind == 1) return p.c0 + (p.p1 - 1.0) * log(x) - p.p2 * x;
  if (p.kind == 2) {
    const double lx = log(x), u = (lx - p.p1) / p.p2;
    return p.c0 - lx - 0.5 * u * u;
  }
  return 0.0;
}
SCAML_HD double prior_dlogp(const HyperPrior& p, double x) {
  if (p.kind == 1) return (p.p1 - 1.0) / x - p.p2;
  if (p.kind == 2) return -(1.0 + (log(x) - p.p1) / (p.p2 * p.p2)) / x;
  return 0.0;
}

// Bounds and prior of variable i of the D + 2 (raw lengthscales, raw outputscale, raw noise)
struct HyperVar {
  double lo, hi;
  const HyperPrior& prior;
};
SCAML_HD HyperVar hyper_var(const HyperSpec& sp, int i, int D) {
  return HyperVar{i < D ? sp.ls_lo : (i == D ? sp.os_lo : sp.nz_lo), i < D ? sp.ls_hi : (i == D ? sp.os_hi : sp.nz_hi),
                  i < D ? sp.ls_prior : (i == D ? sp.os_prior : sp.nz_prior)};
}

// The Interval constraint: theta = lo + (hi - lo) s, d theta / d raw = (hi - lo) s (1 - s), s = sigmoid(raw)
SCAML_HD double interval_sigmoid(double raw) { return 1.0 / (1.0 + exp(-raw)); }
SCAML_HD double interval_value(const HyperVar& v, double s) { return v.lo + (v.hi - v.lo) * s; }
SCAML_HD double interval_slope(const HyperVar& v, double s) { return (v.hi - v.lo) * s * (1.0 - s); }

// ---- the caller's block of doubles (host) ------------------------------------------------------------------------------------
// [0..5] the six bounds, then (kind, p1, p2) per prior: lengthscale, outputscale, noise -- 15 doubles; the target's block goes on
// with the weights' triple and w_lower -- 19.  false: a value out of range.
static inline bool hyper_prior_from_host(const double* t, HyperPrior& pr) {
  const int kind = (int)t[0];
  const double p1 = t[1], p2 = t[2];
  if (kind < 0 || kind > 2) return false;
  if (kind == 1 && !(p1 > 0.0 && p2 > 0.0)) return false;
  if (kind == 2 && !(p2 > 0.0)) return false;
  pr.kind = kind; pr.pad_ = 0; pr.p1 = p1; pr.p2 = p2;
  // Gamma: c ln r - lgamma(c);  LogNormal: -ln scale - ln(2 pi) / 2
  pr.c0 = kind == 1 ? p1 * log(p2) - lgamma(p1) : (kind == 2 ? -log(p2) - 0.9189385332046727 : 0.0);
  return true;
}
static inline bool hyper_spec_from_host(const double* s, HyperSpec& sp) {
  sp.ls_lo = s[0]; sp.ls_hi = s[1]; sp.os_lo = s[2]; sp.os_hi = s[3]; sp.nz_lo = s[4]; sp.nz_hi = s[5];
  if (!(sp.ls_hi > sp.ls_lo) || !(sp.os_hi > sp.os_lo) || !(sp.nz_hi > sp.nz_lo)) return false;
  return hyper_prior_from_host(s + 6, sp.ls_prior) && hyper_prior_from_host(s + 9, sp.os_prior) && hyper_prior_from_host(s + 12, sp.nz_prior);
}
static inline bool target_spec_from_host(const double* s, TargetSpec& sp) {
  sp.w_lower = s[18];
  return hyper_spec_from_host(s, sp) && hyper_prior_from_host(s + 15, sp.w_prior);
}

}  // namespace scaml
