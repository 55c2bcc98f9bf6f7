// TEST INFRASTRUCTURE, not product code: csrc/gp_target_fit.hip compiled as single-threaded host code (SCAML_HOST_EMUL: one
// "thread", barriers are no-ops, every cooperative loop runs sequentially), so that the arithmetic of the target-GP objective,
// its analytic gradient and the L-BFGS driver can be checked against the oracle on a machine without a GPU.  Never linked into
// libscaml_hip.so; only tests/test_target_fit_emul.py builds and loads it.
#include "target_fit_emul_common.h"

extern "C" int emul_target_fit(const double* means_t, const double* covs_p, const double* X, const double* y, double m_all, double s_all,
                               const double* spec, double* z, int B, int n, int T, int D, int kind, int mode, int max_iter, int history,
                               double gtol, double ftol, double* value, double* grad, int32_t* info, double* jitter, int32_t* stats) {
  return emul::target_fit(means_t, covs_p, X, y, m_all, s_all, spec, z, B, n, T, D, kind, mode, max_iter, history, gtol, ftol, value, grad, info,
                          jitter, stats);
}

// The LDS footprint twice: where the kernel's carve ends, and what the host launcher asks for (csrc/gp_target_params.h).
extern "C" long long emul_target_fit_carve_doubles(int n, int T, int D, int waves, int mfma) {
  std::vector<double> lds(scaml::target_fit_lds_doubles(n, T, D, mfma != 0, waves) + 4096);
  scaml::TfCtx c;
  return (long long)(scaml::tf_carve(c, lds.data(), n, T, D, waves, mfma) - lds.data());
}
extern "C" long long emul_target_fit_lds_doubles(int n, int T, int D, int waves, int mfma) {
  return (long long)scaml::target_fit_lds_doubles(n, T, D, mfma != 0, waves);
}
