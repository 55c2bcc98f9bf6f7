// gp_acqf_transform.hip -- the acquisition value of M given posteriors and its chain-rule factors, elementwise (gfx950):
// include/scaml_gp.h (7o).  One thread per element; the arithmetic is sa_acquisition of csrc/gp_studies_formulas.h, the statement the
// fantasy kernel (7f) and the studies' kernels (7g) / (7i) / (7k) evaluate -- UCB, EI and LogEI with the clamps of scamlgp_amd/utils.py.
#include <hip/hip_runtime.h>
#include "gp_studies_formulas.h"

extern "C" __global__ __launch_bounds__(256) void scaml_acqf_transform_kernel(const double* mu, const double* var, double acqf_param, int M,
                                                                              int acqf, double* A, double* Amu, double* Av) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;   // (unsigned: M up to INT_MAX leaves the last block's indices representable)
  if (i >= (unsigned)M) return;
  double a, amu, av;
  scaml::sa_acquisition(acqf, acqf_param, mu[i], var[i], a, amu, av);
  A[i] = a;
  if (Amu) Amu[i] = amu;
  if (Av) Av[i] = av;
}
