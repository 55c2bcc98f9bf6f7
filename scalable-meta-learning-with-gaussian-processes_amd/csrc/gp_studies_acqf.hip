// gp_studies_acqf.hip — the acquisition value and input gradient of MANY BO studies' query points in one launch (gfx950):
// include/scaml_gp.h (7g), behind the grouped GRAD source pass (5e).  One launch in place of, per study, the weighted task sums, the
// target assemble, the Cholesky solve, the finish and gradient kernels and the chain rule of UCB / EI in torch.
//
// A workgroup of 256 threads per query point; the arithmetic is sa_block<1> of csrc/gp_studies_acqf.h (also built for the host by the CPU tests).
// The work per query is ~T n 16 loads and an n x n substitution, n <= 96: latency bound like csrc/gp_fantasy.hip, no matrix cores.
// What a study contributes (factor, block inverses, alpha) is staged in LDS once; the substitution then runs by 16-row blocks, two
// barriers per block, instead of one per column.
#include <hip/hip_runtime.h>
#include "gp_studies_acqf.h"

extern "C" __global__ __launch_bounds__(scaml::STUDIES_ACQF_THREADS) void scaml_target_acqf_batched_kernel(scaml::StudiesAcqfParams p) {
  extern __shared__ double sa_lds[];
  scaml::sa_query(p, sa_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}
