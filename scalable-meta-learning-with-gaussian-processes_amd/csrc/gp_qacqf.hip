// gp_qacqf.hip — the joint Monte-Carlo acquisition function of B q-batches, qEI or qUCB over the joint posterior of each batch's q
// points, and its exact input gradient in one launch (gfx950): include/scaml_gp.h (7p), behind the joint GRAD source pass (5g) and
// the target GP's value path.  One launch in place of torch's q x q Cholesky, the sampling, the utility and autograd back through all
// of them.
//
// A workgroup of 256 threads per batch; the arithmetic is qa_batch of csrc/gp_qacqf.h (also built for the host by the CPU tests).
// The work per batch is a q x q factorisation (q <= 8), S <= 512 samples of q values and (n + q) q kernel slopes: latency bound like
// csrc/gp_fantasy.hip, no matrix cores.  The q x q matrices live in LDS, the samples are dealt to the threads, and every sum over the
// samples is formed by one thread in a fixed order: no atomics, no waiting on another workgroup, every loop bound known at launch.
#include <hip/hip_runtime.h>
#include "gp_qacqf.h"

extern "C" __global__ __launch_bounds__(scaml::QACQF_THREADS) void scaml_target_qacqf_kernel(scaml::QAcqfParams p) {
  extern __shared__ double qa_lds[];
  scaml::qa_batch(p, qa_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}
