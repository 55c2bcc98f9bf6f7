// gp_qacqf_pending.hip — the joint Monte-Carlo acquisition function (qEI, qUCB) of B q-batches with p evaluations pending, and its exact
// gradient with respect to the q moving points, in one launch (gfx950): include/scaml_gp.h (7q), behind the joint GRAD source pass (5g)
// called with the pending points as leading points (Ma = n + p).
//
// The batch body is (7p)'s, qa_batch<true> of csrc/gp_qacqf.h: a workgroup of 256 threads per batch of q moving points, the
// (q + p) x (q + p) factorisation and the samples in LDS, every sum over the samples formed by one thread in a fixed order.  Same
// regime as csrc/gp_qacqf.hip: latency bound, no matrix cores, no atomics, every loop bound known at launch.
// A file of its own: a second kernel next to scaml_target_qacqf_kernel in one translation unit changes that kernel's instruction
// stream (tools/dev_isa_diff.py), and (7p) is to stay as it was.
#include <hip/hip_runtime.h>
#include "gp_qacqf.h"

extern "C" __global__ __launch_bounds__(scaml::QACQF_THREADS) void scaml_target_qacqf_pending_kernel(scaml::QAcqfPendingParams p) {
  extern __shared__ double qa_pending_lds[];
  scaml::qa_batch_pending(p, qa_pending_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}
