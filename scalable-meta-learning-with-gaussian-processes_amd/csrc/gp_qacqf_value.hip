// gp_qacqf_value.hip — the joint Monte-Carlo acquisition function (qEI, qUCB) of B q-batches, with p >= 0 evaluations pending, VALUE
// ONLY (gfx950): include/scaml_gp.h (7r), behind the value-layout joint source pass (5h).  The scoring pass of a batch optimiser's raw
// candidates: 16 points per strip of the source pass instead of one, and no derivative column anywhere.
//
// The batch body is (7p)'s / (7q)'s, qa_batch<true, true> of csrc/gp_qacqf.h: a workgroup of 256 threads per batch, the
// (q + p) x (q + p) factorisation and the samples in LDS, every sum over the samples formed by one thread in a fixed order -- value,
// jitter and info are those kernels' bits.  Same regime: latency bound, no matrix cores, no atomics, every loop bound known at launch.
// A file of its own, as csrc/gp_qacqf_pending.hip is: a further kernel in one translation unit changes the instruction streams of
// the ones already there (tools/dev_isa_diff.py).
#include <hip/hip_runtime.h>
#include "gp_qacqf.h"

extern "C" __global__ __launch_bounds__(scaml::QACQF_THREADS) void scaml_target_qacqf_value_kernel(scaml::QAcqfPendingParams p) {
  extern __shared__ double qa_value_lds[];
  scaml::qa_batch_value(p, qa_value_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}
