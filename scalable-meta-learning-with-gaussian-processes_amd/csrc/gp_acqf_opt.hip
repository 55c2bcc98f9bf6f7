// gp_acqf_opt.hip -- the optimiser step of the device-side acquisition optimiser (gfx950): include/scaml_gp.h (7h).
//
// scaml_studies_acqf_opt_f64 enqueues, per round, the grouped GRAD source pass (5e), the batched target acquisition (7g) and ONE launch
// of the kernel below, which turns that evaluation into the next trial point of every start of every study: one wave per start, one
// lane per coordinate (D <= 15), the optimiser state in the caller's workspace, no LDS, no hand-off between workgroups -- the stream
// orders the rounds.  A start that has stopped hands the evaluation kernels group -1 and costs them nothing from then on.
// The arithmetic is csrc/gp_acqf_opt.h (also built for the host by the CPU tests).  No matrix cores: a few hundred flops per start.
#include <hip/hip_runtime.h>
#include "gp_acqf_opt.h"

extern "C" __global__ __launch_bounds__(64) void scaml_acqf_opt_step_kernel(scaml::AcqfOptParams p) {
  scaml::ao_step(p, (int)blockIdx.x, (int)threadIdx.x);
}
