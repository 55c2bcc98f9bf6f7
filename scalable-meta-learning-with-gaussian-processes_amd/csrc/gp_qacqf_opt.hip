// gp_qacqf_opt.hip -- the optimiser step and the gather of the device-side optimiser of the joint q-point acquisition (gfx950):
// include/scaml_gp.h (7s), (7t).
//
// scaml_qacqf_opt_f64 enqueues, per round, the launches of ScaMLGP.joint_acqf_inputs and the joint acquisition kernel at the Bs * q
// points of the live slots, with the gather kernel below where Python concatenates, and ONE launch of the step kernel, which turns
// that evaluation into the next trial batch of every slot: one wave per slot, two variables per lane (P = q * D <= 128), the optimiser
// state in the caller's workspace, no LDS, no hand-off between workgroups -- the stream orders the rounds.
// The arithmetic is csrc/gp_qacqf_opt.h (also built for the host by the CPU tests).  No matrix cores: a few thousand flops per start.
#include <hip/hip_runtime.h>
#include "gp_qacqf_opt.h"

extern "C" __global__ __launch_bounds__(64) void scaml_qacqf_opt_step_kernel(scaml::QAcqfOptParams p) {
  scaml::qo_step(p, (int)blockIdx.x, (int)threadIdx.x);
}

extern "C" __global__ __launch_bounds__(256) void scaml_qacqf_opt_gather_kernel(scaml::QAcqfOptGatherParams p) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < scaml::qo_gather_elems(p)) scaml::qo_gather_elem(p, e);
}
