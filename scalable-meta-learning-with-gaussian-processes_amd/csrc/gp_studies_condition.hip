// gp_studies_condition.hip — the fantasy set-up of MANY BO studies with pending evaluations (gfx950): include/scaml_gp.h (7m), (7n), in
// place of, per such study, ScaMLGP.fantasize + condition_on_observations + the first fantasy_acqf call.  Behind ONE value-mode grouped
// source pass (5f) over the studies' own X' = cat(train_X, X_pend) strips:
//   (7m) the training blocks K' of the conditioned models, the observed rows' residuals and the prior mean at the pending rows;
//   (2)  scaml_potrf_batched_f64 factors all blocks (ragged sizes, the jitter ladder and info per study);
//   (7n) v = L_nn^-1 resid, the fantasy targets mu~_p + L_pp eps_f and alpha_f = L'^-T [v ; eps_f] for the F columns.
// The arithmetic is csrc/gp_studies_condition.h (also built for the host by the CPU tests): a workgroup of 256 threads per study, fp64,
// every sum by one thread in a fixed order.  Latency bound like (7f) / (7g) / (7k) -- an n' x n' substitution with n' <= 96 and at most
// 64 columns --: plain vector loads and stores, LDS for the factor and the right-hand sides, no matrix cores.
#include <hip/hip_runtime.h>
#include "gp_studies_condition.h"

extern "C" __global__ __launch_bounds__(scaml::STUDIES_CONDITION_THREADS) void scaml_studies_condition_block_kernel(scaml::StudiesConditionBlockParams p) {
  extern __shared__ double sc_lds[];
  scaml::sc_condition_block(p, sc_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}

extern "C" __global__ __launch_bounds__(scaml::STUDIES_CONDITION_THREADS) void scaml_studies_fantasy_condition_kernel(scaml::StudiesFantasyConditionParams p) {
  extern __shared__ double sc_lds[];
  scaml::sc_fantasy_condition(p, sc_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}
