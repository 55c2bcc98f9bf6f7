// gp_studies_fantasy.hip — the batched target acquisition of MANY BO studies of which some hold pending evaluations (gfx950):
// include/scaml_gp.h (7k), behind the grouped source passes (5e) / (5f).  A study with pending points is a fantasy model
// (ScaMLGP.fantasize): its training block holds the pending inputs too, and UCB / EI are averaged over the F_g columns of alpha_f, the
// formula of csrc/gp_fantasy.hip (7f).  In place of, per such study, its own ScaMLGPBOLoop.suggest().
//
// The arithmetic is sa_block<R> of csrc/gp_studies_acqf.h with the StudiesFantasyParams block: the text of (7g) / (7i) up to z = Knn^-1 Knq,
// then per group either their phases 3 and 4 (F_g == 1: an ordinary study, bit for bit what (7g) / (7i) give) or the fantasy average.
// A workgroup of 256 threads per query point (value + gradient) or per strip of 16 candidates (value).  alpha_f is read from global
// memory: a workgroup reads each of its n F_g entries once per right-hand side, consecutive threads consecutive fantasies.  Latency bound
// like (7f) and (7g): plain vector loads and stores, no matrix cores.
#include <hip/hip_runtime.h>
#include "gp_studies_acqf.h"

extern "C" __global__ __launch_bounds__(scaml::STUDIES_ACQF_THREADS) void scaml_target_fantasy_acqf_batched_kernel(scaml::StudiesFantasyParams p) {
  extern __shared__ double sf_lds[];
  scaml::sa_fantasy_query(p, sf_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}

extern "C" __global__ __launch_bounds__(scaml::STUDIES_ACQF_THREADS) void scaml_target_fantasy_score_batched_kernel(scaml::StudiesFantasyParams p) {
  extern __shared__ double sf_lds[];
  scaml::sa_fantasy_strip(p, sf_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}
