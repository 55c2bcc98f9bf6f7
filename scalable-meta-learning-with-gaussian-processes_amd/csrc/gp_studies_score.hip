// gp_studies_score.hip — stage 1 of the studies' acquisition optimiser on the device (gfx950): the acquisition value of a whole table
// of raw candidates of MANY BO studies in one launch (include/scaml_gp.h (7i)), behind the value-only grouped source pass (5f); and the
// training blocks of all studies in one launch (7j), whose factors (2) then computes together.
//
// (7i) A workgroup of 256 threads per strip of 16 candidates of one study; the arithmetic is sa_block<16> of csrc/gp_studies_acqf.h (also built
// for the host by the CPU tests).  The study's factor, block inverses and alpha go to LDS once and serve 16 right-hand sides: thread <->
// (row, candidate).  (7g) is sa_block<1>, the same text, so the two kernels agree bit for bit; like (7g) the work is latency
// bound (T n 16 loads and an n x n substitution, n <= 96) and uses no matrix cores.
#include "scaml_common.hpp"
#include "gp_studies_score.h"

extern "C" __global__ __launch_bounds__(scaml::STUDIES_SCORE_THREADS) void scaml_target_score_batched_kernel(scaml::StudiesScoreParams p) {
  extern __shared__ double ss_lds[];
  scaml::sa_score_strip(p, ss_lds, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}

// (7j) One workgroup per study, an element of Knn per thread and round.  The weighted task sums are (6)'s, in (6)'s order -- four
// quarters of the task axis, each ascending in chunks of eight, met as (q0 + q1) + (q2 + q3) --, the element is (7)'s assemble:
// Knn[i][c] = cov_s / s^2 + os k_t(x_i, x_c) (+ noise on the diagonal), resid[i] = y_i - (mean_s[i] - m) / s.  The packed covariance
// holds the lower triangle, which is the triangle (2) reads; the upper one is its mirror image.
namespace scaml {

template <int KIND>
__device__ __forceinline__ void target_train_block(const TrainBlockParams& p) {
  __shared__ double exptab[64];
  exp2_table_init(exptab, threadIdx.x);
  __syncthreads();
  const int g = blockIdx.x, n_max = p.n_max, T = p.T, D = p.D;
  int n = p.n_points[g];
  n = n < 0 ? 0 : (n > n_max ? n_max : n);   // (kept inside the rows the host sized everything for)
  const size_t packed = (size_t)n_max * (n_max + 1) / 2;
  const double* mt = p.means_t + (size_t)g * T * n_max;
  const double* cp = p.covs_p + (size_t)g * T * packed;
  const double* Xg = p.X + (size_t)g * n_max * D;
  const double* th = p.theta + (size_t)g * (D + 2);
  const double* wg = p.w + (size_t)g * T;
  const uint8_t* ag = p.active + (size_t)g * T;
  const double m_all = p.m_all[g], s_all = p.s_all[g], s2 = s_all * s_all;
  const double os = th[D], noise = th[D + 1];
  double* Kg = p.Knn + (size_t)g * n_max * n_max;
  for (int e = threadIdx.x; e < n * (n + 1) / 2; e += blockDim.x) {
    // e -> (i, c), c <= i: the row of the packed triangle that holds e
    int i = (int)((__builtin_sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    while (i * (i + 1) / 2 > e) --i;
    const int c = e - i * (i + 1) / 2;
    const double cov_s = sa_weighted_sum(cp + e, packed, wg, ag, T, 2);
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (Xg[(size_t)i * D + d] - Xg[(size_t)c * D + d]) / th[d];
      d2 = __builtin_fma(df, df, d2);
    }
    const double v = cov_s / s2 + os * kernel_from_sqdist<KIND>(d2, exptab);
    Kg[(size_t)i * n_max + c] = v + (i == c ? noise : 0.0);
    if (i != c) Kg[(size_t)c * n_max + i] = v;
  }
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const double mean_s = sa_weighted_sum(mt + e, (size_t)n_max, wg, ag, T, 1);
    p.resid[(size_t)g * n_max + e] = p.y[(size_t)g * n_max + e] - (mean_s - m_all) / s_all;
  }
}

}  // namespace scaml

extern "C" __global__ __launch_bounds__(256) void scaml_target_train_block_rbf_kernel(scaml::TrainBlockParams p) {
  scaml::target_train_block<0>(p);
}
extern "C" __global__ __launch_bounds__(256) void scaml_target_train_block_matern_kernel(scaml::TrainBlockParams p) {
  scaml::target_train_block<1>(p);
}
