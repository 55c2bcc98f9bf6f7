// gp_studies_score.h -- scoring a TABLE of candidates for many BO studies (include/scaml_gp.h (7i)): stage 1 of the studies'
// acquisition optimiser, 1,024 raw candidates per study, value only.  One source for the device kernel (csrc/gp_studies_score.hip: a
// workgroup per strip of 16 candidates of one study), the host launcher and the single-threaded host build the CPU tests run
// (tests/host_emul/studies_score_emul.cpp).
//
// Inputs are the VALUE layout of the grouped source pass (5f): mu, var (T, Mq), cov (T, n_max, Mq), 16 different candidates per strip,
// all of one study, group[strip] names it.  What csrc/gp_studies_acqf.h (7g) does for one query point with its 16 gradient columns
// -- a workgroup that stages the study's factor in LDS for a single right-hand side -- is done here for 16 candidates against ONE
// copy of the factor: thread <-> (row, candidate), the 16 columns are the parallelism.
//
// Arithmetic contract: value, mu_out and var_out of a candidate equal (7g)'s bit for bit.  The two kernels are two instantiations of
// ONE text, sa_block<R> of csrc/gp_studies_acqf.h (R = 1 there, R = 16 here): per candidate the same operations in the same order --
// the task sums ascending in chunks of eight, the target-kernel term, the blocked forward and backward substitution with the 16 x 16
// block inverses, Knq . alpha and Knq . z ascending over the training points, UCB / EI with the clamps, the non-finite-coordinate rule
// -- and only the indexing (element e of an [.][R] array) and the gradient columns of R = 1 depend on R.  Every output comes from one
// thread, no atomics.  tests/test_studies_score_emul.py and tests/test_studies_score_gpu.py compare the two instantiations.
#pragma once
#include "gp_studies_acqf.h"   // StudiesAcqfParams, the limits, and through it csrc/gp_studies_formulas.h

namespace scaml {

constexpr int STUDIES_SCORE_THREADS = 256;   // 16 rows x 16 candidates

// The argument block is (7g)'s, read in the value layout: mu, var (T, Mq), cov (T, n_max, Mq), group (Mq / 16) per STRIP, Xq (Mq, D),
// value / mu_out / var_out (Mq); Mq is a multiple of 16 and `grad` is not used.
using StudiesScoreParams = StudiesAcqfParams;

constexpr size_t studies_score_lds_doubles(int n_max) { return sa_lds_doubles<16>(n_max); }

// One strip of 16 candidates: the R = 16 instantiation.
SA_DEV void sa_score_strip(const StudiesScoreParams& p, double* lds, int strip, int tid, int nthr) { sa_block<16>(p, lds, strip, tid, nthr); }

// ---- the studies' training blocks, all at once (include/scaml_gp.h (7j)): Knn and resid of G studies from the padded per-study
// source terms the batched refit (8b) already holds, as (7)'s assemble forms them for one study behind (6')'s weighted sums.
struct TrainBlockParams {
  const double* means_t;      // (G, T, n_max) source means at the training inputs
  const double* covs_p;       // (G, T, n_max (n_max + 1) / 2) source covariances, lower triangle packed row by row
  const double* X;            // (G, n_max, D)
  const double* y;            // (G, n_max) standardised targets
  const int32_t* n_points;    // (G)
  const double* m_all;        // (G)
  const double* s_all;        // (G)
  const double* w;            // (G, T) pruned weights
  const uint8_t* active;      // (G, T)
  const double* theta;        // (G, D + 2)
  double* Knn;                // (G, n_max, n_max): the leading n_g x n_g block is written, both triangles
  double* resid;              // (G, n_max): the leading n_g entries
  int G, n_max, T, D;
};

}  // namespace scaml
