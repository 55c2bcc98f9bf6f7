// Kernel-argument blocks of the posterior kernels, shared by device source and host launcher.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace scaml {

struct PosteriorParams {
  const double* Xq;         // (M, D) query points, shared by all tasks
  const double* X;          // (T, N, D)
  const double* theta;      // (T, D+2)
  const double* L;          // (T, N, N)
  const double* Linv_diag;  // (T, ceil(N/16), 16, 16)
  const double* alpha;      // (T, N)
  const double* y_mean;     // (T) or NULL
  const double* y_std;      // (T) or NULL
  const int32_t* n_points;  // (T) or NULL
  double* mu;               // (T, M) or NULL
  double* var;              // (T, M) or NULL
  double* V;                // (T, N, M) or NULL
  int T, N, M, D;
  int x_in_lds;
  int xq_per_task;  // Xq is (T, M, D) instead of (M, D)
  int mean_only;    // skip the triangular solve: only mu = m + s K_* alpha is produced
  // fused covariance block (gp_posterior_linv_kernel only): with VA = V[:, :Ma] (T, N, Ma) of the first Ma query points given,
  // cov (T, Ma, M) = s^2 (os k(xq_a, xq_c) - VA^T V) comes out of the same pass and V itself never reaches memory
  const double* VA;
  double* cov;
  int Ma;
  int pad_;
  // the Ma leading points of the covariance block when they are not the head of Xq (input-gradient pass: Xq holds the query
  // points only); NULL: the first Ma rows of Xq
  const double* Xa;
};

// The grouped GRAD pass (scaml_posterior_linv_grad_grouped_f64): query point q belongs to group[q], every group has its own leading
// points.  In `base`: Ma = Ma_max (row count of cov and of a group's slice of Xa), VA / Xa unused.
// T = the task slots of a group (rows of mu / var / cov).
struct PosteriorGroupArgs {
  const int32_t* group;         // (Mq) group of a query point; negative: a padding row.  Value mode (5f): one entry per STRIP of 16
  const int32_t* n_a;           // (G) leading points per group, 1 <= n_a[g] <= Ma_max
  const double* const* VA_tab;  // (G) device pointers: group g's V of its leading points, (T, N, n_a[g]) with row stride n_a[g]
  const double* Xa;             // (G, Ma_max, D) the leading points, padded
  int G;
  int pad_;
  // per-group source tasks (scaml_posterior_linv_grad_grouped_own_f64, the kernel's OWN instantiation; unused otherwise -- appended, so
  // that the block above keeps its offsets): task slot t of group g reads source task task_base[g] + t of the Tsrc tasks in the source
  // arrays (X, theta, L, alpha, y_mean, y_std, n_points); outputs and VA_tab[g] stay indexed by the slot
  const int32_t* task_base;     // (G)
  int Tsrc;
  int pad2_;
#ifdef __HIPCC__
  __device__ int count(int g, int ma_max) const {   // a group's count, kept inside the rows the host sized everything for
    const int c = n_a[g];
    return c < 0 ? 0 : (c > ma_max ? ma_max : c);
  }
#endif
};
struct PosteriorGroupedParams {
  PosteriorParams base;
  PosteriorGroupArgs ga;
};

// The joint GRAD pass (scaml_posterior_linv_grad_joint_f64): the query points move in batches of q; the covariance block of a strip
// gets q more rows, against the strip's batch mates.  In `base`: Ma = the leading points alone, cov has Ma + q rows.
struct PosteriorJointArgs {
  const double* VQ;   // (T, N, Mq) the V of all query points, from the value pass
  int q;              // points per batch; Mq is a multiple of it
  int pad_;
};
struct PosteriorJointParams {
  PosteriorParams base;
  PosteriorJointArgs ja;
};

// The joint pass in VALUE layout (scaml_posterior_linv_cov_joint_f64, (5h)): a strip holds 16 different query points, the B batches of q
// packed as csrc/gp_qacqf_columns.h lays them (M = Mp columns); the covariance block gets q more rows, against the column's batch
// mates, from the Gram tile of the strip's V with itself.  In `base`: Ma = the leading points alone, cov has Ma + q rows.
struct PosteriorJointValueArgs {
  int q;   // points per batch
  int B;   // batches: the columns behind the last one are padding
};
struct PosteriorJointValueParams {
  PosteriorParams base;
  PosteriorJointValueArgs jv;
};

struct PosteriorCovParams {
  const double* Xq;     // (M, D)
  const double* theta;  // (T, D+2)
  const double* V;      // (T, N, M)
  const double* y_std;  // (T) or NULL
  double* cov;          // (T, Ma, M)
  int T, N, M, Ma, D;
  int xq_per_task;
};

struct ChoSolveParams {
  const double* L;          // (T, N, N)
  const double* Linv_diag;  // (T, ceil(N/16), 16, 16)
  const double* B;          // (T, N, R) right-hand sides
  const int32_t* n_points;  // (T) or NULL
  double* Xout;             // (T, N, R): (L L^T)^-1 B, or L^-T B (mode 1)
  int T, N, R;
  int mode;                 // 0: forward + backward substitution, 1: backward only (L^T x = b)
};

struct KernelMatrixParams {
  const double* X1;     // (T, N1, D)
  const double* X2;     // (T, N2, D), (N2, D) when x2_shared, or NULL: X2 = X1 (square, symmetric)
  const double* theta;  // (T, D+2)
  double* K;            // (T, N1, N2)
  int T, N1, N2, D;
  int x2_shared, add_noise;
};

struct LinvParams {
  const double* L;          // (T, N, N)
  const double* Linv_diag;  // (T, ceil(N/16), 16, 16)
  const int32_t* n_points;  // (T) or NULL
  double* Linv;             // (T, N, N) out: L^-1 (dense, zero above the diagonal)
  int T, N;
  int lower_only;           // 1: the block rows above a strip's diagonal block are not written (callers that never read them)
};

struct MllGradParams {
  const double* X;          // (T, N, D)
  const double* theta;      // (T, D+2)
  const double* alpha;      // (T, N)
  const double* Linv;       // (T, N, N)
  const int32_t* n_points;  // (T) or NULL
  double* partials;         // (T, tiles, D+2), tiles = nb (nb + 1) / 2, nb = ceil(N/16)
  int T, N, D;
};

struct TargetAssembleParams {
  const double* cov_s;          // (n, n + M) weighted source covariance block, original units
  const double* mean_s;         // (n + M)   weighted source mean
  const double* var_s;          // (n + M)   weighted source variances (only [n:] is read)
  const double* Xall;           // (n + M, D) target training inputs, then the query points
  const double* theta;          // (D + 2) target kernel: lengthscales, outputscale, noise
  const double* train_targets;  // (n) standardised target observations
  double m_all, s_all;
  double* Knn;                  // (n, n)
  double* resid;                // (n)
  double* Knq;                  // (n, M)
  double* mean_q;               // (M)
  double* var_q;                // (M)
  int n, M, D;
};

struct MllGradFusedParams {
  const double* X;          // (T, N, D)
  const double* theta;      // (T, D+2)
  const double* L;          // (T, N, N) lower factor (strict upper triangle never read)
  const double* Linv_diag;  // (T, ceil(N/16), 16, 16)
  const double* alpha;      // (T, N)
  const int32_t* n_points;  // (T) or NULL
  double* partials;         // (T, tiles, D+2): the task's totals go into tile slot 0, zeros into the others
  int T, N, D;
};

// ---- dynamic LDS footprints, in doubles (see csrc/gp_fit_params.h: one definition for the host launcher and the kernels) ----
// gp_posterior_kernel: exp table | alpha [np] | 1/l (+ pad) | X^T [D][np] when x_in_lds | per wave: xq [D][16], V strip [np][16]
constexpr size_t posterior_lds_doubles(int N, int D, int waves, bool x_in_lds) {
  const size_t np = (size_t)((N + 15) / 16) * 16;
  return 64 + np + D + (D & 1) + (x_in_lds ? (size_t)D * np : 0) + (size_t)waves * (16 * D + np * 16);
}

// gp_posterior_linv_kernel: exp table | alpha [np] | 1/l [d4] | xq [d4][16] | red [32] | |xq|^2 [16] | |x|^2 [np] | K_*^T strip [np][16]
constexpr size_t posterior_linv_lds_doubles(int N, int D) {
  const size_t np = (size_t)((N + 15) / 16) * 16;
  const size_t d4 = (size_t)((D + 3) & ~3);   // query points, 1 / lengthscale zero-padded to the MFMA k-step
  return 64 + np + d4 + 16 * d4 + 32 + 16 + np + np * 16;
}
// ... its JOINTV instantiation (5h): the same carve, then the [256] register image of the strip's Gram tile -- the epilogue lays the
// ceil(Ma / 16) images of the leading tiles into the K_*^T strip, and with Ma > 16 (np / 16 - 1) one more does not fit there
constexpr size_t posterior_linv_jointv_lds_doubles(int N, int D) { return posterior_linv_lds_doubles(N, D) + 256; }

// gp_linv_kernel, gp_cho_solve_kernel: one [np][16] strip per wave
constexpr size_t strip_solve_lds_doubles(int np, int waves) { return (size_t)waves * np * 16; }

// gp_mll_grad_kernel: [4 waves][64][(D + 1) | 1] scaled points + alpha of a super-tile (next to 1 KiB of static LDS)
constexpr size_t mll_grad_lds_doubles(int D) { return (size_t)4 * 64 * ((D + 1) | 1); }

// gp_mll_grad_fused_kernel <NBT = nbt>: buf [2][16][np + 2] | Xs [np][9] + 16 | Xq [np][9] | alpha [np] | per wave 2 x 256 |
// exp table | 1/l [8] | per wave 10.  The launcher sizes every instance for waves = nbt / 2, split workgroups included.
constexpr size_t mll_grad_fused_lds_doubles(int nbt, int waves) {
  const size_t np = (size_t)16 * nbt;
  return 2 * 16 * (np + 2) + 2 * np * 9 + 16 + np + (size_t)waves * 512 + 64 + 8 + (size_t)waves * 10;
}

}  // namespace scaml
