/*
 * scaml_gp.h — C ABI of libscaml_hip.so: the MI355X (gfx950) batched exact-GP inference
 * hot path of ScaML-GP.
 *
 * The reference (boschresearch/Scalable-Meta-Learning-with-Gaussian-Processes) has no
 * FFI: the path sits behind the Python call surface of scamlgp/model.py and, beneath it,
 * gpytorch's operator seam.  Each entry point below cites the reference site(s) whose
 * arithmetic it replaces (paths relative to the reference checkout).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer into memory owned by the caller (e.g. PyTorch's
 *     caching allocator); the library allocates nothing persistent and keeps no state;
 *   - all matrices/stacks are dense, contiguous, row-major fp64:
 *       X      (T, N, D)      point stacks            theta (T, D+2) = [l_0..l_{D-1}, os, noise]
 *       y      (T, N)         standardised targets    L     (T, N, N) lower Cholesky factors
 *       alpha  (T, N)         (K + noise I)^-1 y
 *     theta holds CONSTRAINED values (lengthscales, outputscale, noise variance);
 *   - `n_points` (T) int32, may be NULL: per-task number of valid points n_t <= N (ragged
 *     tasks; rows/cols >= n_t are treated as an identity block and never written);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); work is only
 *     enqueued, never synchronised;
 *   - return value: 0 ok; <0 bad argument (SCAML_E_*); never throws.  Numerical status
 *     is per task in the caller-provided `info` (LAPACK convention: info[t] = k > 0 means
 *     the leading minor of order k is not positive definite after the last jitter try).
 */
#ifndef SCAML_GP_H
#define SCAML_GP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCAML_KIND_RBF 0      /* gpytorch RBFKernel:    exp(-r^2/2)                        */
#define SCAML_KIND_MATERN52 1 /* gpytorch MaternKernel(nu=2.5): (1+√5r+5r²/3)exp(-√5r)      */

/* acquisition codes (`acqf`): UCB, EI, and EI | LOG = 17 for LogEI; SCAML_ACQF_LOG alone is refused */
#define SCAML_ACQF_UCB 0
#define SCAML_ACQF_EI 1
#define SCAML_ACQF_LOG 0x10

#define SCAML_OK 0
#define SCAML_E_BADARG -1      /* NULL pointer / negative size                              */
#define SCAML_E_TOOLARGE -2    /* N or D beyond what the kernels support (see *_max_*)      */
#define SCAML_E_LAUNCH -3      /* hipLaunch / attribute call failed (see scaml_last_error)  */

/* flags for scaml_gp_fit_fused_f64 */
#define SCAML_FIT_STORE_L 1u     /* write L (T,N,N); without it only alpha + scalars (MLL-only mode) */
#define SCAML_FIT_ZERO_UPPER 2u  /* also write zeros to the strict upper triangle of L       */
#define SCAML_FIT_NO_RETRY 4u    /* single attempt: no in-kernel jitter escalation           */

/* Library / limits ------------------------------------------------------------------ */
int scaml_version(void);            /* 10000*major + 100*minor + patch */
const char* scaml_last_error(void); /* text of the last HIP error seen by this thread    */
int scaml_fit_max_n(void);          /* largest N of the register-resident fused fit       */
int scaml_fit_max_d(int N);         /* largest D for that N (LDS budget)                  */

/*
 * (3) Fused "task-posterior": kernel matrix + noise, jittered Cholesky, alpha, quad,
 * logdet and the marginal log-likelihood for a stack of T independent tasks.
 * Replaces, for the whole stack at once, the per-task chain the reference runs inside
 *   scamlgp/model.py:176-188  (for task in meta_data: SingleTaskGP + optimize_marginal_likelihood)
 *   scamlgp/utils.py:171-177  (ExactMarginalLogLikelihood -> MVN.log_prob -> inv_quad_logdet ->
 *                              psd_safe_cholesky -> torch.linalg.cholesky_ex / solve_triangular)
 * with the kernels of scamlgp/model.py:36-70 / :73-105 and the noise of :25-33.
 *   quad[t]   = y^T (K+noise I)^-1 y          logdet[t] = log det (K+noise I)
 *   mll[t]    = -(quad + logdet + n_t log 2pi) / (2 n_t)      (no prior terms)
 * Jitter: like linear_operator's psd_safe_cholesky the first attempt adds nothing; a task
 * whose factorisation hits a non-positive pivot is retried IN-KERNEL with 1e-8, 1e-7, 1e-6
 * added to its diagonal (only that task); jitter_used[t] reports the value that succeeded,
 * info[t] > 0 that all attempts failed.  `jitter_in` (T) may be NULL; if given it is added to
 * every attempt (caller-controlled extra jitter) and is NOT part of jitter_used[t], which reports
 * the ladder's value only (0 for a task that succeeds at the first attempt with jitter_in alone).
 * Linv_diag (T, ceil(N/16), 16, 16), optional: the inverses of the 16x16 diagonal blocks of L
 * (identity-padded past n_t); scaml_posterior_batched_f64 needs them.
 * Outputs L, alpha, quad, logdet, mll, jitter_used, Linv_diag may individually be NULL (not
 * written); info must not be NULL.
 */
int scaml_gp_fit_fused_f64(const double* X, const double* y, const double* theta,
                           const int32_t* n_points, const double* jitter_in,
                           int T, int N, int D, int kind,
                           double* L, double* alpha, double* quad, double* logdet, double* mll,
                           int32_t* info, double* jitter_used, double* Linv_diag, unsigned flags, void* stream);

/*
 * (3b) The same fit for scaml_fit_max_n() < N <= scaml_fit_blocked_max_n() points per task (the 512-point source
 * tasks of scamlgp/benchmarking/configurations/hartmann6_ablation_num_points_per_task.py:17-18, fitted in the
 * reference by the same scamlgp/model.py:176-188 / scamlgp/utils.py:171-177 chain), with no host synchronisation
 * and nothing but this library's kernels (and one memset of a few words) on the stream.  Two implementations behind
 * the one entry point, chosen by shape: while the stack leaves CUs idle (3 T <= #CUs; 2 T <= #CUs for N <= 320;
 * D <= 16) ONE launch in which up to eight workgroups share a task (csrc/gp_fit_coop.hip); otherwise a 2 x 2 block
 * factorisation enqueued as one sequence of launches -- fused fit of the first 256 points in place, L21 =
 * (L11^-1 K12)^T by column strips, Schur complement, fused factorisation of the Schur complement in place, alpha /
 * MLL assembly.  Same results to rounding (tests/test_blocked_fit_gpu.py runs every test through both; info[t] = -1:
 * the one-launch kernel gave a task up after a bounded wait, which no correct run does).  Arguments, outputs and the jitter
 * ladder (one value for the whole matrix of a failing task: 0, 1e-8, 1e-7, 1e-6) are those of
 * scaml_gp_fit_fused_f64; info[t] = k > 0 counts pivots over the full matrix.  Requirements: N a multiple of 16,
 * D <= scaml_fit_blocked_max_d(); L, alpha, info and Linv_diag must be given (the later launches read the earlier
 * ones' results from them), SCAML_FIT_STORE_L is implied.  `workspace` is device memory of at least
 * scaml_gp_fit_blocked_workspace_bytes(T, N) bytes, 16-byte aligned, owned by the caller and free again when the
 * stream has passed the call.  Returns SCAML_E_TOOLARGE for shapes it does not take.
 */
int scaml_fit_blocked_max_n(void);
int scaml_fit_blocked_max_d(void);
long long scaml_gp_fit_blocked_workspace_bytes(int T, int N);
int scaml_gp_fit_blocked_f64(const double* X, const double* y, const double* theta,
                             const int32_t* n_points, const double* jitter_in,
                             int T, int N, int D, int kind,
                             double* L, double* alpha, double* quad, double* logdet, double* mll,
                             int32_t* info, double* jitter_used, double* Linv_diag, unsigned flags,
                             void* workspace, long long workspace_bytes, void* stream);

/*
 * (1) Stand-alone kernel matrix K[t] = os_t k(X1_t / l_t, X2_t / l_t), (T, N1, N2).  X2 == NULL means
 * X2 = X1 (N2 must equal N1; with add_noise != 0 the noise variance is added to the diagonal: the
 * training matrix of scamlgp/model.py:36-70 + :25-33); x2_shared != 0 means X2 is one (N2, D) set
 * used for every task (the cross-kernel K_* of gp.posterior(x), scamlgp/model.py:128).  The fused
 * entry points never materialise K; this one exists for callers that want it.
 */
int scaml_kernel_matrix_f64(const double* X1, const double* X2, const double* theta, int T, int N1, int N2, int D,
                            int kind, int x2_shared, int add_noise, double* K, void* stream);

/*
 * (2) Batched jittered Cholesky of GIVEN symmetric matrices A (T, N, N) (lower triangle read):
 * the psd_safe_cholesky of linear_operator (reached from scamlgp/utils.py:171-177) for a whole
 * stack, same in-kernel jitter escalation, status and outputs as scaml_gp_fit_fused_f64.  With a
 * right-hand side y (T, N) it also returns alpha = A^-1 y, quad = y^T A^-1 y and logdet.  y, alpha,
 * quad, logdet, jitter_used, Linv_diag may be NULL.  N <= scaml_fit_max_n().
 */
int scaml_potrf_batched_f64(const double* A, const double* y, const int32_t* n_points, const double* jitter_in,
                            int T, int N, double* L, double* alpha, double* quad, double* logdet,
                            int32_t* info, double* jitter_used, double* Linv_diag, unsigned flags, void* stream);

/*
 * (5) Batched source-GP posteriors at M query points shared by all tasks.
 * Replaces the per-source loop `[gp.posterior(x) for gp in source_gps]` of
 *   scamlgp/model.py:128 (inside _compute_target_prior) and :281 (ScaMLGP.__init__ caches)
 * i.e. gpytorch's exact prediction mu~ = K_* alpha, Sigma~ = k(x,x) - V^T V with V = L^-1 K_*^T,
 * followed by botorch's Standardize.untransform_posterior (mu = m + s mu~, Sigma = s^2 Sigma~;
 * y_mean / y_std (T) may be NULL = 0 / 1).  No observation noise is added.
 *   Xq (M, D); L, alpha, Linv_diag as produced by scaml_gp_fit_fused_f64 with the same X, theta.
 *   mu (T, M), var (T, M) = diagonal of Sigma, V (T, N, M) = L^-1 K_*^T (un-scaled): each may be
 *   NULL.  N <= scaml_posterior_max_n().
 *   flags: SCAML_POST_XQ_PER_TASK — Xq is (T, M, D), one query set per task;
 *          SCAML_POST_MEAN_ONLY   — only mu = m + s K_* alpha (no solve; L, Linv_diag, var, V unused/NULL).
 * Non-finite query points: a query point with a NaN or infinite coordinate gives NaN in its own mu, var and column of V (and,
 * in (5b), in its row / column of cov); the other query points are not affected.
 */
#define SCAML_POST_XQ_PER_TASK 1u
#define SCAML_POST_MEAN_ONLY 2u
int scaml_posterior_max_n(void);
int scaml_posterior_batched_f64(const double* Xq, const double* X, const double* theta, const double* L,
                                const double* Linv_diag, const double* alpha, const double* y_mean,
                                const double* y_std, const int32_t* n_points, int T, int N, int M, int D, int kind,
                                double* mu, double* var, double* V, unsigned flags, void* stream);

/*
 * (5b) Covariance block of the same posteriors between the first Ma query points and all M:
 *   cov[t][a][c] = y_std[t]^2 (os k(xq_a, xq_c) - sum_i V[t][i][a] V[t][i][c]),  cov (T, Ma, M).
 * With the target's training points placed first in Xq this yields Sigma_nn and Sigma_nq of
 * scamlgp/model.py:287-289 / :131 without recomputing the train block per query.
 */
int scaml_posterior_cov_f64(const double* Xq, const double* theta, const double* V, const double* y_std,
                            int T, int N, int M, int Ma, int D, int kind, double* cov, unsigned flags, void* stream);

/*
 * (5c) The explicit inverse factor Linv = L^-1 (T, N, N; zero above the diagonal; identity rows past n_t) of a
 * fused fit / POTRF, and the source posteriors computed from it.  gpytorch keeps such a cache
 * (DefaultPredictionStrategy.covar_cache, the root of K^-1) for fast predictive variances; here it turns
 * V = L^-1 K_*^T from a substitution with a serial dependency into a triangular matrix product, which is what
 * the BO loop wants: the source GPs of scamlgp/model.py:128, :281 are fixed while every acquisition step
 * scores thousands of candidates.  scaml_posterior_linv_f64 has the semantics of
 * scaml_posterior_batched_f64 (same mu, var, V; SCAML_POST_XQ_PER_TASK allowed, SCAML_POST_MEAN_ONLY not).
 * Non-finite query points, every pass over Linv ((5c), (5c'), (5d), (5e)): a query point with a NaN or infinite coordinate gives NaN
 * in its own mu, var and column of cov -- in (5d) / (5e) in all 16 columns of its strip --, and the other query points are not
 * affected.  The NaN is put back where those results are written; the point's column of V (scaml_posterior_linv_f64) is
 * unspecified (finite): use mu / var to detect such a point.
 */
int scaml_linv_batched_f64(const double* L, const double* Linv_diag, const int32_t* n_points, int T, int N, double* Linv,
                           void* stream);
/* The same inverse factor with only the block rows at or below each 16-column strip's diagonal block written (the 16 x 16
 * diagonal blocks complete, zeros above the diagonal inside them): what scaml_posterior_linv*_f64 read.
 * Everything above is left untouched -- half of the matrix not written (67 of 134 MB at T = 256, N = 256). */
int scaml_linv_batched_lower_f64(const double* L, const double* Linv_diag, const int32_t* n_points, int T, int N, double* Linv,
                                 void* stream);
int scaml_posterior_linv_f64(const double* Xq, const double* X, const double* theta, const double* Linv, const double* alpha,
                             const double* y_mean, const double* y_std, const int32_t* n_points, int T, int N, int M, int D,
                             int kind, double* mu, double* var, double* V, unsigned flags, void* stream);

/*
 * Batched Cholesky solve Xout = (L L^T)^-1 B for R right-hand sides per task, B and Xout (T, N, R), with
 * the L and Linv_diag of a fused fit / POTRF (gpytorch's cholesky_solve behind prediction caches and
 * inv_quad for new right-hand sides).  Forward and backward substitution as blocked MFMA products.
 */
int scaml_cho_solve_batched_f64(const double* L, const double* Linv_diag, const double* B, const int32_t* n_points,
                                int T, int N, int R, double* Xout, void* stream);
/* The backward half alone: Xout = L^-T B (linear_operator's TriangularLinearOperator.solve with upper = True behind
 * the same caches).  With V = L^-1 K_* at hand, K^-1 K_* a = L^-T (V a) needs only this. */
int scaml_solve_lt_batched_f64(const double* L, const double* Linv_diag, const double* B, const int32_t* n_points,
                               int T, int N, int R, double* Xout, void* stream);

/*
 * (6) Weighted sum over the task axis: out[e] = sum_t c_t in[t][e], c_t = w_t (power 1) or w_t^2
 * (power 2), tasks with active[t] == 0 skipped (active may be NULL).  in (T, len), out (len).
 * Replaces scamlgp/model.py:129-135: mean = sum_i w_i mu_i (power 1), cov = sum_i w_i^2 Sigma_i
 * (power 2, PsdSumLinearOperator) over the significant tasks of model.py:368-372.
 */
int scaml_weighted_task_sum_f64(const double* in, const double* w, const uint8_t* active, int T, long long len,
                                int power, double* out, void* stream);

/*
 * (6') The ScaML-GP target prior of scamlgp/model.py:108-135 in one call, on the outputs of (5)/(5b):
 *   mu_s[q] = sum_t w_t mu[t][q]  (mu (T, M)),   cov_s[a][q] = sum_t w_t^2 cov[t][a][q]  (cov (T, Ma, M)),
 * over the tasks with active[t] != 0 (the pruning mask of model.py:368-372; NULL = all).  Either of mu / cov may
 * be NULL.  Two launches of the weighted-sum kernel.
 */
int scaml_weighted_prior_reduce_f64(const double* mu, const double* cov, const double* w, const uint8_t* active, int T, int M,
                                    int Ma, double* mu_s, double* cov_s, void* stream);

/*
 * (4) Analytic gradient of mll[t] (as defined for scaml_gp_fit_fused_f64, no prior terms) w.r.t. the
 * constrained hyper-parameters theta[t] = [l_0..l_{D-1}, os, noise].  Replaces the autograd pass of
 * botorch's fit_gpytorch_mll through kernel, Cholesky and solve (scamlgp/utils.py:175, 190).
 *   d mll / d theta_p = (1 / 2 n_t) sum_ij (alpha alpha^T - K^-1)_ij dK_ij / d theta_p.
 * Inputs are the X, theta and the L, Linv_diag, alpha produced by the fused fit.  `workspace` must
 * hold scaml_mll_backward_workspace_doubles(T, N, D) doubles (L^-1 per task, then per-tile partial
 * sums).  Result: partial sums (T, tiles, D+2), tiles = nb (nb+1)/2 with nb = ceil(N/16), written
 * to `partials_out` if given, else to the tail of the workspace; the caller adds them over the tile
 * axis and divides by 2 n_t (deterministic: no atomics).  Only the sum over the tile axis is defined: the
 * kernel works on 2 x 2 groups of tiles and leaves a group's total in the slot of its first tile.  D <= 76.
 */
long long scaml_mll_backward_workspace_doubles(int T, int N, int D);
int scaml_mll_backward_f64(const double* X, const double* theta, const double* L, const double* Linv_diag,
                           const double* alpha, const int32_t* n_points, int T, int N, int D, int kind,
                           double* workspace, double* partials_out, void* stream);

/*
 * (5c') The covariance block of (5b) fused into the posterior pass of (5c): with VA = V[:, :Ma] (T, N, Ma) -- the V of the
 * first Ma query points, produced by a call of scaml_posterior_linv_f64 on those points alone -- one pass over all M
 * query points gives mu, var AND cov (T, Ma, M) = s_t^2 (os k(xq_a, xq_c) - VA^T V); V (T, N, M) itself never reaches
 * memory (at BASELINE configs[4]: 145 MB not written and not re-read per acquisition-function evaluation).  Replaces the
 * same reference sites as (5) / (5b): scamlgp/model.py:128-134, 281-289.  Ma <= 96, Ma <= N, Ma <= M.
 */
int scaml_posterior_linv_cov_f64(const double* Xq, const double* X, const double* theta, const double* Linv, const double* alpha,
                                 const double* y_mean, const double* y_std, const int32_t* n_points, const double* VA, int T, int N,
                                 int M, int Ma, int D, int kind, double* mu, double* var, double* cov, unsigned flags, void* stream);

/*
 * (7) Target GP posterior on top of the weighted source prior (scamlgp/model.py:359-384 eval branch, then gpytorch's
 * exact prediction: botorch GPyTorchModel.posterior -> ExactGP.__call__ in eval mode).
 * The reference evaluates it per acquisition-function call with ~40 small torch ops; here it is four launches and no
 * host synchronisation:
 *   scaml_target_assemble_f64   Knn = cov_s[:, :n] / s^2 + os_t k_t(Xt, Xt) + noise I,  Knq = cov_s[:, n:] / s^2 + os_t k_t(Xt, Xq),
 *                               resid = y~ - (mean_s[:n] - m) / s,  mean_q = (mean_s[n:] - m) / s,  var_q = var_s[n:] / s^2 + os_t
 *   scaml_potrf_batched_f64     (T = 1) L L^T = Knn with psd_safe_cholesky's jitter ladder, alpha = Knn^-1 resid
 *   scaml_cho_solve_batched_f64 (T = 1, R = M) Z = Knn^-1 Knq
 *   scaml_target_finish_f64     mu[q] = m + s (mean_q + Knq[:, q] . alpha),  var[q] = s^2 (var_q - Knq[:, q] . Z[:, q] + noise_add);
 *                               `info` (1) int32 or NULL: the POTRF's status -- a factorisation that failed even with jitter
 *                               (psd_safe_cholesky would raise NotPSDError) turns every output into NaN on the device
 * Inputs: cov_s (n, n + M), mean_s (n + M), var_s (n + M) from (6') at cat(train_X, Xq); Xall (n + M, D) = cat(train_X, Xq);
 * theta (D + 2) of the TARGET kernel; train_targets (n) standardised with (m_all, s_all).  n >= 1.
 * Non-finite query points: a query point with a NaN or infinite coordinate gives NaN in exactly its column of Knq from the assemble
 * (mean_q / var_q carry whatever the source sums hold: NaN from (5) / (5c)), hence in its column of Z and in its mu and var from the
 * finish; the other query points are not affected.  (tests/_target_bounds.py states the accuracy every stage is held to.)
 */
int scaml_target_assemble_f64(const double* cov_s, const double* mean_s, const double* var_s, const double* Xall,
                              const double* theta, const double* train_targets, double m_all, double s_all, int n, int M, int D,
                              int kind, double* Knn, double* resid, double* Knq, double* mean_q, double* var_q, void* stream);
int scaml_target_finish_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                            double m_all, double s_all, double noise_add, const int32_t* info, int n, int M, double* mu, double* var,
                            void* stream);

/*
 * (5d) Input gradients of the posterior -- what botorch's optimize_acqf differentiates through model.posterior for when it
 * maximises the acquisition function (the caller behind scamlgp/utils.py:215-224; SURVEY 3.3, HOT LOOP #4; the reference gets
 * them from torch autograd through kernel, solves and PsdSum per L-BFGS-B iteration).
 * scaml_posterior_linv_grad_f64: the (5c') pass with 16 output columns per query point x_q = [value, d/dx_0 .. d/dx_{D-1}, 0 ..]:
 *   mu  (T, Mq, 16): mu[t][q][0] = posterior mean of source t at x_q,   mu[t][q][1 + d]  = d mean / d x_d
 *   var (T, Mq, 16): var[t][q][0] = posterior variance,                 var[t][q][1 + d] = d variance / d x_d
 *   cov (T, Ma, Mq * 16): cov[t][a][16 q] = Cov(f(xa_a), f(x_q)),       cov[t][a][16 q + 1 + d] = d Cov / d x_d
 * (un-standardised with y_mean / y_std as in (5)), Xq (Mq, D) the query points, Xa (Ma, D) the Ma leading points (the target's
 * training inputs) and VA (T, N, Ma) their V as in (5c').  Ma = 0: no covariance block (VA, Xa, cov may be NULL).  D <= 15, Ma <= 96.
 * scaml_target_posterior_grad_f64: d mu* / d x (Mq, D) and d var* / d x (Mq, D) of the ScaML-GP TARGET posterior (original units;
 * scamlgp/model.py:359-384 eval branch + gpytorch's exact prediction) from the weighted task sums of those outputs
 * (cov_g (n, Mq * 16), mu_g / var_g (Mq * 16): (6') applied to cov / mu / var above), the target inputs Xt (n, D), the target
 * kernel theta (D + 2), and alpha (n), Z (n, Mq) = Knn^-1 Knq of the value path ((7): the POTRF's alpha, the Cholesky solve's result).
 * info (1) int32 or NULL: a failed target factorisation turns the outputs into NaN.
 * Non-finite query points (scaml_target_posterior_grad_f64): a query point with a NaN or infinite coordinate gives NaN in EVERY entry
 * of its dmu and dvar, whatever mu_g / var_g / cov_g hold for it (the kernel clamps drop a NaN: without this only the entry of that
 * coordinate would show it); the other query points are not affected.  D > 15: SCAML_E_TOOLARGE, nothing is written.
 */
int scaml_posterior_linv_grad_f64(const double* Xq, const double* Xa, const double* X, const double* theta, const double* Linv,
                                  const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                  const double* VA, int T, int N, int Mq, int Ma, int D, int kind, double* mu, double* var, double* cov,
                                  unsigned flags, void* stream);
int scaml_target_posterior_grad_f64(const double* cov_g, const double* mu_g, const double* var_g, const double* Xt, const double* Xq,
                                    const double* theta, const double* alpha, const double* Z, double s_all, const int32_t* info, int n,
                                    int Mq, int D, int kind, double* dmu, double* dvar, void* stream);

/*
 * (7f) The acquisition function of a FANTASY model (ScaMLGP.fantasize: the target GP conditioned on p pending points with F sampled
 * outcomes each; Monte-Carlo integration over the pending evaluations) in place of (7)'s finish and (5d)'s target gradient:
 *   mu_f[q]  = m + s (mean_q[q] + Knq[:, q] . alpha[:, f])             f = 0 .. F-1, alpha (n, F) = Knn^-1 [r_0 .. r_{F-1}]
 *   v[q]     = s^2 (var_q[q] - Knq[:, q] . Z[:, q] + noise_add)         (shared by all fantasies)
 *   value[q] = (1/F) sum_f A(mu_f[q], v[q])
 * acqf 0: UCB, A = -mu + sqrt(beta max(v, 0)), acqf_param = beta; acqf 1: EI (minimisation), sigma = sqrt(max(v, 1e-9)),
 * u = -(mu - best_f) / sigma, A = sigma (phi(u) + u Phi(u)), acqf_param = best_f.  Knq, Z (n, M), mean_q, var_q (M) as in (7).
 * acqf 17 (SCAML_ACQF_EI | SCAML_ACQF_LOG): LogEI, the logarithm of EI, with EI's clamp and acqf_param:
 *   A = log sigma + g(u),  g(u) = log(phi(u) + u Phi(u)),  dA/dmu = -g'(u) / sigma,  dA/dv = (1 - u g'(u)) / (2 sigma^2) above the
 *   floor and exactly 0 on it (v <= 1e-9), as EI has it.  g and g' are evaluated without cancellation (a continued fraction of the
 *   Mills ratio below u = -2, csrc/gp_studies_formulas.h): finite and accurate to a few ulp for u in [-1e8, 40], where EI and its
 *   gradient are exactly 0 below u of about -38.  Over the fantasies the average is taken in the log domain, the log of the mean EI:
 *   value[q] = mx + log(sum_f exp(A_f - mx)) - log F with mx = max_f A_f, and the gradient weights each fantasy's chain-rule factors
 *   by exp(A_f - mx) / sum_f' exp(A_f' - mx) in place of the 1 / F.  F = 1 gives A_0 and its gradient bit for bit.
 * Any other code (2, 3, 0x10 alone, 0x12, negative) is SCAML_E_BADARG, here and on every entry point that takes `acqf`.
 * grad (M, D) or NULL: d value / d x_q from the GRAD pass's weighted sums (cov_g (n, M * 16), mu_g / var_g (M * 16)), the training
 * inputs Xt (n, D), the queries Xq (M, D) and the target kernel theta (D + 2) of family `kind`, as (5d) takes them; the gradient
 * contracts over the training points once per query with abar = sum_f dA/dmu_f alpha[:, f].  info (1) int32 or NULL: a factorisation
 * that failed even with jitter turns every output into NaN.  One wave per query point, no host synchronisation.
 * Non-finite queries: a query point with a NaN or infinite coordinate in Xq[q] gives NaN in EVERY entry of grad[q], whatever mu_g /
 * var_g / cov_g hold (as (5d)), and a query whose value[q] is NaN (a NaN in its column of Knq or Z, in mean_q[q] or var_q[q]) gives NaN
 * in every entry of grad[q] too; the other query points are not affected.  (value[q] itself reads no coordinate.)
 * Limits: F <= 64, n <= scaml_fit_max_n(); with grad also n <= 96 and D <= 15.  SCAML_E_TOOLARGE beyond them.
 */
int scaml_target_fantasy_acqf_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                  double m_all, double s_all, double noise_add, const int32_t* info, int acqf, double acqf_param,
                                  const double* cov_g, const double* mu_g, const double* var_g, const double* Xt, const double* Xq,
                                  const double* theta, int n, int M, int F, int D, int kind, double* value, double* grad, void* stream);

/*
 * (5g), (7p) JOINT q-point Monte-Carlo acquisition (qEI, qUCB) with exact input gradients: B batches X_b = (x_1 .. x_q) of query points
 * that are scored -- and moved by the optimiser -- together, Mq = B q points in all (botorch's optimize_acqf(q = ...) on a
 * Monte-Carlo acquisition function over the joint posterior; scamlgp_amd.ScaMLGP.joint_acqf, utils.qExpectedImprovement /
 * qUpperConfidenceBound, ScaMLGPBOLoop.suggest_batch).
 * scaml_posterior_linv_grad_joint_f64 (5g): (5d) with q more rows in the covariance block of every strip.  VQ (T, N, Mq): the V of ALL
 *   Mq query points from one value pass (5c) that keeps V;  cov (T, Ma + q, Mq * 16).  Rows a < Ma of strip j are (5d)'s (against the
 *   leading points Xa / VA); row Ma + r is the covariance of x_j with its batch mate x_{b q + r}, b = j / q (V: column b q + r of VQ,
 *   coordinates: Xq[b q + r]): column 16 j the covariance, columns 16 j + 1 + d its derivative with respect to x_j WITH THE MATE HELD
 *   FIXED -- the row of the point itself (r = j mod q) therefore holds var and half of var's derivative.  mu, var as (5d) (may be NULL).
 *   Ma >= 1, Mq a multiple of q; NULL Xa / VA / VQ / cov, q < 1: SCAML_E_BADARG.  q <= scaml_qacqf_max_q() = 8, Ma + q <= 96,
 *   Ma + q <= N, D <= 15 and (5d)'s limits: SCAML_E_TOOLARGE beyond them.  Everything is checked before the first HIP call.
 * scaml_target_qacqf_f64 (7p): per batch, from the value path's outputs as (7f) takes them (Knq, Z (n, Mq), alpha (n), mean_q, var_q
 *   (Mq), m_all, s_all, info) and the weighted task sums (6') of (5g) as (7f) takes those of (5d) (cov_g (n + q, Mq * 16), mu_g, var_g
 *   (Mq * 16)):
 *     mu_j  = m + s (mean_q[j] + Knq[:, j] . alpha)
 *     S_jk  = P_jk - Knq[:, j] . Z[:, k],  P_jj = var_q[j],  P_jk = cov_g[n + k][16 j] / s^2 + os_t k_t(x_j, x_k),  Sigma = s^2 S
 *             (no observation noise)
 *     C C^T = Sigma + jitter I;  the ladder 0, 1e-8, 1e-7, 1e-6 of psd_safe_cholesky: an attempt fails on a pivot <= 0 or not finite,
 *             after the fourth failure info_out[b] = 1 and the batch's outputs are NaN.  The jitter is a constant for the gradient.
 *     f_s   = mu + C eps_s with the caller's base samples eps = base_samples (S, q), shared by all batches
 *     acqf SCAML_ACQF_EI  (acqf_param = best_f): a_s = max_j max(best_f - f_sj, 0)          (minimisation, as everywhere)
 *     acqf SCAML_ACQF_UCB (acqf_param = beta):   a_s = max_j (-mu_j + sqrt(beta pi / 2) |(C eps_s)_j|)
 *     value[b] = (1/S) sum_s a_s
 *   Every other code -- 17 (LogEI) and 0x10 among them -- is SCAML_E_BADARG here: a joint LogEI is not defined.
 *   grad (Mq, D) or NULL: d value[b] / d x_j for the q points of batch b.  Sub-gradients: the arg-max is the lowest j that attains the
 *   maximum; max(., 0) and |.| have slope 0 at 0.  Adjoint: mubar and Cbar summed over the samples, Phi = tril(C^T Cbar) with its
 *   diagonal halved, Sigmabar = sym(C^-T Phi C^-1), Sbar = s^2 Sigmabar, mbar = s mubar; then
 *     grad_j = mbar_j dm_j/dx_j + Sbar_jj dvar_q[j]/dx_j + 2 sum_{k != j} Sbar_jk dP_jk/dx_j - (dKnq[:, j]/dx_j)^T (2 sum_k Sbar_jk Z[:, k])
 *   and the sum over the training points is contracted once per query point against mbar_j alpha - 2 sum_k Sbar_jk Z[:, k], as (7f)
 *   does with its abar.  jitter_used (B) or NULL: the rung that passed.  info_out (B) int32 or NULL.
 *   One workgroup per batch; the q x q work is done in LDS, the samples are dealt to the threads, every sum over the samples is formed
 *   by one thread in a fixed order: no atomics, the outputs are a pure function of the inputs (two calls agree bit for bit).
 *   Non-finite values: a query point with a NaN / infinite coordinate, or a NaN in anything the batch's VALUE reads (its columns of
 *   Knq, Z, mean_q, var_q, a value column 16 j of a mate row), gives NaN in that batch's value and in all q rows of its grad -- where
 *   it enters Sigma, the ladder fails on it (jitter NaN, info_out 1); other batches are not affected.  A NaN base sample is shared: the value and
 *   the gradient of EVERY batch are NaN (jitter and info_out are the factor's).  A NaN that only the gradient reads -- a derivative
 *   column 16 j + 1 + d of mu_g, var_g or any row of cov_g -- leaves value, jitter and info_out finite and gives NaN in EVERY entry of
 *   point j's row of grad, never in some of them (a select where the row is stored: finite inputs keep their bits); the other rows
 *   are not affected.  info[0] != 0 (the target's factorisation failed): every output is NaN (info_out 1).
 *   Limits: 1 <= q <= scaml_qacqf_max_q() = 8, 1 <= S <= scaml_qacqf_max_samples() = 512, n + q <= 96, D <= 15: SCAML_E_TOOLARGE
 *   beyond them; n < 1, Mq not a multiple of q, a NULL input or value, s_all <= 0, an unknown kind: SCAML_E_BADARG (first).  Mq == 0
 *   enqueues nothing.  No host synchronisation.
 */
int scaml_qacqf_max_q(void);
int scaml_qacqf_max_samples(void);
int scaml_posterior_linv_grad_joint_f64(const double* Xq, const double* Xa, const double* X, const double* theta, const double* Linv,
                                        const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                        const double* VA, const double* VQ, int T, int N, int Mq, int Ma, int q, int D, int kind, double* mu,
                                        double* var, double* cov, unsigned flags, void* stream);
int scaml_target_qacqf_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q, double m_all,
                           double s_all, const int32_t* info, const double* cov_g, const double* mu_g, const double* var_g, const double* Xt,
                           const double* Xq, const double* theta, const double* base_samples, int acqf, double acqf_param, int n, int Mq, int q,
                           int S, int D, int kind, double* value, double* grad, double* jitter_used, int32_t* info_out, void* stream);

/*
 * (7q) (7p) with p EVALUATIONS PENDING (botorch's X_pending): every batch is its q moving points followed by the same p pending
 * points Xp (p, D); the joint vector has Q = q + p entries (moving first, pending point k at index q + k), the utility's maximum runs
 * over all Q of them, base_samples is (S, q + p), and only the q moving points get a gradient (grad (Mq, D)): a pending point is held
 * fixed.  scamlgp_amd.ScaMLGP.joint_acqf(X_pending=...), utils.qExpectedImprovement / qUpperConfidenceBound(X_pending=...),
 * ScaMLGPBOLoop(joint_pending="joint").suggest_batch.
 * The pending points are the same in every batch, so they are LEADING points of (5g), not batch mates: call (5g) with
 * Xa = cat(Xt, Xp), VA = cat(V_train, V_pending), Ma = n + p.  The source pass then keeps B q strips, and cov_g is
 * (n + p + q, Mq * 16): rows a < n the training points, rows n + k pending point k, rows n + p + r batch mate r.
 *   Zp (n, p) = Knn^-1 Knp;  mu_p (p), Sigma_pp (p, p): the target posterior of the pending points among themselves, original units,
 *   no observation noise (they do not depend on the batch: computed once per pending set).
 *   mu_j, S_jk for j, k < q: (7p)'s, the mate rows read at n + p + k.
 *   S_{j, q+k} = cov_g[n + k][16 j] / s^2 + os_t k_t(x_j, xp_k) - Knq[:, j] . Zp[:, k],  Sigma = s^2 S   (j < q)
 *   the pending block of Sigma and mu: Sigma_pp (its lower triangle is read) and mu_p as given.
 *   The ladder, f = mu + C eps, qEI / qUCB, the lowest-index arg-max and the adjoint (mubar, Cbar, Phi, Sigmabar) are (7p)'s at Q.
 *   grad_j = (7p)'s terms + 2 sum_k Sbar_{j,q+k} dP_{j,q+k}/dx_j (the source part from columns 16 j + 1 + d of row n + k, the target
 *   kernel's slope against xp_k), and the weight vector on dKnq[:, j] is
 *   mbar_j alpha - 2 sum_{k<q} Sbar_jk Z[:, k] - 2 sum_{k<p} Sbar_{j,q+k} Zp[:, k].  The pending rows of mbar and Sbar are not used.
 *   One workgroup of 256 threads per batch, the Q x Q work in LDS, every sum over the samples by one thread in (7p)'s fixed order: no
 *   atomics, two calls agree bit for bit, and with p == 0 the outputs are (7p)'s bits (Xp, Zp, mu_p, Sigma_pp may be NULL then).
 *   Non-finite values: a NaN / infinite coordinate of a moving point turns its batch NaN (value and its q rows of grad) as in (7p);
 *   a NaN anywhere in Xp, Zp, mu_p or Sigma_pp turns EVERY batch NaN, the pending set being shared.  info[0] != 0 as in (7p).
 *   Limits: 1 <= q, 0 <= p, q + p <= scaml_qacqf_max_q() = 8, n + p + q <= 96, S <= 512, D <= 15: SCAML_E_TOOLARGE beyond them;
 *   (7p)'s bad arguments, p < 0, or a NULL Xp / Zp / mu_p / Sigma_pp with p > 0: SCAML_E_BADARG (first).  Mq == 0 enqueues nothing.
 *   No host synchronisation.
 */
int scaml_target_qacqf_pending_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                   double m_all, double s_all, const int32_t* info, const double* cov_g, const double* mu_g,
                                   const double* var_g, const double* Xt, const double* Xq, const double* theta, const double* base_samples,
                                   const double* Xp, const double* Zp, const double* mu_p, const double* Sigma_pp, int acqf,
                                   double acqf_param, int n, int Mq, int q, int p, int S, int D, int kind, double* value, double* grad,
                                   double* jitter_used, int32_t* info_out, void* stream);

/*
 * (5h), (7r) The joint acquisition VALUE ONLY: what the scoring stage of a batch optimiser needs of its raw candidates -- no
 * derivative column is computed or stored anywhere.  scamlgp_amd.ScaMLGP.joint_acqf_value, utils.qExpectedImprovement /
 * qUpperConfidenceBound(score_mode="value_pass"), ScaMLGPBOLoop(joint_score_mode="value_pass").
 * Column packing (csrc/gp_qacqf_columns.h): the B batches of q points are laid into strips of 16 columns, whole batches only --
 *   bps = 16 / q batches per strip (integer division), point j of batch b in column 16 (b / bps) + (b % bps) q + j,
 *   Mp = scaml_qacqf_value_columns(B, q) = 16 ceil(B / bps) columns (-1 for q outside 1 .. 8 or B < 0).  Dense for q in {1, 2, 4, 8};
 *   q = 3, 5, 6, 7 leave 1, 1, 4, 2 padding columns per strip, and the last strip is padded behind batch B - 1.
 * scaml_posterior_linv_cov_joint_f64 (5h): (5c') -- the value pass with its fused covariance block against Ma leading points Xa
 *   (Ma, D) / VA (T, N, Ma) -- at the PACKED query points Xq (Mp, D), with q more covariance rows: cov (T, Ma + q, Mp).  Rows a < Ma
 *   are (5c')'s.  Row Ma + r of column c is s_t^2 (os k(x_c, x_mate) - G[mate][c]) with the mate = point r of c's batch and
 *   G = V^T V the Gram tile of the strip's V with itself, formed on the matrix cores from the V block in its accumulator (V never
 *   reaches memory); the row of the point itself (r = c's index in its batch) is its variance.  Rows Ma + r of a padding column are
 *   zeros.  Padding columns of Xq must hold finite coordinates (their mu / var / leading rows are computed like any point's).
 *   mu, var (T, Mp) or NULL.  Pending evaluations are leading points exactly as in (7q): Xa = cat(Xt, Xp), Ma = n + p.
 *   Non-finite values: a query point with a NaN / infinite coordinate gives NaN in its own mu, var and column of cov, as in (5c);
 *   the other columns -- those of its strip included -- are not affected (mate rows that involve it need not show the NaN: (7r)
 *   tests the batch's coordinates itself).
 *   T < 0, N < 1, Mp < 0, Ma < 1, B < 0, q < 1, D < 1, a NULL Xq / Xa / X / theta / Linv / alpha / VA / cov, an unknown kind,
 *   SCAML_POST_MEAN_ONLY, or (q <= 8) Mp != scaml_qacqf_value_columns(B, q): SCAML_E_BADARG (first).  q > 8, Ma + q > 96, Ma + q > N,
 *   N > scaml_posterior_max_n(): SCAML_E_TOOLARGE.  Everything is checked before the first HIP call.  B == 0 enqueues nothing.
 * scaml_target_qacqf_value_f64 (7r): (7p) / (7q) without the gradient, for p >= 0 pending points, from the value layout: Knq, Z
 *   (n, Mp), mean_q, var_q (Mp) and Xq (Mp, D) are read at the batch's columns, and cov_s (n + p + q, Mp) -- the weighted sums (6')
 *   of (5h) -- replaces cov_g:  P_jk = cov_s[n + p + k][col(b, j)] / s^2 + os_t k_t(x_j, x_k), the mixed block of a pending point k
 *   from cov_s[n + k][col(b, j)].  mu, Sigma, the ladder, f = mu + C eps, qEI / qUCB and the lowest-index arg-max are (7p)'s / (7q)'s:
 *   given the same numbers in both layouts value, jitter_used and info_out are those kernels' bit for bit (same sums, same order),
 *   and two calls agree bit for bit.  base_samples (S, q + p).  Outputs: value (B), jitter_used (B) or NULL, info_out (B) or NULL.
 *   Non-finite values as (7p) / (7q): a NaN / infinite coordinate of a batch's point or a NaN in its inputs turns that batch NaN;
 *   a NaN anywhere in Xp, Zp, mu_p or Sigma_pp turns every batch NaN; info[0] != 0 turns everything NaN (info_out 1).
 *   Limits and refusals are (7q)'s: q + p <= 8, n + p + q <= 96, S <= 512, D <= 15 (SCAML_E_TOOLARGE); its bad arguments, every
 *   acquisition code but SCAML_ACQF_EI / SCAML_ACQF_UCB, B < 0 or Mp != scaml_qacqf_value_columns(B, q): SCAML_E_BADARG (first).
 *   One workgroup of 256 threads per batch.  B == 0 enqueues nothing.  No host synchronisation.
 */
int scaml_qacqf_value_columns(int B, int q);
int scaml_posterior_linv_cov_joint_f64(const double* Xq, const double* Xa, const double* X, const double* theta, const double* Linv,
                                       const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                       const double* VA, int T, int N, int Mp, int Ma, int B, int q, int D, int kind, double* mu, double* var,
                                       double* cov, unsigned flags, void* stream);
int scaml_target_qacqf_value_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                 double m_all, double s_all, const int32_t* info, const double* cov_s, const double* Xq, const double* theta,
                                 const double* base_samples, const double* Xp, const double* Zp, const double* mu_p, const double* Sigma_pp,
                                 int acqf, double acqf_param, int n, int Mp, int B, int q, int p, int S, int D, int kind, double* value,
                                 double* jitter_used, int32_t* info_out, void* stream);

/*
 * (7o)The acquisition function of M given posteriors, elementwise: A[i] and its partial derivatives Amu[i] = dA / dmu, Av[i] = dA / dv
 * at (mu[i], var[i]) (original units), i = 0 .. M-1, one thread per element -- the statement (7f), (7g), (7i) and (7k) evaluate
 * (sa_acquisition of csrc/gp_studies_formulas.h), with their clamps.  acqf: SCAML_ACQF_UCB (acqf_param = beta), SCAML_ACQF_EI or
 * SCAML_ACQF_EI | SCAML_ACQF_LOG (acqf_param = best_f); anything else is SCAML_E_BADARG.  Amu and Av may be NULL.  The input gradient
 * of an ordinary model's acquisition value is Amu * dmu + Av * dvar with (5d)'s dmu, dvar.  A NaN mu or var gives NaN.
 * M == 0 enqueues nothing; M < 0 or a NULL mu / var / A with M > 0: SCAML_E_BADARG.  No host synchronisation.
 */
int scaml_acqf_transform_f64(const double* mu, const double* var, double acqf_param, int M, int acqf, double* A, double* Amu, double* Av,
                             void* stream);

/*
 * (5e), (7g) The acquisition function of MANY Bayesian-optimisation studies against one source stack, evaluated in two launches
 * whatever their number: every study's start points of the acquisition optimiser in one pass (scamlgp_amd.bo.ScaMLGPBOStudies with
 * suggest_mode="lockstep"), where (5d) + (6') + (7) + (5d)'s target gradient run once per study.
 * scaml_posterior_linv_grad_grouped_f64: (5d)'s source pass with the Mq query points divided among G groups (studies).
 *   group (Mq) int32: the group of query q; a negative entry is a padding row -- its strips of mu / var are zeros, nothing of any
 *       group is read for it and no row of cov is written.
 *   n_points_a (G) int32, 1 <= Ma_g <= Ma_max: the leading points (the study's training inputs) per group.
 *   Xa (G, Ma_max, D): their coordinates, padded; VA_tab (G): DEVICE array of device pointers, VA_tab[g] = the group's V as in (5c'),
 *       (T, N, Ma_g) with row stride Ma_g (the models cache it: no padded copy).
 *   mu, var (T, Mq, 16) as in (5d); cov (T, Ma_max, Mq * 16): rows a < Ma_{group[q]} of strip q are written, the rest is untouched.
 *   Limits: D <= 15, Ma_max <= 96 and <= N, N <= scaml_posterior_max_n().  Mq == 0, G == 0 or T == 0: nothing is enqueued.
 * scaml_target_acqf_batched_f64: per query q of group g = group[q], from (5e)'s mu / var / cov (cov with n_max rows per task) and the
 * group's slices of  w (G, T) weights (zero where pruned) and active (G, T) uint8 (a masked task is skipped),  Xt (G, n_max, D),
 * theta (G, D + 2),  L (G, n_max, n_max) / Linv_diag (G, ceil(n_max / 16), 16, 16): the factor of Knn as (2) returns it for the
 * group's n_g points, in the leading block of its slice,  alpha (G, n_max) = Knn^-1 resid,  n_points (G) int32,  m_all, s_all (G),
 * info (G) int32,  acqf_param (G) (acqf 0: beta, acqf 1: best_f, as (7f)):
 *   the weighted sums of the 16 columns over the active tasks (t ascending), Knq[a] = cov_g[a][0] / s^2 + os k_t(Xt_a, x_q),
 *   mean_q / var_q as (7)'s assemble, z = Knn^-1 Knq against the factor, mu* / var* as (7)'s finish, their input gradients as (5d)'s
 *   target gradient, then value (Mq) = UCB or EI and grad (Mq, D) (may be NULL) with (7f)'s clamps.  mu_out, var_out (Mq) or NULL:
 *   the posterior itself.  Sums run in a fixed order (tasks, then training points, ascending): the result is a pure function of the
 *   inputs.  info[g] != 0 (or n_points[g] outside 1 .. n_max) turns that group's outputs into NaN; a padding query gives zeros.
 *   What lies past n_g in a group's slices is never read.  A query point with a NaN or infinite coordinate gives NaN in its value, every
 *   entry of its grad, mu_out and var_out, as in (5d) / (7); the other query points are not affected.
 *   Limits: n_max <= 96, D <= 15; SCAML_E_TOOLARGE beyond them (bad arguments answer first).  Mq == 0 or G == 0: nothing is enqueued.
 * Neither call synchronises; every status stays on the device (both can be stream-captured).
 */
int scaml_posterior_linv_grad_grouped_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                          const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                          const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points, int T,
                                          int N, int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var, double* cov,
                                          void* stream);
int scaml_target_acqf_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                  const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                  const double* Linv_diag, const double* alpha, const int32_t* n_points, const double* m_all,
                                  const double* s_all, const int32_t* info, const double* acqf_param, int Mq, int G, int n_max, int T,
                                  int D, int kind, int acqf, double* value, double* grad, double* mu_out, double* var_out, void* stream);

/*
 * (5e') (5e) for studies that each own their source tasks (one source stack per study, scamlgp/benchmarking/local_runner.py:51-65:
 * every study draws its own meta-tasks): the source arrays hold the tasks of ALL studies, Tsrc of them, and a group reads T of them.
 *   task_base (G) int32: task slot t (0 <= t < T) of group g is source task src = task_base[g] + t.  X, theta, Linv, alpha, y_mean,
 *       y_std and n_points -- (Tsrc, ...) arrays here -- are read at src; mu, var, cov and VA_tab[g] (T, N, Ma_g) stay indexed by the
 *       slot, so (7g) takes the results with w / active (G, T) unchanged.
 *   A src outside 0 .. Tsrc-1 makes (slot, query) a padding row: zeros in its strips of mu / var, no row of cov written, nothing read.
 *   The grid is T x Mq workgroups as in (5e); a slot's workgroups stay on one XCD, and a study's query points are neighbours there.
 *   Checks and limits: those of (5e), and task_base != NULL, Tsrc >= 1 (SCAML_E_BADARG).  Mq == 0, G == 0 or T == 0: nothing is enqueued.
 * With task_base[g] = 0 for every g and Tsrc = T the results equal (5e)'s within the pass's own run-to-run scatter (the means are summed
 * with LDS float atomics, and this is another kernel instance).
 */
int scaml_posterior_linv_grad_grouped_own_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                              const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                              const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                              int T, int N, int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var,
                                              double* cov, const int32_t* task_base, int Tsrc, void* stream);

/*
 * (5f), (5f') The grouped pass in VALUE mode: (5c')'s posteriors and covariance block for a TABLE of candidates divided among G groups
 * -- stage 1 of the studies' acquisition optimiser (scamlgp_amd.bo.ScaMLGPBOStudies with score_mode="batched"): every study's raw
 * candidates in one launch, no gradient columns.  The arguments are (5e)'s / (5e')'s; what differs:
 *   Mq: the number of candidates, a multiple of 16 (SCAML_E_BADARG otherwise).  A strip is 16 DIFFERENT query points of ONE group.
 *   group (Mq / 16) int32: the group of a strip.  A negative or out-of-range entry marks a padding strip: zeros in its 16 entries of
 *       mu / var, no row of cov written, nothing of any group read -- as (5e) treats a padding row.
 *   mu, var (T, Mq); cov (T, Ma_max, Mq): rows a < Ma_g of a strip are written, the rest is untouched.
 *   The group's leading points, count and V pointer (Xa, n_points_a, VA_tab) are (5e)'s; task_base / Tsrc are (5e')'s.
 * Limits and error codes: those of (5e) / (5e'), everything checked before the first HIP call.  Mq == 0, G == 0 or T == 0: nothing is
 * enqueued.  A candidate with a non-finite coordinate gives NaN in its own mu, var and column of cov only.
 */
int scaml_posterior_linv_grouped_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                     const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                     const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points, int T, int N,
                                     int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var, double* cov, void* stream);
int scaml_posterior_linv_grouped_own_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                         const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                         const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points, int T,
                                         int N, int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var, double* cov,
                                         const int32_t* task_base, int Tsrc, void* stream);

/*
 * (8) The target GP's training objective with its analytic gradient, and the whole refit, in ONE launch.
 * Replaces what the reference runs on every report(): scamlgp/optimizer.py:176-185 rebuilds ScaMLGP and calls
 * optimize_marginal_likelihood (scamlgp/utils.py:139-212), which drives scipy L-BFGS-B through torch autograd over
 *   mll(z) = [ log N(y~ | mean, cov + noise I) + sum log priors ] / n                       (scamlgp/model.py:360-363, 376-383)
 *   mean = (source_means w - m_all) / s_all,   cov = source_covs w^2 / s_all^2 + os k_t(X, X; l)
 * with the source terms cached at construction (scamlgp/model.py:279-289) and the priors / constraints of
 * scamlgp/model.py:25-33, 73-105, 318-338.
 *   z (B, P), P = D + 2 + T: B independent parameter vectors [raw lengthscales (D), raw outputscale, raw noise, weights (T)] --
 *       the warm start and the prior-sampled restarts of utils.py:184-199 side by side; raw = unconstrained values of the
 *       sigmoid Interval constraints, weights as they are (GreaterThan(1e-10, transform=None): a box bound for the optimiser).
 *   means_t (T, n): source posterior means at the target inputs (source_means transposed), original units.
 *   covs_packed (T, n (n + 1) / 2): source posterior covariances, lower triangle packed row-wise -- element (a, b), a >= b, at
 *       a (a + 1) / 2 + b (source_covs[a, b, t]).
 *   X (n, D), y (n): target inputs and observations standardised with (m_all, s_all) (scamlgp/model.py:264-276, 309-316).
 *   spec_host: HOST pointer to 19 doubles (read during the call; the one exception to "every pointer is a device pointer"):
 *       [ls_lo, ls_hi, os_lo, os_hi, noise_lo, noise_hi,  then (kind, p1, p2) for the lengthscale, outputscale, noise and
 *       weight priors -- kind 0 none, 1 Gamma(concentration p1, rate p2), 2 LogNormal(loc p1, scale p2) --,  w_lower].
 * scaml_target_mll_f64: value (B) = mll(z_b), grad (B, P) = d mll / d z_b, info (B) (k > 0: pivot k not positive even with
 *   jitter 1e-6 -- psd_safe_cholesky's ladder runs in-kernel --, value = NaN then), jitter_used (B, may be NULL).
 * scaml_target_fit_f64: maximises mll from every row of z (in: start points, out: optima) with an L-BFGS (history pairs,
 *   projected backtracking line search on w >= w_lower, scipy L-BFGS-B's stopping rules: projected gradient <= gtol, relative
 *   decrease <= ftol, max_iter iterations), entirely on the device; value (B) = mll at the returned point, stats (B, 4)
 *   (may be NULL) = [iterations, evaluations, status, 0], status 1 / 2 converged (gradient / decrease), 0 max_iter,
 *   3 line search failed, 4 objective not finite at the start point.  workspace: scaml_target_fit_workspace_doubles(...) doubles.
 * Non-finite inputs: a NaN weight or raw lengthscale in a row of z, or a NaN or infinite coordinate of X, makes every element of the
 *   matrix that it enters NaN in BOTH kernel families (the Matern clamp and exp(-inf) = 0 do not hide it), so the factorisation
 *   fails on every rung of the ladder: that row answers info > 0, value NaN and a zero gradient (n >= 2 for a lengthscale or a
 *   coordinate: a single point has no distance).  The other rows of the launch -- in (8b) the other problems -- are not affected.
 * One workgroup per row of z, the n x n matrix in LDS: n <= scaml_target_fit_max_n(T, D) (128 at T = 32, D = 6),
 * D <= scaml_target_fit_max_d(); SCAML_E_TOOLARGE otherwise.
 */
int scaml_target_fit_max_n(int T, int D);
int scaml_target_fit_max_d(void);
long long scaml_target_fit_workspace_doubles(int B, int T, int D, int history);
int scaml_target_mll_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, double m_all, double s_all,
                         const double* spec_host, const double* z, int B, int n, int T, int D, int kind, double* value, double* grad,
                         int32_t* info, double* jitter_used, void* stream);
int scaml_target_fit_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, double m_all, double s_all,
                         const double* spec_host, double* z, int B, int n, int T, int D, int kind, int max_iter, int history, double gtol,
                         double ftol, double* value, int32_t* info, double* jitter_used, int32_t* stats, double* workspace,
                         long long workspace_doubles, void* stream);

/*
 * (8b) The objective and the refit of (8) over a BATCH of training sets: S problems x B start points in ONE launch of S * B
 * workgroups (workgroup r works on row r of z: start r % B of problem r / B).  The use: S Bayesian-optimisation studies against
 * one fitted source stack (the repeated runs behind a regret curve, scamlgp/benchmarking/local_runner.py:174-181, which the reference
 * fans out over a process pool) refitted in lock-step -- one study's refit occupies B of the chip's 256 CUs for its whole latency.
 *   z (S, B, P), P = D + 2 + T, as in (8); value (S, B), grad (S, B, P), info (S, B), jitter_used (S, B), stats (S, B, 4).
 *   means_t (S, T, n_max), covs_packed (S, T, n_max (n_max + 1) / 2), X (S, n_max, D), y (S, n_max): problem s in the leading
 *       n_s columns / n_s (n_s + 1) / 2 packed entries / n_s rows of its slice (the packed index a (a + 1) / 2 + b does not depend
 *       on n); what lies beyond is never read.
 *   n_points (S) int32, 1 <= n_s <= n_max: the problems may differ in size (a study with a pending or failed evaluation is a
 *       point behind).  A count outside the range gives value NaN, info -1 (stats status 4) for that problem's rows; nothing is read.
 *   m_all (S), s_all (S) > 0: the standardisers, DEVICE arrays here (by value in (8)).
 *   spec_host: HOST pointer to 19 doubles as in (8), shared by all problems; T, D, kind, the optimiser's options likewise.
 * Every row runs the instruction sequence the single-problem kernel runs on that problem (the matrix-core factorisation where ITS
 * n_s <= 112, the column-by-column elimination beyond), so the results equal those of (8) called per problem bit for bit.
 * workspace: scaml_target_fit_batched_workspace_doubles(S, B, T, D, history) doubles.
 * Limits as in (8): n_max <= scaml_target_fit_max_n(T, D), D <= scaml_target_fit_max_d(); SCAML_E_TOOLARGE otherwise.
 * S == 0 or B == 0: nothing is enqueued.
 */
long long scaml_target_fit_batched_workspace_doubles(int S, int B, int T, int D, int history);
int scaml_target_mll_batched_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, const int32_t* n_points,
                                 const double* m_all, const double* s_all, const double* spec_host, const double* z, int S, int B, int n_max,
                                 int T, int D, int kind, double* value, double* grad, int32_t* info, double* jitter_used, void* stream);
int scaml_target_fit_batched_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, const int32_t* n_points,
                                 const double* m_all, const double* s_all, const double* spec_host, double* z, int S, int B, int n_max, int T,
                                 int D, int kind, int max_iter, int history, double gtol, double ftol, double* value, int32_t* info,
                                 double* jitter_used, int32_t* stats, double* workspace, long long workspace_doubles, void* stream);

/*
 * (9) Training the source GPs on the device: the hyper-parameter fit of a whole stack, B = tasks x starts problems side by side
 * (scamlgp/model.py:176-188 -> scamlgp/utils.py:139-212: L-BFGS on -(mll + sum log p(theta) / n) over the raw parameters of the
 * sigmoid Interval constraints, from the warm start and from every prior-sampled restart).
 * One call enqueues n_evals rounds of { fit at the trial point ((3) / (3b)), MLL gradient (4), optimiser step } on `stream` and
 * returns; nothing is synchronised.  The step kernel (csrc/gp_stack_fit.hip, one wave per problem) runs the per-problem state
 * machine of a backtracking L-BFGS: Armijo test with halving (c1 = 1e-4, 20 trials), curvature pairs (`history` <= 16 of them),
 * stopping rules max|g| <= gtol, relative decrease <= ftol, max_iter iterations.  Problems do not wait for each other; a finished
 * problem is still evaluated (at its accepted point) until the caller stops calling.
 *   X (B, N, D), y (B, N), n_points (B) or NULL: the data, replicated per start by the caller (problem b = start * T + task).
 *   spec_host: HOST pointer to 15 doubles, the first 15 of (8)'s block: Interval bounds and (kind, p1, p2) of the lengthscale,
 *       outputscale and noise priors.
 *   z (B, D + 2): raw start points in; after every call the accepted point of each problem.
 *   value (B): mll + sum log p(theta) / n at z.   stats (B, 4) int32: [iterations, evaluations, status, 0], status 0 still running,
 *       1 / 2 converged (gradient / decrease), 3 line search failed, 4 objective not finite at the start point, 5 max_iter.
 *   flags: SCAML_STACK_FIT_CONTINUE resumes from the state the previous call left in `workspace` (same arguments otherwise);
 *       without it the first round evaluates z and initialises the state.  The caller reads stats and calls again while any
 *       problem is still running.  Chunking does not change the result.
 *   workspace: scaml_stack_fit_workspace_bytes(B, N, D, history) bytes, 16-byte aligned; it starts with the per-problem state of
 *       the L-BFGS state machine that (9) and (7h) share (csrc/gp_lbfgs_core.h), P = D + 2 variables here:
 *       (4 + 2 history) P + history + 16 doubles each -- accepted point x[P], gradient g[P] of the minimised function there (here
 *       d objective / d raw, objective = -value), direction d[P], trial point xt[P], the pairs S[history][P], Y[history][P] (a ring),
 *       rho[history], and 16 scalars: f, step, g . d ((7h): g . (xt - x)), iteration, evaluations, status, failed trials of this
 *       line search, pairs held, ring head, phase.
 * Shapes: what (3) / (3b) and (4) take (N <= 512, a multiple of 16 beyond 256; their D limits) and D <= scaml_stack_fit_max_d();
 * SCAML_E_TOOLARGE otherwise.  B == 0 or n_evals == 0: nothing is enqueued.
 */
#define SCAML_STACK_FIT_CONTINUE 1u
int scaml_stack_fit_max_d(void);
long long scaml_stack_fit_workspace_bytes(int B, int N, int D, int history);
int scaml_stack_fit_f64(const double* X, const double* y, const int32_t* n_points, const double* spec_host, double* z, int B, int N,
                        int D, int kind, int n_evals, unsigned flags, int max_iter, int history, double gtol, double ftol,
                        double* value, int32_t* stats, void* workspace, long long workspace_bytes, void* stream);

/*
 * (7h) The acquisition OPTIMISER of many studies' start points on the device: a box-constrained L-BFGS per start around the two
 * evaluation launches of (5e) / (7g) (scamlgp_amd.bo.ScaMLGPBOStudies with suggest_mode="device"; botorch's optimize_acqf runs scipy
 * L-BFGS-B on the host around every evaluation).  One call enqueues n_evals rounds of { grouped GRAD source pass (5e), batched target
 * acquisition (7g), optimiser step } on `stream` and returns; no graph, nothing is synchronised.  The step kernel
 * (csrc/gp_acqf_opt.hip, one wave per start, one lane per coordinate) runs the per-start state machine of a projected L-BFGS that
 * MAXIMISES the acquisition value: the start projected onto the box, coordinates at a bound with the gradient pointing outward held,
 * two-loop direction (`history` <= 16 pairs, kept when s . y > 0), projected trial points, Armijo test on g . (trial - x) with halving
 * (c1, max_ls trials), scipy L-BFGS-B's stopping rules max |P(x - g) - x| <= gtol, relative decrease <= ftol, max_iter iterations.
 * Starts do not wait for each other, and a start that has stopped is no longer evaluated: each launch writes the next trial points
 * and a LIVE group table (the start's study while it runs, -1 afterwards) that the evaluation kernels are handed in place of `group`.
 *   x0 (B, D): the start points; group (B) int32: the study of start b, negative = a padding row (status 6, never evaluated).
 *   VA_tab, X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s: the source stack as (5e) takes it (theta / alpha / n_points of the
 *       SOURCE GPs; y_mean, y_std, n_points_s may be NULL);  w, active, Xt, theta_t, L, Linv_diag, alpha_t, n_points_t, m_all, s_all,
 *       info, acqf_param: the studies as (7g) takes them -- Xt / n_points_t are also (5e)'s leading points Xa / n_points_a, n_max its
 *       Ma_max.  info[g] != 0: the study's starts fail at their first evaluation (status 4).
 *   kind_s: the kernel family of the source stack, kind_t: of the studies' target kernels; acqf 0: UCB, 1: EI, as (7g).
 *   lo, hi (D): the box (device arrays), lo <= hi.
 *   flags: SCAML_ACQF_OPT_CONTINUE resumes from the state the previous call left in `workspace` (same arguments otherwise); without it
 *       a reset launch first makes the projected x0 the first trial.  The caller reads stats and calls again while any start is still
 *       running (at most 1 + max_iter max_ls evaluations per start).  Chunking does not change what a start does with the
 *       evaluations it is given.
 *   x (B, D), f (B): the accepted point of each start and the acquisition value THERE (the evaluation made when it was accepted: no
 *       re-scoring pass is needed); -inf for a failed start, 0 for a padding row.
 *   stats (B, 4) int32: [iterations, evaluations, status, pairs held], status 0 still running, 1 converged on the projected gradient,
 *       2 stopped on ftol, 3 line search failed, 4 acquisition not finite at the start point, 5 max_iter, 6 padding row.
 *   workspace: scaml_studies_acqf_opt_workspace_bytes(B, G, n_max, T, D, history) bytes (0 for shapes the call does not take),
 *       16-byte aligned; it starts with the per-start state in the layout given under (9), P = D variables and the minimised function
 *       -acquisition; then Xq, the live group table, mu / var / cov of (5e) and value / grad of (7g).
 * Limits: those of (5e) / (7g) -- n_max <= 96 and <= N, N <= scaml_posterior_max_n(), D <= scaml_studies_acqf_opt_max_d() = 15;
 * SCAML_E_TOOLARGE beyond them (bad arguments answer first).  B == 0 or G == 0: nothing is enqueued.  Everything is checked once,
 * before the first launch; SCAML_E_LAUNCH from a later round leaves the rounds before it enqueued -- start the optimisation again.
 */
#define SCAML_ACQF_OPT_CONTINUE 1u
int scaml_studies_acqf_opt_max_d(void);
long long scaml_studies_acqf_opt_workspace_bytes(int B, int G, int n_max, int T, int D, int history);
int scaml_studies_acqf_opt_f64(const double* x0, const int32_t* group, const double* const* VA_tab, const double* X, const double* theta_s,
                               const double* Linv, const double* alpha_s, const double* y_mean, const double* y_std,
                               const int32_t* n_points_s, const double* w, const uint8_t* active, const double* Xt, const double* theta_t,
                               const double* L, const double* Linv_diag, const double* alpha_t, const int32_t* n_points_t,
                               const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int B, int G,
                               int n_max, int T, int N, int D, int kind_s, int kind_t, int acqf, const double* lo, const double* hi, int max_iter,
                               int history, int max_ls, double gtol, double ftol, double c1, int n_evals, unsigned flags, void* workspace,
                               double* x, double* f, int32_t* stats, void* stream);

/*
 * (7h') (7h) for studies that each own their source tasks: the same workspace (scaml_studies_acqf_opt_workspace_bytes with T = the
 * tasks per study), the same state machine and step kernel; only the evaluation launch of every round is (5e') instead of (5e).
 *   task_base (G) int32, Tsrc: as (5e') takes them -- X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s hold Tsrc tasks, study g
 *       reads tasks task_base[g] .. task_base[g] + T - 1; w, active (G, T) and VA_tab[g] (T, N, n_g) are per slot.
 * Checks and limits: those of (7h), and task_base != NULL, Tsrc >= 1 (SCAML_E_BADARG), all before the first launch.
 */
int scaml_studies_acqf_opt_own_f64(const double* x0, const int32_t* group, const double* const* VA_tab, const double* X, const double* theta_s,
                                   const double* Linv, const double* alpha_s, const double* y_mean, const double* y_std,
                                   const int32_t* n_points_s, const double* w, const uint8_t* active, const double* Xt, const double* theta_t,
                                   const double* L, const double* Linv_diag, const double* alpha_t, const int32_t* n_points_t,
                                   const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int B, int G,
                                   int n_max, int T, int N, int D, int kind_s, int kind_t, int acqf, const double* lo, const double* hi,
                                   int max_iter, int history, int max_ls, double gtol, double ftol, double c1, int n_evals, unsigned flags,
                                   void* workspace, double* x, double* f, int32_t* stats, const int32_t* task_base, int Tsrc, void* stream);

/*
 * (7i) The acquisition VALUE of a table of candidates of many studies, behind (5f): one workgroup per strip of 16 candidates of one
 * study; the study's L, Linv_diag and alpha are staged in LDS once per workgroup and serve all 16 columns (csrc/gp_studies_acqf.h).
 *   mu, var (T, Mq), cov (T, n_max, Mq): (5f)'s outputs; group (Mq / 16) int32 per strip; Xq (Mq, D); Mq a multiple of 16.
 *   w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info, acqf_param: the studies as (7g) takes them.
 *   value (Mq); mu_out, var_out (Mq) or NULL.  No gradient.
 * (7g) and (7i) are two instantiations of ONE kernel body (sa_block<R> of csrc/gp_studies_acqf.h: R = 1 right-hand side with 15 gradient
 * columns, or R = 16): per candidate the operations are (7g)'s on column 0 of its 16-column layout, in (7g)'s order, each output by one thread
 * and without atomics: value, mu_out and var_out are a pure function of the inputs and BIT-IDENTICAL to (7g)'s for the same per-task numbers.
 * info[g] != 0 (or n_points[g] outside 1 .. n_max) gives NaN for the study's candidates, a padding strip zeros; an inactive task is
 * skipped, not multiplied by zero; what lies past n_g in a study's slices is never read; a candidate with a NaN or infinite coordinate
 * gives NaN in its own outputs only.
 * Checks: sizes (Mq < 0 or not a multiple of 16, G < 0, n_max < 1, T < 1, D < 1), NULL required pointers, kind, acqf: SCAML_E_BADARG.
 * Limits: n_max <= 96, D <= 15 and the LDS footprint of a strip (a constexpr of csrc/gp_studies_acqf.h): SCAML_E_TOOLARGE beyond them
 * (bad arguments answer first).  Mq == 0 or G == 0: nothing is enqueued.  Does not synchronise.
 */
int scaml_target_score_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                   const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                   const double* Linv_diag, const double* alpha, const int32_t* n_points, const double* m_all,
                                   const double* s_all, const int32_t* info, const double* acqf_param, int Mq, int G, int n_max, int T,
                                   int D, int kind, int acqf, double* value, double* mu_out, double* var_out, void* stream);

/*
 * (7j) The training blocks of G studies in one launch, a workgroup per study: what (6') and (7)'s assemble produce for ONE study's
 * training block, from the padded per-study source terms in the layout (8b) takes:
 *   means_t (G, T, n_max), covs_packed (G, T, n_max (n_max + 1) / 2), X (G, n_max, D), y (G, n_max), n_points (G) int32,
 *   m_all, s_all (G); and each study's pruned w (G, T), active (G, T) uint8 and theta (G, D + 2).
 *   Knn (G, n_max, n_max): the leading n_g x n_g block, Knn[i][c] = sum_t w_t^2 cov_t[i][c] / s^2 + os k_t(x_i, x_c) (+ noise on the
 *   diagonal); resid (G, n_max): y_i - (sum_t w_t mean_t[i] - m) / s.  The task sums run in (6)'s order.  The rest is untouched.
 * One call of (2) with n_points then factors all blocks (ragged sizes, the jitter ladder and info per study).
 * Checks: G < 0, n_max < 1, T < 1, D < 1, a NULL pointer, kind: SCAML_E_BADARG.  n_max > scaml_fit_max_n(): SCAML_E_TOOLARGE.
 * G == 0: nothing is enqueued.
 */
int scaml_target_train_block_batched_f64(const double* means_t, const double* covs_packed, const double* X, const double* y,
                                         const int32_t* n_points, const double* m_all, const double* s_all, const double* w,
                                         const uint8_t* active, const double* theta, int G, int n_max, int T, int D, int kind, double* Knn,
                                         double* resid, void* stream);

/*
 * (7k) (7g) and (7i) for studies of which some hold PENDING evaluations (scamlgp_amd.bo.ScaMLGPBOStudies with pending_mode="batched"):
 * such a study is a fantasy model as in (7f) -- its training block holds the pending inputs too (n_g counts them), and UCB / EI are
 * averaged over its F_g sampled outcomes, which differ in alpha only.  The arguments are (7g)'s / (7i)'s with `alpha` replaced by
 *   alpha_f (G, n_max, F_max): row a of study g holds its F_g values Knn^-1 [resid_0 .. resid_{F_g - 1}][a] contiguously (the (n, F)
 *       layout of (7f), row stride F_max);  n_fant (G) int32, 1 <= F_g <= F_max;  F_max >= 1.
 * Per right-hand side, with Knq, dKnq, z = Knn^-1 Knq, mean_q, var_q, S_mu, S_var as (7g) forms them:
 *   r_f = sum_a Knq[a] alpha_f[a][f],  mu_f = m + s (mean_q + r_f),  vr = s^2 (var_q - Knq . z)  (shared by the fantasies),
 *   value = (sum_f A(mu_f, vr)) / F_g, and with the chain-rule factors Amu_f, Av_f of A:  abar[a] = sum_f Amu_f alpha_f[a][f],
 *   grad[d] = ((sum_f Amu_f) S_mu[1 + d] + s sum_a abar[a] dKnq[a][d] + (sum_f Av_f) (S_var[1 + d] - 2 s^2 sum_a z[a] dKnq[a][d])) / F_g.
 * Every sum is formed by one thread in a fixed order (tasks, training points, fantasies ascending), without atomics: the outputs are
 * a pure function of the inputs.  A study with F_g == 1 is an ordinary one -- alpha_f[g, :, 0] is its alpha -- and its value and grad are
 * BIT-IDENTICAL to (7g)'s / (7i)'s: the workgroup takes their statements, so a mixed launch does not perturb the studies that have
 * nothing pending.  The strip layout gives the value of the query layout bit for bit, as (7i) does of (7g).
 *   value (Mq); grad (Mq, D) or NULL in the query layout.  No mu_out / var_out: a fantasy model has F_g posterior means.
 * The refusals are (7g)'s: a padding query (strip) gives zeros; info[g] != 0, n_points[g] outside 1 .. n_max or n_fant[g] outside
 * 1 .. F_max gives NaN for that study; a query with a NaN or infinite coordinate gives NaN in all of its own outputs; nothing past n_g
 * or F_g in a study's slices is read.
 * Checks: (7g)'s / (7i)'s, and F_max < 1 or a NULL alpha_f / n_fant: SCAML_E_BADARG.  Limits: n_max <= 96, D <= 15, F_max <= 64 (all at
 * once, in both layouts) and the LDS footprint (sa_fantasy_lds_doubles of csrc/gp_studies_acqf.h; alpha_f is read from global memory):
 * SCAML_E_TOOLARGE beyond them (bad arguments answer first).  Mq == 0 or G == 0: nothing is enqueued.  Neither call synchronises;
 * every status stays on the device (both can be stream-captured).
 */
int scaml_target_fantasy_acqf_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                          const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                          const double* Linv_diag, const double* alpha_f, const int32_t* n_fant, const int32_t* n_points,
                                          const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int Mq,
                                          int G, int n_max, int F_max, int T, int D, int kind, int acqf, double* value, double* grad,
                                          void* stream);
int scaml_target_fantasy_score_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                           const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                           const double* Linv_diag, const double* alpha_f, const int32_t* n_fant, const int32_t* n_points,
                                           const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int Mq,
                                           int G, int n_max, int F_max, int T, int D, int kind, int acqf, double* value, void* stream);

/*
 * (7l) (7h) on (7k)'s block: the acquisition optimiser of many studies' start points where studies may hold pending evaluations.  The
 * same rounds of { grouped GRAD source pass, acquisition launch ((7k) in the query layout), optimiser step }, the same step kernel,
 * workspace (scaml_studies_acqf_opt_workspace_bytes) and state layout, the same flags, outputs and stats as (7h).
 * The source pass of a round is (5e) / (5e') in an instantiation of its own that adds the waves' shares of a mean and of a variance in
 * wave order instead of with LDS float atomics: with (7k) and the step kernel every round is then a pure function of the state, and
 * x, f and stats do not depend on how the rounds are divided among calls, BIT FOR BIT ((7h) is chunking-independent only within the
 * run-to-run scatter of its pass).
 *   alpha_f, n_fant, F_max: as (7k) takes them, in place of (7h)'s alpha_t; n_points_t counts the pending inputs of a study, which
 *       are the last rows of its slice of Xt and columns of VA_tab[g].
 *   task_base (G) int32 / Tsrc: as (7h') takes them; task_base == NULL: every study reads the same source stack (Tsrc is ignored), as
 *       (7h) -- one entry serves both.
 * Checks and limits: those of (7h) / (7h') and (7k), bad arguments first, everything before the first launch.  B == 0 or G == 0:
 * nothing is enqueued.  Does not synchronise.
 */
int scaml_studies_fantasy_acqf_opt_f64(const double* x0, const int32_t* group, const double* const* VA_tab, const double* X, const double* theta_s,
                                       const double* Linv, const double* alpha_s, const double* y_mean, const double* y_std,
                                       const int32_t* n_points_s, const double* w, const uint8_t* active, const double* Xt,
                                       const double* theta_t, const double* L, const double* Linv_diag, const double* alpha_f,
                                       const int32_t* n_fant, const int32_t* n_points_t, const double* m_all, const double* s_all,
                                       const int32_t* info, const double* acqf_param, int B, int G, int n_max, int F_max, int T, int N, int D,
                                       int kind_s, int kind_t, int acqf, const double* lo, const double* hi, int max_iter, int history, int max_ls,
                                       double gtol, double ftol, double c1, int n_evals, unsigned flags, void* workspace, double* x, double* f,
                                       int32_t* stats, const int32_t* task_base, int Tsrc, void* stream);

/*
 * (7m), (7n) The fantasy SET-UP of G studies with pending evaluations in a constant number of launches
 * (scamlgp_amd.model.fantasize_studies; bo.ScaMLGPBOStudies with fantasy_setup="batched"), in place of, per study, ScaMLGP.fantasize,
 * condition_on_observations and the conditioned model's first pass.  With X' = cat(train_X, X_pend), n' = n + p points, K' the training
 * block of the conditioned model (standardised units, noise on the diagonal), mean' the standardised weighted source mean at X' and
 * L' = chol(K') = [[L_nn, 0], [L_pn, L_pp]]:  v = L_nn^-1 (y~_n - mean'_n);  the posterior mean at the pending points is
 * mean'_p + L_pn v and L_pp L_pp^T their posterior covariance with observation noise, so the fantasy targets are
 * y~_p^f = mean'_p + L_pn v + L_pp eps_f;  the residual of fantasy f is L' [v ; eps_f], hence alpha_f[:, f] = L'^-T [v ; eps_f].
 * The calls: (5f) / (5f') ONCE with every study's own X' as its query strips, (7m), (2) with n_points and Linv_diag, (7n).
 *
 * (7m) scaml_studies_condition_block_f64: the training blocks of the conditioned models -- (7j) on (5f)'s layout.
 *   mu (T, Mq), cov (T, n_max, Mq): (5f)'s outputs (its var is not needed: the diagonal of K' comes from cov, as its other elements do).
 *       Strip j of study g holds points 16 j .. 16 j + 15 of X'_g, padded with any point of the box; Mq a multiple of 16.
 *   strip_base (G) int32: the first strip of study g;  w, active (G, T), Xt (G, n_max, D) = X'_g, theta (G, D + 2): as (7g) takes them;
 *   y (G, n_max): standardised targets of the observed rows (rows >= n_obs are not read);  n_points (G) int32 = n'_g;  n_obs (G) int32
 *       = n_g, 1 <= n_g <= n'_g <= n_max (n_g == n'_g: nothing pending);  m_all, s_all (G).
 *   Knn (G, n_max, n_max): the leading n'_g block.  Element (i, c) with c <= i is
 *       sum_t w_t^2 cov[t][i][16 strip_base[g] + c] / s^2 + os k(x_i, x_c) (+ noise if i == c) -- the ROW of the later point, the COLUMN
 *       of the earlier one -- and (c, i) is its copy; (2) reads the lower triangle only.
 *   resid (G, n_max): y_i - mean'_i for i < n_obs, ZERO for the pending rows;  mean_p (G, n_max): mean'_i at rows n_obs .. n' - 1.
 *   The task sums run in (6)'s order, masked tasks skipped.  Nothing past n'_g in a study's slices is read or written.  A point of
 *   X'_g with a NaN or infinite coordinate, n_obs[g] outside 1 .. n'_g or strips outside the Mq columns make THAT study's outputs NaN;
 *   n_points[g] outside 1 .. n_max: nothing is written for the study ((7n) answers NaN for it).
 *   Checks: Mq < 0 or not a multiple of 16, G < 0, n_max < 1, T < 1, D < 1, a NULL pointer, kind: SCAML_E_BADARG.  Limits: n_max <= 96,
 *   D <= 15, Mq <= 2^26 (as (7g)) and the LDS footprint (sc_block_lds_doubles of csrc/gp_studies_condition.h): SCAML_E_TOOLARGE (bad arguments answer first).
 *
 * (7n) scaml_studies_fantasy_condition_f64: the fantasies and alpha_f from the factor.
 *   L (G, n_max, n_max), info (G) int32: (2)'s outputs for Knn;  resid, mean_p, n_points, n_obs, m_all, s_all: as (7m);
 *   eps (G, p_max, F_max): standard-normal draws, row i of study g holds the F_g values of pending point i contiguously;
 *   n_fant (G) int32, 1 <= F_g <= F_max;  p_max >= 1, every n'_g - n_g <= p_max.
 *   alpha_f (G, n_max, F_max): exactly (7k)'s layout;  y_fant (G, p_max, F_max): the fantasy targets in original units, m + s y~;
 *   mu_p (G, p_max): the posterior mean at the pending points in original units.
 *   Per study: v by forward substitution against the leading n_g block, the samples by the formula above, L'^T x = [v ; eps_f] by
 *   backward substitution, one thread per fantasy column.  A study with n_g == n'_g is an ordinary one: F_g must be 1, column 0 of
 *   alpha_f is L'^-T v = K^-1 resid and nothing is written to y_fant / mu_p.
 *   info[g] != 0, n_points[g] outside 1 .. n_max, n_obs[g] outside 1 .. n'_g, n_fant[g] outside 1 .. F_max, more than p_max pending points
 *   or an ordinary study with F_g != 1: that study's outputs are NaN (and (7k) answers NaN for it).  Nothing past n'_g, p_g or F_g is
 *   read or written.
 *   Checks: G < 0, n_max < 1, p_max < 1, F_max < 1, a NULL pointer: SCAML_E_BADARG.  Limits: n_max <= 96, p_max <= 96, F_max <= 64 and the
 *   LDS footprint (sc_fantasy_lds_doubles): SCAML_E_TOOLARGE (bad arguments answer first).
 * Both: fp64, a workgroup of 256 threads per study, every sum formed by one thread in a fixed ascending order, no atomics -- the outputs
 * are a pure function of the inputs.  Everything is checked before the first HIP call; G == 0: nothing is enqueued.  Neither call
 * synchronises and both can be stream-captured.
 */
int scaml_studies_condition_block_f64(const double* mu, const double* cov, const int32_t* strip_base, const double* w, const uint8_t* active,
                                      const double* Xt, const double* theta, const double* y, const int32_t* n_points, const int32_t* n_obs,
                                      const double* m_all, const double* s_all, int Mq, int G, int n_max, int T, int D, int kind, double* Knn,
                                      double* resid, double* mean_p, void* stream);
int scaml_studies_fantasy_condition_f64(const double* L, const double* resid, const double* mean_p, const int32_t* n_points, const int32_t* n_obs,
                                        const int32_t* info, const double* eps, const int32_t* n_fant, const double* m_all, const double* s_all,
                                        int G, int n_max, int p_max, int F_max, double* alpha_f, double* y_fant, double* mu_p, void* stream);

/*
 * (7s), (7t) The OPTIMISER of the joint q-point acquisition (5g) / (7p) / (7q) on the device: a box-constrained L-BFGS per start
 * batch (scamlgp_amd.bo with joint_opt_mode="device"; the default runs scipy L-BFGS-B on the host around every evaluation).  A start
 * is one batch of q points, P = q D <= scaml_qacqf_opt_max_p() = 128 variables.  The state machine is (7h)'s (csrc/gp_lbfgs_core.h,
 * the box instance) with two variables per lane (csrc/gp_qacqf_opt.hip: one wave per SLOT, no LDS); every dot product adds variable 0
 * first, ascending, and no product is contracted, so that, given the same evaluations, the iterates are hyper.batched_lbfgs(bounds=)'s
 * bit for bit.  It MAXIMISES.
 *
 * The slot table.  slots (Bs) int32, distinct entries within [0, B) (NULL: the identity, Bs == B): slot s works on start slots[s].  It
 * reads value[s] / grad[s, :P], advances state[slots[s]], writes the next trial batch to Xq[s, :P] -- Xq (Bs, q D) IS the (Bs q, D)
 * array the evaluation kernels read -- and the accepted point, its value and the counters to x / f / stats[slots[s]].  Starts that are
 * not in the table are not touched.  A start that stops inside a call keeps its slot until the call ends (its row of Xq is its accepted
 * point, what comes back for it is ignored); the caller reads stats between calls anyway and hands the next call the table of the
 * starts still running, so that the cost of a round follows them without a live table inside (5g) / (7p).  An entry outside [0, B) is
 * skipped.
 *
 * (7t) scaml_qacqf_opt_step_f64: the step alone, on the caller's evaluation -- a device-side box L-BFGS for ANY function of P <= 128
 * variables per start.  mode 0: the start x0[slots[s]] projected onto the box is the accepted point and the first trial, the state is
 * reset.  mode 1: one evaluation (value (Bs), grad (Bs, P), of the maximised function at Xq) is consumed.  mode 2: neither; the outputs
 * are written again from the state as it is -- the first launch after the table has changed, which puts the trial points in its order.
 *   x0 (B, P); lo, hi (P): the box, lo <= hi; state (B, scaml_qacqf_opt_step_workspace_bytes(B, P, history) / (8 B)) doubles per start in
 *   the layout given under (9); x (B, P), f (B) (-inf for a failed start), stats (B, 4) int32 as (7h).  max_iter, history <= 16, max_ls,
 *   gtol, ftol, c1: as (7h).
 *   Checks: B, Bs < 0, Bs > B, slots NULL with Bs != B, P < 1, mode, max_iter < 0, max_ls < 1, history outside 1 .. 16, a NULL pointer
 *   (x0 in mode 0; value, grad in mode 1), gtol < 0 or NaN, c1 <= 0, ftol NaN: SCAML_E_BADARG.  P > 128, B > 2^26: SCAML_E_TOOLARGE (bad
 *   arguments answer first).  Bs == 0: nothing is enqueued.  One launch, does not synchronise.
 *
 * (7s) scaml_qacqf_opt_f64: n_evals rounds enqueued on `stream` with (7h)'s contract -- no graph, nothing is synchronised, every
 * argument and size checked once before the first launch (SCAML_E_BADARG answers before SCAML_E_TOOLARGE), SCAML_ACQF_OPT_CONTINUE
 * resumes, B == 0, Bs == 0 or n_evals == 0 enqueues nothing, SCAML_E_LAUNCH from a later round leaves the rounds before it enqueued.
 * A call opens with the step in mode 0 (mode 2 when it continues) and the training block of the joint prior; a round is then, at
 * Mq = Bs q points and with the arguments scamlgp_amd.model.ScaMLGP.joint_acqf_inputs hands them: the value pass
 * scaml_posterior_linv_f64 with V kept, (5g), scaml_weighted_prior_reduce_f64 and scaml_weighted_task_sum_f64, the gather (column 0 of
 * every point's 16 of mu_g, var_g and of rows a < n of cov_g go behind the training block of mean_s, var_s (n + Mq), cov_s (n, n + Mq),
 * the points into xall[n:]), scaml_target_assemble_f64, scaml_cho_solve_batched_f64 against the caller's target factor, (7p) -- (7q)
 * when p > 0 --, the step.
 *   x0 (B, q D); slots (Bs) or NULL;
 *   Xa (n + p, D), X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s, VA (T, N, n + p): the source stack and the leading points as
 *       (5g) takes them (the pending points behind the training inputs); w (T), active (T) or NULL: as (6);
 *   mu_t (n), cov_tt (n, n), var_t (n): the weighted source sums at the training inputs;
 *   Xt (n, D), theta_t (D + 2), targets (n) standardised, L (n, n), Linv_diag, alpha_t (n), info (1) or NULL: the target GP and the
 *       factor of its training block as (2) leaves it; m_all, s_all.  info[0] != 0: every start fails at its first evaluation (status 4);
 *   base_samples (S, q + p); Xp (p, D), Zp (n, p), mu_p (p), Sigma_pp (p, p): as (7q) takes them, read when p > 0;
 *   acqf, acqf_param: as (7p); lo, hi (q D): the box; the optimiser's options as (7h).
 *   workspace: scaml_qacqf_opt_workspace_bytes(B, n, p, q, T, N, D, history) bytes (0 for shapes the call does not take), 16-byte
 *       aligned; it starts with the per-start state, P = q D; the evaluation arrays behind it are packed at the call's Bs.
 * Limits: those of (5g) / (7p) / (7q) -- q + p <= 8, n + p + q <= 96 and <= N, S <= 512, D <= 15, N <= scaml_posterior_max_n() --,
 * history <= 16, B <= 2^20.  The evaluations of a round scatter by the source pass's float atomics: between runs and chunkings the
 * results agree to rounding, not bit for bit.
 */
int scaml_qacqf_opt_max_p(void);
long long scaml_qacqf_opt_step_workspace_bytes(int B, int P, int history);
long long scaml_qacqf_opt_workspace_bytes(int B, int n, int p, int q, int T, int N, int D, int history);
int scaml_qacqf_opt_step_f64(const double* value, const double* grad, const int32_t* slots, const double* x0, const double* lo, const double* hi,
                             int B, int Bs, int P, int mode, int max_iter, int history, int max_ls, double gtol, double ftol, double c1,
                             double* state, double* Xq, double* x, double* f, int32_t* stats, void* stream);
int scaml_qacqf_opt_f64(const double* x0, const int32_t* slots, const double* Xa, const double* X, const double* theta_s, const double* Linv,
                        const double* alpha_s, const double* y_mean, const double* y_std, const int32_t* n_points_s, const double* VA,
                        const double* w, const uint8_t* active, const double* mu_t, const double* cov_tt, const double* var_t, const double* Xt,
                        const double* theta_t, const double* targets, const double* L, const double* Linv_diag, const double* alpha_t,
                        double m_all, double s_all, const int32_t* info, const double* base_samples, const double* Xp, const double* Zp,
                        const double* mu_p, const double* Sigma_pp, int B, int Bs, int n, int p, int q, int S, int T, int N, int D, int kind_s,
                        int kind_t, int acqf, double acqf_param, const double* lo, const double* hi, int max_iter, int history, int max_ls,
                        double gtol, double ftol, double c1, int n_evals, unsigned flags, void* workspace, long long workspace_bytes, double* x,
                        double* f, int32_t* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCAML_GP_H */
