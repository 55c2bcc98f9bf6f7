// gp_dispatch.h — dispatch by shape: which kernel instance a call gets, with how many waves or workgroups and how much LDS.
// Pure host functions of plain values (shape, CU count, the developer switches as ints and bools, pointer alignment, workspace
// size): csrc/scaml_host.cpp asks them and launches what they say, tests/host_emul/dispatch_emul.cpp hands the same functions to
// tests/test_dispatch.py and to the test helpers that name the instance a case exercises.  No kernel includes this header.
#pragma once
#include <stddef.h>
#include <initializer_list>

#include "gp_fit_params.h"
#include "gp_posterior_params.h"
#include "gp_target_params.h"
#include "gp_studies_condition.h"
#include "gp_qacqf.h"

namespace scaml {

constexpr size_t LDS_LIMIT = 160 * 1024;   // bytes of LDS a workgroup may ask for on gfx950
static_assert(TARGET_FIT_LDS_LIMIT == LDS_LIMIT, "the matrix-core rule and the launcher count the same LDS");

// ---- fused fit / batched POTRF (N <= 256) ----------------------------------------------------------------------------------
// The instances <NB 16-blocks, WU update waves> of gp_fit_fused_kernel / gp_fit_blocked_kernel, in the order of Module::fit
struct FitInstance {
  int nb, wu;
};
constexpr int FIT_INSTANCES = 5;
constexpr FitInstance fit_instance(int variant) {
  constexpr FitInstance v[FIT_INSTANCES] = {{2, 1}, {4, 3}, {8, 3}, {16, 7}, {8, 7}};   // [4]: wide variant for 64 < N <= 128
  return v[variant];
}

constexpr int fit_class(int N) { return N <= 32 ? 0 : (N <= 64 ? 1 : (N <= 128 ? 2 : 3)); }

// largest D whose staged point stack fits the 160 KiB LDS next to the vectors
constexpr int fit_class_max_d(int N) {
  const int d = fit_max_d(32 << fit_class(N), (int)(LDS_LIMIT / sizeof(double)));
  return d > 1024 ? 1024 : d;
}

struct FitPlan {
  int variant, nb, wu;   // index into Module::fit and its template arguments
  unsigned block;
  size_t lds_doubles;    // more than LDS_LIMIT: the shape is too large
};
constexpr FitPlan fit_plan(int T, int N, int D, int cus) {
  int vi = fit_class(N);
  // 64 < N <= 128: four waves per task let two workgroups share a CU; when the stack does not fill the CUs even
  // once that buys nothing, and eight waves on the task's kernel matrix and trailing update are faster
  if (vi == 2 && T <= cus) vi = 4;
  const FitInstance v = fit_instance(vi);
  return {vi, v.nb, v.wu, (unsigned)(v.wu + 1) * 64, fit_lds_doubles(v.nb, v.wu, D)};
}

// The full-tile instance gp_fit_fused_kernel<16, 7, kind, true> (csrc/gp_fit_fused.hip, FULL): whether a launch of instance
// <nb, wu> may take it.  Its contract, every clause a compile-time fact inside the kernel: the N <= 256 class with N == 16 nb (no
// padded rows), no n_points (every point valid), kernel-matrix mode (no given matrix), dense addressing (not a diagonal block of
// a blocked fit: LD == N), and -- when the call stores L -- an L on a 16-byte boundary (N is even, so every row is then).
// mode: 0 by arguments, 1 never (the environment variable SCAML_FIT_NO_FULL, csrc/scaml_host.cpp).  l_addr: the L pointer as an
// integer, read on the host (no device work).
constexpr bool fit_full_instance(int nb, int wu, int N, bool ragged, bool from_matrix, bool blocked, bool stores_l, size_t l_addr, int mode) {
  return mode == 0 && nb == 16 && wu == 7 && N == 16 * nb && !ragged && !from_matrix && !blocked && (!stores_l || l_addr % 16 == 0);
}

// ---- blocked fit (256 < N <= 512, N a multiple of 16) --------------------------------------------------------------------------
struct BlockedPlan {
  int path;            // 1 the 2 x 2 sequence of launches, 2 the several-CUs-per-task kernel in one launch
  int t8;              // tasks ride on grid.x, dealt to the XCDs (bk_task_part)
  // one launch
  int parts;           // workgroups per task
  size_t lds_coop;     // bytes requested
  size_t flag_bytes;   // zeroed head of the workspace
  size_t need;         // workspace bytes the one launch uses
  // sequence
  int nt;              // 64-row tiles of the second block
  int solve_small_d;   // index of gp_blocked_solve_kernel's SMALLD
  int rounds;
  size_t lds_solve, lds_syrk;   // bytes
};
// mode: scaml_debug_blocked_fit_path (0 by shape, 1 the sequence only, 2 one launch whenever it is launchable)
constexpr BlockedPlan blocked_plan(int T, int N, int D, int cus, int mode, long long workspace_bytes, bool no_retry) {
  BlockedPlan b{};
  b.t8 = (T + 7) / 8 * 8;
  // Several CUs per task (csrc/gp_fit_coop.hip) while the stack leaves CUs idle: P workgroups per task, ALL resident at once
  // (one per CU: the dynamic LDS request is kept above half a CU's), so the launch is only taken when T P <= #CUs.
  const int nbc = (N + 31) / 32;
  int parts = T > 0 ? cus / T : 0;
  parts = parts > 8 ? 8 : parts;
  parts = parts > nbc ? nbc : parts;
  const size_t lds_coop = coop_fit_lds_doubles(N, D) * sizeof(double);
  b.parts = parts;
  b.flag_bytes = (((size_t)T * 44 * 4) + 15) & ~(size_t)15;
  b.need = b.flag_bytes + (size_t)T * N * 8 + (size_t)T * 64 * 8;
  const size_t half_cu = 82 * 1024;   // (more than half a CU's LDS: one workgroup per CU)
  b.lds_coop = lds_coop > half_cu ? lds_coop : half_cu;
  // by shape (dev_coop_time.py, profiles/r03_notes.md): three or more workgroups per task always pay; two only while a workgroup's eight
  // or fewer block columns leave it time to keep up with the diagonal chain (N <= 320)
  const bool take = mode == 2 ? parts >= 1 : (mode == 0 && (parts >= 3 || (parts == 2 && nbc <= 10)));
  b.path = take && D <= 16 && lds_coop <= LDS_LIMIT && b.need <= (size_t)workspace_bytes ? 2 : 1;
  b.nt = (N - 256 + 63) / 64;
  b.solve_small_d = D <= 8 ? 1 : 0;
  b.rounds = no_retry ? 1 : 4;
  b.lds_solve = blocked_solve_lds_doubles(D) * sizeof(double);
  b.lds_syrk = blocked_syrk_lds_doubles(D) * sizeof(double);
  return b;
}

// ---- explicit inverse factor, Cholesky solve -----------------------------------------------------------------------------
// waves per workgroup of gp_linv_kernel / gp_cho_solve_kernel: as many [np][16] strips as fit the LDS
constexpr int strip_solve_waves(int np) {
  for (int waves : {4, 2}) {
    if (strip_solve_lds_doubles(np, waves) * sizeof(double) <= LDS_LIMIT) return waves;
  }
  return 1;
}

// The workgroup slots gp_linv_kernel's split aims to fill.  A constant of the rule (the MI355X's 256 CUs when it was measured),
// NOT the CU count of the device the call runs on.
constexpr int LINV_TARGET_WORKGROUPS = 256;
// one workgroup per task takes all strips (balanced over its waves); small stacks are split over more
// workgroups so that the 256 CUs stay busy
constexpr int linv_groups(int T, int nb, int waves) {
  int groups = 1;
  while (groups * 2 * waves <= nb && (long long)T * groups * 2 <= LINV_TARGET_WORKGROUPS) groups *= 2;
  return groups;
}

// ---- batched source posteriors (gp_posterior_kernel) -----------------------------------------------------------------------
struct PosteriorPlan {
  int waves;   // 0: too large
  bool xl;     // X staged in LDS
};
// waves per workgroup / X staging: the largest configuration whose LDS fits 160 KiB
constexpr PosteriorPlan posterior_plan(int N, int D) {
  for (int cand : {4, 2, 1}) {
    if (posterior_lds_doubles(N, D, cand, true) * sizeof(double) <= LDS_LIMIT) return {cand, true};
    if (posterior_lds_doubles(N, D, cand, false) * sizeof(double) <= LDS_LIMIT) return {cand, false};
  }
  return {0, true};
}

// ---- gradient of the marginal log-likelihood ---------------------------------------------------------------------------------
struct GradPlan {
  bool single;   // one launch (csrc/gp_mll_grad_fused.hip); else L^-1 (linv_groups) and then the tile kernel
  // one launch: mllgrad_fused[sc][kind][dma] (split == 1) or mllgrad_split[sc - 2][kind][split == 2 ? 0 : 1]
  int sc, nbt, dma, split;
  unsigned grid_x, grid_y, block;
  size_t lds_doubles;
};
// mode: scaml_debug_force_two_launch_grad (0 by shape, 1 two launches, 2 single launch); no_split: SCAML_GRAD_NO_SPLIT;
// ragged: n_points given; aligned16: L and Linv_diag on 16-byte boundaries
constexpr GradPlan grad_plan(int T, int N, int D, int cus, int mode, bool no_split, bool ragged, bool aligned16) {
  GradPlan g{};
  // N <= 256, D <= 8: ONE launch, one workgroup per task, K^-1 by column strips held in registers; neither L^-1 nor
  // K^-1 touches memory (csrc/gp_mll_grad_fused.hip).  Larger problems take the two-launch path below.
  // (measured, tools/dev_grad_select.py: a stack of at most 64 tasks of more than 64 points leaves most CUs idle with one
  //  workgroup per task, and there the two launches below -- L^-1 strips and K^-1 tiles spread over the chip -- win: 96 vs 120 us at
  //  T = 32, N = 256; 44 vs 49 us at T = 64, N = 128)
  const bool small_stack = N > 64 && T <= 64;
  g.single = N <= 256 && D <= 8 && mode != 1 && !(small_stack && mode != 2 && !no_split);
  if (g.single) {
    g.sc = fit_class(N);
    g.nbt = 2 << g.sc;
    // direct-to-LDS staging moves raw 16-byte pieces: only where no element needs masking and every row is 16-byte aligned
    g.dma = (!ragged && N % 16 == 0 && aligned16) ? 1 : 0;
    // a stack that leaves CUs idle with one workgroup per task is split over 2 or 4 workgroups per task (strips are
    // independent): BASELINE configs[3] runs 128 tasks per GPU on 256 CUs
    // (split tasks pay for themselves in the N <= 256 class between 65 and 128 tasks only: 100 vs 105 us at T = 128; in the N <= 128
    //  class every split measured slower than one workgroup per task: 57 vs 49 us at T = 64)
    g.split = (g.sc == 3 && g.dma && !no_split && 2 * T <= cus) ? 2 : 1;
    g.grid_x = (unsigned)T;
    g.grid_y = (unsigned)g.split;
    g.block = (unsigned)(g.nbt * 32 / g.split);
    g.lds_doubles = mll_grad_fused_lds_doubles(g.nbt, g.nbt / 2);
    return g;
  }
  // 1-D grid, XCD-aware (task, tile group) map inside the kernel
  const int nb = (N + 15) / 16;
  const int nbs = (nb + 1) / 2, ns = nbs * (nbs + 1) / 2;   // 2 x 2 super-tiles, one per wave
  g.grid_x = (unsigned)(((T + 7) / 8) * 8) * (unsigned)((ns + 3) / 4);
  g.grid_y = 1;
  g.block = 256;
  g.lds_doubles = mll_grad_lds_doubles(D);   // staged points of four waves (D <= 76)
  return g;
}

// ---- target GP: objective + gradient and the L-BFGS refit ---------------------------------------------------------------------
constexpr int TARGET_FIT_THREADS = 512;
struct TargetFitPlan {
  bool use_mfma;   // matrix-core factorisation (batched: wherever a problem's own n admits it), else column by column
  size_t lds_doubles;
};
// mode: scaml_debug_target_fit_path (0 by shape, 1 column-by-column elimination only).
// the matrix-core factorisation takes n <= 112 (two block triangles of 16 x 17 tiles in LDS)
constexpr TargetFitPlan target_fit_plan(int n, int T, int D, int mode) {
  const bool mfma = mode == 0 && target_fit_mfma_shape(n, T, D, TARGET_FIT_THREADS / 64);
  return {mfma, target_fit_lds_doubles(n, T, D, mfma, TARGET_FIT_THREADS / 64)};
}
constexpr TargetFitPlan target_fit_batched_plan(int n_max, int T, int D, int mode) {
  return {mode == 0, target_fit_batched_lds_doubles(n_max, T, D, mode == 0, TARGET_FIT_THREADS / 64)};
}

// ---- studies' batched fantasy set-up (7m), (7n): a workgroup per study ---------------------------------------------------------
struct StudiesConditionPlan {
  unsigned grid, block;
  size_t lds_doubles;   // more than LDS_LIMIT: the shape is too large
};
constexpr StudiesConditionPlan studies_condition_block_plan(int G, int n_max, int D) {
  return {(unsigned)G, (unsigned)STUDIES_CONDITION_THREADS, sc_block_lds_doubles(n_max, D)};
}
constexpr StudiesConditionPlan studies_fantasy_condition_plan(int G, int n_max, int F_max) {
  return {(unsigned)G, (unsigned)STUDIES_CONDITION_THREADS, sc_fantasy_lds_doubles(n_max, F_max)};
}

// ---- joint q-point acquisition (7p): a workgroup per batch -----------------------------------------------------------------------
struct QAcqfPlan {
  unsigned grid, block;
  size_t lds_doubles;   // more than LDS_LIMIT: the shape is too large
};
constexpr QAcqfPlan qacqf_plan(int B, int n, int q, int S) { return {(unsigned)B, (unsigned)QACQF_THREADS, qa_lds_doubles(n, q, S)}; }
// ... with p evaluations pending (7q): still a workgroup per batch of q moving points
constexpr QAcqfPlan qacqf_pending_plan(int B, int n, int q, int p, int S) {
  return {(unsigned)B, (unsigned)QACQF_THREADS, qa_pending_lds_doubles(n, q, p, S)};
}
// ... value only (7r), p >= 0: still a workgroup per batch
constexpr QAcqfPlan qacqf_value_plan(int B, int n, int q, int p, int S) {
  return {(unsigned)B, (unsigned)QACQF_THREADS, qa_value_lds_doubles(n, q, p, S)};
}

// ---- the value-layout joint source pass (5h): a workgroup per (task, strip of 16 packed columns), XCD-aware map inside the kernel ----
struct PosteriorJointValuePlan {
  unsigned grid, block;
  size_t lds_doubles;
};
constexpr PosteriorJointValuePlan posterior_jointv_plan(int T, int N, int D, int Mp) {
  return {(unsigned)(((T + 7) / 8) * 8) * (unsigned)(Mp / 16), 512u, posterior_linv_jointv_lds_doubles(N, D)};
}

}  // namespace scaml
