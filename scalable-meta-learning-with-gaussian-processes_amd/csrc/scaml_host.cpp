// scaml_host.cpp — host side of libscaml_hip.so: the C ABI of include/scaml_gp.h on top of the
// gfx950 code object built from csrc/*.hip.
//
// The device code is compiled separately (see __graft_entry__.build): hipcc emits device LLVM IR,
// csrc/patch_ir.py adds the function attributes clang cannot express ("amdgpu-agpr-alloc"="0":
// the compiler may not touch the AGPR half of the register file, which the kernels manage by
// hand; per-kernel "amdgpu-num-vgpr"), clang lowers it to a code object that is embedded below
// and loaded through the HIP module API on first use.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/scaml_gp.h"
#include "../../include/scaml_gp_debug.h"
#include "gp_dispatch.h"       // (dispatch by shape; brings the fit, posterior and target argument blocks and LDS footprints)
#include "gp_fantasy_params.h"
#include "gp_stack_fit_params.h"
#include "gp_studies_acqf.h"   // (argument block and LDS footprint; its arithmetic is not called here)
#include "gp_acqf_opt.h"       // (argument block and state stride; likewise)
#include "gp_qacqf_opt.h"      // (likewise: the joint optimiser's step and gather blocks)
#include "gp_studies_score.h"  // (likewise: the strip scoring kernel's LDS footprint, the train-block arguments)
#include <math.h>

extern "C" const unsigned char scaml_hsaco_blob[];   // generated: lib/hsaco_blob.c
extern "C" const unsigned long scaml_hsaco_blob_len;

namespace {

thread_local char g_last_error[256] = "";

void set_error(const char* what, hipError_t e) {
  snprintf(g_last_error, sizeof(g_last_error), "%s: %s", what, hipGetErrorString(e));
}

constexpr size_t kLdsLimit = scaml::LDS_LIMIT;
// static LDS of the grouped GRAD pass with ordered sums (DET of csrc/gp_posterior.hip): the eight waves' shares of 16 means and of 16 variances
constexpr size_t kOrderedSumsLds = 2 * 8 * 16 * sizeof(double);

bool valid_kind(int kind) { return kind == SCAML_KIND_RBF || kind == SCAML_KIND_MATERN52; }

struct FitVariant {
  hipFunction_t fn[2][2];  // [dense | blocked addressing][kind]
};

// One family of kernel instances: the handles (consecutive, the last axis fastest), the symbol name as a printf pattern over
// the template arguments it is instantiated for, the dynamic LDS it may be launched with (0: none), and the argument values.
struct KernelAxis {
  int n = 1;
  int v[4] = {0};
};
struct KernelRow {
  hipFunction_t* slot;
  const char* pattern;
  size_t lds_cap;
  KernelAxis ax[3];
};

struct Module {
  std::mutex mu;
  bool loaded = false;
  hipModule_t mod = nullptr;
  std::atomic<int> num_cus{0};
  FitVariant fit[scaml::FIT_INSTANCES] = {};   // (NB, WU) of each: scaml::fit_instance
  hipFunction_t fit_full[2] = {};              // the full-tile instance of <16, 7> per kind: scaml::fit_full_instance
  hipFunction_t post[2] = {}, post_cov[2] = {}, post_linv[2] = {}, post_linv_cov[2] = {}, post_linv_grad[2] = {};
  hipFunction_t wsum = nullptr, linv = nullptr, chosolve = nullptr, kmat[2] = {}, mllgrad[2] = {};
  hipFunction_t tgt_assemble[2] = {}, tgt_finish = nullptr, tgt_fit = nullptr, tgt_fit_batched = nullptr, tgt_grad[2] = {};
  hipFunction_t tgt_fantasy = nullptr, tgt_fantasy_grad[2] = {};   // value only; value + gradient per kind
  hipFunction_t acqf_transform = nullptr;                          // the elementwise acquisition of given posteriors (7o)
  hipFunction_t post_linv_grad_joint[2] = {}, tgt_qacqf = nullptr;   // joint q-point acquisition: the GRAD pass with batch mates (5g), qEI / qUCB (7p)
  hipFunction_t tgt_qacqf_pending = nullptr;                         // ... with evaluations pending (7q)
  hipFunction_t post_linv_cov_joint[2] = {}, tgt_qacqf_value = nullptr;   // ... value only: the value-layout pass with batch mates (5h), (7r)
  hipFunction_t post_linv_grouped[2] = {}, tgt_acqf_batched = nullptr;   // lock-step studies: grouped GRAD pass, batched acquisition
  hipFunction_t post_linv_grouped_own[2] = {};                           // the grouped pass with per-group source tasks
  hipFunction_t post_linv_grouped_det[2] = {}, post_linv_grouped_det_own[2] = {};   // the GRAD grouped pass with ordered sums: (7l)'s rounds
  hipFunction_t post_linv_grouped_val[2] = {}, post_linv_grouped_val_own[2] = {};   // the value-only grouped pass (16 candidates per strip)
  hipFunction_t tgt_score_batched = nullptr, tgt_train_block[2] = {};     // studies' stage 1: strip scoring; the training blocks of all studies
  hipFunction_t tgt_fantasy_acqf_batched = nullptr, tgt_fantasy_score_batched = nullptr;   // both with pending evaluations (7k)
  hipFunction_t cond_block = nullptr, cond_fantasy = nullptr;   // the batched fantasy set-up of studies with pending evaluations (7m), (7n)
  hipFunction_t blk_round = nullptr, blk_finish = nullptr, coop[2] = {}, stack_step = nullptr, acqf_opt_step = nullptr;
  hipFunction_t qacqf_opt_step = nullptr, qacqf_opt_gather = nullptr;   // the joint acquisition's optimiser: step (7t), gather of a round (7s)
  hipFunction_t blk_solve[2][2] = {}, blk_syrk[2] = {};   // solve: [kind][D <= 8]
  hipFunction_t mllgrad_fused[4][2][2] = {};   // [size class NBT = 2, 4, 8, 16][kind][LDS-DMA staging]
  hipFunction_t mllgrad_split[2][2][2] = {};   // LDS-DMA staging, [N <= 128 | N <= 256 class][kind][2 | 4 workgroups per task]

  // `what` receives the step that failed (with the symbol, when one is missing)
  hipError_t load(char* what, size_t what_len) {
    std::lock_guard<std::mutex> lk(mu);
    if (loaded) return hipSuccess;
    snprintf(what, what_len, "loading the gfx950 code object");
    hipError_t e = hipModuleLoadData(&mod, scaml_hsaco_blob);
    if (e != hipSuccess) return e;
    // To add a kernel: a handle member above and one row here.  A kernel launched with dynamic LDS names its cap, or it
    // fails as soon as a shape asks for more than 64 KiB.
    const KernelAxis K{2, {0, 1}}, B{2, {0, 1}};   // kernel kind; a bool template argument
    std::vector<KernelRow> rows = {
        {post, "_ZN5scaml19gp_posterior_kernelILi%dEEEvNS_15PosteriorParamsE", kLdsLimit, {K}},
        {post_cov, "_ZN5scaml23gp_posterior_cov_kernelILi%dEEEvNS_18PosteriorCovParamsE", 0, {K}},
        {post_linv, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb0ELb0ELb0ELb0ELb0ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {post_linv_cov, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb0ELb0ELb0ELb0ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {post_linv_grad, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb1ELb0ELb0ELb0ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {post_linv_grouped, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb1ELb1ELb0ELb0ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {post_linv_grouped_own, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb1ELb1ELb1ELb0ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {post_linv_grouped_det, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb1ELb1ELb0ELb1ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit - kOrderedSumsLds, {K}},   // (static LDS: the waves' shares)
        {post_linv_grouped_det_own, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb1ELb1ELb1ELb1ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit - kOrderedSumsLds, {K}},   // (static LDS: the waves' shares)
        {post_linv_grouped_val, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb0ELb1ELb0ELb0ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {post_linv_grouped_val_own, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb0ELb1ELb1ELb0ELb0ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {post_linv_grad_joint, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb1ELb0ELb0ELb0ELb1ELb0EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {&tgt_qacqf, "scaml_target_qacqf_kernel", kLdsLimit, {}},
        {&tgt_qacqf_pending, "scaml_target_qacqf_pending_kernel", kLdsLimit, {}},
        {post_linv_cov_joint, "_ZN5scaml24gp_posterior_linv_kernelILi%dELb1ELb0ELb0ELb0ELb0ELb0ELb1EEEvNS_13PosteriorArgsIXT2_EXT5_EXT6_EE4typeE", kLdsLimit, {K}},
        {&tgt_qacqf_value, "scaml_target_qacqf_value_kernel", kLdsLimit, {}},
        {&tgt_acqf_batched, "scaml_target_acqf_batched_kernel", kLdsLimit, {}},
        {&tgt_score_batched, "scaml_target_score_batched_kernel", kLdsLimit, {}},
        {&tgt_fantasy_acqf_batched, "scaml_target_fantasy_acqf_batched_kernel", kLdsLimit, {}},
        {&tgt_fantasy_score_batched, "scaml_target_fantasy_score_batched_kernel", kLdsLimit, {}},
        {&cond_block, "scaml_studies_condition_block_kernel", kLdsLimit, {}},
        {&cond_fantasy, "scaml_studies_fantasy_condition_kernel", kLdsLimit, {}},
        {&tgt_train_block[0], "scaml_target_train_block_rbf_kernel", 0, {}},
        {&tgt_train_block[1], "scaml_target_train_block_matern_kernel", 0, {}},
        {&wsum, "scaml_weighted_task_sum_kernel", 0, {}},
        {&linv, "_ZN5scaml14gp_linv_kernelENS_10LinvParamsE", kLdsLimit, {}},
        {&chosolve, "_ZN5scaml19gp_cho_solve_kernelENS_14ChoSolveParamsE", kLdsLimit, {}},
        {mllgrad, "_ZN5scaml18gp_mll_grad_kernelILi%dEEEvNS_13MllGradParamsE", kLdsLimit - 2048, {K}},   // (the kernel also has 1 KB of static LDS)
        {kmat, "_Z23gp_kernel_matrix_kernelILi%dEEvN5scaml18KernelMatrixParamsE", 0, {K}},
        {&mllgrad_fused[0][0][0], "_ZN5scaml24gp_mll_grad_fused_kernelILi%dELi%dELb%dELi1EEEvNS_18MllGradFusedParamsE", kLdsLimit, {{4, {2, 4, 8, 16}}, K, B}},
        {&mllgrad_split[0][0][0], "_ZN5scaml24gp_mll_grad_fused_kernelILi%dELi%dELb1ELi%dEEEvNS_18MllGradFusedParamsE", kLdsLimit, {{2, {8, 16}}, K, {2, {2, 4}}}},
        {tgt_assemble, "_Z28scaml_target_assemble_kernelILi%dEEvN5scaml20TargetAssembleParamsE", 0, {K}},
        {tgt_grad, "_Z24scaml_target_grad_kernelILi%dEEvPKdS1_S1_S1_S1_S1_S1_S1_dPKiiiiPdS4_", 0, {K}},
        {&tgt_finish, "scaml_target_finish_kernel", 0, {}},
        {&tgt_fantasy, "scaml_target_fantasy_acqf_kernel", 0, {}},
        {&tgt_fantasy_grad[0], "scaml_target_fantasy_acqf_grad_rbf_kernel", 0, {}},
        {&tgt_fantasy_grad[1], "scaml_target_fantasy_acqf_grad_matern_kernel", 0, {}},
        {&acqf_transform, "scaml_acqf_transform_kernel", 0, {}},
        {&tgt_fit, "scaml_target_fit_kernel", kLdsLimit, {}},
        {&tgt_fit_batched, "scaml_target_fit_batched_kernel", kLdsLimit, {}},
        {coop, "_ZN5scaml18gp_fit_coop_kernelILi%dEEEvNS_13CoopFitParamsE", kLdsLimit, {K}},
        {&stack_step, "scaml_stack_fit_step_kernel", 0, {}},
        {&acqf_opt_step, "scaml_acqf_opt_step_kernel", 0, {}},
        {&qacqf_opt_step, "scaml_qacqf_opt_step_kernel", 0, {}},
        {&qacqf_opt_gather, "scaml_qacqf_opt_gather_kernel", 0, {}},
        {&blk_round, "scaml_blocked_round_kernel", 0, {}},
        {&blk_finish, "scaml_blocked_finish_kernel", 0, {}},
        {&blk_solve[0][0], "_ZN5scaml23gp_blocked_solve_kernelILi%dELb%dEEEvNS_16BlockedFitParamsE", kLdsLimit, {K, B}},
        {blk_syrk, "_ZN5scaml22gp_blocked_syrk_kernelILi%dEEEvNS_16BlockedFitParamsE", kLdsLimit, {K}},
    };
    for (int i = 0; i < scaml::FIT_INSTANCES; ++i) {   // the kernels use up to the full 160 KiB of LDS
      const scaml::FitInstance v = scaml::fit_instance(i);
      rows.push_back({fit[i].fn[0], "_ZN5scaml19gp_fit_fused_kernelILi%dELi%dELi%dELb0EEEvNS_9FitParamsE", kLdsLimit, {{1, {v.nb}}, {1, {v.wu}}, K}});
      rows.push_back({fit[i].fn[1], "_ZN5scaml21gp_fit_blocked_kernelILi%dELi%dELi%dEEEvNS_9FitParamsENS_14FitBlockParamsE", kLdsLimit, {{1, {v.nb}}, {1, {v.wu}}, K}});
    }
    rows.push_back({fit_full, "_ZN5scaml19gp_fit_fused_kernelILi16ELi7ELi%dELb1EEEvNS_9FitParamsE", kLdsLimit, {K}});
    for (const KernelRow& r : rows) {
      hipFunction_t* slot = r.slot;
      for (int i = 0; i < r.ax[0].n; ++i) {
        for (int j = 0; j < r.ax[1].n; ++j) {
          for (int k = 0; k < r.ax[2].n; ++k, ++slot) {
            char name[160];
            snprintf(name, sizeof(name), r.pattern, r.ax[0].v[i], r.ax[1].v[j], r.ax[2].v[k]);
            e = hipModuleGetFunction(slot, mod, name);
            if (e == hipSuccess && r.lds_cap) e = hipFuncSetAttribute((const void*)*slot, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds_cap);
            if (e != hipSuccess) {
              snprintf(what, what_len, "loading the gfx950 code object (%s)", name);
              return e;
            }
          }
        }
      }
    }
    loaded = true;
    return hipSuccess;
  }
};

// One Module per device ordinal: hipModuleLoadData loads the code object into the CURRENT device's context and the
// hipFunction_t handles are only valid there, so a process that works on several GPUs (cuda:0, then cuda:1) gets one
// lazily loaded copy per device.  Every entry point runs on the current device (hipGetDevice), which therefore has
// to be the device the pointers and the stream belong to.
constexpr int kMaxDevices = 64;
Module& module() {
  static std::mutex mu;
  static Module* mods[kMaxDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (!mods[dev]) mods[dev] = new Module();
  return *mods[dev];
}

// the current device's module with every kernel loaded, or NULL with the last error set
Module* ready() {
  Module& m = module();
  char what[192];
  const hipError_t e = m.load(what, sizeof(what));
  if (e == hipSuccess) return &m;
  set_error(what, e);
  return nullptr;
}

int num_cus(Module& m) {
  int cus = m.num_cus.load(std::memory_order_relaxed);
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    m.num_cus.store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// The one launch: `args` non-NULL passes plain arguments, otherwise `size` bytes at `kernarg` are the kernel-argument block.
int launch_raw(hipFunction_t fn, dim3 grid, unsigned block, size_t lds_bytes, void* stream, const char* label, void* kernarg, size_t size,
               void** args) {
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, kernarg, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  const hipError_t e = hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, block, 1, 1, (unsigned)lds_bytes, (hipStream_t)stream, args,
                                             args ? nullptr : config);
  if (e == hipSuccess) return SCAML_OK;
  char what[96];
  snprintf(what, sizeof(what), "hipModuleLaunchKernel(%s)", label);
  set_error(what, e);
  return SCAML_E_LAUNCH;
}
template <class Params>
int launch(hipFunction_t fn, dim3 grid, unsigned block, size_t lds_bytes, void* stream, const char* label, Params& p, size_t size = sizeof(Params)) {
  return launch_raw(fn, grid, block, lds_bytes, stream, label, &p, size, nullptr);
}
int launch_args(hipFunction_t fn, dim3 grid, unsigned block, void* stream, const char* label, void** args) {
  return launch_raw(fn, grid, block, 0, stream, label, nullptr, 0, args);
}

}  // namespace

extern "C" {

// ---- developer switches ---------------------------------------------------------------------------------------------
// Process-global, outside the stable ABI (include/scaml_gp_debug.h); each starts from its environment variable.
namespace {
struct DevSwitches {
  const bool no_grad_split = getenv("SCAML_GRAD_NO_SPLIT") != nullptr;   // A/B: never split a gradient task over workgroups
  std::atomic<int> grad_path{getenv("SCAML_GRAD_LEGACY") ? 1 : (getenv("SCAML_GRAD_FUSED") ? 2 : 0)};   // 0 by shape, 1 two launches, 2 single launch
  // 0 by shape, 1 the 2 x 2 sequence of launches only, 2 the several-CUs-per-task kernel whenever it is launchable
  std::atomic<int> blocked_fit_path{getenv("SCAML_BLOCKED_FIT_PATH") ? atoi(getenv("SCAML_BLOCKED_FIT_PATH")) : 0};
  std::atomic<int> blocked_fit_last{0};   // which one the last call took (1 / 2)
  std::atomic<int> coop_far{getenv("SCAML_COOP_FAR") != nullptr};   // A/B / tests: write-through payload stores even when a task's workgroups share an XCD
  std::atomic<int> target_fit_path{getenv("SCAML_TARGET_FIT_NO_MFMA") ? 1 : 0};   // 0 by shape, 1 column-by-column elimination only
  std::atomic<int> grouped_ordered{getenv("SCAML_GROUPED_ORDERED_SUMS") ? 1 : 0};   // tests: 1 (5e) / (5e') launch the instance with ordered sums
} g_dev;
constexpr auto kRelaxed = std::memory_order_relaxed;
}  // namespace

int scaml_debug_coop_far(int on) {
  const int was = g_dev.coop_far.load(kRelaxed);
  if (on == 0 || on == 1) g_dev.coop_far.store(on, kRelaxed);
  return was;
}
int scaml_debug_blocked_fit_path(int mode) {
  const int was = g_dev.blocked_fit_path.load(kRelaxed);
  if (mode >= 0 && mode <= 2) g_dev.blocked_fit_path.store(mode, kRelaxed);
  return mode == -1 ? g_dev.blocked_fit_last.load(kRelaxed) : was;
}
int scaml_debug_target_fit_path(int mode) { return g_dev.target_fit_path.exchange(mode == 1 ? 1 : 0, kRelaxed); }
int scaml_debug_force_two_launch_grad(int mode) { return g_dev.grad_path.exchange(mode == 1 ? 1 : (mode == 2 ? 2 : 0), kRelaxed); }
int scaml_debug_grouped_ordered_sums(int mode) { return g_dev.grouped_ordered.exchange(mode == 1 ? 1 : 0, kRelaxed); }
int scaml_debug_set_stamp_buffer(long long* buf) {
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  hipDeviceptr_t sym = nullptr;
  size_t bytes = 0;
  if (hipModuleGetGlobal(&sym, &bytes, m->mod, "g_stamp_buf") != hipSuccess) return SCAML_E_BADARG;
  if (hipMemcpyHtoD(sym, &buf, sizeof(buf)) != hipSuccess) return SCAML_E_LAUNCH;
  // (the full-tile fit instances are a translation unit of their own, with a pointer of their own)
  if (hipModuleGetGlobal(&sym, &bytes, m->mod, "g_stamp_buf_full") != hipSuccess) return SCAML_E_BADARG;
  return hipMemcpyHtoD(sym, &buf, sizeof(buf)) == hipSuccess ? 0 : SCAML_E_LAUNCH;
}

int scaml_version(void) { return 400; }  // 0.4.0 = 10000 * 0 + 100 * 4 + 0
const char* scaml_last_error(void) { return g_last_error; }
int scaml_fit_max_n(void) { return 256; }

int scaml_fit_max_d(int N) { return scaml::fit_class_max_d(N); }

static int fit_common(scaml::FitParams p, int kind, void* stream, const scaml::FitBlockParams* blk = nullptr) {
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  const scaml::FitPlan plan = scaml::fit_plan(p.T, p.N, p.D, num_cus(*m));
  const size_t lds = plan.lds_doubles * sizeof(double);
  if (lds > kLdsLimit) return SCAML_E_TOOLARGE;
  struct { scaml::FitParams p; scaml::FitBlockParams b; } args{p, blk ? *blk : scaml::FitBlockParams{}};   // (kernarg layout: both 8-byte aligned)
  // the full-tile instance where the arguments satisfy its contract (pointer values only: nothing here touches the device).
  // SCAML_FIT_NO_FULL (set, not empty, not "0"): never -- read at every launch, so that one process can run both instances on
  // the same input by changing its environment between two calls (include/scaml_gp_debug.h)
  const char* no_full = getenv("SCAML_FIT_NO_FULL");
  const int full_mode = (no_full && no_full[0] && !(no_full[0] == '0' && !no_full[1])) ? 1 : 0;
  const bool full = scaml::fit_full_instance(plan.nb, plan.wu, p.N, p.n_points != nullptr, p.A_in != nullptr, blk != nullptr,
                                             (p.flags & SCAML_FIT_STORE_L) != 0, (size_t)p.L, full_mode);
  return launch(full ? m->fit_full[kind] : m->fit[plan.variant].fn[blk ? 1 : 0][kind], dim3((unsigned)p.T), plan.block, lds, stream, "gp_fit_fused", args,
                blk ? sizeof(args) : sizeof(p));
}

int scaml_gp_fit_fused_f64(const double* X, const double* y, const double* theta,
                           const int32_t* n_points, const double* jitter_in,
                           int T, int N, int D, int kind,
                           double* L, double* alpha, double* quad, double* logdet, double* mll,
                           int32_t* info, double* jitter_used, double* Linv_diag, unsigned flags, void* stream) {
  if (T < 0 || N < 1 || D < 1) return SCAML_E_BADARG;
  if (!X || !y || !theta || !info) return SCAML_E_BADARG;
  if ((flags & SCAML_FIT_STORE_L) && !L) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (N > scaml_fit_max_n()) return SCAML_E_TOOLARGE;
  if (D > scaml_fit_max_d(N)) return SCAML_E_TOOLARGE;
  if (T == 0) return SCAML_OK;
  scaml::FitParams p{X, y, theta, n_points, jitter_in, nullptr, L, alpha, quad, logdet, mll, info, jitter_used, Linv_diag, T, N, D, flags};
  return fit_common(p, kind, stream);
}

// ---- (3b) blocked fit, 256 < N <= 512 ---------------------------------------------------------------------
int scaml_fit_blocked_max_n(void) { return 512; }

int scaml_fit_blocked_max_d(void) {
  static int dmax = 0;
  if (!dmax) {
    int d = 1;
    while (scaml::blocked_solve_lds_doubles(d + 1) * sizeof(double) <= kLdsLimit) ++d;
    const int dfit = scaml_fit_max_d(256);
    dmax = d < dfit ? d : dfit;
  }
  return dmax;
}

namespace {
struct BlockedLayout {
  size_t S, Vimg, r2, q12, jit_cur, jit_ladder, n1, n2, active, info1, info2, total;
};
BlockedLayout blocked_layout(int T, int N) {
  const size_t n2 = (size_t)(N - 256), t = (size_t)T, tp = (t + 1) & ~(size_t)1;   // (int arrays: 8-byte multiples)
  BlockedLayout l{};
  size_t o = 0;
  l.S = o; o += t * n2 * n2 * 8;
  l.Vimg = o; o += t * 256 * 256 * 8;
  l.r2 = o; o += t * (size_t)N * 8;
  l.q12 = o; o += 4 * t * 8;
  l.jit_cur = o; o += t * 8;
  l.jit_ladder = o; o += t * 8;
  l.n1 = o; o += tp * 4;
  l.n2 = o; o += tp * 4;
  l.active = o; o += tp * 4;
  l.info1 = o; o += tp * 4;
  l.info2 = o; o += tp * 4;
  l.total = o;
  return l;
}
}  // namespace

long long scaml_gp_fit_blocked_workspace_bytes(int T, int N) {
  if (T < 0 || N <= 256 || N > 512) return 0;
  return (long long)blocked_layout(T, N).total;
}

int scaml_gp_fit_blocked_f64(const double* X, const double* y, const double* theta,
                             const int32_t* n_points, const double* jitter_in,
                             int T, int N, int D, int kind,
                             double* L, double* alpha, double* quad, double* logdet, double* mll,
                             int32_t* info, double* jitter_used, double* Linv_diag, unsigned flags,
                             void* workspace, long long workspace_bytes, void* stream) {
  if (T < 0 || N < 1 || D < 1) return SCAML_E_BADARG;
  if (!X || !y || !theta || !info || !L || !alpha || !Linv_diag) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (N <= scaml_fit_max_n() || N > scaml_fit_blocked_max_n() || (N & 15)) return SCAML_E_TOOLARGE;
  if (D > scaml_fit_blocked_max_d()) return SCAML_E_TOOLARGE;
  if (T == 0) return SCAML_OK;
  const BlockedLayout lay = blocked_layout(T, N);
  if (!workspace || workspace_bytes < (long long)lay.total || ((uintptr_t)workspace & 15)) return SCAML_E_BADARG;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  char* ws = (char*)workspace;
  const scaml::BlockedPlan plan =
      scaml::blocked_plan(T, N, D, num_cus(*m), g_dev.blocked_fit_path.load(kRelaxed), workspace_bytes, (flags & SCAML_FIT_NO_RETRY) != 0);
  const int t8 = plan.t8;
  if (plan.path == 2) {
    const size_t flag_bytes = plan.flag_bytes;
    const hipError_t e = hipMemsetAsync(ws, 0, flag_bytes, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("hipMemsetAsync(coop flags)", e); return SCAML_E_LAUNCH; }
    scaml::CoopFitParams c{X, y, theta, n_points, jitter_in, L, alpha, quad, logdet, mll, info, jitter_used, Linv_diag,
                           (unsigned*)ws, (unsigned*)ws + (size_t)T * 32, (unsigned*)ws + (size_t)T * 36, (double*)(ws + flag_bytes), (double*)(ws + flag_bytes) + (size_t)T * N,
                           T, N, D, flags | (g_dev.coop_far.load(kRelaxed) ? 0x80000000u : 0u), plan.parts};
    const int rc = launch(m->coop[kind], dim3((unsigned)(t8 * plan.parts)), 512, plan.lds_coop, stream, "gp_fit_coop", c);
    if (rc == SCAML_OK) g_dev.blocked_fit_last.store(2, kRelaxed);
    return rc;
  }
  g_dev.blocked_fit_last.store(1, kRelaxed);
  const int N1 = 256, N2 = N - N1, NBT = N / 16;
  scaml::BlockedFitParams p{X, y, theta, n_points, jitter_in, L, alpha, quad, logdet, mll, info, jitter_used, Linv_diag,
                            (double*)(ws + lay.S), (double*)(ws + lay.Vimg), (double*)(ws + lay.r2), (double*)(ws + lay.q12), (double*)(ws + lay.jit_cur),
                            (double*)(ws + lay.jit_ladder), (int32_t*)(ws + lay.n1), (int32_t*)(ws + lay.n2), (int32_t*)(ws + lay.active),
                            (int32_t*)(ws + lay.info1), (int32_t*)(ws + lay.info2), T, N, D, flags, 0};
  const unsigned fl = SCAML_FIT_STORE_L | SCAML_FIT_NO_RETRY | (flags & SCAML_FIT_ZERO_UPPER);
  scaml::FitParams f1{X, y, theta, p.n1, p.jit_cur, nullptr, L, alpha, p.q12, p.q12 + T, nullptr, p.info1, nullptr, Linv_diag, T, N1, D, fl | scaml::FIT_FORWARD_ONLY};
  const scaml::FitBlockParams b1{(long long)N * D, N, (long long)N * N, (long long)NBT * 256, p.active, N};
  scaml::FitParams f2{nullptr, p.r2 + N1, nullptr, p.n2, nullptr, p.S, L + (size_t)N1 * N + N1, alpha + N1, p.q12 + 2 * (size_t)T, p.q12 + 3 * (size_t)T,
                      nullptr, p.info2, nullptr, Linv_diag + (size_t)(N1 / 16) * 256, T, N2, 1, fl};
  const scaml::FitBlockParams b2{0, N, (long long)N * N, (long long)NBT * 256, p.active, N};
  const int nt = plan.nt;
  int rc = SCAML_OK;
  for (int r = 0; r < plan.rounds; ++r) {
    p.round = r;
    if ((rc = launch(m->blk_round, dim3((unsigned)((T + 255) / 256)), 256, 0, stream, "blocked_round", p)) != SCAML_OK) return rc;
    if ((rc = fit_common(f1, kind, stream, &b1)) != SCAML_OK) return rc;
    if ((rc = launch(m->blk_solve[kind][plan.solve_small_d], dim3((unsigned)(t8 * nt)), 512, plan.lds_solve, stream, "gp_blocked_solve", p)) != SCAML_OK) return rc;
    if ((rc = launch(m->blk_syrk[kind], dim3((unsigned)(t8 * (nt * (nt + 1) / 2))), 512, plan.lds_syrk, stream, "gp_blocked_syrk", p)) != SCAML_OK) return rc;
    if ((rc = fit_common(f2, SCAML_KIND_RBF, stream, &b2)) != SCAML_OK) return rc;
  }
  return launch(m->blk_finish, dim3((unsigned)T), 1024, 0, stream, "blocked_finish", p);
}

// ---- (2) batched jittered Cholesky of given matrices ------------------------------------------------
int scaml_potrf_batched_f64(const double* A, const double* y, const int32_t* n_points, const double* jitter_in,
                            int T, int N, double* L, double* alpha, double* quad, double* logdet,
                            int32_t* info, double* jitter_used, double* Linv_diag, unsigned flags, void* stream) {
  if (T < 0 || N < 1) return SCAML_E_BADARG;
  if (!A || !info) return SCAML_E_BADARG;
  if ((flags & SCAML_FIT_STORE_L) && !L) return SCAML_E_BADARG;
  if (alpha && !y) return SCAML_E_BADARG;
  if (N > scaml_fit_max_n()) return SCAML_E_TOOLARGE;
  if (T == 0) return SCAML_OK;
  scaml::FitParams p{nullptr, y, nullptr, n_points, jitter_in, A, L, alpha, quad, logdet, nullptr, info, jitter_used, Linv_diag, T, N, 1, flags};
  return fit_common(p, SCAML_KIND_RBF, stream);
}

// ---- (5) batched source posteriors ------------------------------------------------------------
int scaml_posterior_max_n(void) { return 512; }

int scaml_posterior_batched_f64(const double* Xq, const double* X, const double* theta, const double* L,
                                const double* Linv_diag, const double* alpha, const double* y_mean,
                                const double* y_std, const int32_t* n_points, int T, int N, int M, int D, int kind,
                                double* mu, double* var, double* V, unsigned flags, void* stream) {
  if (T < 0 || N < 1 || M < 0 || D < 1) return SCAML_E_BADARG;
  if (!Xq || !X || !theta || !alpha) return SCAML_E_BADARG;
  if (!(flags & SCAML_POST_MEAN_ONLY) && (!L || !Linv_diag)) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (N > scaml_posterior_max_n()) return SCAML_E_TOOLARGE;
  if (T == 0 || M == 0) return SCAML_OK;
  const scaml::PosteriorPlan plan = scaml::posterior_plan(N, D);
  const int waves = plan.waves;
  const bool xl = plan.xl;
  if (!waves) return SCAML_E_TOOLARGE;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  const int per_task = (flags & SCAML_POST_XQ_PER_TASK) ? 1 : 0, mean_only = (flags & SCAML_POST_MEAN_ONLY) ? 1 : 0;
  if (mean_only && (var || V)) return SCAML_E_BADARG;
  scaml::PosteriorParams p{Xq, X, theta, L, Linv_diag, alpha, y_mean, y_std, n_points, mu, var, V, T, N, M, D, xl ? 1 : 0, per_task, mean_only};
  const int strips = (M + 15) / 16;
  return launch(m->post[kind], dim3((unsigned)((strips + waves - 1) / waves), (unsigned)T), (unsigned)waves * 64,
                scaml::posterior_lds_doubles(N, D, waves, xl) * sizeof(double), stream, "gp_posterior", p);
}

int scaml_posterior_cov_f64(const double* Xq, const double* theta, const double* V, const double* y_std,
                            int T, int N, int M, int Ma, int D, int kind, double* cov, unsigned flags, void* stream) {
  if (T < 0 || N < 1 || M < 0 || Ma < 0 || Ma > M || D < 1) return SCAML_E_BADARG;
  if (!Xq || !theta || !V || !cov) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (T == 0 || M == 0 || Ma == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::PosteriorCovParams p{Xq, theta, V, y_std, cov, T, N, M, Ma, D, (flags & SCAML_POST_XQ_PER_TASK) ? 1 : 0};
  const int tiles_c = (M + 15) / 16, tiles_a = (Ma + 15) / 16;
  return launch(m->post_cov[kind], dim3((unsigned)((tiles_c + 3) / 4), (unsigned)tiles_a, (unsigned)T), 256, 0, stream, "gp_posterior_cov", p);
}

// ---- (6) weighted sum over tasks ---------------------------------------------------------------
// (check and launch apart, here and below for every launch of a joint acquisition round: (7s) checks each once and launches it per round)
static int wsum_check(const double* in, const double* w, int T, long long len, int power, const double* out) {
  if (T < 0 || len < 0 || (power != 1 && power != 2)) return SCAML_E_BADARG;
  if (!in || !w || !out) return SCAML_E_BADARG;
  return SCAML_OK;
}
static int wsum_launch(Module& m, const double* in, const double* w, const uint8_t* active, int T, long long len, int power, double* out,
                       void* stream) {   // checked, len > 0
  void* args[] = {(void*)&in, (void*)&w, (void*)&active, (void*)&T, (void*)&len, (void*)&power, (void*)&out};
  return launch_args(m.wsum, dim3((unsigned)((len + 63) / 64)), 256, stream, "weighted_task_sum", args);
}
int scaml_weighted_task_sum_f64(const double* in, const double* w, const uint8_t* active, int T, long long len,
                                int power, double* out, void* stream) {
  if (const int rc = wsum_check(in, w, T, len, power, out)) return rc;
  if (len == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return wsum_launch(*m, in, w, active, T, len, power, out, stream);
}

// ---- (1) stand-alone kernel matrix ---------------------------------------------------------------
int scaml_kernel_matrix_f64(const double* X1, const double* X2, const double* theta, int T, int N1, int N2, int D,
                            int kind, int x2_shared, int add_noise, double* K, void* stream) {
  if (T < 0 || N1 < 1 || N2 < 1 || D < 1) return SCAML_E_BADARG;
  if (!X1 || !theta || !K) return SCAML_E_BADARG;
  if (!X2 && N1 != N2) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (T == 0) return SCAML_OK;
  if (N1 > 65535 || T > 65535) return SCAML_E_TOOLARGE;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::KernelMatrixParams p{X1, X2, theta, K, T, N1, N2, D, x2_shared, add_noise};
  return launch(m->kmat[kind], dim3((unsigned)((N2 + 127) / 128), (unsigned)N1, (unsigned)T), 128, 0, stream, "gp_kernel_matrix", p);
}

// ---- batched Cholesky solve ----------------------------------------------------------------------
static int cho_solve_check(const scaml::ChoSolveParams& p) {
  if (p.T < 0 || p.N < 1 || p.R < 0) return SCAML_E_BADARG;
  if (!p.L || !p.Linv_diag || !p.B || !p.Xout) return SCAML_E_BADARG;
  if (p.N > scaml_posterior_max_n()) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
static int cho_solve_launch(Module& m, scaml::ChoSolveParams& p, void* stream) {   // a checked, non-empty block
  const int nb = (p.N + 15) / 16, np = nb * 16, strips = (p.R + 15) / 16;
  int waves = scaml::strip_solve_waves(np);
  if (waves > strips) waves = strips;
  return launch(m.chosolve, dim3((unsigned)((strips + waves - 1) / waves), (unsigned)p.T), (unsigned)waves * 64,
                scaml::strip_solve_lds_doubles(np, waves) * sizeof(double), stream, "gp_cho_solve", p);
}
static int cho_solve_common(const double* L, const double* Linv_diag, const double* B, const int32_t* n_points,
                           int T, int N, int R, double* Xout, int mode, void* stream) {
  scaml::ChoSolveParams p{L, Linv_diag, B, n_points, Xout, T, N, R, mode};
  if (const int rc = cho_solve_check(p)) return rc;
  if (T == 0 || R == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return cho_solve_launch(*m, p, stream);
}

int scaml_cho_solve_batched_f64(const double* L, const double* Linv_diag, const double* B, const int32_t* n_points,
                                int T, int N, int R, double* Xout, void* stream) {
  return cho_solve_common(L, Linv_diag, B, n_points, T, N, R, Xout, 0, stream);
}

int scaml_solve_lt_batched_f64(const double* L, const double* Linv_diag, const double* B, const int32_t* n_points,
                               int T, int N, int R, double* Xout, void* stream) {
  return cho_solve_common(L, Linv_diag, B, n_points, T, N, R, Xout, 1, stream);
}

// the weighted target prior in one call: mean with w, covariance with w^2 (two launches of the sum kernel)
int scaml_weighted_prior_reduce_f64(const double* mu, const double* cov, const double* w, const uint8_t* active, int T, int M,
                                    int Ma, double* mu_s, double* cov_s, void* stream) {
  if (T < 0 || M < 0 || Ma < 0) return SCAML_E_BADARG;
  if (!w || (mu && !mu_s) || (cov && !cov_s) || (!mu && !cov)) return SCAML_E_BADARG;
  int rc = SCAML_OK;
  if (mu) rc = scaml_weighted_task_sum_f64(mu, w, active, T, (long long)M, 1, mu_s, stream);
  if (rc == SCAML_OK && cov) rc = scaml_weighted_task_sum_f64(cov, w, active, T, (long long)Ma * M, 2, cov_s, stream);
  return rc;
}

// ---- explicit inverse factor + posteriors from it -------------------------------------------------
static int launch_linv(Module& m, const double* L, const double* Linv_diag, const int32_t* n_points, int T, int N,
                       double* Linv, void* stream, int lower_only = 0) {
  const int nb = (N + 15) / 16, np = nb * 16;
  const int waves = scaml::strip_solve_waves(np);
  scaml::LinvParams p{L, Linv_diag, n_points, Linv, T, N, lower_only};
  return launch(m.linv, dim3((unsigned)scaml::linv_groups(T, nb, waves), (unsigned)T), (unsigned)waves * 64, scaml::strip_solve_lds_doubles(np, waves) * sizeof(double),
                stream, "gp_linv", p);
}

static int linv_batched(const double* L, const double* Linv_diag, const int32_t* n_points, int T, int N, double* Linv, void* stream,
                        int lower_only) {
  if (T < 0 || N < 1) return SCAML_E_BADARG;
  if (!L || !Linv_diag || !Linv) return SCAML_E_BADARG;
  if (N > scaml_posterior_max_n()) return SCAML_E_TOOLARGE;
  if (T == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return launch_linv(*m, L, Linv_diag, n_points, T, N, Linv, stream, lower_only);
}

int scaml_linv_batched_f64(const double* L, const double* Linv_diag, const int32_t* n_points, int T, int N, double* Linv,
                           void* stream) {
  return linv_batched(L, Linv_diag, n_points, T, N, Linv, stream, 0);
}

int scaml_linv_batched_lower_f64(const double* L, const double* Linv_diag, const int32_t* n_points, int T, int N, double* Linv,
                                 void* stream) {
  return linv_batched(L, Linv_diag, n_points, T, N, Linv, stream, 1);
}

// The inverse-factor pass's block (L = Linv; Ma = 0 without VA): the arguments, then the LDS strip, then the launch.
static int posterior_linv_check(const scaml::PosteriorParams& p, int kind, unsigned flags, bool grad) {
  if (p.T < 0 || p.N < 1 || p.M < 0 || p.D < 1) return SCAML_E_BADARG;
  if (!p.Xq || !p.X || !p.theta || !p.L || !p.alpha) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (flags & SCAML_POST_MEAN_ONLY) return SCAML_E_BADARG;   // (use scaml_posterior_batched_f64 for that)
  if (p.N > scaml_posterior_max_n()) return SCAML_E_TOOLARGE;
  if (p.VA && (!p.cov || p.Ma < 1 || (!grad && p.Ma > p.M))) return SCAML_E_BADARG;
  if (p.VA && (p.Ma > 96 || p.Ma > p.N)) return SCAML_E_TOOLARGE;      // six 16-point strips of leading query points at most
  return SCAML_OK;
}
static int posterior_linv_fits(const scaml::PosteriorParams& p) {
  return scaml::posterior_linv_lds_doubles(p.N, p.D) * sizeof(double) > kLdsLimit ? SCAML_E_TOOLARGE : SCAML_OK;
}
static int posterior_linv_launch(Module& m, scaml::PosteriorParams& p, int kind, bool grad, void* stream) {   // a checked, non-empty block that fits
  const size_t lds = scaml::posterior_linv_lds_doubles(p.N, p.D) * sizeof(double);
  const unsigned strips = (unsigned)((p.M + 15) / 16);
  const unsigned blocks = (unsigned)(((p.T + 7) / 8) * 8) * strips;   // XCD-aware (task, strip) map inside the kernel
  return launch(grad ? m.post_linv_grad[kind] : (p.VA ? m.post_linv_cov[kind] : m.post_linv[kind]), dim3(blocks), 512, lds, stream,
                "gp_posterior_linv", p);
}

static int posterior_linv_common(const double* Xq, const double* X, const double* theta, const double* Linv, const double* alpha,
                                 const double* y_mean, const double* y_std, const int32_t* n_points, const double* VA, int T, int N,
                                 int M, int Ma, int D, int kind, double* mu, double* var, double* V, double* cov, unsigned flags,
                                 void* stream, bool grad = false, const double* Xa = nullptr) {
  // (x_in_lds = 0: the task's points are MFMA operands read from memory, nothing to stage)
  scaml::PosteriorParams p{Xq, X, theta, Linv, nullptr, alpha, y_mean, y_std, n_points, mu, var, V, T, N, M, D, 0,
                           (flags & SCAML_POST_XQ_PER_TASK) ? 1 : 0, 0, VA, cov, VA ? Ma : 0, 0, Xa};
  if (const int rc = posterior_linv_check(p, kind, flags, grad)) return rc;
  if (T == 0 || M == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  if (const int rc = posterior_linv_fits(p)) return rc;
  return posterior_linv_launch(*m, p, kind, grad, stream);
}

int scaml_posterior_linv_f64(const double* Xq, const double* X, const double* theta, const double* Linv, const double* alpha,
                             const double* y_mean, const double* y_std, const int32_t* n_points, int T, int N, int M, int D,
                             int kind, double* mu, double* var, double* V, unsigned flags, void* stream) {
  return posterior_linv_common(Xq, X, theta, Linv, alpha, y_mean, y_std, n_points, nullptr, T, N, M, 0, D, kind, mu, var, V, nullptr,
                               flags, stream);
}

int scaml_posterior_linv_cov_f64(const double* Xq, const double* X, const double* theta, const double* Linv, const double* alpha,
                                 const double* y_mean, const double* y_std, const int32_t* n_points, const double* VA, int T, int N,
                                 int M, int Ma, int D, int kind, double* mu, double* var, double* cov, unsigned flags, void* stream) {
  if (!VA || !cov) return SCAML_E_BADARG;
  return posterior_linv_common(Xq, X, theta, Linv, alpha, y_mean, y_std, n_points, VA, T, N, M, Ma, D, kind, mu, var, nullptr, cov,
                               flags, stream);
}

// (5d) the posterior pass with input gradients: 16 columns per query point = [value, d/dx_0 .. d/dx_{D-1}, zeros]
int scaml_posterior_linv_grad_f64(const double* Xq, const double* Xa, const double* X, const double* theta, const double* Linv,
                                  const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                  const double* VA, int T, int N, int Mq, int Ma, int D, int kind, double* mu, double* var, double* cov,
                                  unsigned flags, void* stream) {
  if (Mq < 0 || Ma < 0 || D > 15) return D > 15 ? SCAML_E_TOOLARGE : SCAML_E_BADARG;
  if (Ma > 0 && (!VA || !cov || !Xa)) return SCAML_E_BADARG;
  if (Mq > (1 << 26)) return SCAML_E_TOOLARGE;
  return posterior_linv_common(Xq, X, theta, Linv, alpha, y_mean, y_std, n_points, Ma > 0 ? VA : nullptr, T, N, 16 * Mq, Ma > 0 ? Ma : 0, D, kind,
                               mu, var, nullptr, Ma > 0 ? cov : nullptr, flags, stream, true, Xa);
}

// (5g) (5d) for query points that move in batches of q: q more covariance rows per strip, against the strip's batch mates
int scaml_qacqf_max_q(void) { return scaml::QACQF_MAX_Q; }
int scaml_qacqf_max_samples(void) { return scaml::QACQF_MAX_SAMPLES; }

// (5g)'s block: base.M = 16 columns per query point (saturated: the check refuses what does not fit), Mq handed on beside it
static scaml::PosteriorJointParams grad_joint_block(const double* Xq, const double* Xa, const double* X, const double* theta, const double* Linv,
                                                    const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                                    const double* VA, const double* VQ, int T, int N, int Mq, int Ma, int q, int D, double* mu,
                                                    double* var, double* cov, unsigned flags) {
  const long long M = 16LL * Mq;
  return scaml::PosteriorJointParams{{Xq, X, theta, Linv, nullptr, alpha, y_mean, y_std, n_points, mu, var, nullptr, T, N,
                                      M > INT32_MAX ? INT32_MAX : (int)M, D, 0, (flags & SCAML_POST_XQ_PER_TASK) ? 1 : 0, 0, VA, cov, Ma, 0, Xa},
                                     {VQ, q, 0}};
}
static int grad_joint_check(const scaml::PosteriorJointParams& p, int Mq, int kind, unsigned flags) {
  const scaml::PosteriorParams& b = p.base;
  const int q = p.ja.q;
  if (b.T < 0 || b.N < 1 || Mq < 0 || b.Ma < 1 || q < 1 || b.D < 1 || Mq % q != 0) return SCAML_E_BADARG;
  if (!b.Xq || !b.Xa || !b.X || !b.theta || !b.L || !b.alpha || !b.VA || !p.ja.VQ || !b.cov) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (flags & SCAML_POST_MEAN_ONLY) return SCAML_E_BADARG;
  if (b.D > 15 || q > scaml::QACQF_MAX_Q || Mq > (1 << 26)) return SCAML_E_TOOLARGE;
  if (b.N > scaml_posterior_max_n()) return SCAML_E_TOOLARGE;
  if (b.Ma + q > scaml::QACQF_MAX_ROWS || b.Ma + q > b.N) return SCAML_E_TOOLARGE;   // six 16-row strips of the covariance block, staged in the N x 16 LDS strip
  return posterior_linv_fits(b);
}
static int grad_joint_launch(Module& m, scaml::PosteriorJointParams& p, int Mq, int kind, void* stream) {   // a checked, non-empty block
  const size_t lds = scaml::posterior_linv_lds_doubles(p.base.N, p.base.D) * sizeof(double);
  const unsigned blocks = (unsigned)(((p.base.T + 7) / 8) * 8) * (unsigned)Mq;   // XCD-aware (task, strip) map inside the kernel, a strip per query point
  return launch(m.post_linv_grad_joint[kind], dim3(blocks), 512, lds, stream, "gp_posterior_linv_joint", p);
}

int scaml_posterior_linv_grad_joint_f64(const double* Xq, const double* Xa, const double* X, const double* theta, const double* Linv,
                                        const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                        const double* VA, const double* VQ, int T, int N, int Mq, int Ma, int q, int D, int kind, double* mu,
                                        double* var, double* cov, unsigned flags, void* stream) {
  scaml::PosteriorJointParams p = grad_joint_block(Xq, Xa, X, theta, Linv, alpha, y_mean, y_std, n_points, VA, VQ, T, N, Mq, Ma, q, D, mu, var, cov, flags);
  if (const int rc = grad_joint_check(p, Mq, kind, flags)) return rc;
  if (T == 0 || Mq == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return grad_joint_launch(*m, p, Mq, kind, stream);
}

// ---- (4) gradient of the marginal log-likelihood ------------------------------------------------
long long scaml_mll_backward_workspace_doubles(int T, int N, int D) {
  const long long nb = (N + 15) / 16;
  return (long long)T * N * N + (long long)T * (nb * (nb + 1) / 2) * (D + 2);
}

int scaml_mll_backward_f64(const double* X, const double* theta, const double* L, const double* Linv_diag,
                           const double* alpha, const int32_t* n_points, int T, int N, int D, int kind,
                           double* workspace, double* partials_out, void* stream) {
  if (T < 0 || N < 1 || D < 1) return SCAML_E_BADARG;
  if (!X || !theta || !L || !Linv_diag || !alpha || !workspace) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (N > scaml_posterior_max_n()) return SCAML_E_TOOLARGE;
  const size_t lds_tiles = scaml::mll_grad_lds_doubles(D) * sizeof(double);   // staged points of four waves (D <= 76)
  if (lds_tiles > kLdsLimit - 2048) return SCAML_E_TOOLARGE;
  if (T == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  double* Linv = workspace;
  double* partials = partials_out ? partials_out : workspace + (size_t)T * N * N;
  const bool aligned16 = ((uintptr_t)L % 16) == 0 && ((uintptr_t)Linv_diag % 16) == 0;
  const scaml::GradPlan plan =
      scaml::grad_plan(T, N, D, num_cus(*m), g_dev.grad_path.load(kRelaxed), g_dev.no_grad_split, n_points != nullptr, aligned16);
  const size_t lds = plan.lds_doubles * sizeof(double);
  if (plan.single) {
    scaml::MllGradFusedParams p{X, theta, L, Linv_diag, alpha, n_points, partials, T, N, D};
    hipFunction_t fn = plan.split == 1 ? m->mllgrad_fused[plan.sc][kind][plan.dma] : m->mllgrad_split[plan.sc - 2][kind][plan.split == 2 ? 0 : 1];
    return launch(fn, dim3(plan.grid_x, plan.grid_y), plan.block, lds, stream, "gp_mll_grad_fused", p);
  }
  const int rc = launch_linv(*m, L, Linv_diag, n_points, T, N, Linv, stream);   // (dense: the 2 x 2 super-tiles of the tile kernel read zero blocks above the diagonal)
  if (rc != SCAML_OK) return rc;
  scaml::MllGradParams p{X, theta, alpha, Linv, n_points, partials, T, N, D};
  return launch(m->mllgrad[kind], dim3(plan.grid_x), plan.block, lds, stream, "gp_mll_grad", p);
}

// ---- target GP: assemble the joint prior block / finish the posterior (a10) -----------------------------------------
static int target_assemble_check(const scaml::TargetAssembleParams& p, int kind) {
  if (p.n < 1 || p.M < 0 || p.D < 1) return SCAML_E_BADARG;
  if (!p.cov_s || !p.mean_s || !p.var_s || !p.Xall || !p.theta || !p.train_targets || !p.Knn || !p.resid) return SCAML_E_BADARG;
  if (p.M > 0 && (!p.Knq || !p.mean_q || !p.var_q)) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (!(p.s_all > 0.0)) return SCAML_E_BADARG;
  return SCAML_OK;
}
static int target_assemble_launch(Module& m, scaml::TargetAssembleParams& p, int kind, void* stream) {   // a checked block
  long long elems = (long long)p.n * (p.n + p.M);
  if (elems < p.M) elems = p.M;
  return launch(m.tgt_assemble[kind], dim3((unsigned)((elems + 255) / 256)), 256, 0, stream, "target_assemble", p);
}

int scaml_target_assemble_f64(const double* cov_s, const double* mean_s, const double* var_s, const double* Xall,
                              const double* theta, const double* train_targets, double m_all, double s_all, int n, int M, int D,
                              int kind, double* Knn, double* resid, double* Knq, double* mean_q, double* var_q, void* stream) {
  scaml::TargetAssembleParams p{cov_s, mean_s, var_s, Xall, theta, train_targets, m_all, s_all, Knn, resid, Knq, mean_q, var_q, n, M, D};
  if (const int rc = target_assemble_check(p, kind)) return rc;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return target_assemble_launch(*m, p, kind, stream);
}

int scaml_target_finish_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                            double m_all, double s_all, double noise_add, const int32_t* info, int n, int M, double* mu, double* var,
                            void* stream) {
  if (n < 1 || M < 0) return SCAML_E_BADARG;
  if (M == 0) return SCAML_OK;
  if (!Knq || !Z || !alpha || !mean_q || !var_q || !mu || !var) return SCAML_E_BADARG;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  void* args[] = {(void*)&Knq, (void*)&Z, (void*)&alpha, (void*)&mean_q, (void*)&var_q, (void*)&m_all, (void*)&s_all, (void*)&noise_add,
                  (void*)&info, (void*)&n, (void*)&M, (void*)&mu, (void*)&var};
  return launch_args(m->tgt_finish, dim3((unsigned)((M + 127) / 128)), 128, stream, "target_finish", args);
}

int scaml_target_posterior_grad_f64(const double* cov_g, const double* mu_g, const double* var_g, const double* Xt, const double* Xq,
                                    const double* theta, const double* alpha, const double* Z, double s_all, const int32_t* info, int n,
                                    int Mq, int D, int kind, double* dmu, double* dvar, void* stream) {
  if (n < 0 || Mq < 0 || D < 1) return SCAML_E_BADARG;
  if (!mu_g || !var_g || !Xq || !theta || !dmu || !dvar) return SCAML_E_BADARG;
  if (n > 0 && (!cov_g || !Xt || !alpha || !Z)) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (!(s_all > 0.0)) return SCAML_E_BADARG;
  if (Mq == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  void* args[] = {(void*)&cov_g, (void*)&mu_g, (void*)&var_g, (void*)&Xt, (void*)&Xq, (void*)&theta, (void*)&alpha, (void*)&Z, (void*)&s_all,
                  (void*)&info, (void*)&n, (void*)&Mq, (void*)&D, (void*)&dmu, (void*)&dvar};
  if (D > 15) return SCAML_E_TOOLARGE;
  return launch_args(m->tgt_grad[kind], dim3((unsigned)Mq), 64, stream, "target_grad", args);   // one wave per query point
}

// ---- (7f) fantasy model: acquisition value (+ input gradient) averaged over the fantasies (csrc/gp_fantasy.hip) ---------------
int scaml_target_fantasy_acqf_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                  double m_all, double s_all, double noise_add, const int32_t* info, int acqf, double acqf_param,
                                  const double* cov_g, const double* mu_g, const double* var_g, const double* Xt, const double* Xq,
                                  const double* theta, int n, int M, int F, int D, int kind, double* value, double* grad, void* stream) {
  if (n < 1 || M < 0 || F < 1) return SCAML_E_BADARG;
  if (!Knq || !Z || !alpha || !mean_q || !var_q || !value) return SCAML_E_BADARG;
  if (!scaml::sa_acqf_valid(acqf)) return SCAML_E_BADARG;
  if (!(s_all > 0.0)) return SCAML_E_BADARG;
  if (grad) {
    if (D < 1 || !cov_g || !mu_g || !var_g || !Xt || !Xq || !theta) return SCAML_E_BADARG;
    if (!valid_kind(kind)) return SCAML_E_BADARG;
  }
  if (F > scaml::FANTASY_MAX_F || n > scaml::FANTASY_MAX_N) return SCAML_E_TOOLARGE;
  if (grad && (n > scaml::FANTASY_GRAD_MAX_N || D > scaml::FANTASY_GRAD_MAX_D)) return SCAML_E_TOOLARGE;
  if (M == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::FantasyAcqfParams p{Knq, Z, alpha, mean_q, var_q, m_all, s_all, noise_add, info, acqf_param, cov_g, mu_g, var_g, Xt, Xq, theta,
                             value, grad, n, M, F, grad ? D : 0, acqf, 0};
  // one wave per query point
  return launch(grad ? m->tgt_fantasy_grad[kind] : m->tgt_fantasy, dim3((unsigned)M), 64, 0, stream, "target_fantasy_acqf", p);
}

// ---- (7p) joint q-point Monte-Carlo acquisition, qEI / qUCB, and its input gradient: a workgroup per batch (csrc/gp_qacqf.hip) ----
static int qacqf_check(const scaml::QAcqfParams& p) {
  if (p.n < 1 || p.Mq < 0 || p.q < 1 || p.S < 1 || p.D < 1 || p.Mq % p.q != 0) return SCAML_E_BADARG;
  if (!p.Knq || !p.Z || !p.alpha || !p.mean_q || !p.var_q || !p.cov_g || !p.mu_g || !p.var_g || !p.Xt || !p.Xq || !p.theta || !p.base_samples || !p.value)
    return SCAML_E_BADARG;
  if (!scaml::qa_acqf_valid(p.acqf)) return SCAML_E_BADARG;   // (a joint LogEI is not defined: 17 and 0x10 are refused like 2)
  if (!valid_kind(p.kind)) return SCAML_E_BADARG;
  if (!(p.s_all > 0.0)) return SCAML_E_BADARG;
  if (p.q > scaml::QACQF_MAX_Q || p.S > scaml::QACQF_MAX_SAMPLES || p.n + p.q > scaml::QACQF_MAX_ROWS || p.D > scaml::QACQF_MAX_D) return SCAML_E_TOOLARGE;
  if (scaml::qacqf_plan(p.Mq / p.q, p.n, p.q, p.S).lds_doubles * sizeof(double) > kLdsLimit) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
static int qacqf_launch(Module& m, scaml::QAcqfParams& p, void* stream) {   // a checked, non-empty block
  const scaml::QAcqfPlan plan = scaml::qacqf_plan(p.Mq / p.q, p.n, p.q, p.S);
  return launch(m.tgt_qacqf, dim3(plan.grid), plan.block, plan.lds_doubles * sizeof(double), stream, "target_qacqf", p);
}

int scaml_target_qacqf_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q, double m_all,
                           double s_all, const int32_t* info, const double* cov_g, const double* mu_g, const double* var_g, const double* Xt,
                           const double* Xq, const double* theta, const double* base_samples, int acqf, double acqf_param, int n, int Mq, int q,
                           int S, int D, int kind, double* value, double* grad, double* jitter_used, int32_t* info_out, void* stream) {
  scaml::QAcqfParams p{Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_g, mu_g, var_g, Xt, Xq, theta, base_samples, acqf_param,
                       value, grad, jitter_used, info_out, n, Mq, q, S, D, kind, acqf, 0};
  if (const int rc = qacqf_check(p)) return rc;
  if (Mq == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return qacqf_launch(*m, p, stream);
}

// ---- (7q) (7p) with p evaluations pending behind every batch: the same workgroup per batch, the joint at q + p ----
static int qacqf_pending_check(const scaml::QAcqfPendingParams& pp) {
  const scaml::QAcqfParams& a = pp.a;
  const int p = pp.pe.p;
  if (a.n < 1 || a.Mq < 0 || a.q < 1 || p < 0 || a.S < 1 || a.D < 1 || a.Mq % a.q != 0) return SCAML_E_BADARG;
  if (!a.Knq || !a.Z || !a.alpha || !a.mean_q || !a.var_q || !a.cov_g || !a.mu_g || !a.var_g || !a.Xt || !a.Xq || !a.theta || !a.base_samples || !a.value)
    return SCAML_E_BADARG;
  if (p > 0 && (!pp.pe.Xp || !pp.pe.Zp || !pp.pe.mu_p || !pp.pe.Sigma_pp)) return SCAML_E_BADARG;
  if (!scaml::qa_acqf_valid(a.acqf)) return SCAML_E_BADARG;
  if (!valid_kind(a.kind)) return SCAML_E_BADARG;
  if (!(a.s_all > 0.0)) return SCAML_E_BADARG;
  if (a.q > scaml::QACQF_MAX_Q || p > scaml::QACQF_MAX_Q || a.q + p > scaml::QACQF_MAX_Q || a.S > scaml::QACQF_MAX_SAMPLES ||
      a.n > scaml::QACQF_MAX_ROWS || a.n + p + a.q > scaml::QACQF_MAX_ROWS || a.D > scaml::QACQF_MAX_D)
    return SCAML_E_TOOLARGE;
  if (scaml::qacqf_pending_plan(a.Mq / a.q, a.n, a.q, p, a.S).lds_doubles * sizeof(double) > kLdsLimit) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
static int qacqf_pending_launch(Module& m, scaml::QAcqfPendingParams& pp, void* stream) {   // a checked, non-empty block
  const scaml::QAcqfPlan plan = scaml::qacqf_pending_plan(pp.a.Mq / pp.a.q, pp.a.n, pp.a.q, pp.pe.p, pp.a.S);
  return launch(m.tgt_qacqf_pending, dim3(plan.grid), plan.block, plan.lds_doubles * sizeof(double), stream, "target_qacqf_pending", pp);
}

int scaml_target_qacqf_pending_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                   double m_all, double s_all, const int32_t* info, const double* cov_g, const double* mu_g,
                                   const double* var_g, const double* Xt, const double* Xq, const double* theta, const double* base_samples,
                                   const double* Xp, const double* Zp, const double* mu_p, const double* Sigma_pp, int acqf,
                                   double acqf_param, int n, int Mq, int q, int p, int S, int D, int kind, double* value, double* grad,
                                   double* jitter_used, int32_t* info_out, void* stream) {
  scaml::QAcqfPendingParams pp{{Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_g, mu_g, var_g, Xt, Xq, theta, base_samples, acqf_param,
                                value, grad, jitter_used, info_out, n, Mq, q, S, D, kind, acqf, 0},
                               {Xp, Zp, mu_p, Sigma_pp, p, 0}};
  if (const int rc = qacqf_pending_check(pp)) return rc;
  if (Mq == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return qacqf_pending_launch(*m, pp, stream);
}

// ---- (5h) the joint source pass in value layout: 16 packed query points per strip, the mates' covariances from the strip's Gram tile ----
int scaml_qacqf_value_columns(int B, int q) {
  if (B < 0 || q < 1 || q > scaml::QACQF_MAX_Q || B > (1 << 26)) return -1;
  return scaml::qav_columns(B, q);
}

int scaml_posterior_linv_cov_joint_f64(const double* Xq, const double* Xa, const double* X, const double* theta, const double* Linv,
                                       const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                       const double* VA, int T, int N, int Mp, int Ma, int B, int q, int D, int kind, double* mu, double* var,
                                       double* cov, unsigned flags, void* stream) {
  if (T < 0 || N < 1 || Mp < 0 || Ma < 1 || B < 0 || q < 1 || D < 1) return SCAML_E_BADARG;
  if (!Xq || !Xa || !X || !theta || !Linv || !alpha || !VA || !cov) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (flags & SCAML_POST_MEAN_ONLY) return SCAML_E_BADARG;
  if (q <= scaml::QACQF_MAX_Q && B <= (1 << 26) && Mp != scaml::qav_columns(B, q)) return SCAML_E_BADARG;   // (the packing is defined up to q = 8)
  if (q > scaml::QACQF_MAX_Q || B > (1 << 26)) return SCAML_E_TOOLARGE;
  if (N > scaml_posterior_max_n()) return SCAML_E_TOOLARGE;
  if (Ma > scaml::QACQF_MAX_ROWS || Ma + q > scaml::QACQF_MAX_ROWS || Ma + q > N) return SCAML_E_TOOLARGE;   // six 16-row strips of leading points, staged in the N x 16 LDS strip
  const scaml::PosteriorJointValuePlan plan = scaml::posterior_jointv_plan(T, N, D, Mp);
  const size_t lds = plan.lds_doubles * sizeof(double);
  if (lds > kLdsLimit) return SCAML_E_TOOLARGE;
  if (T == 0 || B == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::PosteriorJointValueParams p{{Xq, X, theta, Linv, nullptr, alpha, y_mean, y_std, n_points, mu, var, nullptr, T, N, Mp, D, 0,
                                      (flags & SCAML_POST_XQ_PER_TASK) ? 1 : 0, 0, VA, cov, Ma, 0, Xa},
                                     {q, B}};
  return launch(m->post_linv_cov_joint[kind], dim3(plan.grid), plan.block, lds, stream, "gp_posterior_linv_cov_joint", p);
}

// ---- (7r) (7p) / (7q) value only, from the value layout of (5h): a workgroup per batch (csrc/gp_qacqf_value.hip) ----
int scaml_target_qacqf_value_f64(const double* Knq, const double* Z, const double* alpha, const double* mean_q, const double* var_q,
                                 double m_all, double s_all, const int32_t* info, const double* cov_s, const double* Xq, const double* theta,
                                 const double* base_samples, const double* Xp, const double* Zp, const double* mu_p, const double* Sigma_pp,
                                 int acqf, double acqf_param, int n, int Mp, int B, int q, int p, int S, int D, int kind, double* value,
                                 double* jitter_used, int32_t* info_out, void* stream) {
  if (n < 1 || Mp < 0 || B < 0 || q < 1 || p < 0 || S < 1 || D < 1) return SCAML_E_BADARG;
  if (!Knq || !Z || !alpha || !mean_q || !var_q || !cov_s || !Xq || !theta || !base_samples || !value) return SCAML_E_BADARG;
  if (p > 0 && (!Xp || !Zp || !mu_p || !Sigma_pp)) return SCAML_E_BADARG;
  if (!scaml::qa_acqf_valid(acqf)) return SCAML_E_BADARG;   // (a joint LogEI is not defined)
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (!(s_all > 0.0)) return SCAML_E_BADARG;
  if (q <= scaml::QACQF_MAX_Q && B <= (1 << 26) && Mp != scaml::qav_columns(B, q)) return SCAML_E_BADARG;
  if (q > scaml::QACQF_MAX_Q || p > scaml::QACQF_MAX_Q || q + p > scaml::QACQF_MAX_Q || S > scaml::QACQF_MAX_SAMPLES || B > (1 << 26) ||
      n > scaml::QACQF_MAX_ROWS || n + p + q > scaml::QACQF_MAX_ROWS || D > scaml::QACQF_MAX_D)
    return SCAML_E_TOOLARGE;
  const scaml::QAcqfPlan plan = scaml::qacqf_value_plan(B, n, q, p, S);
  if (plan.lds_doubles * sizeof(double) > kLdsLimit) return SCAML_E_TOOLARGE;
  if (B == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::QAcqfPendingParams pp{{Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_s, nullptr, nullptr, nullptr, Xq, theta, base_samples,
                                acqf_param, value, nullptr, jitter_used, info_out, n, Mp, q, S, D, kind, acqf, 0},
                               {p > 0 ? Xp : nullptr, p > 0 ? Zp : nullptr, p > 0 ? mu_p : nullptr, p > 0 ? Sigma_pp : nullptr, p, 0}};
  return launch(m->tgt_qacqf_value, dim3(plan.grid), plan.block, plan.lds_doubles * sizeof(double), stream, "target_qacqf_value", pp);
}

// ---- (7o) the acquisition value and chain-rule factors of M given posteriors, elementwise (csrc/gp_acqf_transform.hip) ----------
int scaml_acqf_transform_f64(const double* mu, const double* var, double acqf_param, int M, int acqf, double* A, double* Amu, double* Av,
                             void* stream) {
  if (M < 0 || !scaml::sa_acqf_valid(acqf)) return SCAML_E_BADARG;
  if (M == 0) return SCAML_OK;
  if (!mu || !var || !A) return SCAML_E_BADARG;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  void* args[] = {(void*)&mu, (void*)&var, (void*)&acqf_param, (void*)&M, (void*)&acqf, (void*)&A, (void*)&Amu, (void*)&Av};
  return launch_args(m->acqf_transform, dim3(((unsigned)M + 255u) / 256u), 256, stream, "acqf_transform", args);   // one thread per element (unsigned: no overflow near INT_MAX)
}

// ---- (5e) the GRAD pass with the query points divided among groups, (5f) the same pass in VALUE mode; (7g), (7i) the batched target
// acquisition behind them ----
// Every entry point fills its kernel's argument block once -- the block names each pointer --; one check and one launch per block take
// it from there.  (7h) builds both blocks once, checks them once and launches them per round.
// The order of the checks that can be observed: every SCAML_E_BADARG check comes before every SCAML_E_TOOLARGE check, and an empty
// shape is SCAML_OK only after both.
namespace {
int sat_int(long long v) { return v > INT32_MAX ? INT32_MAX : (v < INT32_MIN ? INT32_MIN : (int)v); }

// The grouped pass's block.  `value`: (5f), Mq candidates in strips of 16, `group` has one entry per strip; else (5e), 16 columns per
// query point.  Either way base.M is the row width of mu / var / cov (saturated: grouped_check refuses what does not fit) and base.M / 16
// the number of strips.  task_base NULL: every group reads the same source tasks; with the table, T = task slots per group.
scaml::PosteriorGroupedParams grouped_block(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                            const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                            const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points, int T,
                                            int N, int Mq, int G, int Ma_max, int D, double* mu, double* var, double* cov,
                                            const int32_t* task_base, int Tsrc, bool value) {
  scaml::PosteriorGroupedParams p{};
  p.base = scaml::PosteriorParams{Xq, X, theta, Linv, nullptr, alpha, y_mean, y_std, n_points, mu, var, nullptr, T, N,
                                  sat_int((long long)Mq * (value ? 1 : 16)), D, 0, 0, 0, nullptr, cov, Ma_max, 0, nullptr};
  p.ga = scaml::PosteriorGroupArgs{group, n_points_a, VA_tab, Xa, G, 0, task_base, Tsrc, 0};
  return p;
}
// `own`: the entry point takes task_base / Tsrc.  SCAML_OK: the shapes are within the kernel's limits (they may be empty).
int grouped_check(const scaml::PosteriorGroupedParams& p, int kind, bool value, bool own) {
  const scaml::PosteriorParams& b = p.base;
  if (b.T < 0 || b.N < 1 || b.M < 0 || p.ga.G < 0 || b.Ma < 1 || b.D < 1) return SCAML_E_BADARG;
  if (value && (b.M & 15)) return SCAML_E_BADARG;   // (5f): whole strips of 16 candidates
  if (!b.Xq || !p.ga.group || !p.ga.Xa || !p.ga.n_a || !p.ga.VA_tab || !b.X || !b.theta || !b.L || !b.alpha || !b.mu || !b.var || !b.cov)
    return SCAML_E_BADARG;
  if (own && (!p.ga.task_base || p.ga.Tsrc < 1)) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (b.D > 15 || b.Ma > 96 || b.Ma > b.N || b.N > scaml_posterior_max_n() || (value ? b.M : b.M / 16) > (1 << 26)) return SCAML_E_TOOLARGE;
  if (scaml::posterior_linv_lds_doubles(b.N, b.D) * sizeof(double) > kLdsLimit) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
// `ordered`: the GRAD pass whose mu / var do not depend on the order in which the waves finish (DET of csrc/gp_posterior.hip)
int grouped_launch(Module& m, scaml::PosteriorGroupedParams& p, int kind, bool value, void* stream, bool ordered = false) {   // a checked, non-empty block
  const size_t lds = scaml::posterior_linv_lds_doubles(p.base.N, p.base.D) * sizeof(double);
  const unsigned blocks = (unsigned)(((p.base.T + 7) / 8) * 8) * (unsigned)(p.base.M / 16);   // XCD-aware (task, strip) map inside the kernel
  const bool own = p.ga.task_base != nullptr;
  hipFunction_t fn = value ? (own ? m.post_linv_grouped_val_own[kind] : m.post_linv_grouped_val[kind])
                           : (own ? m.post_linv_grouped_own[kind] : m.post_linv_grouped[kind]);
  if (ordered && !value) fn = own ? m.post_linv_grouped_det_own[kind] : m.post_linv_grouped_det[kind];
  return launch(fn, dim3(blocks), 512, lds, stream, own ? "gp_posterior_linv_grouped_own" : "gp_posterior_linv_grouped", p);
}
int grouped_run(scaml::PosteriorGroupedParams p, int kind, bool value, bool own, void* stream) {
  if (const int rc = grouped_check(p, kind, value, own)) return rc;
  // scaml_debug_grouped_ordered_sums: (5e) / (5e') through the instance with ordered sums, under (7l)'s LDS limit (its static shares)
  const bool ordered = !value && g_dev.grouped_ordered.load(kRelaxed) == 1;
  if (ordered && scaml::posterior_linv_lds_doubles(p.base.N, p.base.D) * sizeof(double) > kLdsLimit - kOrderedSumsLds) return SCAML_E_TOOLARGE;
  if (p.base.T == 0 || p.base.M == 0 || p.ga.G == 0) return SCAML_OK;
  Module* m = ready();
  return m ? grouped_launch(*m, p, kind, value, stream, ordered) : SCAML_E_LAUNCH;
}

// The studies' acquisition block (csrc/gp_studies_acqf.h).  `strips`: (7i), the value layout, a workgroup per strip of 16 candidates
// (sa_block<16>); else (7g), a workgroup per query point (sa_block<1>).
size_t acqf_lds_bytes(int n_max, bool strips) {
  return (strips ? scaml::sa_lds_doubles<16>(n_max) : scaml::sa_lds_doubles<1>(n_max)) * sizeof(double);
}
int acqf_check(const scaml::StudiesAcqfParams& p, bool strips) {
  if (p.Mq < 0 || (strips && (p.Mq & 15)) || p.G < 0 || p.n_max < 1 || p.T < 1 || p.D < 1) return SCAML_E_BADARG;
  if (!p.mu || !p.var || !p.cov || !p.group || !p.Xq || !p.w || !p.active || !p.Xt || !p.theta || !p.L || !p.Linv_diag || !p.alpha ||
      !p.n_points || !p.m_all || !p.s_all || !p.info || !p.acqf_param || !p.value)
    return SCAML_E_BADARG;
  if (!valid_kind(p.kind) || !scaml::sa_acqf_valid(p.acqf)) return SCAML_E_BADARG;
  if (p.n_max > scaml::STUDIES_ACQF_MAX_N || p.D > scaml::STUDIES_ACQF_MAX_D || p.Mq > (1 << 26)) return SCAML_E_TOOLARGE;
  if (acqf_lds_bytes(p.n_max, strips) > kLdsLimit) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
static_assert(scaml::sa_lds_doubles<16>(scaml::STUDIES_ACQF_MAX_N) * sizeof(double) <= kLdsLimit, "a strip at n_max = 96 fits the LDS");
int acqf_launch(Module& m, scaml::StudiesAcqfParams& p, bool strips, void* stream) {   // a checked, non-empty block
  const size_t lds = acqf_lds_bytes(p.n_max, strips);
  if (strips) return launch(m.tgt_score_batched, dim3((unsigned)(p.Mq / 16)), scaml::STUDIES_SCORE_THREADS, lds, stream, "target_score_batched", p);
  return launch(m.tgt_acqf_batched, dim3((unsigned)p.Mq), scaml::STUDIES_ACQF_THREADS, lds, stream, "target_acqf_batched", p);
}
int acqf_run(scaml::StudiesAcqfParams p, bool strips, void* stream) {
  if (const int rc = acqf_check(p, strips)) return rc;
  if (p.Mq == 0 || p.G == 0) return SCAML_OK;
  Module* m = ready();
  return m ? acqf_launch(*m, p, strips, stream) : SCAML_E_LAUNCH;
}

// The same block for studies with pending evaluations (7k): (7g)'s arguments with alpha_f (handed to the base block's check as its
// `alpha`), n_fant and F_max.
scaml::StudiesFantasyParams fantasy_block(const scaml::StudiesAcqfParams& base, const double* alpha_f, const int32_t* n_fant, int F_max) {
  scaml::StudiesFantasyParams p{};
  static_cast<scaml::StudiesAcqfParams&>(p) = base;
  p.alpha = alpha_f;
  p.alpha_f = alpha_f;
  p.n_fant = n_fant;
  p.F_max = F_max;
  return p;
}
size_t fantasy_lds_bytes(int n_max, int F_max, bool strips) {
  return (strips ? scaml::sa_fantasy_lds_doubles<16>(n_max, F_max) : scaml::sa_fantasy_lds_doubles<1>(n_max, F_max)) * sizeof(double);
}
int fantasy_check(const scaml::StudiesFantasyParams& p, bool strips) {
  const int rb = acqf_check(p, strips);
  if (rb == SCAML_E_BADARG || p.F_max < 1 || !p.alpha_f || !p.n_fant) return SCAML_E_BADARG;
  if (rb != SCAML_OK || p.F_max > scaml::STUDIES_FANTASY_MAX_F) return SCAML_E_TOOLARGE;
  if (fantasy_lds_bytes(p.n_max, p.F_max, strips) > kLdsLimit) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
static_assert(scaml::sa_fantasy_lds_doubles<16>(scaml::STUDIES_ACQF_MAX_N, scaml::STUDIES_FANTASY_MAX_F) * sizeof(double) <= kLdsLimit &&
                  scaml::sa_fantasy_lds_doubles<1>(scaml::STUDIES_ACQF_MAX_N, scaml::STUDIES_FANTASY_MAX_F) * sizeof(double) <= kLdsLimit,
              "n_max = 96 with F_max = 64 fits the LDS in both layouts");
int fantasy_launch(Module& m, scaml::StudiesFantasyParams& p, bool strips, void* stream) {   // a checked, non-empty block
  const size_t lds = fantasy_lds_bytes(p.n_max, p.F_max, strips);
  if (strips)
    return launch(m.tgt_fantasy_score_batched, dim3((unsigned)(p.Mq / 16)), scaml::STUDIES_ACQF_THREADS, lds, stream, "target_fantasy_score_batched", p);
  return launch(m.tgt_fantasy_acqf_batched, dim3((unsigned)p.Mq), scaml::STUDIES_ACQF_THREADS, lds, stream, "target_fantasy_acqf_batched", p);
}
int fantasy_run(scaml::StudiesFantasyParams p, bool strips, void* stream) {
  if (const int rc = fantasy_check(p, strips)) return rc;
  if (p.Mq == 0 || p.G == 0) return SCAML_OK;
  Module* m = ready();
  return m ? fantasy_launch(*m, p, strips, stream) : SCAML_E_LAUNCH;
}
}  // namespace

int scaml_posterior_linv_grad_grouped_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                          const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                          const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points, int T,
                                          int N, int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var, double* cov,
                                          void* stream) {
  return grouped_run(grouped_block(Xq, group, Xa, n_points_a, VA_tab, X, theta, Linv, alpha, y_mean, y_std, n_points, T, N, Mq, G, Ma_max, D, mu,
                                   var, cov, nullptr, 0, false),
                     kind, false, false, stream);
}
int scaml_posterior_linv_grad_grouped_own_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                              const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                              const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points,
                                              int T, int N, int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var,
                                              double* cov, const int32_t* task_base, int Tsrc, void* stream) {
  return grouped_run(grouped_block(Xq, group, Xa, n_points_a, VA_tab, X, theta, Linv, alpha, y_mean, y_std, n_points, T, N, Mq, G, Ma_max, D, mu,
                                   var, cov, task_base, Tsrc, false),
                     kind, false, true, stream);
}

int scaml_target_acqf_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                  const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                  const double* Linv_diag, const double* alpha, const int32_t* n_points, const double* m_all,
                                  const double* s_all, const int32_t* info, const double* acqf_param, int Mq, int G, int n_max, int T,
                                  int D, int kind, int acqf, double* value, double* grad, double* mu_out, double* var_out, void* stream) {
  return acqf_run(scaml::StudiesAcqfParams{mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info,
                                           acqf_param, value, grad, mu_out, var_out, Mq, G, n_max, T, D, kind, acqf, 0},
                  false, stream);
}

// ---- (5f), (5f') the grouped pass in VALUE mode: a strip is 16 different candidates of one group, `group` has one entry per strip ----
int scaml_posterior_linv_grouped_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                     const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                     const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points, int T, int N,
                                     int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var, double* cov, void* stream) {
  return grouped_run(grouped_block(Xq, group, Xa, n_points_a, VA_tab, X, theta, Linv, alpha, y_mean, y_std, n_points, T, N, Mq, G, Ma_max, D, mu,
                                   var, cov, nullptr, 0, true),
                     kind, true, false, stream);
}
int scaml_posterior_linv_grouped_own_f64(const double* Xq, const int32_t* group, const double* Xa, const int32_t* n_points_a,
                                         const double* const* VA_tab, const double* X, const double* theta, const double* Linv,
                                         const double* alpha, const double* y_mean, const double* y_std, const int32_t* n_points, int T,
                                         int N, int Mq, int G, int Ma_max, int D, int kind, double* mu, double* var, double* cov,
                                         const int32_t* task_base, int Tsrc, void* stream) {
  return grouped_run(grouped_block(Xq, group, Xa, n_points_a, VA_tab, X, theta, Linv, alpha, y_mean, y_std, n_points, T, N, Mq, G, Ma_max, D, mu,
                                   var, cov, task_base, Tsrc, true),
                     kind, true, true, stream);
}

// ---- (7i) the acquisition value of a table of candidates of many studies, a workgroup per strip of 16 (csrc/gp_studies_score.hip) ----
int scaml_target_score_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                   const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                   const double* Linv_diag, const double* alpha, const int32_t* n_points, const double* m_all,
                                   const double* s_all, const int32_t* info, const double* acqf_param, int Mq, int G, int n_max, int T,
                                   int D, int kind, int acqf, double* value, double* mu_out, double* var_out, void* stream) {
  return acqf_run(scaml::StudiesAcqfParams{mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info,
                                           acqf_param, value, nullptr, mu_out, var_out, Mq, G, n_max, T, D, kind, acqf, 0},
                  true, stream);
}

// ---- (7k) (7g) / (7i) for studies of which some hold pending evaluations: UCB / EI averaged over a study's fantasies
// (csrc/gp_studies_fantasy.hip) ----
int scaml_target_fantasy_acqf_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                          const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                          const double* Linv_diag, const double* alpha_f, const int32_t* n_fant, const int32_t* n_points,
                                          const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int Mq,
                                          int G, int n_max, int F_max, int T, int D, int kind, int acqf, double* value, double* grad,
                                          void* stream) {
  return fantasy_run(fantasy_block(scaml::StudiesAcqfParams{mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, nullptr, n_points, m_all,
                                                            s_all, info, acqf_param, value, grad, nullptr, nullptr, Mq, G, n_max, T, D, kind, acqf, 0},
                                   alpha_f, n_fant, F_max),
                     false, stream);
}
int scaml_target_fantasy_score_batched_f64(const double* mu, const double* var, const double* cov, const int32_t* group, const double* Xq,
                                           const double* w, const uint8_t* active, const double* Xt, const double* theta, const double* L,
                                           const double* Linv_diag, const double* alpha_f, const int32_t* n_fant, const int32_t* n_points,
                                           const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int Mq,
                                           int G, int n_max, int F_max, int T, int D, int kind, int acqf, double* value, void* stream) {
  return fantasy_run(fantasy_block(scaml::StudiesAcqfParams{mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, nullptr, n_points, m_all,
                                                            s_all, info, acqf_param, value, nullptr, nullptr, nullptr, Mq, G, n_max, T, D, kind, acqf, 0},
                                   alpha_f, n_fant, F_max),
                     true, stream);
}

// ---- (7j) the training blocks Knn / resid of G studies in one launch (csrc/gp_studies_score.hip); (2) factors them together ----
int scaml_target_train_block_batched_f64(const double* means_t, const double* covs_packed, const double* X, const double* y,
                                         const int32_t* n_points, const double* m_all, const double* s_all, const double* w,
                                         const uint8_t* active, const double* theta, int G, int n_max, int T, int D, int kind, double* Knn,
                                         double* resid, void* stream) {
  if (G < 0 || n_max < 1 || T < 1 || D < 1) return SCAML_E_BADARG;
  if (!means_t || !covs_packed || !X || !y || !n_points || !m_all || !s_all || !w || !active || !theta || !Knn || !resid) return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (n_max > scaml_fit_max_n()) return SCAML_E_TOOLARGE;   // what (2) factors
  if (G == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::TrainBlockParams p{means_t, covs_packed, X, y, n_points, m_all, s_all, w, active, theta, Knn, resid, G, n_max, T, D};
  return launch(m->tgt_train_block[kind], dim3((unsigned)G), 256, 0, stream, "target_train_block_batched", p);
}

// ---- (7m), (7n) the fantasy set-up of G studies with pending evaluations (csrc/gp_studies_condition.hip); (2) factors the blocks between them ----
static_assert(scaml::studies_condition_block_plan(1, scaml::STUDIES_ACQF_MAX_N, scaml::STUDIES_ACQF_MAX_D).lds_doubles * sizeof(double) <= kLdsLimit &&
                  scaml::studies_fantasy_condition_plan(1, scaml::STUDIES_ACQF_MAX_N, scaml::STUDIES_FANTASY_MAX_F).lds_doubles * sizeof(double) <= kLdsLimit,
              "n_max = 96 with D = 15 and with F_max = 64 fits the LDS");
int scaml_studies_condition_block_f64(const double* mu, const double* cov, const int32_t* strip_base, const double* w, const uint8_t* active,
                                      const double* Xt, const double* theta, const double* y, const int32_t* n_points, const int32_t* n_obs,
                                      const double* m_all, const double* s_all, int Mq, int G, int n_max, int T, int D, int kind, double* Knn,
                                      double* resid, double* mean_p, void* stream) {
  if (Mq < 0 || (Mq & 15) || G < 0 || n_max < 1 || T < 1 || D < 1) return SCAML_E_BADARG;
  if (!mu || !cov || !strip_base || !w || !active || !Xt || !theta || !y || !n_points || !n_obs || !m_all || !s_all || !Knn || !resid || !mean_p)
    return SCAML_E_BADARG;
  if (!valid_kind(kind)) return SCAML_E_BADARG;
  if (n_max > scaml::STUDIES_ACQF_MAX_N || D > scaml::STUDIES_ACQF_MAX_D || Mq > (1 << 26)) return SCAML_E_TOOLARGE;
  const scaml::StudiesConditionPlan plan = scaml::studies_condition_block_plan(G, n_max, D);
  if (plan.lds_doubles * sizeof(double) > kLdsLimit) return SCAML_E_TOOLARGE;
  if (G == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::StudiesConditionBlockParams p{mu, cov, strip_base, w, active, Xt, theta, y, n_points, n_obs, m_all, s_all, Knn, resid, mean_p,
                                       Mq, G, n_max, T, D, kind};
  return launch(m->cond_block, dim3(plan.grid), plan.block, plan.lds_doubles * sizeof(double), stream, "studies_condition_block", p);
}

int scaml_studies_fantasy_condition_f64(const double* L, const double* resid, const double* mean_p, const int32_t* n_points, const int32_t* n_obs,
                                        const int32_t* info, const double* eps, const int32_t* n_fant, const double* m_all, const double* s_all,
                                        int G, int n_max, int p_max, int F_max, double* alpha_f, double* y_fant, double* mu_p, void* stream) {
  if (G < 0 || n_max < 1 || p_max < 1 || F_max < 1) return SCAML_E_BADARG;
  if (!L || !resid || !mean_p || !n_points || !n_obs || !info || !eps || !n_fant || !m_all || !s_all || !alpha_f || !y_fant || !mu_p)
    return SCAML_E_BADARG;
  if (n_max > scaml::STUDIES_ACQF_MAX_N || p_max > scaml::STUDIES_ACQF_MAX_N || F_max > scaml::STUDIES_FANTASY_MAX_F) return SCAML_E_TOOLARGE;
  const scaml::StudiesConditionPlan plan = scaml::studies_fantasy_condition_plan(G, n_max, F_max);
  if (plan.lds_doubles * sizeof(double) > kLdsLimit) return SCAML_E_TOOLARGE;
  if (G == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::StudiesFantasyConditionParams p{L, resid, mean_p, n_points, n_obs, info, eps, n_fant, m_all, s_all, alpha_f, y_fant, mu_p, G, n_max, p_max, F_max};
  return launch(m->cond_fantasy, dim3(plan.grid), plan.block, plan.lds_doubles * sizeof(double), stream, "studies_fantasy_condition", p);
}

// ---- (8) target GP: objective + gradient, and the whole L-BFGS refit, in one launch (csrc/gp_target_fit.hip) -------------
namespace {
constexpr int kTargetFitThreads = scaml::TARGET_FIT_THREADS;
// Argument checks of both launchers.  The order that can be observed is kept by both: every SCAML_E_BADARG check (the entry point's,
// the filler's, the launcher's own, these) comes before every SCAML_E_TOOLARGE check (D here, then the launcher's sizes), and an empty
// launch is SCAML_OK only after all of them.
int target_fit_check(const scaml::TargetFitParams& p) {
  if (p.B < 0 || p.n < 1 || p.T < 1 || p.D < 1) return SCAML_E_BADARG;
  if (!p.means_t || !p.covs_p || !p.X || !p.y || !p.z || !p.value || !p.info) return SCAML_E_BADARG;
  if (!valid_kind(p.kind)) return SCAML_E_BADARG;
  if (p.D > scaml::TARGET_FIT_DMAX) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
int target_fit_launch(scaml::TargetFitParams& p, void* stream) {
  if (!(p.s_all > 0.0)) return SCAML_E_BADARG;
  if (const int rc = target_fit_check(p)) return rc;
  const scaml::TargetFitPlan plan = scaml::target_fit_plan(p.n, p.T, p.D, g_dev.target_fit_path.load(kRelaxed));
  p.use_mfma = plan.use_mfma ? 1 : 0;
  const size_t lds = plan.lds_doubles * sizeof(double);
  if (lds > kLdsLimit) return SCAML_E_TOOLARGE;
  if (p.B == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return launch(m->tgt_fit, dim3((unsigned)p.B), kTargetFitThreads, lds, stream, "target_fit", p);
}
// Fillers of the kernel arguments both pairs of entry points share (the single problem's m_all / s_all, the batch's arrays and S are
// the caller's): evaluation mode, value + gradient at z ...
int target_fill_mll(scaml::TargetFitParams& p, const double* means_t, const double* covs_packed, const double* X, const double* y,
                    const double* spec_host, const double* z, int B, int n, int T, int D, int kind, double* value, double* grad,
                    int32_t* info, double* jitter_used) {
  if (!spec_host || !grad) return SCAML_E_BADARG;
  if (!scaml::target_spec_from_host(spec_host, p.spec)) return SCAML_E_BADARG;
  p.means_t = means_t; p.covs_p = covs_packed; p.X = X; p.y = y;
  p.z = const_cast<double*>(z); p.value = value; p.grad = grad; p.info = info; p.jitter = jitter_used;
  p.B = B; p.n = n; p.T = T; p.D = D; p.kind = kind; p.mode = 0; p.history = 1; p.max_ls = 0;
  return SCAML_OK;
}
// ... and optimiser mode, L-BFGS from z (`workspace_needed`: the entry point's own scaml_target_fit*_workspace_doubles)
int target_fill_fit(scaml::TargetFitParams& p, const double* means_t, const double* covs_packed, const double* X, const double* y,
                    const double* spec_host, double* z, int B, int n, int T, int D, int kind, int max_iter, int history, double gtol,
                    double ftol, double* value, int32_t* info, double* jitter_used, int32_t* stats, double* workspace,
                    long long workspace_doubles, long long workspace_needed) {
  if (!spec_host || !workspace) return SCAML_E_BADARG;
  if (max_iter < 0 || history < 1 || history > scaml::TARGET_FIT_HMAX) return SCAML_E_BADARG;
  if (workspace_doubles < workspace_needed) return SCAML_E_BADARG;
  if (!scaml::target_spec_from_host(spec_host, p.spec)) return SCAML_E_BADARG;
  p.means_t = means_t; p.covs_p = covs_packed; p.X = X; p.y = y;
  p.z = z; p.value = value; p.grad = nullptr; p.info = info; p.jitter = jitter_used; p.workspace = workspace; p.stats = stats;
  p.B = B; p.n = n; p.T = T; p.D = D; p.kind = kind; p.mode = 1; p.max_iter = max_iter; p.history = history; p.max_ls = 20;
  p.gtol = gtol; p.ftol = ftol;
  return SCAML_OK;
}
}  // namespace

int scaml_target_fit_max_d(void) { return scaml::TARGET_FIT_DMAX; }

int scaml_target_fit_max_n(int T, int D) {
  if (T < 1 || D < 1 || D > scaml::TARGET_FIT_DMAX) return 0;
  int n = 0;
  while (n < 4096 && scaml::target_fit_plan(n + 1, T, D, 1).lds_doubles * sizeof(double) <= kLdsLimit) ++n;   // (mode 1: column by column)
  return n;
}

long long scaml_target_fit_workspace_doubles(int B, int T, int D, int history) {
  if (B < 0 || T < 1 || D < 1 || history < 1) return 0;
  return (long long)B * (6 + 2 * (long long)history) * (D + 2 + T);
}

int scaml_target_mll_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, double m_all, double s_all,
                         const double* spec_host, const double* z, int B, int n, int T, int D, int kind, double* value, double* grad,
                         int32_t* info, double* jitter_used, void* stream) {
  scaml::TargetFitParams p{};
  p.m_all = m_all; p.s_all = s_all;
  const int rc = target_fill_mll(p, means_t, covs_packed, X, y, spec_host, z, B, n, T, D, kind, value, grad, info, jitter_used);
  return rc ? rc : target_fit_launch(p, stream);
}

int scaml_target_fit_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, double m_all, double s_all,
                         const double* spec_host, double* z, int B, int n, int T, int D, int kind, int max_iter, int history, double gtol,
                         double ftol, double* value, int32_t* info, double* jitter_used, int32_t* stats, double* workspace,
                         long long workspace_doubles, void* stream) {
  scaml::TargetFitParams p{};
  p.m_all = m_all; p.s_all = s_all;
  const int rc = target_fill_fit(p, means_t, covs_packed, X, y, spec_host, z, B, n, T, D, kind, max_iter, history, gtol, ftol, value, info,
                                 jitter_used, stats, workspace, workspace_doubles, scaml_target_fit_workspace_doubles(B, T, D, history));
  return rc ? rc : target_fit_launch(p, stream);
}

// ---- (8b) the same objective and refit over S problems x B start points in one launch ---------------------------------------
namespace {
// `p.base` filled by the caller except use_mfma; S, the per-problem arrays and the limits are checked here.  There is no host value
// of s_all to check; n_max against scaml_target_fit_max_n comes before the LDS size (which is a loop over 1 .. n_max).
int target_fit_batched_launch(scaml::TargetFitBatchParams& bp, void* stream) {
  scaml::TargetFitParams& p = bp.base;
  if (bp.S < 0 || !bp.n_points || !bp.m_all || !bp.s_all) return SCAML_E_BADARG;
  if (const int rc = target_fit_check(p)) return rc;
  if (p.n > scaml_target_fit_max_n(p.T, p.D)) return SCAML_E_TOOLARGE;
  if ((long long)bp.S * p.B > 0x7fffffffLL) return SCAML_E_TOOLARGE;
  const scaml::TargetFitPlan plan = scaml::target_fit_batched_plan(p.n, p.T, p.D, g_dev.target_fit_path.load(kRelaxed));
  p.use_mfma = plan.use_mfma ? 1 : 0;
  const size_t lds = plan.lds_doubles * sizeof(double);
  if (lds > kLdsLimit) return SCAML_E_TOOLARGE;
  if (bp.S == 0 || p.B == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return launch(m->tgt_fit_batched, dim3((unsigned)(bp.S * p.B)), kTargetFitThreads, lds, stream, "target_fit_batched", bp);
}
}  // namespace

long long scaml_target_fit_batched_workspace_doubles(int S, int B, int T, int D, int history) {
  if (S < 0 || B < 0 || T < 1 || D < 1 || history < 1) return 0;
  return (long long)S * B * (6 + 2 * (long long)history) * (D + 2 + T);
}

int scaml_target_mll_batched_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, const int32_t* n_points,
                                 const double* m_all, const double* s_all, const double* spec_host, const double* z, int S, int B, int n_max,
                                 int T, int D, int kind, double* value, double* grad, int32_t* info, double* jitter_used, void* stream) {
  scaml::TargetFitBatchParams bp{};
  bp.n_points = n_points; bp.m_all = m_all; bp.s_all = s_all; bp.S = S;
  const int rc = target_fill_mll(bp.base, means_t, covs_packed, X, y, spec_host, z, B, n_max, T, D, kind, value, grad, info, jitter_used);
  return rc ? rc : target_fit_batched_launch(bp, stream);
}

int scaml_target_fit_batched_f64(const double* means_t, const double* covs_packed, const double* X, const double* y, const int32_t* n_points,
                                 const double* m_all, const double* s_all, const double* spec_host, double* z, int S, int B, int n_max, int T,
                                 int D, int kind, int max_iter, int history, double gtol, double ftol, double* value, int32_t* info,
                                 double* jitter_used, int32_t* stats, double* workspace, long long workspace_doubles, void* stream) {
  scaml::TargetFitBatchParams bp{};
  bp.n_points = n_points; bp.m_all = m_all; bp.s_all = s_all; bp.S = S;
  const int rc = target_fill_fit(bp.base, means_t, covs_packed, X, y, spec_host, z, B, n_max, T, D, kind, max_iter, history, gtol, ftol, value, info,
                                 jitter_used, stats, workspace, workspace_doubles, scaml_target_fit_batched_workspace_doubles(S, B, T, D, history));
  return rc ? rc : target_fit_batched_launch(bp, stream);
}

// ---- (9) source stack: the whole hyper-parameter fit as rounds of { fit, MLL gradient, optimiser step } (csrc/gp_stack_fit.hip) ----
namespace {
struct StackFitLayout {
  size_t state, theta, L, alpha, linv, quad, logdet, mll, jitter, info, grad, blocked, total;
};
StackFitLayout stack_fit_layout(int B, int N, int D, int history) {
  const size_t b = (size_t)B, n = (size_t)N, P = (size_t)D + 2, nb = (n + 15) / 16;
  StackFitLayout l{};
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  l.state = take(b * scaml::stack_fit_state_doubles((int)P, history) * 8);   // (first: the caller may read the state, include/scaml_gp.h)
  l.theta = take(b * P * 8);
  l.L = take(b * n * n * 8);
  l.alpha = take(b * n * 8);
  l.linv = take(b * nb * 256 * 8);
  l.quad = take(b * 8);
  l.logdet = take(b * 8);
  l.mll = take(b * 8);
  l.jitter = take(b * 8);
  l.info = take(b * 4);
  l.grad = take((size_t)scaml_mll_backward_workspace_doubles(B, N, D) * 8);
  l.blocked = take(N > 256 ? (size_t)scaml_gp_fit_blocked_workspace_bytes(B, N) : 0);
  l.total = o;
  return l;
}
}  // namespace

int scaml_stack_fit_max_d(void) { return scaml::STACK_FIT_PMAX - 2; }

long long scaml_stack_fit_workspace_bytes(int B, int N, int D, int history) {
  if (B < 0 || N < 1 || N > scaml_fit_blocked_max_n() || D < 1 || D > scaml_stack_fit_max_d() || history < 1 || history > scaml::STACK_FIT_HMAX) return 0;
  return (long long)stack_fit_layout(B, N, D, history).total;
}

int scaml_stack_fit_f64(const double* X, const double* y, const int32_t* n_points, const double* spec_host, double* z, int B, int N,
                        int D, int kind, int n_evals, unsigned flags, int max_iter, int history, double gtol, double ftol,
                        double* value, int32_t* stats, void* workspace, long long workspace_bytes, void* stream) {
  if (B < 0 || N < 1 || D < 1 || n_evals < 0 || max_iter < 0) return SCAML_E_BADARG;
  if (!X || !y || !spec_host || !z || !value || !stats || !workspace) return SCAML_E_BADARG;
  if (!valid_kind(kind) || (flags & ~SCAML_STACK_FIT_CONTINUE)) return SCAML_E_BADARG;
  if (history < 1 || history > scaml::STACK_FIT_HMAX) return SCAML_E_BADARG;
  scaml::HyperSpec sp{};
  if (!scaml::hyper_spec_from_host(spec_host, sp)) return SCAML_E_BADARG;
  // the shapes the fit and gradient paths take
  const bool blocked = N > scaml_fit_max_n();
  if (N > scaml_fit_blocked_max_n() || (blocked && (N & 15))) return SCAML_E_TOOLARGE;
  if (D > scaml_stack_fit_max_d() || D > (blocked ? scaml_fit_blocked_max_d() : scaml_fit_max_d(N))) return SCAML_E_TOOLARGE;
  if (scaml::mll_grad_lds_doubles(D) * sizeof(double) > kLdsLimit - 2048) return SCAML_E_TOOLARGE;
  const StackFitLayout lay = stack_fit_layout(B, N, D, history);
  if (workspace_bytes < (long long)lay.total || ((uintptr_t)workspace & 15)) return SCAML_E_BADARG;
  if (B == 0 || n_evals == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  char* ws = (char*)workspace;
  double *theta = (double*)(ws + lay.theta), *L = (double*)(ws + lay.L), *alpha = (double*)(ws + lay.alpha), *linv = (double*)(ws + lay.linv);
  double *quad = (double*)(ws + lay.quad), *logdet = (double*)(ws + lay.logdet), *mll = (double*)(ws + lay.mll), *jit = (double*)(ws + lay.jitter);
  int32_t* info = (int32_t*)(ws + lay.info);
  double* gwork = (double*)(ws + lay.grad);
  const int nb = (N + 15) / 16, tiles = nb * (nb + 1) / 2;
  double* partials = gwork + (size_t)B * N * N;
  scaml::StackFitParams p{mll, info, partials, n_points, sp, z, theta, value, stats, (double*)(ws + lay.state), B, N, D, tiles, 1,
                          max_iter, history, 20, gtol, ftol, 1e-4};
  int rc = SCAML_OK;
  if (!(flags & SCAML_STACK_FIT_CONTINUE)) {
    if (n_points) {   // ragged stacks: rows past n_t are never written by the fit but read by the solves
      hipError_t e = hipMemsetAsync(L, 0, (size_t)B * N * N * 8, (hipStream_t)stream);
      if (e == hipSuccess) e = hipMemsetAsync(alpha, 0, (size_t)B * N * 8, (hipStream_t)stream);
      if (e != hipSuccess) { set_error("hipMemsetAsync(stack fit factors)", e); return SCAML_E_LAUNCH; }
    }
    p.mode = 0;
    if ((rc = launch(m->stack_step, dim3((unsigned)B), 64, 0, stream, "stack_fit_step", p)) != SCAML_OK) return rc;
    p.mode = 1;
  }
  for (int r = 0; r < n_evals; ++r) {
    if (blocked) {
      rc = scaml_gp_fit_blocked_f64(X, y, theta, n_points, nullptr, B, N, D, kind, L, alpha, quad, logdet, mll, info, jit, linv, SCAML_FIT_STORE_L,
                                    ws + lay.blocked, (long long)(lay.total - lay.blocked), stream);
    } else {
      scaml::FitParams f{X, y, theta, n_points, nullptr, nullptr, L, alpha, quad, logdet, mll, info, jit, linv, B, N, D, SCAML_FIT_STORE_L};
      rc = fit_common(f, kind, stream);
    }
    if (rc != SCAML_OK) return rc;
    if ((rc = scaml_mll_backward_f64(X, theta, L, linv, alpha, n_points, B, N, D, kind, gwork, partials, stream)) != SCAML_OK) return rc;
    if ((rc = launch(m->stack_step, dim3((unsigned)B), 64, 0, stream, "stack_fit_step", p)) != SCAML_OK) return rc;
  }
  return SCAML_OK;
}

// ---- (7h) the acquisition optimiser of many studies' start points as rounds of { (5e), (7g), optimiser step } (csrc/gp_acqf_opt.hip) ----
namespace {
struct AcqfOptLayout {
  size_t state, Xq, group_live, mu, var, cov, value, grad, total;
};
AcqfOptLayout acqf_opt_layout(int B, int n_max, int T, int D, int history) {
  const size_t b = (size_t)B, t = (size_t)T, d = (size_t)D;
  AcqfOptLayout l{};
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  l.state = take(b * scaml::acqf_opt_state_doubles(D, history) * 8);   // (first: the caller may read the state, include/scaml_gp.h)
  l.Xq = take(b * d * 8);
  l.group_live = take(b * 4);
  l.mu = take(t * b * 16 * 8);
  l.var = take(t * b * 16 * 8);
  l.cov = take(t * (size_t)n_max * b * 16 * 8);
  l.value = take(b * 8);
  l.grad = take(b * d * 8);
  l.total = o;
  return l;
}
}  // namespace

int scaml_studies_acqf_opt_max_d(void) { return scaml::ACQF_OPT_MAX_D; }

long long scaml_studies_acqf_opt_workspace_bytes(int B, int G, int n_max, int T, int D, int history) {
  if (B < 0 || G < 0 || n_max < 1 || n_max > scaml::STUDIES_ACQF_MAX_N || T < 1 || D < 1 || D > scaml::ACQF_OPT_MAX_D || history < 1 ||
      history > scaml::ACQF_OPT_HMAX || B > (1 << 26))
    return 0;
  return (long long)acqf_opt_layout(B, n_max, T, D, history).total;
}

namespace {
// (7h) and its per-group-source-task form (`own`): only the evaluation launch of a round is handed the table.  `fant` non-NULL: (7l),
// the rounds' acquisition launch is (7k)'s with these fantasy arrays (alpha_t is not read then).
struct AcqfOptFantasy {
  const double* alpha_f;
  const int32_t* n_fant;
  int F_max;
};
int studies_acqf_opt_checked(const double* x0, const int32_t* group, const double* const* VA_tab, const double* X, const double* theta_s,
                             const double* Linv, const double* alpha_s, const double* y_mean, const double* y_std,
                             const int32_t* n_points_s, const double* w, const uint8_t* active, const double* Xt, const double* theta_t,
                             const double* L, const double* Linv_diag, const double* alpha_t, const int32_t* n_points_t,
                             const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int B, int G,
                             int n_max, int T, int N, int D, int kind_s, int kind_t, int acqf, const double* lo, const double* hi, int max_iter,
                             int history, int max_ls, double gtol, double ftol, double c1, int n_evals, unsigned flags, void* workspace,
                             double* x, double* f, int32_t* stats, bool own, const int32_t* task_base, int Tsrc, void* stream,
                             const AcqfOptFantasy* fant = nullptr) {
  // what is the optimiser's own, and what the workspace layout is sized by
  if (B < 0 || n_max < 1 || T < 1 || D < 1 || n_evals < 0 || max_iter < 0 || max_ls < 1) return SCAML_E_BADARG;
  if (!x0 || !group || !lo || !hi || !workspace || !x || !f || !stats) return SCAML_E_BADARG;
  if (flags & ~SCAML_ACQF_OPT_CONTINUE) return SCAML_E_BADARG;
  if (history < 1 || history > scaml::ACQF_OPT_HMAX || ((uintptr_t)workspace & 15)) return SCAML_E_BADARG;
  if (!(gtol >= 0.0) || !(c1 > 0.0) || ftol != ftol) return SCAML_E_BADARG;
  const AcqfOptLayout lay = acqf_opt_layout(B, n_max, T, D, history);
  auto ws = [workspace](size_t off) { return (double*)((uintptr_t)workspace + off); };
  double *Xq = ws(lay.Xq), *mu = ws(lay.mu), *var = ws(lay.var), *cov = ws(lay.cov), *value = ws(lay.value), *grad = ws(lay.grad);
  int32_t* live = (int32_t*)ws(lay.group_live);
  // the evaluation kernels are handed group_live where they were handed group: a stopped start (and a padding row) returns at once
  scaml::PosteriorGroupedParams ps = grouped_block(Xq, live, Xt, n_points_t, VA_tab, X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s, T, N, B, G,
                                                   n_max, D, mu, var, cov, own ? task_base : nullptr, Tsrc, false);
  scaml::StudiesAcqfParams pt{mu, var, cov, live, Xq, w, active, Xt, theta_t, L, Linv_diag, alpha_t, n_points_t, m_all, s_all, info, acqf_param,
                              value, grad, nullptr, nullptr, B, G, n_max, T, D, kind_t, acqf, 0};
  // the arguments and shapes (5e) and (7g) take: both blocks' SCAML_E_BADARG before either's SCAML_E_TOOLARGE
  scaml::StudiesFantasyParams pf = fant ? fantasy_block(pt, fant->alpha_f, fant->n_fant, fant->F_max) : scaml::StudiesFantasyParams{};
  const int rs = grouped_check(ps, kind_s, false, own), rt = fant ? fantasy_check(pf, false) : acqf_check(pt, false);
  if (rs == SCAML_E_BADARG || rt == SCAML_E_BADARG) return SCAML_E_BADARG;
  if (rs != SCAML_OK || rt != SCAML_OK || D > scaml::ACQF_OPT_MAX_D) return SCAML_E_TOOLARGE;
  // (7l)'s pass keeps the waves' shares in static LDS next to the dynamic block that grouped_check admits (no N within
  // scaml_posterior_max_n() comes near it today; the rule stands for the day that limit rises)
  if (fant && scaml::posterior_linv_lds_doubles(N, D) * sizeof(double) > kLdsLimit - kOrderedSumsLds) return SCAML_E_TOOLARGE;
  if (B == 0 || G == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  scaml::AcqfOptParams p{value, grad, group, x0, lo, hi, ws(lay.state), Xq, live, x, f, stats, B, G, D, 1, max_iter, history,
                         max_ls, 0, gtol, ftol, c1};
  int rc = SCAML_OK;
  if (!(flags & SCAML_ACQF_OPT_CONTINUE)) {
    p.mode = 0;
    if ((rc = launch(m->acqf_opt_step, dim3((unsigned)B), 64, 0, stream, "acqf_opt_step", p)) != SCAML_OK) return rc;
    p.mode = 1;
  }
  for (int r = 0; r < n_evals; ++r) {
    // (Arguments and sizes were checked above, once; only a failing launch can end the call here, with the rounds before it enqueued.)
    // ((7l): the pass with ordered sums, so that a round is a pure function of the state and chunking cannot change the result)
    if ((rc = grouped_launch(*m, ps, kind_s, false, stream, fant != nullptr)) != SCAML_OK) return rc;
    if ((rc = fant ? fantasy_launch(*m, pf, false, stream) : acqf_launch(*m, pt, false, stream)) != SCAML_OK) return rc;
    if ((rc = launch(m->acqf_opt_step, dim3((unsigned)B), 64, 0, stream, "acqf_opt_step", p)) != SCAML_OK) return rc;
  }
  return SCAML_OK;
}
}  // namespace

int scaml_studies_acqf_opt_f64(const double* x0, const int32_t* group, const double* const* VA_tab, const double* X, const double* theta_s,
                               const double* Linv, const double* alpha_s, const double* y_mean, const double* y_std,
                               const int32_t* n_points_s, const double* w, const uint8_t* active, const double* Xt, const double* theta_t,
                               const double* L, const double* Linv_diag, const double* alpha_t, const int32_t* n_points_t,
                               const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int B, int G,
                               int n_max, int T, int N, int D, int kind_s, int kind_t, int acqf, const double* lo, const double* hi, int max_iter,
                               int history, int max_ls, double gtol, double ftol, double c1, int n_evals, unsigned flags, void* workspace,
                               double* x, double* f, int32_t* stats, void* stream) {
  return studies_acqf_opt_checked(x0, group, VA_tab, X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s, w, active, Xt, theta_t, L, Linv_diag,
                                  alpha_t, n_points_t, m_all, s_all, info, acqf_param, B, G, n_max, T, N, D, kind_s, kind_t, acqf, lo, hi,
                                  max_iter, history, max_ls, gtol, ftol, c1, n_evals, flags, workspace, x, f, stats, false, nullptr, 0, stream);
}

int scaml_studies_acqf_opt_own_f64(const double* x0, const int32_t* group, const double* const* VA_tab, const double* X, const double* theta_s,
                                   const double* Linv, const double* alpha_s, const double* y_mean, const double* y_std,
                                   const int32_t* n_points_s, const double* w, const uint8_t* active, const double* Xt, const double* theta_t,
                                   const double* L, const double* Linv_diag, const double* alpha_t, const int32_t* n_points_t,
                                   const double* m_all, const double* s_all, const int32_t* info, const double* acqf_param, int B, int G,
                                   int n_max, int T, int N, int D, int kind_s, int kind_t, int acqf, const double* lo, const double* hi,
                                   int max_iter, int history, int max_ls, double gtol, double ftol, double c1, int n_evals, unsigned flags,
                                   void* workspace, double* x, double* f, int32_t* stats, const int32_t* task_base, int Tsrc, void* stream) {
  return studies_acqf_opt_checked(x0, group, VA_tab, X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s, w, active, Xt, theta_t, L, Linv_diag,
                                  alpha_t, n_points_t, m_all, s_all, info, acqf_param, B, G, n_max, T, N, D, kind_s, kind_t, acqf, lo, hi,
                                  max_iter, history, max_ls, gtol, ftol, c1, n_evals, flags, workspace, x, f, stats, true, task_base, Tsrc, stream);
}

// ---- (7l) (7h) / (7h') on (7k)'s block: the studies may hold pending evaluations; task_base NULL: a shared source stack ----
int scaml_studies_fantasy_acqf_opt_f64(const double* x0, const int32_t* group, const double* const* VA_tab, const double* X, const double* theta_s,
                                       const double* Linv, const double* alpha_s, const double* y_mean, const double* y_std,
                                       const int32_t* n_points_s, const double* w, const uint8_t* active, const double* Xt,
                                       const double* theta_t, const double* L, const double* Linv_diag, const double* alpha_f,
                                       const int32_t* n_fant, const int32_t* n_points_t, const double* m_all, const double* s_all,
                                       const int32_t* info, const double* acqf_param, int B, int G, int n_max, int F_max, int T, int N, int D,
                                       int kind_s, int kind_t, int acqf, const double* lo, const double* hi, int max_iter, int history, int max_ls,
                                       double gtol, double ftol, double c1, int n_evals, unsigned flags, void* workspace, double* x, double* f,
                                       int32_t* stats, const int32_t* task_base, int Tsrc, void* stream) {
  const AcqfOptFantasy fant{alpha_f, n_fant, F_max};
  return studies_acqf_opt_checked(x0, group, VA_tab, X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s, w, active, Xt, theta_t, L, Linv_diag,
                                  alpha_f, n_points_t, m_all, s_all, info, acqf_param, B, G, n_max, T, N, D, kind_s, kind_t, acqf, lo, hi,
                                  max_iter, history, max_ls, gtol, ftol, c1, n_evals, flags, workspace, x, f, stats, task_base != nullptr, task_base,
                                  Tsrc, stream, &fant);
}

// ---- (7t) the box L-BFGS step for P <= 128 variables per start with a slot table; (7s) the optimiser of the joint q-point acquisition
// as rounds of { value pass, (5g), weighted sums, gather, assemble, solve, (7p) / (7q), step } (csrc/gp_qacqf_opt.hip) ----
namespace {
int qacqf_opt_step_check(const scaml::QAcqfOptParams& p) {
  if (p.B < 0 || p.Bs < 0 || p.Bs > p.B || (!p.slots && p.Bs != p.B) || p.P < 1 || p.mode < 0 || p.mode > 2) return SCAML_E_BADARG;
  if (p.max_iter < 0 || p.max_ls < 1 || p.history < 1 || p.history > scaml::QACQF_OPT_HMAX) return SCAML_E_BADARG;
  if (!p.lo || !p.hi || !p.state || !p.Xq || !p.x || !p.f || !p.stats) return SCAML_E_BADARG;
  if ((p.mode == 0 && !p.x0) || (p.mode == 1 && (!p.value || !p.grad))) return SCAML_E_BADARG;
  if (!(p.gtol >= 0.0) || !(p.c1 > 0.0) || p.ftol != p.ftol) return SCAML_E_BADARG;
  if (p.P > scaml::QACQF_OPT_MAX_P || p.B > (1 << 26)) return SCAML_E_TOOLARGE;
  return SCAML_OK;
}
int qacqf_opt_step_launch(Module& m, scaml::QAcqfOptParams& p, void* stream) {   // a checked block, Bs > 0
  return launch(m.qacqf_opt_step, dim3((unsigned)p.Bs), 64, 0, stream, "qacqf_opt_step", p);
}
int qacqf_opt_gather_launch(Module& m, scaml::QAcqfOptGatherParams& p, void* stream) {
  const long long elems = scaml::qo_gather_elems(p);
  return launch(m.qacqf_opt_gather, dim3((unsigned)((elems + 255) / 256)), 256, 0, stream, "qacqf_opt_gather", p);
}

struct QAcqfOptLayout {
  size_t state, Xq, value, grad, mu_v, VQ, mu, var, cov, mu_g, var_g, cov_g, mean_s, var_s, cov_s, xall, Knn, resid, Knq, mean_q, var_q, Z,
      jitter, info_out, total;
};
// sized by all B starts: a call at Bs <= B slots packs its arrays (Mq = Bs * q columns) into the same places
QAcqfOptLayout qacqf_opt_layout(int B, int n, int p, int q, int T, int N, int D, int history) {
  const size_t b = (size_t)B, nn = (size_t)n, t = (size_t)T, d = (size_t)D, Mq = b * (size_t)q, rows = nn + (size_t)p + (size_t)q;
  QAcqfOptLayout l{};
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  l.state = take(b * scaml::qacqf_opt_state_doubles(q * D, history) * 8);   // (first: the caller may read the state, include/scaml_gp.h)
  l.Xq = take(Mq * d * 8);
  l.value = take(b * 8);
  l.grad = take(Mq * d * 8);
  l.mu_v = take(t * Mq * 8);
  l.VQ = take(t * (size_t)N * Mq * 8);
  l.mu = take(t * Mq * 16 * 8);
  l.var = take(t * Mq * 16 * 8);
  l.cov = take(t * rows * Mq * 16 * 8);
  l.mu_g = take(Mq * 16 * 8);
  l.var_g = take(Mq * 16 * 8);
  l.cov_g = take(rows * Mq * 16 * 8);
  l.mean_s = take((nn + Mq) * 8);
  l.var_s = take((nn + Mq) * 8);
  l.cov_s = take(nn * (nn + Mq) * 8);
  l.xall = take((nn + Mq) * d * 8);
  l.Knn = take(nn * nn * 8);
  l.resid = take(nn * 8);
  l.Knq = take(nn * Mq * 8);
  l.mean_q = take(Mq * 8);
  l.var_q = take(Mq * 8);
  l.Z = take(nn * Mq * 8);
  l.jitter = take(b * 8);
  l.info_out = take(b * 4);
  l.total = o;
  return l;
}
}  // namespace

int scaml_qacqf_opt_max_p(void) { return scaml::QACQF_OPT_MAX_P; }

long long scaml_qacqf_opt_step_workspace_bytes(int B, int P, int history) {
  if (B < 0 || B > (1 << 26) || P < 1 || P > scaml::QACQF_OPT_MAX_P || history < 1 || history > scaml::QACQF_OPT_HMAX) return 0;
  return (long long)B * (long long)scaml::qacqf_opt_state_doubles(P, history) * 8;
}

long long scaml_qacqf_opt_workspace_bytes(int B, int n, int p, int q, int T, int N, int D, int history) {
  if (B < 0 || B > (1 << 20) || n < 1 || p < 0 || q < 1 || T < 1 || N < 1 || D < 1 || history < 1 || history > scaml::QACQF_OPT_HMAX) return 0;
  if (q > scaml::QACQF_MAX_Q || q + p > scaml::QACQF_MAX_Q || n + p + q > scaml::QACQF_MAX_ROWS || n + p + q > N || N > scaml_posterior_max_n() ||
      D > scaml::QACQF_MAX_D)
    return 0;
  return (long long)qacqf_opt_layout(B, n, p, q, T, N, D, history).total;
}

int scaml_qacqf_opt_step_f64(const double* value, const double* grad, const int32_t* slots, const double* x0, const double* lo, const double* hi,
                             int B, int Bs, int P, int mode, int max_iter, int history, int max_ls, double gtol, double ftol, double c1,
                             double* state, double* Xq, double* x, double* f, int32_t* stats, void* stream) {
  scaml::QAcqfOptParams p{value, grad, slots, x0, lo, hi, state, Xq, x, f, stats, B, Bs, P, mode, max_iter, history, max_ls, 0, gtol, ftol, c1};
  if (const int rc = qacqf_opt_step_check(p)) return rc;
  if (Bs == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  return qacqf_opt_step_launch(*m, p, stream);
}

int scaml_qacqf_opt_f64(const double* x0, const int32_t* slots, const double* Xa, const double* X, const double* theta_s, const double* Linv,
                        const double* alpha_s, const double* y_mean, const double* y_std, const int32_t* n_points_s, const double* VA,
                        const double* w, const uint8_t* active, const double* mu_t, const double* cov_tt, const double* var_t, const double* Xt,
                        const double* theta_t, const double* targets, const double* L, const double* Linv_diag, const double* alpha_t,
                        double m_all, double s_all, const int32_t* info, const double* base_samples, const double* Xp, const double* Zp,
                        const double* mu_p, const double* Sigma_pp, int B, int Bs, int n, int p, int q, int S, int T, int N, int D, int kind_s,
                        int kind_t, int acqf, double acqf_param, const double* lo, const double* hi, int max_iter, int history, int max_ls,
                        double gtol, double ftol, double c1, int n_evals, unsigned flags, void* workspace, long long workspace_bytes, double* x,
                        double* f, int32_t* stats, void* stream) {
  // what is the optimiser's own, and what the workspace layout is sized by
  if (B < 0 || Bs < 0 || n < 1 || p < 0 || q < 1 || T < 1 || N < 1 || D < 1 || n_evals < 0) return SCAML_E_BADARG;
  if (!workspace || ((uintptr_t)workspace & 15) || (flags & ~SCAML_ACQF_OPT_CONTINUE)) return SCAML_E_BADARG;
  if (!mu_t || !cov_tt || !var_t || Bs > B) return SCAML_E_BADARG;
  const bool sized = B <= (1 << 20) && q <= scaml::QACQF_MAX_Q && p <= scaml::QACQF_MAX_Q && D <= scaml::QACQF_MAX_D && n <= scaml::QACQF_MAX_ROWS &&
                     N <= scaml_posterior_max_n() && history >= 1 && history <= scaml::QACQF_OPT_HMAX;
  // (a shape beyond the limits: the checks below refuse it, as SCAML_E_BADARG first if an argument is bad as well; the layout is not needed then)
  const QAcqfOptLayout lay = sized ? qacqf_opt_layout(B, n, p, q, T, N, D, history) : QAcqfOptLayout{};
  if (sized && workspace_bytes < (long long)lay.total) return SCAML_E_BADARG;
  auto ws = [workspace](size_t off) { return (double*)((uintptr_t)workspace + off); };
  const int P = sized ? q * D : 1, Mq = sized ? Bs * q : 0, Ma = n + p;
  double *Xq = ws(lay.Xq), *value = ws(lay.value), *grad = ws(lay.grad), *VQ = ws(lay.VQ), *mu = ws(lay.mu), *var = ws(lay.var), *cov = ws(lay.cov);
  double *mu_g = ws(lay.mu_g), *var_g = ws(lay.var_g), *cov_g = ws(lay.cov_g), *mean_s = ws(lay.mean_s), *var_s = ws(lay.var_s), *cov_s = ws(lay.cov_s);
  double *xall = ws(lay.xall), *Knq = ws(lay.Knq), *mean_q = ws(lay.mean_q), *var_q = ws(lay.var_q), *Z = ws(lay.Z);
  // the blocks of a round, in its order
  scaml::PosteriorParams pv{Xq, X, theta_s, Linv, nullptr, alpha_s, y_mean, y_std, n_points_s, ws(lay.mu_v), nullptr, VQ, T, N, Mq, D, 0, 0, 0,
                            nullptr, nullptr, 0, 0, nullptr};
  scaml::PosteriorJointParams pj = grad_joint_block(Xq, Xa, X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s, VA, VQ, T, N, Mq, Ma, q, D, mu, var, cov, 0);
  const long long len = 16LL * Mq, len_cov = (long long)(Ma + q) * len;
  scaml::QAcqfOptGatherParams pg{mu_g, var_g, cov_g, Xq, mu_t, var_t, cov_tt, Xt, mean_s, var_s, cov_s, xall, n, Mq, D, 0};
  scaml::TargetAssembleParams pa{cov_s, mean_s, var_s, xall, theta_t, targets, m_all, s_all, ws(lay.Knn), ws(lay.resid), Knq, mean_q, var_q, n, Mq, D};
  scaml::ChoSolveParams pc{L, Linv_diag, Knq, nullptr, Z, 1, n, Mq, 0};
  scaml::QAcqfPendingParams pq{{Knq, Z, alpha_t, mean_q, var_q, m_all, s_all, info, cov_g, mu_g, var_g, Xt, Xq, theta_t, base_samples, acqf_param,
                                value, grad, ws(lay.jitter), (int32_t*)ws(lay.info_out), n, Mq, q, S, D, kind_t, acqf, 0},
                               {Xp, Zp, mu_p, Sigma_pp, p, 0}};
  scaml::QAcqfOptParams po{value, grad, slots, x0, lo, hi, ws(lay.state), Xq, x, f, stats, B, Bs, P, 1, max_iter, history, max_ls, 0, gtol, ftol, c1};
  if (!x0) return SCAML_E_BADARG;   // (the step's own check asks for it at a reset only; a continued call is handed the same arguments)
  // every block's SCAML_E_BADARG before any block's SCAML_E_TOOLARGE
  const int rcs[] = {qacqf_opt_step_check(po),
                     posterior_linv_check(pv, kind_s, 0, false),
                     grad_joint_check(pj, Mq, kind_s, 0),
                     wsum_check(mu, w, T, len, 1, mu_g),
                     target_assemble_check(pa, kind_t),
                     cho_solve_check(pc),
                     p > 0 ? qacqf_pending_check(pq) : qacqf_check(pq.a)};
  for (const int rc : rcs)
    if (rc == SCAML_E_BADARG) return SCAML_E_BADARG;
  for (const int rc : rcs)
    if (rc != SCAML_OK) return SCAML_E_TOOLARGE;
  if (!sized || posterior_linv_fits(pv) != SCAML_OK) return SCAML_E_TOOLARGE;
  if (B == 0 || Bs == 0 || n_evals == 0) return SCAML_OK;
  Module* m = ready();
  if (!m) return SCAML_E_LAUNCH;
  int rc = SCAML_OK;
  // the start of a call: the trial points of the slots (from a reset, or again from the state: the table may have changed) and the
  // training block of the joint prior at this call's row width
  po.mode = (flags & SCAML_ACQF_OPT_CONTINUE) ? 2 : 0;
  if ((rc = qacqf_opt_step_launch(*m, po, stream)) != SCAML_OK) return rc;
  po.mode = 1;
  pg.left = 1;
  if ((rc = qacqf_opt_gather_launch(*m, pg, stream)) != SCAML_OK) return rc;
  pg.left = 0;
  for (int r = 0; r < n_evals; ++r) {
    // (Arguments and sizes were checked above, once; only a failing launch can end the call here, with the rounds before it enqueued.)
    if ((rc = posterior_linv_launch(*m, pv, kind_s, false, stream)) != SCAML_OK) return rc;
    if ((rc = grad_joint_launch(*m, pj, Mq, kind_s, stream)) != SCAML_OK) return rc;
    if ((rc = wsum_launch(*m, mu, w, active, T, len, 1, mu_g, stream)) != SCAML_OK) return rc;
    if ((rc = wsum_launch(*m, cov, w, active, T, len_cov, 2, cov_g, stream)) != SCAML_OK) return rc;
    if ((rc = wsum_launch(*m, var, w, active, T, len, 2, var_g, stream)) != SCAML_OK) return rc;
    if ((rc = qacqf_opt_gather_launch(*m, pg, stream)) != SCAML_OK) return rc;
    if ((rc = target_assemble_launch(*m, pa, kind_t, stream)) != SCAML_OK) return rc;
    if ((rc = cho_solve_launch(*m, pc, stream)) != SCAML_OK) return rc;
    if ((rc = p > 0 ? qacqf_pending_launch(*m, pq, stream) : qacqf_launch(*m, pq.a, stream)) != SCAML_OK) return rc;
    if ((rc = qacqf_opt_step_launch(*m, po, stream)) != SCAML_OK) return rc;
  }
  return SCAML_OK;
}

}  // extern "C"
