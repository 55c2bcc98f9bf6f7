/*
 * scaml_gp_debug.h — developer switches of libscaml_hip.so.
 *
 * These functions are NOT part of the stable ABI of scaml_gp.h.  They flip process-global
 * switches that route an entry point through one of its implementations regardless of the
 * problem shape, for A/B timing and for testing one path against the other; each switch
 * starts from an environment variable read when the library is loaded.  A switch applies to
 * every thread and every device of the process; setting one while another thread is inside
 * an entry point is free of data races, and that call takes either the old or the new path.
 * They may change or disappear in any release.
 */
#ifndef SCAML_GP_DEBUG_H
#define SCAML_GP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* scaml_mll_backward_f64: 1 the two-launch path (L^-1 in the workspace, then the K^-1 tile kernel) even where the
 * single-launch kernel applies, 2 the single-launch kernel even for the small stacks the two launches serve by default,
 * anything else the choice by shape.  Starts from SCAML_GRAD_LEGACY (1) / SCAML_GRAD_FUSED (2).  Returns the previous mode. */
int scaml_debug_force_two_launch_grad(int mode);

/* scaml_gp_fit_blocked_f64: 0 by shape, 1 the 2 x 2 sequence of launches only, 2 the several-CUs-per-task kernel whenever
 * it is launchable; any other value changes nothing.  Starts from SCAML_BLOCKED_FIT_PATH.  Returns the previous mode, or,
 * for mode == -1, the path the last call took (1 / 2). */
int scaml_debug_blocked_fit_path(int mode);

/* Several-CUs-per-task fit: 1 write-through payload stores even when a task's workgroups share an XCD, 0 by placement;
 * any other value changes nothing.  Starts from SCAML_COOP_FAR (set: 1).  Returns the previous value. */
int scaml_debug_coop_far(int on);

/* scaml_target_mll_f64 / scaml_target_fit_f64: 1 the column-by-column elimination where the matrix-core factorisation
 * would apply, anything else the choice by shape.  Starts from SCAML_TARGET_FIT_NO_MFMA (set: 1).  Returns the previous mode. */
int scaml_debug_target_fit_path(int mode);

/* scaml_posterior_linv_grad_grouped_f64 / _own_f64 ((5e), (5e')): 1 launch the instance with ordered sums -- the one the rounds of
 * scaml_studies_fantasy_acqf_opt_f64 run, whose mu / var do not depend on the order in which the waves finish -- under that entry
 * point's limit (SCAML_E_TOOLARGE where the strip and the waves' shares do not fit the LDS together); anything else the default
 * instance.  The value-mode passes (5f) / (5f') have no such instance and are not affected.  Starts from
 * SCAML_GROUPED_ORDERED_SUMS (set: 1).  Returns the previous value. */
int scaml_debug_grouped_ordered_sums(int mode);

/* scaml_gp_fit_fused_f64 has a switch without a function: the environment variable SCAML_FIT_NO_FULL.  Set (not empty, not "0"),
 * every call takes the generic instance of its size class, never the full-tile instance of the N <= 256 class (N == 256, no
 * n_points, L -- when stored -- on a 16-byte boundary).  Unlike the switches above it is read at EVERY launch, so a process runs
 * both instances on the same input by changing its environment between two calls; changing the environment while another thread
 * is inside the entry point is a data race of the C library's. */

/* Diagnostic builds only (SCAML_STAMPS): point the device-side stamp buffer at caller memory.  0 ok, SCAML_E_BADARG
 * when the code object has no stamp buffer, SCAML_E_LAUNCH on a HIP error. */
int scaml_debug_set_stamp_buffer(long long* buf);

#ifdef __cplusplus
}
#endif
#endif /* SCAML_GP_DEBUG_H */
