"""ctypes binding of libscaml_hip.so (the C ABI declared in include/scaml_gp.h).

The product path has no CPU fallback: if the HIP library is missing or a symbol cannot be
resolved, importing this module raises.  Build it with ``python -c "import __graft_entry__ as
g; g.build()"`` from the repository root (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_int, c_uint, c_void_p

# torch must be imported BEFORE the library is loaded: torch ships its own libamdhip64.so.7 and
# libscaml_hip.so links against the same SONAME, so whichever loads first serves both.  Device
# pointers and streams handed across the C ABI come from torch's runtime instance; loading the
# system copy first would give this library a second, unrelated HIP runtime ("no ROCm-capable
# device is detected" at the first launch).
import torch  # noqa: F401  (side effect: HIP runtime loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libscaml_hip.so")

KIND_RBF = 0
KIND_MATERN52 = 1

FIT_STORE_L = 1
FIT_ZERO_UPPER = 2
FIT_NO_RETRY = 4
POST_XQ_PER_TASK = 1
POST_MEAN_ONLY = 2
STACK_FIT_CONTINUE = 1
ACQF_OPT_CONTINUE = 1

E_BADARG = -1
E_TOOLARGE = -2
E_LAUNCH = -3

_dp = c_void_p  # device pointers travel as integers


class ScamlLibraryError(RuntimeError):
    pass


_i, _u, _ll, _f = c_int, c_uint, ctypes.c_longlong, ctypes.c_double
_host_spec = ctypes.POINTER(_f)   # (the one host pointer of the ABI: 19 doubles -- stack fit: 15 -- read during the call)

# The C ABI, once: name -> (restype, argtypes).  include/scaml_gp.h declares the entry points, include/scaml_gp_debug.h the
# scaml_debug_* developer switches.
SIGNATURES = {
    "scaml_version": (_i, []),
    "scaml_last_error": (c_char_p, []),
    "scaml_fit_max_n": (_i, []),
    "scaml_fit_max_d": (_i, [_i]),
    "scaml_gp_fit_fused_f64": (_i, [
        _dp, _dp, _dp, _dp, _dp,  # X, y, theta, n_points, jitter_in
        _i, _i, _i, _i,  # T, N, D, kind
        _dp, _dp, _dp, _dp, _dp,  # L, alpha, quad, logdet, mll
        _dp, _dp, _dp, _u, c_void_p,  # info, jitter_used, Linv_diag, flags, stream
    ]),
    "scaml_fit_blocked_max_n": (_i, []),
    "scaml_fit_blocked_max_d": (_i, []),
    "scaml_gp_fit_blocked_workspace_bytes": (_ll, [_i, _i]),
    "scaml_gp_fit_blocked_f64": (_i, [
        _dp, _dp, _dp, _dp, _dp,  # X, y, theta, n_points, jitter_in
        _i, _i, _i, _i,  # T, N, D, kind
        _dp, _dp, _dp, _dp, _dp,  # L, alpha, quad, logdet, mll
        _dp, _dp, _dp, _u,  # info, jitter_used, Linv_diag, flags
        _dp, _ll, _dp,  # workspace, workspace_bytes, stream
    ]),
    "scaml_kernel_matrix_f64": (_i, [_dp, _dp, _dp, _i, _i, _i, _i, _i, _i, _i, _dp, c_void_p]),
    "scaml_potrf_batched_f64": (_i, [_dp, _dp, _dp, _dp, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _u, c_void_p]),
    "scaml_posterior_max_n": (_i, []),
    "scaml_posterior_batched_f64": (_i, [
        _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,  # Xq, X, theta, L, Linv_diag, alpha, y_mean, y_std, n_points
        _i, _i, _i, _i, _i,  # T, N, M, D, kind
        _dp, _dp, _dp, _u, c_void_p,  # mu, var, V, flags, stream
    ]),
    "scaml_posterior_cov_f64": (_i, [_dp, _dp, _dp, _dp, _i, _i, _i, _i, _i, _i, _dp, _u, c_void_p]),
    "scaml_linv_batched_f64": (_i, [_dp, _dp, _dp, _i, _i, _dp, c_void_p]),
    "scaml_linv_batched_lower_f64": (_i, [_dp, _dp, _dp, _i, _i, _dp, c_void_p]),
    "scaml_posterior_linv_f64": (_i, [
        _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,  # Xq, X, theta, Linv, alpha, y_mean, y_std, n_points
        _i, _i, _i, _i, _i,  # T, N, M, D, kind
        _dp, _dp, _dp, _u, c_void_p,  # mu, var, V, flags, stream
    ]),
    "scaml_cho_solve_batched_f64": (_i, [_dp, _dp, _dp, _dp, _i, _i, _i, _dp, c_void_p]),
    "scaml_solve_lt_batched_f64": (_i, [_dp, _dp, _dp, _dp, _i, _i, _i, _dp, c_void_p]),
    "scaml_weighted_task_sum_f64": (_i, [_dp, _dp, _dp, _i, _ll, _i, _dp, c_void_p]),
    "scaml_weighted_prior_reduce_f64": (_i, [_dp, _dp, _dp, _dp, _i, _i, _i, _dp, _dp, c_void_p]),
    "scaml_mll_backward_workspace_doubles": (_ll, [_i, _i, _i]),
    "scaml_mll_backward_f64": (_i, [_dp, _dp, _dp, _dp, _dp, _dp, _i, _i, _i, _i, _dp, _dp, c_void_p]),
    "scaml_posterior_linv_cov_f64": (_i, [_dp] * 9 + [_i] * 6 + [_dp, _dp, _dp, _u, c_void_p]),
    "scaml_target_assemble_f64": (_i, [_dp] * 6 + [_f, _f, _i, _i, _i, _i] + [_dp] * 5 + [c_void_p]),
    "scaml_target_finish_f64": (_i, [_dp] * 5 + [_f, _f, _f, _dp, _i, _i, _dp, _dp, c_void_p]),
    "scaml_posterior_linv_grad_f64": (_i, [_dp] * 10 + [_i] * 6 + [_dp, _dp, _dp, _u, c_void_p]),
    "scaml_target_posterior_grad_f64": (_i, [_dp] * 8 + [_f, _dp, _i, _i, _i, _i, _dp, _dp, c_void_p]),
    "scaml_target_fantasy_acqf_f64": (_i, [_dp] * 5 + [_f, _f, _f, _dp, _i, _f] + [_dp] * 6 + [_i] * 5 + [_dp, _dp, c_void_p]),
    "scaml_qacqf_max_q": (_i, []),
    "scaml_qacqf_max_samples": (_i, []),
    # (5g) (5d)'s arrays with VQ after VA; T, N, Mq, Ma, q, D, kind; mu, var, cov, flags
    "scaml_posterior_linv_grad_joint_f64": (_i, [_dp] * 11 + [_i] * 7 + [_dp, _dp, _dp, _u, c_void_p]),
    # (7p) Knq, Z, alpha, mean_q, var_q; m_all, s_all; info; cov_g, mu_g, var_g, Xt, Xq, theta, base_samples; acqf, acqf_param;
    # n, Mq, q, S, D, kind; value, grad, jitter_used, info_out
    "scaml_target_qacqf_f64": (_i, [_dp] * 5 + [_f, _f, _dp] + [_dp] * 7 + [_i, _f] + [_i] * 6 + [_dp] * 4 + [c_void_p]),
    # (7q) (7p)'s arrays, then Xp, Zp, mu_p, Sigma_pp; acqf, acqf_param; n, Mq, q, p, S, D, kind; value, grad, jitter_used, info_out
    "scaml_target_qacqf_pending_f64": (_i, [_dp] * 5 + [_f, _f, _dp] + [_dp] * 11 + [_i, _f] + [_i] * 7 + [_dp] * 4 + [c_void_p]),
    "scaml_qacqf_value_columns": (_i, [_i, _i]),
    # (5h) Xq, Xa, X, theta, Linv, alpha, y_mean, y_std, n_points, VA; T, N, Mp, Ma, B, q, D, kind; mu, var, cov, flags
    "scaml_posterior_linv_cov_joint_f64": (_i, [_dp] * 10 + [_i] * 8 + [_dp, _dp, _dp, _u, c_void_p]),
    # (7r) Knq, Z, alpha, mean_q, var_q; m_all, s_all; info; cov_s, Xq, theta, base_samples, Xp, Zp, mu_p, Sigma_pp; acqf, acqf_param;
    # n, Mp, B, q, p, S, D, kind; value, jitter_used, info_out
    "scaml_target_qacqf_value_f64": (_i, [_dp] * 5 + [_f, _f, _dp] + [_dp] * 8 + [_i, _f] + [_i] * 8 + [_dp] * 3 + [c_void_p]),
    # (7o) mu, var; acqf_param, M, acqf; A, Amu, Av
    "scaml_acqf_transform_f64": (_i, [_dp, _dp, _f, _i, _i, _dp, _dp, _dp, c_void_p]),
    # (5e) Xq, group, Xa, n_points_a, VA_tab, X, theta, Linv, alpha, y_mean, y_std, n_points; T, N, Mq, G, Ma_max, D, kind; mu, var, cov
    "scaml_posterior_linv_grad_grouped_f64": (_i, [_dp] * 12 + [_i] * 7 + [_dp, _dp, _dp, c_void_p]),
    # (5e') (5e)'s arrays and shapes; mu, var, cov; task_base, Tsrc
    "scaml_posterior_linv_grad_grouped_own_f64": (_i, [_dp] * 12 + [_i] * 7 + [_dp, _dp, _dp, _dp, _i, c_void_p]),
    # (7g) 17 arrays; Mq, G, n_max, T, D, kind, acqf; value, grad, mu_out, var_out
    "scaml_target_acqf_batched_f64": (_i, [_dp] * 17 + [_i] * 7 + [_dp] * 4 + [c_void_p]),
    # (5f), (5f') the value-only grouped pass: (5e)'s / (5e')'s argument lists, Mq candidates in strips of 16
    "scaml_posterior_linv_grouped_f64": (_i, [_dp] * 12 + [_i] * 7 + [_dp, _dp, _dp, c_void_p]),
    "scaml_posterior_linv_grouped_own_f64": (_i, [_dp] * 12 + [_i] * 7 + [_dp, _dp, _dp, _dp, _i, c_void_p]),
    # (7i) (7g)'s 17 arrays; Mq, G, n_max, T, D, kind, acqf; value, mu_out, var_out
    "scaml_target_score_batched_f64": (_i, [_dp] * 17 + [_i] * 7 + [_dp] * 3 + [c_void_p]),
    # (7j) means_t, covs_packed, X, y, n_points, m_all, s_all, w, active, theta; G, n_max, T, D, kind; Knn, resid
    "scaml_target_train_block_batched_f64": (_i, [_dp] * 10 + [_i] * 5 + [_dp, _dp, c_void_p]),
    "scaml_target_fit_max_n": (_i, [_i, _i]),
    "scaml_target_fit_max_d": (_i, []),
    "scaml_target_fit_workspace_doubles": (_ll, [_i, _i, _i, _i]),
    "scaml_target_mll_f64": (_i, [_dp] * 4 + [_f, _f, _host_spec, _dp] + [_i] * 5 + [_dp] * 4 + [c_void_p]),
    "scaml_target_fit_f64": (_i, [_dp] * 4 + [_f, _f, _host_spec, _dp] + [_i] * 7 + [_f, _f] + [_dp] * 5 + [_ll, c_void_p]),
    "scaml_target_fit_batched_workspace_doubles": (_ll, [_i, _i, _i, _i, _i]),
    # problem block: means_t, covs_packed, X, y, n_points, m_all, s_all (device), spec (host), z; S, B, n_max, T, D, kind
    "scaml_target_mll_batched_f64": (_i, [_dp] * 7 + [_host_spec, _dp] + [_i] * 6 + [_dp] * 4 + [c_void_p]),
    "scaml_target_fit_batched_f64": (_i, [_dp] * 7 + [_host_spec, _dp] + [_i] * 8 + [_f, _f] + [_dp] * 5 + [_ll, c_void_p]),
    "scaml_stack_fit_max_d": (_i, []),
    "scaml_stack_fit_workspace_bytes": (_ll, [_i, _i, _i, _i]),
    "scaml_stack_fit_f64": (_i, [_dp, _dp, _dp, _host_spec, _dp] + [_i] * 5 + [_u, _i, _i, _f, _f, _dp, _dp, _dp, _ll, c_void_p]),
    "scaml_studies_acqf_opt_max_d": (_i, []),
    "scaml_studies_acqf_opt_workspace_bytes": (_ll, [_i] * 6),
    # (7h) x0, group; 8 source-stack arrays (5e); 12 study arrays (7g); B, G, n_max, T, N, D, kind_s, kind_t, acqf; lo, hi; max_iter, history, max_ls;
    # gtol, ftol, c1; n_evals, flags; workspace, x, f, stats
    "scaml_studies_acqf_opt_f64": (_i, [_dp] * 22 + [_i] * 9 + [_dp, _dp] + [_i] * 3 + [_f] * 3 + [_i, _u] + [_dp] * 4 + [c_void_p]),
    # (7h') (7h)'s arguments; task_base, Tsrc
    "scaml_studies_acqf_opt_own_f64": (_i, [_dp] * 22 + [_i] * 9 + [_dp, _dp] + [_i] * 3 + [_f] * 3 + [_i, _u] + [_dp] * 4 + [_dp, _i, c_void_p]),
    # (7k) (7g)'s arrays with alpha_f, n_fant for alpha (18); Mq, G, n_max, F_max, T, D, kind, acqf; value, grad -- and (7i)'s likewise: value
    "scaml_target_fantasy_acqf_batched_f64": (_i, [_dp] * 18 + [_i] * 8 + [_dp] * 2 + [c_void_p]),
    "scaml_target_fantasy_score_batched_f64": (_i, [_dp] * 18 + [_i] * 8 + [_dp] + [c_void_p]),
    # (7l) (7h)'s arguments with alpha_f, n_fant for alpha_t and F_max after n_max; task_base (or NULL), Tsrc
    "scaml_studies_fantasy_acqf_opt_f64": (_i, [_dp] * 23 + [_i] * 10 + [_dp, _dp] + [_i] * 3 + [_f] * 3 + [_i, _u] + [_dp] * 4
                                           + [_dp, _i, c_void_p]),
    # (7m) mu, cov, strip_base, w, active, Xt, theta, y, n_points, n_obs, m_all, s_all; Mq, G, n_max, T, D, kind; Knn, resid, mean_p
    "scaml_studies_condition_block_f64": (_i, [_dp] * 12 + [_i] * 6 + [_dp] * 3 + [c_void_p]),
    # (7n) L, resid, mean_p, n_points, n_obs, info, eps, n_fant, m_all, s_all; G, n_max, p_max, F_max; alpha_f, y_fant, mu_p
    "scaml_studies_fantasy_condition_f64": (_i, [_dp] * 10 + [_i] * 4 + [_dp] * 3 + [c_void_p]),
    "scaml_qacqf_opt_max_p": (_i, []),
    "scaml_qacqf_opt_step_workspace_bytes": (_ll, [_i] * 3),
    "scaml_qacqf_opt_workspace_bytes": (_ll, [_i] * 8),
    # (7t) value, grad, slots, x0, lo, hi; B, Bs, P, mode, max_iter, history, max_ls; gtol, ftol, c1; state, Xq, x, f, stats
    "scaml_qacqf_opt_step_f64": (_i, [_dp] * 6 + [_i] * 7 + [_f] * 3 + [_dp] * 5 + [c_void_p]),
    # (7s) x0, slots; Xa, 8 source-stack arrays, VA; w, active; mu_t, cov_tt, var_t; Xt, theta_t, targets, L, Linv_diag, alpha_t; m_all, s_all;
    # info, base_samples, Xp, Zp, mu_p, Sigma_pp; B, Bs, n, p, q, S, T, N, D, kind_s, kind_t, acqf; acqf_param; lo, hi; max_iter, history, max_ls;
    # gtol, ftol, c1; n_evals, flags; workspace, workspace_bytes; x, f, stats
    "scaml_qacqf_opt_f64": (_i, [_dp] * 22 + [_f, _f] + [_dp] * 6 + [_i] * 12 + [_f] + [_dp, _dp] + [_i] * 3 + [_f] * 3 + [_i, _u]
                            + [_dp, _ll] + [_dp] * 3 + [c_void_p]),
    "scaml_debug_target_fit_path": (_i, [_i]),
    "scaml_debug_blocked_fit_path": (_i, [_i]),
    "scaml_debug_coop_far": (_i, [_i]),
    "scaml_debug_force_two_launch_grad": (_i, [_i]),
    "scaml_debug_grouped_ordered_sums": (_i, [_i]),
    "scaml_debug_set_stamp_buffer": (_i, [c_void_p]),
}

# Every symbol include/scaml_gp.h declares; tests check the built library exports them all.
EXPORTED_SYMBOLS = tuple(name for name in SIGNATURES if not name.startswith("scaml_debug_"))


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ScamlLibraryError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run __graft_entry__.build()); there is no CPU fallback for the GP hot path."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


lib = _load()


def check_rc(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc == E_BADARG:
        raise ValueError(f"{what}: bad argument")
    if rc == E_TOOLARGE:
        raise ValueError(f"{what}: problem size exceeds kernel limits")
    msg = lib.scaml_last_error().decode("utf-8", "replace")
    raise RuntimeError(f"{what}: HIP launch failed ({msg})")
