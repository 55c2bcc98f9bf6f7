"""Torch-tensor front end of the C ABI (device memory, streams; no arithmetic here).

Every function takes CUDA(=HIP) fp64 tensors, passes raw device pointers plus the current
stream to libscaml_hip.so and returns freshly allocated output tensors.  Nothing is
synchronised; ``info`` tensors stay on the device until the caller inspects them.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib
from ._lib import KIND_MATERN52, KIND_RBF  # noqa: F401  (re-export)


class NotPSDError(RuntimeError):
    """Cholesky failed for at least one task even after the jitter escalation
    (mirrors linear_operator.utils.errors.NotPSDError, a RuntimeError the reference
    catches at scamlgp/utils.py:180,193)."""


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _check(t: torch.Tensor, name: str, shape=None, dtype=torch.float64) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); the GP hot path has no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)} (got {tuple(t.shape)})")
    return t.contiguous()


def _opt(t: Optional[torch.Tensor], name: str, shape=None, dtype=torch.float64) -> Optional[torch.Tensor]:
    return None if t is None else _check(t, name, shape, dtype)


def _empty(dev, *shape, dtype=torch.float64) -> torch.Tensor:
    return torch.empty(shape, dtype=dtype, device=dev)


def _stream_handle() -> int:
    return torch.cuda.current_stream().cuda_stream


def fit_max_n() -> int:
    """Largest N the single-launch fused fit takes (scaml_fit_max_n)."""
    return int(_lib.lib.scaml_fit_max_n())


def gp_fit_fused(
    X: torch.Tensor,
    y: torch.Tensor,
    theta: torch.Tensor,
    kind: int,
    n_points: Optional[torch.Tensor] = None,
    jitter: Optional[torch.Tensor] = None,
    store_L: bool = True,
    zero_upper: bool = True,
    retry: bool = True,
    want_alpha: bool = True,
    want_linv: bool = False,
    out: Optional[Dict[str, torch.Tensor]] = None,
) -> Dict[str, torch.Tensor]:
    """K + noise, jittered Cholesky, alpha, quad, logdet, MLL for a stack of tasks.

    X (T, N, D), y (T, N), theta (T, D+2) = [lengthscales, outputscale, noise] (constrained).
    Returns dict(L, alpha, quad, logdet, mll, info, jitter, Linv_diag); ``L`` is None when
    store_L=False, ``Linv_diag`` (T, ceil(N/16), 16, 16) only with want_linv=True.
    One launch of ``scaml_gp_fit_fused_f64`` (include/scaml_gp.h).  ``out`` may be the dict a
    previous call returned for the same shapes/flags: its tensors are reused (no allocation).
    """
    if X.dim() != 3:
        raise ValueError("X must be (T, N, D)")
    T, N, D = X.shape
    X = _check(X, "X")
    y = _check(y, "y", (T, N))
    theta = _check(theta, "theta", (T, D + 2))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    jitter = _opt(jitter, "jitter", (T,))
    if N > _lib.lib.scaml_fit_max_n():
        if out is not None:
            raise ValueError("out= is not supported beyond scaml_fit_max_n()")
        if N <= _lib.lib.scaml_fit_blocked_max_n() and N % 16 == 0 and D <= _lib.lib.scaml_fit_blocked_max_d() and not _FORCE_COMPOSED_TWO_BLOCK:
            return _gp_fit_blocked(X, y, theta, kind, n_points, jitter, zero_upper, retry)
        return _gp_fit_two_block(X, y, theta, kind, n_points, jitter, store_L, retry)
    dev = X.device
    with torch.cuda.device(dev):
        if out is not None:
            L, alpha, quad, logdet, mll, info, jit_used = (out[k] for k in ("L", "alpha", "quad", "logdet", "mll", "info", "jitter"))
            linv = out.get("Linv_diag")
            if want_linv and linv is None:
                raise ValueError("out= has no Linv_diag buffer but want_linv=True")
            if not want_linv:
                linv = None
            if (L is None) == store_L or (alpha is None) == want_alpha or quad.shape != (T,) or (store_L and L.shape != (T, N, N)):
                raise ValueError("out= does not match this call's shapes/flags")
        else:
            L = _empty(dev, T, N, N) if store_L else None
            alpha = _empty(dev, T, N) if want_alpha else None
            quad = _empty(dev, T)
            logdet = _empty(dev, T)
            mll = _empty(dev, T)
            info = _empty(dev, T, dtype=torch.int32)
            jit_used = _empty(dev, T)
            linv = _empty(dev, T, (N + 15) // 16, 16, 16) if want_linv else None
        if n_points is not None and want_alpha:
            alpha.zero_()
        flags = 0
        if store_L:
            flags |= _lib.FIT_STORE_L
            if zero_upper:
                flags |= _lib.FIT_ZERO_UPPER
            if n_points is not None:
                L.zero_()
        if not retry:
            flags |= _lib.FIT_NO_RETRY
        rc = _lib.lib.scaml_gp_fit_fused_f64(
            _ptr(X), _ptr(y), _ptr(theta), _ptr(n_points), _ptr(jitter),
            T, N, D, int(kind),
            _ptr(L), _ptr(alpha), _ptr(quad), _ptr(logdet), _ptr(mll),
            _ptr(info), _ptr(jit_used), _ptr(linv), flags, _stream_handle(),
        )
    _lib.check_rc(rc, "scaml_gp_fit_fused_f64")
    return dict(L=L, alpha=alpha, quad=quad, logdet=logdet, mll=mll, info=info, jitter=jit_used, Linv_diag=linv)


_FORCE_COMPOSED_TWO_BLOCK = False   # tests / A-B timing: route 256 < N <= 512 through _gp_fit_two_block


def _gp_fit_blocked(X, y, theta, kind, n_points, jitter, zero_upper, retry) -> Dict[str, torch.Tensor]:
    """Fused fit for scaml_fit_max_n() < N <= scaml_fit_blocked_max_n() (the N = 512 source tasks of BASELINE
    configs[4]): ``scaml_gp_fit_blocked_f64`` -- by shape, ONE launch with several CUs per task (csrc/gp_fit_coop.hip; stacks that
    leave CUs idle) or a 2 x 2 block factorisation enqueued as one sequence of the library's launches (csrc/gp_fit_blocked.hip);
    jitter ladder included, without a host synchronisation or a framework op in between.  L and Linv_diag are always produced."""
    T, N, D = X.shape
    dev = X.device
    with torch.cuda.device(dev):
        # ragged stacks: rows past n_t are never written but READ by the strip solve -> zeros
        L = (torch.zeros if n_points is not None else torch.empty)((T, N, N), dtype=torch.float64, device=dev)
        alpha = (torch.zeros if n_points is not None else torch.empty)((T, N), dtype=torch.float64, device=dev)
        quad, logdet, mll, jit_used = (_empty(dev, T) for _ in range(4))
        info = _empty(dev, T, dtype=torch.int32)
        linv = _empty(dev, T, N // 16, 16, 16)
        nbytes = int(_lib.lib.scaml_gp_fit_blocked_workspace_bytes(T, N))
        ws = _empty(dev, max(nbytes, 16), dtype=torch.uint8)
        flags = _lib.FIT_STORE_L | (_lib.FIT_ZERO_UPPER if zero_upper else 0) | (0 if retry else _lib.FIT_NO_RETRY)
        rc = _lib.lib.scaml_gp_fit_blocked_f64(
            _ptr(X), _ptr(y), _ptr(theta), _ptr(n_points), _ptr(jitter), T, N, D, int(kind),
            _ptr(L), _ptr(alpha), _ptr(quad), _ptr(logdet), _ptr(mll), _ptr(info), _ptr(jit_used), _ptr(linv), flags,
            _ptr(ws), nbytes, _stream_handle())
        ws.record_stream(torch.cuda.current_stream(dev))
    _lib.check_rc(rc, "scaml_gp_fit_blocked_f64")
    return dict(L=L, alpha=alpha, quad=quad, logdet=logdet, mll=mll, info=info, jitter=jit_used, Linv_diag=linv)


_JITTER_LADDER = (1e-8, 1e-7, 1e-6)  # psd_safe_cholesky's escalation


def _gp_fit_two_block(X, y, theta, kind, n_points, jitter, store_L, retry) -> Dict[str, torch.Tensor]:
    """Fused fit for scaml_fit_max_n() < N <= 2 * scaml_fit_max_n() (the N = 512 source tasks of
    BASELINE config 5) as a 2 x 2 block factorisation composed from the library's own launches:

        [K11 K12]   [L11      ] [L11^T  V  ]      L11 = fused fit of block 1 (register-resident kernel)
        [K21 K22] = [V^T   L22] [      L22^T]     V   = L11^-1 K12          (scaml_posterior_batched_f64)
                                                  S   = K22 - V^T V          (scaml_posterior_cov_f64)
                                                  L22 = chol(S + noise I)    (scaml_potrf_batched_f64)

    The posterior of block 1 at the points of block 2 is exactly the conditional the Schur complement
    needs: alpha_2 = S^-1 (y_2 - K21 K11^-1 y_1) falls out of the POTRF's solve, and
    alpha_1 = alpha_1' - K11^-1 K12 alpha_2 = alpha_1' - L11^-T (V alpha_2) (scaml_solve_lt_batched_f64).
    quad and logdet add over the blocks.  The jitter ladder is driven from the host here (one
    status read per attempt; every attempt is single-shot in the kernels) so that, like
    psd_safe_cholesky, one jitter value applies to the whole matrix of a failing task only.
    Torch is used for slicing/concatenation only.
    """
    T, N, D = X.shape
    N1 = _lib.lib.scaml_fit_max_n()
    if N > 2 * N1:
        raise ValueError(f"N = {N} exceeds the supported {2 * N1} points per task")
    N2 = N - N1
    dev = X.device
    X1, X2 = X[:, :N1].contiguous(), X[:, N1:].contiguous()
    y1, y2 = y[:, :N1].contiguous(), y[:, N1:].contiguous()
    n1 = n2 = None
    if n_points is not None:
        n1 = n_points.clamp(max=N1).to(torch.int32)
        n2 = (n_points - N1).clamp(min=0).to(torch.int32)
    noise = theta[:, D + 1].contiguous()
    jit = torch.zeros((T,), dtype=torch.float64, device=dev)
    base = jitter if jitter is not None else torch.zeros((T,), dtype=torch.float64, device=dev)
    for step in range(len(_JITTER_LADDER) + 1):
        f1 = gp_fit_fused(X1, y1, theta, kind, n_points=n1, jitter=base + jit, retry=False, want_linv=True)
        p12 = source_posteriors(X2, X1, theta, kind, f1["L"], f1["Linv_diag"], f1["alpha"], n_points=n1,
                                want_var=False, cov_first=N2, keep_V=True)
        f2 = potrf_batched(p12["cov"], y2 - p12["mean"], n_points=n2, jitter=noise + base + jit, retry=False,
                           want_linv=True)
        info = torch.where(f1["info"] > 0, f1["info"], torch.where(f2["info"] > 0, f2["info"] + N1, f2["info"]))
        failed = info > 0
        if not retry or step == len(_JITTER_LADDER) or not bool(failed.any()):
            break
        jit = torch.where(failed, torch.full_like(jit, _JITTER_LADDER[step]), jit)
    # K11^-1 K12 alpha_2 = L11^-T (V alpha_2) with the V = L11^-1 K12 the Schur complement was formed from: a
    # mat-vec and the backward half of a Cholesky solve (alpha_2 is zero past n2, so V's padded columns drop out)
    u = cho_solve(f1["L"], f1["Linv_diag"], torch.bmm(p12["V"], f2["alpha"].unsqueeze(-1)), n_points=n1, backward_only=True).squeeze(-1)
    alpha = torch.cat([f1["alpha"] - u, f2["alpha"]], 1)
    quad = f1["quad"] + f2["quad"]
    logdet = f1["logdet"] + f2["logdet"]
    n = n_points.to(torch.float64) if n_points is not None else torch.full((T,), float(N), dtype=torch.float64, device=dev)
    mll = -(quad + logdet + n * 1.8378770664093453) / (2.0 * n.clamp_min(1.0))
    L = None
    if store_L:
        L = torch.zeros((T, N, N), dtype=torch.float64, device=dev)
        L[:, :N1, :N1] = f1["L"]
        Vt = p12["V"].transpose(1, 2)
        if n2 is not None:
            Vt = Vt * (torch.arange(N2, device=dev)[None, :, None] < n2[:, None, None])
        L[:, N1:, :N1] = Vt
        L[:, N1:, N1:] = f2["L"]
    linv = torch.cat([f1["Linv_diag"], f2["Linv_diag"]], 1)
    return dict(L=L, alpha=alpha, quad=quad, logdet=logdet, mll=mll, info=info.to(torch.int32), jitter=jit, Linv_diag=linv)


def linv_batched(L: torch.Tensor, Linv_diag: torch.Tensor, n_points: Optional[torch.Tensor] = None, lower_only: bool = False) -> torch.Tensor:
    """L^-1 (T, N, N) of the factors of a fused fit (zero above the diagonal).  scaml_linv_batched_f64; ``lower_only``:
    scaml_linv_batched_lower_f64 -- the block rows above each strip's diagonal block are left unwritten (no kernel of the library
    reads them; the result is then NOT a dense matrix to multiply with)."""
    T, N, _ = L.shape
    L = _check(L, "L", (T, N, N))
    Linv_diag = _check(Linv_diag, "Linv_diag", (T, (N + 15) // 16, 16, 16))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    out = torch.empty_like(L)
    with torch.cuda.device(L.device):
        fn = _lib.lib.scaml_linv_batched_lower_f64 if lower_only else _lib.lib.scaml_linv_batched_f64
        rc = fn(_ptr(L), _ptr(Linv_diag), _ptr(n_points), T, N, _ptr(out), _stream_handle())
    _lib.check_rc(rc, "scaml_linv_batched_f64")
    return out


def cho_solve(L: torch.Tensor, Linv_diag: torch.Tensor, B: torch.Tensor, n_points: Optional[torch.Tensor] = None,
              backward_only: bool = False) -> torch.Tensor:
    """(L L^T)^-1 B for B (T, N, R) with the factors of a fused fit (scaml_cho_solve_batched_f64), or, with
    backward_only, L^-T B (scaml_solve_lt_batched_f64)."""
    T, N, _ = L.shape
    R = B.shape[-1]
    L = _check(L, "L", (T, N, N))
    Linv_diag = _check(Linv_diag, "Linv_diag", (T, (N + 15) // 16, 16, 16))
    B = _check(B, "B", (T, N, R))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    out = torch.empty_like(B)
    with torch.cuda.device(L.device):
        fn = _lib.lib.scaml_solve_lt_batched_f64 if backward_only else _lib.lib.scaml_cho_solve_batched_f64
        rc = fn(_ptr(L), _ptr(Linv_diag), _ptr(B), _ptr(n_points), T, N, R, _ptr(out), _stream_handle())
    _lib.check_rc(rc, "scaml_solve_lt_batched_f64" if backward_only else "scaml_cho_solve_batched_f64")
    return out


def kernel_matrix(X1: torch.Tensor, theta: torch.Tensor, kind: int, X2: Optional[torch.Tensor] = None,
                  add_noise: bool = False) -> torch.Tensor:
    """K (T, N1, N2) = os k(X1 / l, X2 / l).  X2 None: square training matrix (optionally + noise I);
    X2 (N2, D): one query set shared by all tasks; X2 (T, N2, D): per-task.  scaml_kernel_matrix_f64."""
    T, N1, D = X1.shape
    X1 = _check(X1, "X1")
    theta = _check(theta, "theta", (T, D + 2))
    shared = 0
    N2 = N1
    if X2 is not None:
        shared = 1 if X2.dim() == 2 else 0
        N2 = X2.shape[-2]
        X2 = _check(X2, "X2", (N2, D) if shared else (T, N2, D))
    K = _empty(X1.device, T, N1, N2)
    with torch.cuda.device(X1.device):
        rc = _lib.lib.scaml_kernel_matrix_f64(_ptr(X1), _ptr(X2), _ptr(theta), T, N1, N2, D, int(kind), shared,
                                              1 if add_noise else 0, _ptr(K), _stream_handle())
    _lib.check_rc(rc, "scaml_kernel_matrix_f64")
    return K


def potrf_batched(A: torch.Tensor, y: Optional[torch.Tensor] = None, n_points: Optional[torch.Tensor] = None,
                  jitter: Optional[torch.Tensor] = None, zero_upper: bool = True, retry: bool = True,
                  want_linv: bool = False) -> Dict[str, torch.Tensor]:
    """Jittered Cholesky of a stack of given SPD matrices A (T, N, N) (+ optional solve with y (T, N)).
    Returns dict(L, alpha, quad, logdet, info, jitter, Linv_diag).  scaml_potrf_batched_f64."""
    if A.dim() != 3 or A.shape[1] != A.shape[2]:
        raise ValueError("A must be (T, N, N)")
    T, N, _ = A.shape
    A = _check(A, "A")
    y = _opt(y, "y", (T, N))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    jitter = _opt(jitter, "jitter", (T,))
    dev = A.device
    with torch.cuda.device(dev):
        L = torch.zeros((T, N, N), dtype=torch.float64, device=dev) if n_points is not None else _empty(dev, T, N, N)
        alpha = torch.zeros((T, N), dtype=torch.float64, device=dev) if y is not None else None
        quad = _empty(dev, T) if y is not None else None
        logdet = _empty(dev, T)
        info = _empty(dev, T, dtype=torch.int32)
        jit_used = _empty(dev, T)
        linv = _empty(dev, T, (N + 15) // 16, 16, 16) if want_linv else None
        flags = _lib.FIT_STORE_L | (_lib.FIT_ZERO_UPPER if zero_upper else 0) | (0 if retry else _lib.FIT_NO_RETRY)
        rc = _lib.lib.scaml_potrf_batched_f64(_ptr(A), _ptr(y), _ptr(n_points), _ptr(jitter), T, N, _ptr(L), _ptr(alpha),
                                              _ptr(quad), _ptr(logdet), _ptr(info), _ptr(jit_used), _ptr(linv), flags,
                                              _stream_handle())
    _lib.check_rc(rc, "scaml_potrf_batched_f64")
    return dict(L=L, alpha=alpha, quad=quad, logdet=logdet, info=info, jitter=jit_used, Linv_diag=linv)


def source_posteriors(
    Xq: torch.Tensor,
    X: torch.Tensor,
    theta: torch.Tensor,
    kind: int,
    L: torch.Tensor,
    Linv_diag: torch.Tensor,
    alpha: torch.Tensor,
    y_mean: Optional[torch.Tensor] = None,
    y_std: Optional[torch.Tensor] = None,
    n_points: Optional[torch.Tensor] = None,
    want_var: bool = True,
    cov_first: int = 0,
    keep_V: bool = False,
    mean_only: bool = False,
    Linv: Optional[torch.Tensor] = None,
    VA: Optional[torch.Tensor] = None,
) -> Dict[str, torch.Tensor]:
    """Posteriors of all source GPs at the shared query points Xq (M, D), or at per-task query sets
    Xq (T, M, D).  ``mean_only`` skips the triangular solve (mu = m + s K_* alpha only; L and
    Linv_diag may be None); ``keep_V`` also returns V = L^-1 K_*^T (T, N, M).  With ``Linv`` (T, N, N) from
    ``linv_batched`` the posteriors come from the explicit inverse factor (scaml_posterior_linv_f64: a
    triangular matrix product instead of a substitution -- the fast path when one fit serves many queries).
    ``VA`` (T, N, cov_first): the V of the leading ``cov_first`` query points from an earlier call (``keep_V=True`` on those points
    alone) -- the fused covariance pass then skips recomputing it (the leading points are a model's fixed training inputs).

    Returns dict(mean (T, M), var (T, M) or None, cov (T, cov_first, M) or None): ``cov`` is the
    posterior covariance between the first ``cov_first`` query points and all of them (put the
    target's training points first to get Sigma_nn and Sigma_nq in one go).  Un-standardised with
    y_mean / y_std (T) when given.  Launches scaml_posterior_batched_f64 (+ scaml_posterior_cov_f64).
    """
    if X.dim() != 3 or Xq.dim() not in (2, 3):
        raise ValueError("X must be (T, N, D) and Xq (M, D) or (T, M, D)")
    T, N, D = X.shape
    M = Xq.shape[-2]
    if Xq.shape[-1] != D:
        raise ValueError("Xq and X disagree on D")
    flags = 0
    X = _check(X, "X")
    if Xq.dim() == 3:
        Xq = _check(Xq, "Xq", (T, M, D))
        flags |= _lib.POST_XQ_PER_TASK
    else:
        Xq = _check(Xq, "Xq")
    theta = _check(theta, "theta", (T, D + 2))
    if mean_only:
        flags |= _lib.POST_MEAN_ONLY
        want_var, cov_first, keep_V, L, Linv_diag = False, 0, False, None, None
    elif Linv is None:
        L = _check(L, "L", (T, N, N))
        Linv_diag = _check(Linv_diag, "Linv_diag", (T, (N + 15) // 16, 16, 16))
    alpha = _check(alpha, "alpha", (T, N))
    y_mean = _opt(y_mean, "y_mean", (T,))
    y_std = _opt(y_std, "y_std", (T,))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    if not 0 <= cov_first <= M:
        raise ValueError("cov_first must be within [0, M]")
    dev = X.device
    with torch.cuda.device(dev):
        mu = _empty(dev, T, M)
        var = _empty(dev, T, M) if want_var else None
        fused_cov = (Linv is not None and not mean_only and not keep_V and 0 < cov_first <= min(96, N, M))
        V = _empty(dev, T, N, M) if ((cov_first > 0 and not fused_cov) or keep_V) else None
        cov = None
        if fused_cov:
            # the covariance block comes out of the posterior pass itself: V of the leading cov_first points first
            # (T, N, cov_first -- small), then one pass over all M points gives mean, var and cov; V (T, N, M) is never stored
            Linv = _check(Linv, "Linv", (T, N, N))
            if VA is not None:
                VA = _check(VA, "VA", (T, N, cov_first))
            else:
                Xa = Xq[:, :cov_first].contiguous() if Xq.dim() == 3 else Xq[:cov_first].contiguous()
                VA = _empty(dev, T, N, cov_first)
                mu_a = _empty(dev, T, cov_first)
                rc = _lib.lib.scaml_posterior_linv_f64(
                    _ptr(Xa), _ptr(X), _ptr(theta), _ptr(Linv), _ptr(alpha), _ptr(y_mean), _ptr(y_std), _ptr(n_points),
                    T, N, cov_first, D, int(kind), _ptr(mu_a), None, _ptr(VA), flags, _stream_handle())
                _lib.check_rc(rc, "scaml_posterior_linv_f64")
            cov = _empty(dev, T, cov_first, M)
            if var is None:
                var = _empty(dev, T, M)
            rc = _lib.lib.scaml_posterior_linv_cov_f64(
                _ptr(Xq), _ptr(X), _ptr(theta), _ptr(Linv), _ptr(alpha), _ptr(y_mean), _ptr(y_std), _ptr(n_points), _ptr(VA),
                T, N, M, cov_first, D, int(kind), _ptr(mu), _ptr(var), _ptr(cov), flags, _stream_handle())
            _lib.check_rc(rc, "scaml_posterior_linv_cov_f64")
            return dict(mean=mu, var=var if want_var else None, cov=cov, V=None)
        if Linv is not None and not mean_only:
            Linv = _check(Linv, "Linv", (T, N, N))
            rc = _lib.lib.scaml_posterior_linv_f64(
                _ptr(Xq), _ptr(X), _ptr(theta), _ptr(Linv), _ptr(alpha), _ptr(y_mean), _ptr(y_std), _ptr(n_points),
                T, N, M, D, int(kind), _ptr(mu), _ptr(var), _ptr(V), flags, _stream_handle())
            _lib.check_rc(rc, "scaml_posterior_linv_f64")
        else:
            rc = _lib.lib.scaml_posterior_batched_f64(
            _ptr(Xq), _ptr(X), _ptr(theta), _ptr(L), _ptr(Linv_diag), _ptr(alpha), _ptr(y_mean), _ptr(y_std),
                _ptr(n_points), T, N, M, D, int(kind), _ptr(mu), _ptr(var), _ptr(V), flags, _stream_handle())
            _lib.check_rc(rc, "scaml_posterior_batched_f64")
        if cov_first > 0:
            cov = _empty(dev, T, cov_first, M)
            rc = _lib.lib.scaml_posterior_cov_f64(_ptr(Xq), _ptr(theta), _ptr(V), _ptr(y_std), T, N, M, cov_first, D,
                                                  int(kind), _ptr(cov), flags & _lib.POST_XQ_PER_TASK, _stream_handle())
            _lib.check_rc(rc, "scaml_posterior_cov_f64")
    return dict(mean=mu, var=var, cov=cov, V=V if keep_V else None)


def weighted_task_sum(values: torch.Tensor, weights: torch.Tensor, power: int = 1,
                      active: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_t w_t^power * values[t] over the task axis (dim 0), optionally only over active tasks
    (bool mask, scamlgp/model.py:368-372).  Launches scaml_weighted_task_sum_f64."""
    T = values.shape[0]
    values = _check(values, "values")
    weights = _check(weights, "weights", (T,))
    if active is not None:
        if not active.is_cuda or active.shape != (T,):
            raise ValueError("active must be a (T,) GPU tensor")
        active = active.to(torch.uint8).contiguous()
    out = torch.empty(values.shape[1:], dtype=torch.float64, device=values.device)
    with torch.cuda.device(values.device):
        rc = _lib.lib.scaml_weighted_task_sum_f64(_ptr(values), _ptr(weights), _ptr(active), T, out.numel(), int(power),
                                                  _ptr(out), _stream_handle())
    _lib.check_rc(rc, "scaml_weighted_task_sum_f64")
    return out


def weighted_prior_reduce(mu: Optional[torch.Tensor], cov: Optional[torch.Tensor], weights: torch.Tensor,
                          active: Optional[torch.Tensor] = None):
    """Target prior of scamlgp/model.py:108-135 from stacked source posteriors: (sum_t w_t mu[t], sum_t w_t^2 cov[t])
    over the active tasks.  mu (T, M), cov (T, Ma, M); either may be None.  scaml_weighted_prior_reduce_f64."""
    T = weights.shape[0]
    weights = _check(weights, "weights", (T,))
    M = mu.shape[1] if mu is not None else cov.shape[2]
    Ma = cov.shape[1] if cov is not None else 0
    if mu is not None:
        mu = _check(mu, "mu", (T, M))
    if cov is not None:
        cov = _check(cov, "cov", (T, Ma, M))
    if active is not None:
        active = active.to(torch.uint8).contiguous()
    dev = weights.device
    mu_s = _empty(dev, M) if mu is not None else None
    cov_s = _empty(dev, Ma, M) if cov is not None else None
    with torch.cuda.device(dev):
        rc = _lib.lib.scaml_weighted_prior_reduce_f64(_ptr(mu), _ptr(cov), _ptr(weights), _ptr(active), T, M, Ma, _ptr(mu_s),
                                                      _ptr(cov_s), _stream_handle())
    _lib.check_rc(rc, "scaml_weighted_prior_reduce_f64")
    return mu_s, cov_s


def target_posterior(cov_s: torch.Tensor, mean_s: torch.Tensor, var_s: torch.Tensor, Xall: torch.Tensor, theta: torch.Tensor,
                     train_targets: torch.Tensor, m_all: float, s_all: float, kind: int, observation_noise: bool = False,
                     factor: Optional[Dict[str, torch.Tensor]] = None):
    """Posterior mean / variance (original units) of the ScaML-GP target GP at the M query points behind the n training
    points in ``Xall`` (n + M, D), from the weighted source sums at the same points: cov_s (n, n + M), mean_s, var_s
    (n + M).  scaml_target_assemble_f64 -> scaml_potrf_batched_f64 (T = 1, jitter ladder) -> scaml_cho_solve_batched_f64
    -> scaml_target_finish_f64: four launches, no host synchronisation.  A factorisation that fails even with jitter shows as NaN
    in mu / var (the status stays on the device).  Returns (mu (M,), var (M,), info (1,), jitter (1,))."""
    f = target_posterior_full(cov_s, mean_s, var_s, Xall, theta, train_targets, m_all, s_all, kind, observation_noise, factor)
    return f["mu"], f["var"], f["info"], f["jitter"]


def target_posterior_full(cov_s: torch.Tensor, mean_s: torch.Tensor, var_s: torch.Tensor, Xall: torch.Tensor, theta: torch.Tensor,
                          train_targets: torch.Tensor, m_all: float, s_all: float, kind: int, observation_noise: bool = False,
                          factor: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """``target_posterior`` with its intermediates: dict(mu, var, info, jitter, alpha (n,) = Knn^-1 resid, Z (n, M) = Knn^-1 Knq,
    factor) -- alpha and Z are what the input gradient of the posterior contracts against (``target_posterior_grad``).  ``factor``:
    the ``factor`` entry of an earlier call with the SAME training block (cov_s[:, :n], mean_s[:n], theta, targets): the jittered
    Cholesky of Knn is then reused instead of recomputed -- it does not depend on the query points (an acquisition optimisation
    evaluates hundreds of query batches against one factor)."""
    n = int(train_targets.shape[0])
    W, D = Xall.shape
    M = W - n
    if not 1 <= n <= _lib.lib.scaml_fit_max_n():
        raise ValueError(f"target_posterior takes 1 <= n <= {_lib.lib.scaml_fit_max_n()} training points")
    cov_s = _check(cov_s, "cov_s", (n, W))
    mean_s = _check(mean_s, "mean_s", (W,))
    var_s = _check(var_s, "var_s", (W,))
    Xall = _check(Xall, "Xall")
    theta = _check(theta, "theta", (D + 2,))
    train_targets = _check(train_targets, "train_targets", (n,))
    dev = Xall.device
    with torch.cuda.device(dev):
        Knn, resid = _empty(dev, 1, n, n), _empty(dev, 1, n)
        Knq, mean_q, var_q = _empty(dev, 1, n, M), _empty(dev, M), _empty(dev, M)
        rc = _lib.lib.scaml_target_assemble_f64(_ptr(cov_s), _ptr(mean_s), _ptr(var_s), _ptr(Xall), _ptr(theta), _ptr(train_targets),
                                                float(m_all), float(s_all), n, M, D, int(kind), _ptr(Knn), _ptr(resid), _ptr(Knq),
                                                _ptr(mean_q), _ptr(var_q), _stream_handle())
        _lib.check_rc(rc, "scaml_target_assemble_f64")
        f = factor if factor is not None else potrf_batched(Knn, resid, want_linv=True)
        mu, var = _empty(dev, M), _empty(dev, M)
        Z = None
        if M > 0:
            Z = cho_solve(f["L"], f["Linv_diag"], Knq)
            rc = _lib.lib.scaml_target_finish_f64(_ptr(Knq), _ptr(Z), _ptr(f["alpha"]), _ptr(mean_q), _ptr(var_q), float(m_all), float(s_all),
                                                  float(theta[D + 1]) if observation_noise else 0.0, _ptr(f["info"]), n, M, _ptr(mu), _ptr(var),
                                                  _stream_handle())
            _lib.check_rc(rc, "scaml_target_finish_f64")
    return dict(mu=mu, var=var, info=f["info"], jitter=f["jitter"], alpha=f["alpha"][0], Z=None if Z is None else Z[0], factor=f)


def source_posteriors_grad(Xq: torch.Tensor, Xa: Optional[torch.Tensor], X: torch.Tensor, theta: torch.Tensor, kind: int, Linv: torch.Tensor,
                           alpha: torch.Tensor, y_mean: Optional[torch.Tensor] = None, y_std: Optional[torch.Tensor] = None,
                           n_points: Optional[torch.Tensor] = None, VA: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Source posteriors at Xq (Mq, D) WITH their input gradients, one launch of scaml_posterior_linv_grad_f64: dict(mu (T, Mq, 16),
    var (T, Mq, 16), cov (T, Ma, Mq * 16) or None); column 0 of each 16-block is the value, columns 1 .. D the derivative w.r.t.
    x_0 .. x_{D-1}.  Xa (Ma, D), VA (T, N, Ma): the leading points of the covariance block (the target's training inputs) and their
    V = L^-1 K(X, Xa) from ``source_posteriors(..., keep_V=True)``."""
    T, N, D = X.shape
    Mq = Xq.shape[0]
    X = _check(X, "X")
    Xq = _check(Xq, "Xq", (Mq, D))
    theta = _check(theta, "theta", (T, D + 2))
    Linv = _check(Linv, "Linv", (T, N, N))
    alpha = _check(alpha, "alpha", (T, N))
    Ma = 0 if VA is None else int(VA.shape[-1])
    if Ma:
        VA = _check(VA, "VA", (T, N, Ma))
        Xa = _check(Xa, "Xa", (Ma, D))
    y_mean = _opt(y_mean, "y_mean", (T,))
    y_std = _opt(y_std, "y_std", (T,))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    dev = X.device
    with torch.cuda.device(dev):
        mu = _empty(dev, T, Mq, 16)
        var = _empty(dev, T, Mq, 16)
        cov = _empty(dev, T, Ma, Mq * 16) if Ma else None
        rc = _lib.lib.scaml_posterior_linv_grad_f64(_ptr(Xq), _ptr(Xa) if Ma else None, _ptr(X), _ptr(theta), _ptr(Linv), _ptr(alpha), _ptr(y_mean),
                                                    _ptr(y_std), _ptr(n_points), _ptr(VA) if Ma else None, T, N, Mq, Ma, D, int(kind), _ptr(mu),
                                                    _ptr(var), _ptr(cov), 0, _stream_handle())
    _lib.check_rc(rc, "scaml_posterior_linv_grad_f64")
    return dict(mu=mu, var=var, cov=cov)


def target_posterior_grad(cov_g: Optional[torch.Tensor], mu_g: torch.Tensor, var_g: torch.Tensor, Xt: torch.Tensor, Xq: torch.Tensor,
                          theta: torch.Tensor, alpha: Optional[torch.Tensor], Z: Optional[torch.Tensor], s_all: float,
                          info: Optional[torch.Tensor], kind: int):
    """d mu* / d x and d var* / d x (Mq, D) of the target posterior from the weighted task sums of ``source_posteriors_grad``
    (cov_g (n, Mq * 16), mu_g / var_g (Mq * 16)) and the value path's alpha (n,), Z (n, Mq).  scaml_target_posterior_grad_f64."""
    Mq, D = Xq.shape
    n = 0 if cov_g is None else int(cov_g.shape[0])
    mu_g = _check(mu_g.reshape(-1), "mu_g", (Mq * 16,))
    var_g = _check(var_g.reshape(-1), "var_g", (Mq * 16,))
    Xq = _check(Xq, "Xq")
    theta = _check(theta, "theta", (D + 2,))
    if n:
        cov_g = _check(cov_g, "cov_g", (n, Mq * 16))
        Xt = _check(Xt, "Xt", (n, D))
        alpha = _check(alpha, "alpha", (n,))
        Z = _check(Z, "Z", (n, Mq))
    dev = Xq.device
    with torch.cuda.device(dev):
        dmu = _empty(dev, Mq, D)
        dvar = _empty(dev, Mq, D)
        rc = _lib.lib.scaml_target_posterior_grad_f64(_ptr(cov_g) if n else None, _ptr(mu_g), _ptr(var_g), _ptr(Xt) if n else None, _ptr(Xq),
                                                      _ptr(theta), _ptr(alpha) if n else None, _ptr(Z) if n else None, float(s_all), _ptr(info), n, Mq, D,
                                                      int(kind), _ptr(dmu), _ptr(dvar), _stream_handle())
    _lib.check_rc(rc, "scaml_target_posterior_grad_f64")
    return dmu, dvar


ACQF_UCB = 0
ACQF_EI = 1
ACQF_LOG = 0x10
ACQF_LOGEI = ACQF_EI | ACQF_LOG   # 17: the logarithm of EI, stable in the tails (include/scaml_gp.h (7f))


def acqf_transform(mu: torch.Tensor, var: torch.Tensor, acqf: int, acqf_param: float, want_factors: bool = True):
    """The acquisition value of M posteriors (mu, var (M,), original units) and its partial derivatives, elementwise: one launch of
    scaml_acqf_transform_f64 (7o), the statement the fantasy and the studies' kernels evaluate.  ``acqf``: ACQF_UCB (acqf_param = beta),
    ACQF_EI or ACQF_LOGEI (best_f).  Returns (A, dA/dmu, dA/dvar), each (M,); the last two None with ``want_factors=False``."""
    M = int(mu.numel())
    mu = _check(mu.reshape(-1), "mu", (M,))
    var = _check(var.reshape(-1), "var", (M,))
    dev = mu.device
    with torch.cuda.device(dev):
        A = _empty(dev, M)
        Amu = _empty(dev, M) if want_factors else None
        Av = _empty(dev, M) if want_factors else None
        rc = _lib.lib.scaml_acqf_transform_f64(_ptr(mu), _ptr(var), float(acqf_param), M, int(acqf), _ptr(A), _ptr(Amu), _ptr(Av),
                                               _stream_handle())
    _lib.check_rc(rc, "scaml_acqf_transform_f64")
    return A, Amu, Av


def target_fantasy_block(cov_s: torch.Tensor, mean_s: torch.Tensor, var_s: torch.Tensor, Xall: torch.Tensor, theta: torch.Tensor,
                         targets: torch.Tensor, m_all: float, s_all: float, kind: int,
                         factor: Optional[Dict[str, torch.Tensor]] = None, var_noise_add: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """The value path of ``target_posterior_full`` for a fantasy model: the n training points of ``Xall`` carry F target vectors
    ``targets`` (F, n) (standardised; they differ only in the conditioned rows).  scaml_target_assemble_f64 (with targets[0]) and
    scaml_cho_solve_batched_f64 for Z = Knn^-1 Knq, as in (7); ``factor``: that of an earlier call with the same training block, else
    scaml_potrf_batched_f64 (jitter ladder) and ONE scaml_cho_solve_batched_f64 with R = F right-hand sides for alpha (n, F).
    ``var_noise_add`` (not None): also the posterior variance (M,) in original units, + that noise, from scaml_target_finish_f64 (it
    does not depend on the targets).  Returns dict(Knq (n, M), Z (n, M), mean_q, var_q (M,), alpha (n, F), info, factor, var)."""
    F, n = targets.shape
    W, D = Xall.shape
    M = W - n
    if not 1 <= n <= _lib.lib.scaml_fit_max_n():
        raise ValueError(f"target_fantasy_block takes 1 <= n <= {_lib.lib.scaml_fit_max_n()} training points")
    cov_s = _check(cov_s, "cov_s", (n, W))
    mean_s = _check(mean_s, "mean_s", (W,))
    var_s = _check(var_s, "var_s", (W,))
    Xall = _check(Xall, "Xall")
    theta = _check(theta, "theta", (D + 2,))
    targets = _check(targets, "targets", (F, n))
    dev = Xall.device
    with torch.cuda.device(dev):
        Knn, resid = _empty(dev, 1, n, n), _empty(dev, 1, n)
        Knq, mean_q, var_q = _empty(dev, 1, n, M), _empty(dev, M), _empty(dev, M)
        rc = _lib.lib.scaml_target_assemble_f64(_ptr(cov_s), _ptr(mean_s), _ptr(var_s), _ptr(Xall), _ptr(theta), _ptr(targets[0]),
                                                float(m_all), float(s_all), n, M, D, int(kind), _ptr(Knn), _ptr(resid), _ptr(Knq),
                                                _ptr(mean_q), _ptr(var_q), _stream_handle())
        _lib.check_rc(rc, "scaml_target_assemble_f64")
        f = factor
        if f is None:
            f = potrf_batched(Knn, resid, want_linv=True)
            # r_f = r_0 + (y~_f - y~_0): the training rows are shared, only the conditioned rows differ per fantasy
            R = (resid[0].unsqueeze(-1) + (targets - targets[0]).transpose(0, 1)).unsqueeze(0).contiguous()
            f["alpha_f"] = cho_solve(f["L"], f["Linv_diag"], R)[0]
        Z = cho_solve(f["L"], f["Linv_diag"], Knq)[0] if M > 0 else None
        var = None
        if var_noise_add is not None:
            mu0, var = _empty(dev, M), _empty(dev, M)
            if M > 0:
                rc = _lib.lib.scaml_target_finish_f64(_ptr(Knq), _ptr(Z), _ptr(f["alpha"]), _ptr(mean_q), _ptr(var_q), float(m_all), float(s_all),
                                                      float(var_noise_add), _ptr(f["info"]), n, M, _ptr(mu0), _ptr(var), _stream_handle())
                _lib.check_rc(rc, "scaml_target_finish_f64")
    return dict(Knq=Knq[0], Z=Z, mean_q=mean_q, var_q=var_q, alpha=f["alpha_f"], info=f["info"], factor=f, var=var)


def target_fantasy_acqf(Knq: torch.Tensor, Z: torch.Tensor, alpha: torch.Tensor, mean_q: torch.Tensor, var_q: torch.Tensor, m_all: float,
                        s_all: float, info: Optional[torch.Tensor], acqf: int, acqf_param: float, noise_add: float = 0.0,
                        grad_inputs: Optional[Dict[str, torch.Tensor]] = None, kind: int = KIND_RBF):
    """(1/F) sum_f A(mu_f, v) at M query points, A = UCB (``acqf`` ACQF_UCB, acqf_param = beta) or EI (ACQF_EI, acqf_param = best_f),
    from the fantasy block (``target_fantasy_block``: Knq, Z (n, M), alpha (n, F), mean_q, var_q (M,)).  ``grad_inputs``:
    dict(cov_g (n, M * 16), mu_g, var_g (M * 16), Xt (n, D), Xq (M, D), theta (D + 2)) of the GRAD pass -- then also d value / d x
    (M, D).  One launch of scaml_target_fantasy_acqf_f64.  Returns (value (M,), grad (M, D) or None)."""
    n, M = Knq.shape
    F = int(alpha.shape[1])
    Knq = _check(Knq, "Knq", (n, M))
    Z = _check(Z, "Z", (n, M))
    alpha = _check(alpha, "alpha", (n, F))
    mean_q = _check(mean_q, "mean_q", (M,))
    var_q = _check(var_q, "var_q", (M,))
    if info is not None:
        info = _check(info.reshape(-1)[:1], "info", (1,), torch.int32)
    dev = Knq.device
    g, D = None, 0
    if grad_inputs is not None:
        Xq = _check(grad_inputs["Xq"], "Xq")
        D = int(Xq.shape[1])
        g = dict(cov_g=_check(grad_inputs["cov_g"].reshape(n, -1), "cov_g", (n, M * 16)),
                 mu_g=_check(grad_inputs["mu_g"].reshape(-1), "mu_g", (M * 16,)),
                 var_g=_check(grad_inputs["var_g"].reshape(-1), "var_g", (M * 16,)),
                 Xt=_check(grad_inputs["Xt"], "Xt", (n, D)), Xq=_check(Xq, "Xq", (M, D)),
                 theta=_check(grad_inputs["theta"], "theta", (D + 2,)))
    with torch.cuda.device(dev):
        value = _empty(dev, M)
        grad = _empty(dev, M, D) if g is not None else None
        rc = _lib.lib.scaml_target_fantasy_acqf_f64(
            _ptr(Knq), _ptr(Z), _ptr(alpha), _ptr(mean_q), _ptr(var_q), float(m_all), float(s_all), float(noise_add), _ptr(info),
            int(acqf), float(acqf_param), *([_ptr(g[k]) for k in ("cov_g", "mu_g", "var_g", "Xt", "Xq", "theta")] if g else [None] * 6),
            n, M, F, D, int(kind), _ptr(value), _ptr(grad), _stream_handle())
    _lib.check_rc(rc, "scaml_target_fantasy_acqf_f64")
    return value, grad


def qacqf_max_q() -> int:
    """Points per batch of the joint acquisition kernels (5g) / (7p)."""
    return int(_lib.lib.scaml_qacqf_max_q())


def qacqf_max_samples() -> int:
    """Base samples the joint acquisition kernel (7p) takes."""
    return int(_lib.lib.scaml_qacqf_max_samples())


def source_posteriors_grad_joint(Xq: torch.Tensor, q: int, Xa: torch.Tensor, X: torch.Tensor, theta: torch.Tensor, kind: int, Linv: torch.Tensor,
                                 alpha: torch.Tensor, VA: torch.Tensor, VQ: torch.Tensor, y_mean: Optional[torch.Tensor] = None,
                                 y_std: Optional[torch.Tensor] = None, n_points: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``source_posteriors_grad`` for query points Xq (Mq, D) that move in batches of ``q`` (Mq a multiple of q): one launch of
    scaml_posterior_linv_grad_joint_f64 (5g).  cov is (T, Ma + q, Mq * 16): rows a < Ma against the leading points Xa (Ma, D) / VA
    (T, N, Ma), row Ma + r of query point j's strip against its batch mate (j // q) * q + r -- the covariance in column 0, its
    derivative with respect to x_j (mate held fixed) in columns 1 .. D.  VQ (T, N, Mq): the V of the query points themselves
    (``source_posteriors(Xq, ..., keep_V=True, Linv=Linv)["V"]``).  Returns dict(mu (T, Mq, 16), var (T, Mq, 16), cov)."""
    T, N, D = X.shape
    Mq, q = int(Xq.shape[0]), int(q)
    if q < 1 or Mq % q:
        raise ValueError("the query points come in batches of q: Mq must be a multiple of q >= 1")
    X = _check(X, "X")
    Xq = _check(Xq, "Xq", (Mq, D))
    theta = _check(theta, "theta", (T, D + 2))
    Linv = _check(Linv, "Linv", (T, N, N))
    alpha = _check(alpha, "alpha", (T, N))
    Ma = int(VA.shape[-1])
    VA = _check(VA, "VA", (T, N, Ma))
    Xa = _check(Xa, "Xa", (Ma, D))
    VQ = _check(VQ, "VQ", (T, N, Mq))
    y_mean = _opt(y_mean, "y_mean", (T,))
    y_std = _opt(y_std, "y_std", (T,))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    dev = X.device
    with torch.cuda.device(dev):
        mu = _empty(dev, T, Mq, 16)
        var = _empty(dev, T, Mq, 16)
        cov = _empty(dev, T, Ma + q, Mq * 16)
        rc = _lib.lib.scaml_posterior_linv_grad_joint_f64(_ptr(Xq), _ptr(Xa), _ptr(X), _ptr(theta), _ptr(Linv), _ptr(alpha), _ptr(y_mean),
                                                          _ptr(y_std), _ptr(n_points), _ptr(VA), _ptr(VQ), T, N, Mq, Ma, q, D, int(kind),
                                                          _ptr(mu), _ptr(var), _ptr(cov), 0, _stream_handle())
    _lib.check_rc(rc, "scaml_posterior_linv_grad_joint_f64")
    return dict(mu=mu, var=var, cov=cov)


def target_qacqf(Knq: torch.Tensor, Z: torch.Tensor, alpha: torch.Tensor, mean_q: torch.Tensor, var_q: torch.Tensor, m_all: float, s_all: float,
                 info: Optional[torch.Tensor], cov_g: torch.Tensor, mu_g: torch.Tensor, var_g: torch.Tensor, Xt: torch.Tensor, Xq: torch.Tensor,
                 theta: torch.Tensor, base_samples: torch.Tensor, acqf: int, acqf_param: float, kind: int = KIND_RBF,
                 want_grad: bool = True) -> Dict[str, torch.Tensor]:
    """The joint Monte-Carlo acquisition of B = Mq / q batches of q points, qEI (``acqf`` ACQF_EI, acqf_param = best_f) or qUCB
    (ACQF_UCB, beta), over the joint posterior of each batch, with its exact input gradient: one launch of scaml_target_qacqf_f64 (7p).
    Knq, Z (n, Mq), alpha (n,), mean_q, var_q (Mq,) from the value path (``target_fantasy_block``); cov_g (n + q, Mq * 16), mu_g, var_g
    (Mq * 16) the weighted sums of ``source_posteriors_grad_joint``; base_samples (S, q) standard-normal draws shared by all batches.
    Returns dict(value (B,), grad (Mq, D) or None, jitter (B,), info (B,) int32)."""
    n, Mq = Knq.shape
    S, q = base_samples.shape
    D = int(Xq.shape[1])
    if q < 1 or Mq % q:
        raise ValueError("Mq must be a multiple of q = base_samples.shape[1]")
    B = Mq // q
    Knq = _check(Knq, "Knq", (n, Mq))
    Z = _check(Z, "Z", (n, Mq))
    alpha = _check(alpha, "alpha", (n,))
    mean_q = _check(mean_q, "mean_q", (Mq,))
    var_q = _check(var_q, "var_q", (Mq,))
    cov_g = _check(cov_g.reshape(n + q, -1), "cov_g", (n + q, Mq * 16))
    mu_g = _check(mu_g.reshape(-1), "mu_g", (Mq * 16,))
    var_g = _check(var_g.reshape(-1), "var_g", (Mq * 16,))
    Xt = _check(Xt, "Xt", (n, D))
    Xq = _check(Xq, "Xq", (Mq, D))
    theta = _check(theta, "theta", (D + 2,))
    base_samples = _check(base_samples, "base_samples", (S, q))
    if info is not None:
        info = _check(info.reshape(-1)[:1], "info", (1,), torch.int32)
    dev = Knq.device
    with torch.cuda.device(dev):
        value = _empty(dev, B)
        grad = _empty(dev, Mq, D) if want_grad else None
        jitter = _empty(dev, B)
        info_out = _empty(dev, B, dtype=torch.int32)
        rc = _lib.lib.scaml_target_qacqf_f64(_ptr(Knq), _ptr(Z), _ptr(alpha), _ptr(mean_q), _ptr(var_q), float(m_all), float(s_all), _ptr(info),
                                             _ptr(cov_g), _ptr(mu_g), _ptr(var_g), _ptr(Xt), _ptr(Xq), _ptr(theta), _ptr(base_samples),
                                             int(acqf), float(acqf_param), n, Mq, q, S, D, int(kind), _ptr(value), _ptr(grad), _ptr(jitter),
                                             _ptr(info_out), _stream_handle())
    _lib.check_rc(rc, "scaml_target_qacqf_f64")
    return dict(value=value, grad=grad, jitter=jitter, info=info_out)


def target_qacqf_pending(Knq: torch.Tensor, Z: torch.Tensor, alpha: torch.Tensor, mean_q: torch.Tensor, var_q: torch.Tensor, m_all: float,
                         s_all: float, info: Optional[torch.Tensor], cov_g: torch.Tensor, mu_g: torch.Tensor, var_g: torch.Tensor,
                         Xt: torch.Tensor, Xq: torch.Tensor, theta: torch.Tensor, base_samples: torch.Tensor, Xp: torch.Tensor,
                         Zp: Optional[torch.Tensor], mu_p: Optional[torch.Tensor], Sigma_pp: Optional[torch.Tensor], acqf: int,
                         acqf_param: float, kind: int = KIND_RBF, want_grad: bool = True) -> Dict[str, torch.Tensor]:
    """``target_qacqf`` with p = Xp.shape[0] evaluations pending: every batch is its q moving points followed by the same p pending
    points Xp (p, D), the utility's maximum runs over all q + p joint samples (base_samples (S, q + p)) and only the moving points
    get a gradient: one launch of scaml_target_qacqf_pending_f64 (7q).  cov_g (n + p + q, Mq * 16): the weighted sums of
    ``source_posteriors_grad_joint`` called with the pending points behind the training inputs (Ma = n + p).  Zp (n, p) = Knn^-1 Knp;
    mu_p (p,), Sigma_pp (p, p): the target posterior of the pending points among themselves, original units, no observation noise.
    p = 0 (Zp, mu_p, Sigma_pp may be None): ``target_qacqf``'s outputs to the bit.
    Returns dict(value (B,), grad (Mq, D) or None, jitter (B,), info (B,) int32)."""
    n, Mq = Knq.shape
    D = int(Xq.shape[1])
    p = int(Xp.shape[0])
    S, Q = base_samples.shape
    q = Q - p
    if q < 1 or Mq % q:
        raise ValueError("Mq must be a multiple of q = base_samples.shape[1] - Xp.shape[0] >= 1")
    B = Mq // q
    Knq = _check(Knq, "Knq", (n, Mq))
    Z = _check(Z, "Z", (n, Mq))
    alpha = _check(alpha, "alpha", (n,))
    mean_q = _check(mean_q, "mean_q", (Mq,))
    var_q = _check(var_q, "var_q", (Mq,))
    cov_g = _check(cov_g.reshape(n + p + q, -1), "cov_g", (n + p + q, Mq * 16))
    mu_g = _check(mu_g.reshape(-1), "mu_g", (Mq * 16,))
    var_g = _check(var_g.reshape(-1), "var_g", (Mq * 16,))
    Xt = _check(Xt, "Xt", (n, D))
    Xq = _check(Xq, "Xq", (Mq, D))
    theta = _check(theta, "theta", (D + 2,))
    base_samples = _check(base_samples, "base_samples", (S, Q))
    Xp = _check(Xp, "Xp", (p, D))
    if p > 0:
        Zp = _check(Zp, "Zp", (n, p))
        mu_p = _check(mu_p, "mu_p", (p,))
        Sigma_pp = _check(Sigma_pp, "Sigma_pp", (p, p))
    else:
        Xp = Zp = mu_p = Sigma_pp = None
    if info is not None:
        info = _check(info.reshape(-1)[:1], "info", (1,), torch.int32)
    dev = Knq.device
    with torch.cuda.device(dev):
        value = _empty(dev, B)
        grad = _empty(dev, Mq, D) if want_grad else None
        jitter = _empty(dev, B)
        info_out = _empty(dev, B, dtype=torch.int32)
        rc = _lib.lib.scaml_target_qacqf_pending_f64(_ptr(Knq), _ptr(Z), _ptr(alpha), _ptr(mean_q), _ptr(var_q), float(m_all), float(s_all),
                                                     _ptr(info), _ptr(cov_g), _ptr(mu_g), _ptr(var_g), _ptr(Xt), _ptr(Xq), _ptr(theta),
                                                     _ptr(base_samples), _ptr(Xp), _ptr(Zp), _ptr(mu_p), _ptr(Sigma_pp), int(acqf),
                                                     float(acqf_param), n, Mq, q, p, S, D, int(kind), _ptr(value), _ptr(grad), _ptr(jitter),
                                                     _ptr(info_out), _stream_handle())
    _lib.check_rc(rc, "scaml_target_qacqf_pending_f64")
    return dict(value=value, grad=grad, jitter=jitter, info=info_out)


def qacqf_value_columns(B: int, q: int) -> int:
    """Mp: the columns B batches of q points take in the value layout of (5h) / (7r) (scaml_qacqf_value_columns: strips of 16 columns,
    16 // q whole batches each)."""
    Mp = int(_lib.lib.scaml_qacqf_value_columns(int(B), int(q)))
    if Mp < 0:
        raise ValueError(f"the value layout takes B >= 0 batches of 1 <= q <= {qacqf_max_q()} points")
    return Mp


def qacqf_value_column_map(B: int, q: int) -> torch.Tensor:
    """(B, q) int64: the column of point j of batch b in the value layout, 16 (b // bps) + (b % bps) q + j with bps = 16 // q
    (csrc/gp_qacqf_columns.h)."""
    bps = 16 // int(q)
    b = torch.arange(int(B), dtype=torch.int64).unsqueeze(1)
    return 16 * (b // bps) + (b % bps) * int(q) + torch.arange(int(q), dtype=torch.int64).unsqueeze(0)


def qacqf_value_pack(X: torch.Tensor, fill: float = 0.5) -> torch.Tensor:
    """X (B, q, D) -> the packed query points (Mp, D) of (5h); padding columns hold ``fill`` (any finite coordinate will do)."""
    B, q, D = X.shape
    out = X.new_full((qacqf_value_columns(B, q), D), float(fill))
    if B > 0:
        out[qacqf_value_column_map(B, q).reshape(-1).to(X.device)] = X.reshape(B * q, D)
    return out


def source_posteriors_cov_joint(Xq: torch.Tensor, B: int, q: int, Xa: torch.Tensor, X: torch.Tensor, theta: torch.Tensor, kind: int,
                                Linv: torch.Tensor, alpha: torch.Tensor, VA: torch.Tensor, y_mean: Optional[torch.Tensor] = None,
                                y_std: Optional[torch.Tensor] = None, n_points: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The source posteriors of B batches of q points in VALUE layout, Xq (Mp, D) packed by ``qacqf_value_pack``: one launch of
    scaml_posterior_linv_cov_joint_f64 (5h).  cov is (T, Ma + q, Mp): rows a < Ma against the leading points Xa (Ma, D) / VA (T, N, Ma),
    row Ma + r of a column against point r of its batch (zeros in a padding column) -- 16 points per strip and no derivative columns,
    where ``source_posteriors_grad_joint`` spends a strip per point.  Returns dict(mu (T, Mp), var (T, Mp), cov)."""
    T, N, D = X.shape
    B, q = int(B), int(q)
    Mp = qacqf_value_columns(B, q)
    X = _check(X, "X")
    Xq = _check(Xq, "Xq", (Mp, D))
    theta = _check(theta, "theta", (T, D + 2))
    Linv = _check(Linv, "Linv", (T, N, N))
    alpha = _check(alpha, "alpha", (T, N))
    Ma = int(VA.shape[-1])
    VA = _check(VA, "VA", (T, N, Ma))
    Xa = _check(Xa, "Xa", (Ma, D))
    y_mean = _opt(y_mean, "y_mean", (T,))
    y_std = _opt(y_std, "y_std", (T,))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    dev = X.device
    with torch.cuda.device(dev):
        mu = _empty(dev, T, Mp)
        var = _empty(dev, T, Mp)
        cov = _empty(dev, T, Ma + q, Mp)
        rc = _lib.lib.scaml_posterior_linv_cov_joint_f64(_ptr(Xq), _ptr(Xa), _ptr(X), _ptr(theta), _ptr(Linv), _ptr(alpha), _ptr(y_mean),
                                                         _ptr(y_std), _ptr(n_points), _ptr(VA), T, N, Mp, Ma, B, q, D, int(kind), _ptr(mu),
                                                         _ptr(var), _ptr(cov), 0, _stream_handle())
    _lib.check_rc(rc, "scaml_posterior_linv_cov_joint_f64")
    return dict(mu=mu, var=var, cov=cov)


def target_qacqf_value(Knq: torch.Tensor, Z: torch.Tensor, alpha: torch.Tensor, mean_q: torch.Tensor, var_q: torch.Tensor, m_all: float,
                       s_all: float, info: Optional[torch.Tensor], cov_s: torch.Tensor, Xq: torch.Tensor, theta: torch.Tensor,
                       base_samples: torch.Tensor, B: int, acqf: int, acqf_param: float, kind: int = KIND_RBF,
                       Xp: Optional[torch.Tensor] = None, Zp: Optional[torch.Tensor] = None, mu_p: Optional[torch.Tensor] = None,
                       Sigma_pp: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``target_qacqf`` / ``target_qacqf_pending`` without the gradient, from the value layout: one launch of
    scaml_target_qacqf_value_f64 (7r).  Knq, Z (n, Mp), mean_q, var_q (Mp,), Xq (Mp, D) at the packed columns of the B batches;
    cov_s (n + p + q, Mp) the weighted sums of ``source_posteriors_cov_joint``; base_samples (S, q + p) with p = Xp.shape[0] pending
    points (Xp None: p = 0).  Returns dict(value (B,), jitter (B,), info (B,) int32): the bits of the gradient kernels' outputs."""
    n, Mp = Knq.shape
    D = int(Xq.shape[1])
    p = 0 if Xp is None else int(Xp.shape[0])
    S, Q = base_samples.shape
    q, B = Q - p, int(B)
    if q < 1 or B < 0 or Mp != qacqf_value_columns(B, q):
        raise ValueError("Knq must have qacqf_value_columns(B, q) columns, q = base_samples.shape[1] - Xp.shape[0] >= 1")
    Knq = _check(Knq, "Knq", (n, Mp))
    Z = _check(Z, "Z", (n, Mp))
    alpha = _check(alpha, "alpha", (n,))
    mean_q = _check(mean_q, "mean_q", (Mp,))
    var_q = _check(var_q, "var_q", (Mp,))
    cov_s = _check(cov_s, "cov_s", (n + p + q, Mp))
    Xq = _check(Xq, "Xq", (Mp, D))
    theta = _check(theta, "theta", (D + 2,))
    base_samples = _check(base_samples, "base_samples", (S, Q))
    if p > 0:
        Xp = _check(Xp, "Xp", (p, D))
        Zp = _check(Zp, "Zp", (n, p))
        mu_p = _check(mu_p, "mu_p", (p,))
        Sigma_pp = _check(Sigma_pp, "Sigma_pp", (p, p))
    else:
        Xp = Zp = mu_p = Sigma_pp = None
    if info is not None:
        info = _check(info.reshape(-1)[:1], "info", (1,), torch.int32)
    dev = Knq.device
    with torch.cuda.device(dev):
        value = _empty(dev, B)
        jitter = _empty(dev, B)
        info_out = _empty(dev, B, dtype=torch.int32)
        rc = _lib.lib.scaml_target_qacqf_value_f64(_ptr(Knq), _ptr(Z), _ptr(alpha), _ptr(mean_q), _ptr(var_q), float(m_all), float(s_all),
                                                   _ptr(info), _ptr(cov_s), _ptr(Xq), _ptr(theta), _ptr(base_samples), _ptr(Xp), _ptr(Zp),
                                                   _ptr(mu_p), _ptr(Sigma_pp), int(acqf), float(acqf_param), n, Mp, B, q, p, S, D, int(kind),
                                                   _ptr(value), _ptr(jitter), _ptr(info_out), _stream_handle())
    _lib.check_rc(rc, "scaml_target_qacqf_value_f64")
    return dict(value=value, jitter=jitter, info=info_out)


def _source_pass_grouped(value: bool, Xq, group, Xa, n_points_a, VA_tab, X, theta, kind, Linv, alpha, y_mean, y_std, n_points, task_base,
                         tasks_per_group, cov_out) -> Dict[str, torch.Tensor]:
    """The grouped source pass behind ``source_posteriors_grad_grouped`` (``value`` False: 16 columns per query point, ``group`` per query
    point) and ``source_posteriors_grouped`` (``value`` True: a column per candidate, ``group`` per strip of 16).  With ``task_base`` the
    source arrays are (Tsrc, ...) and the outputs (T = tasks_per_group, ...): the ``_own`` entry point.  ``cov_out``: the buffer cov is
    written into (tests prefill it to see which rows a launch writes)."""
    own = task_base is not None
    Tsrc, N, D = X.shape
    T = int(tasks_per_group) if own else Tsrc
    Mq = Xq.shape[0]
    G, Ma_max = int(Xa.shape[0]), int(Xa.shape[1])
    X = _check(X, "X")
    Xq = _check(Xq, "Xq", (Mq, D))
    group = _check(group, "group", (Mq // 16 if value else Mq,), torch.int32)
    Xa = _check(Xa, "Xa", (G, Ma_max, D))
    n_points_a = _check(n_points_a, "n_points_a", (G,), torch.int32)
    VA_tab = _check(VA_tab, "VA_tab", (G,), torch.int64)
    theta = _check(theta, "theta", (Tsrc, D + 2))
    Linv = _check(Linv, "Linv", (Tsrc, N, N))
    alpha = _check(alpha, "alpha", (Tsrc, N))
    y_mean = _opt(y_mean, "y_mean", (Tsrc,))
    y_std = _opt(y_std, "y_std", (Tsrc,))
    n_points = _opt(n_points, "n_points", (Tsrc,), torch.int32)
    if own:
        task_base = _check(task_base, "task_base", (G,), torch.int32)
    row, width = ((Mq,), Mq) if value else ((Mq, 16), Mq * 16)
    name = "scaml_posterior_linv_" + ("" if value else "grad_") + "grouped_" + ("own_" if own else "") + "f64"
    dev = X.device
    with torch.cuda.device(dev):
        mu = _empty(dev, T, *row)
        var = _empty(dev, T, *row)
        cov = _empty(dev, T, Ma_max, width) if cov_out is None else _check(cov_out, "cov_out", (T, Ma_max, width))
        rc = getattr(_lib.lib, name)(_ptr(Xq), _ptr(group), _ptr(Xa), _ptr(n_points_a), _ptr(VA_tab), _ptr(X), _ptr(theta), _ptr(Linv), _ptr(alpha),
                                     _ptr(y_mean), _ptr(y_std), _ptr(n_points), T, N, Mq, G, Ma_max, D, int(kind), _ptr(mu), _ptr(var), _ptr(cov),
                                     *((_ptr(task_base), Tsrc) if own else ()), _stream_handle())
    _lib.check_rc(rc, name)
    return dict(mu=mu, var=var, cov=cov)


def source_posteriors_grad_grouped(Xq: torch.Tensor, group: torch.Tensor, Xa: torch.Tensor, n_points_a: torch.Tensor, VA_tab: torch.Tensor,
                                   X: torch.Tensor, theta: torch.Tensor, kind: int, Linv: torch.Tensor, alpha: torch.Tensor,
                                   y_mean: Optional[torch.Tensor] = None, y_std: Optional[torch.Tensor] = None,
                                   n_points: Optional[torch.Tensor] = None, task_base: Optional[torch.Tensor] = None,
                                   tasks_per_group: Optional[int] = None, cov_out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``source_posteriors_grad`` with the query points Xq (Mq, D) divided among G groups, one launch of
    scaml_posterior_linv_grad_grouped_f64: ``group`` (Mq,) int32 (negative: a padding row, zeros), ``Xa`` (G, Ma_max, D) the groups'
    leading points, ``n_points_a`` (G,) int32 their counts, ``VA_tab`` (G,) int64: the ADDRESSES of the groups' V (T, N, Ma_g) tensors
    (``ScaMLGP._train_VA``; the caller keeps them alive).  Returns dict(mu, var (T, Mq, 16), cov (T, Ma_max, Mq * 16): rows
    a < Ma_{group[q]} of strip q are written, the rest is uninitialised -- or what ``cov_out`` held, when that buffer is given).

    ``task_base`` (G,) int32: every group owns its source tasks (scaml_posterior_linv_grad_grouped_own_f64) -- the source arrays hold
    Tsrc = X.shape[0] tasks, task slot t of group g reads task ``task_base[g] + t``, and T = ``tasks_per_group`` slots are the leading
    axis of the outputs and of the groups' V."""
    if task_base is not None and tasks_per_group is None:
        raise ValueError("task_base needs tasks_per_group (the task slots of a group)")
    if task_base is None and tasks_per_group is not None:
        raise ValueError("tasks_per_group goes with task_base")
    return _source_pass_grouped(False, Xq, group, Xa, n_points_a, VA_tab, X, theta, kind, Linv, alpha, y_mean, y_std, n_points, task_base,
                                tasks_per_group, cov_out)


def _target_pass_studies(strips: bool, mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info,
                         acqf_param, acqf, kind, want_grad, want_posterior, fantasy=None) -> Dict[str, Optional[torch.Tensor]]:
    """The studies' target pass behind ``target_acqf_batched`` (``strips`` False: the GRAD layout, ``group`` per query point, the gradient
    where wanted) and ``target_score_batched`` (``strips`` True: the value layout, ``group`` per strip of 16 candidates, no gradient).
    ``fantasy`` = (alpha_f (G, n_max, F_max), n_fant (G,) int32): their ``target_fantasy_*`` siblings for studies with pending
    evaluations -- ``alpha`` is not used and the posterior is not returned."""
    Mq, D = Xq.shape
    G, n_max = int(Xt.shape[0]), int(Xt.shape[1])
    T = int(w.shape[1])
    row, width = ((Mq,), Mq) if strips else ((Mq, 16), Mq * 16)
    mu = _check(mu, "mu", (T, *row))
    var = _check(var, "var", (T, *row))
    cov = _check(cov, "cov", (T, n_max, width))
    group = _check(group, "group", (Mq // 16 if strips else Mq,), torch.int32)
    Xq = _check(Xq, "Xq")
    w = _check(w, "w", (G, T))
    active = _check(active, "active", (G, T), torch.uint8)
    Xt = _check(Xt, "Xt", (G, n_max, D))
    theta = _check(theta, "theta", (G, D + 2))
    L = _check(L, "L", (G, n_max, n_max))
    Linv_diag = _check(Linv_diag, "Linv_diag", (G, (n_max + 15) // 16, 16, 16))
    if fantasy is None:
        alpha = _check(alpha, "alpha", (G, n_max))
    else:
        if fantasy[0].dim() != 3:
            raise ValueError("alpha_f must be (G, n_max, F_max)")
        F_max = int(fantasy[0].shape[2])
        alpha_f = _check(fantasy[0], "alpha_f", (G, n_max, F_max))
        n_fant = _check(fantasy[1], "n_fant", (G,), torch.int32)
    n_points = _check(n_points, "n_points", (G,), torch.int32)
    m_all = _check(m_all, "m_all", (G,))
    s_all = _check(s_all, "s_all", (G,))
    info = _check(info, "info", (G,), torch.int32)
    acqf_param = _check(acqf_param, "acqf_param", (G,))
    name = "scaml_target_score_batched_f64" if strips else "scaml_target_acqf_batched_f64"
    dev = Xq.device
    with torch.cuda.device(dev):
        value = _empty(dev, Mq)
        grad = _empty(dev, Mq, D) if want_grad else None
        if fantasy is not None:
            name = "scaml_target_fantasy_score_batched_f64" if strips else "scaml_target_fantasy_acqf_batched_f64"
            rc = getattr(_lib.lib, name)(_ptr(mu), _ptr(var), _ptr(cov), _ptr(group), _ptr(Xq), _ptr(w), _ptr(active), _ptr(Xt), _ptr(theta),
                                         _ptr(L), _ptr(Linv_diag), _ptr(alpha_f), _ptr(n_fant), _ptr(n_points), _ptr(m_all), _ptr(s_all),
                                         _ptr(info), _ptr(acqf_param), Mq, G, n_max, F_max, T, D, int(kind), int(acqf), _ptr(value),
                                         *(() if strips else (_ptr(grad),)), _stream_handle())
            _lib.check_rc(rc, name)
            return dict(value=value, grad=grad, mu=None, var=None)
        mu_o = _empty(dev, Mq) if want_posterior else None
        var_o = _empty(dev, Mq) if want_posterior else None
        rc = getattr(_lib.lib, name)(_ptr(mu), _ptr(var), _ptr(cov), _ptr(group), _ptr(Xq), _ptr(w), _ptr(active), _ptr(Xt), _ptr(theta), _ptr(L),
                                     _ptr(Linv_diag), _ptr(alpha), _ptr(n_points), _ptr(m_all), _ptr(s_all), _ptr(info), _ptr(acqf_param), Mq, G,
                                     n_max, T, D, int(kind), int(acqf), _ptr(value), *(() if strips else (_ptr(grad),)), _ptr(mu_o), _ptr(var_o),
                                     _stream_handle())
    _lib.check_rc(rc, name)
    return dict(value=value, grad=grad, mu=mu_o, var=var_o)


def target_acqf_batched(mu: torch.Tensor, var: torch.Tensor, cov: torch.Tensor, group: torch.Tensor, Xq: torch.Tensor, w: torch.Tensor,
                        active: torch.Tensor, Xt: torch.Tensor, theta: torch.Tensor, L: torch.Tensor, Linv_diag: torch.Tensor,
                        alpha: torch.Tensor, n_points: torch.Tensor, m_all: torch.Tensor, s_all: torch.Tensor, info: torch.Tensor,
                        acqf_param: torch.Tensor, acqf: int, kind: int, want_grad: bool = True, want_posterior: bool = False):
    """The acquisition value (and input gradient) of every query point of G studies from the grouped GRAD pass's outputs
    (``source_posteriors_grad_grouped``: mu, var (T, Mq, 16), cov (T, n_max, Mq * 16)) and the studies' padded arrays: w (G, T),
    active (G, T) uint8, Xt (G, n_max, D), theta (G, D + 2), L (G, n_max, n_max), Linv_diag (G, ceil(n_max / 16), 16, 16),
    alpha (G, n_max), n_points, info (G,) int32, m_all, s_all, acqf_param (G,).  One launch of scaml_target_acqf_batched_f64.
    Returns dict(value (Mq,), grad (Mq, D) or None, mu, var (Mq,) or None)."""
    return _target_pass_studies(False, mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info,
                                acqf_param, acqf, kind, want_grad, want_posterior)


def target_fantasy_acqf_batched(mu: torch.Tensor, var: torch.Tensor, cov: torch.Tensor, group: torch.Tensor, Xq: torch.Tensor, w: torch.Tensor,
                                active: torch.Tensor, Xt: torch.Tensor, theta: torch.Tensor, L: torch.Tensor, Linv_diag: torch.Tensor,
                                alpha_f: torch.Tensor, n_fant: torch.Tensor, n_points: torch.Tensor, m_all: torch.Tensor, s_all: torch.Tensor,
                                info: torch.Tensor, acqf_param: torch.Tensor, acqf: int, kind: int, want_grad: bool = True):
    """``target_acqf_batched`` for studies of which some hold pending evaluations: alpha_f (G, n_max, F_max) holds, per study, the F_g =
    ``n_fant[g]`` columns of alpha of its fantasies (row a: F_g values contiguously), and a study's training block -- Xt, L, Linv_diag,
    n_points, the rows of cov -- includes its pending inputs.  UCB / EI are averaged over the fantasies as ``target_fantasy_acqf`` does
    for one model; a study with F_g == 1 gives ``target_acqf_batched``'s bits.  One launch of scaml_target_fantasy_acqf_batched_f64.
    Returns dict(value (Mq,), grad (Mq, D) or None)."""
    out = _target_pass_studies(False, mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, None, n_points, m_all, s_all, info,
                               acqf_param, acqf, kind, want_grad, False, fantasy=(alpha_f, n_fant))
    return dict(value=out["value"], grad=out["grad"])


def target_fantasy_score_batched(mu: torch.Tensor, var: torch.Tensor, cov: torch.Tensor, group: torch.Tensor, Xq: torch.Tensor, w: torch.Tensor,
                                 active: torch.Tensor, Xt: torch.Tensor, theta: torch.Tensor, L: torch.Tensor, Linv_diag: torch.Tensor,
                                 alpha_f: torch.Tensor, n_fant: torch.Tensor, n_points: torch.Tensor, m_all: torch.Tensor, s_all: torch.Tensor,
                                 info: torch.Tensor, acqf_param: torch.Tensor, acqf: int, kind: int):
    """``target_score_batched`` for studies of which some hold pending evaluations (the arrays of ``target_fantasy_acqf_batched``, the
    value layout of ``source_posteriors_grouped``): per candidate the value of ``target_fantasy_acqf_batched``, bit for bit.  One launch
    of scaml_target_fantasy_score_batched_f64.  Returns dict(value (Mq,))."""
    if Xq.shape[0] % 16:
        raise ValueError(f"the candidates come in whole strips of 16, got Mq = {Xq.shape[0]}")
    out = _target_pass_studies(True, mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, None, n_points, m_all, s_all, info,
                               acqf_param, acqf, kind, False, False, fantasy=(alpha_f, n_fant))
    return dict(value=out["value"])


def source_posteriors_grouped(Xq: torch.Tensor, group: torch.Tensor, Xa: torch.Tensor, n_points_a: torch.Tensor, VA_tab: torch.Tensor,
                              X: torch.Tensor, theta: torch.Tensor, kind: int, Linv: torch.Tensor, alpha: torch.Tensor,
                              y_mean: Optional[torch.Tensor] = None, y_std: Optional[torch.Tensor] = None,
                              n_points: Optional[torch.Tensor] = None, task_base: Optional[torch.Tensor] = None,
                              tasks_per_group: Optional[int] = None, cov_out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``source_posteriors_grad_grouped`` without the gradient columns, for a TABLE of candidates: Xq (Mq, D) with Mq a multiple of 16,
    every strip of 16 consecutive candidates belonging to ONE group; ``group`` (Mq / 16,) int32 names it per strip (negative or out of
    range: a padding strip, zeros).  ``Xa`` (G, Ma_max, D), ``n_points_a`` (G,) int32 and ``VA_tab`` (G,) int64 are the groups' leading
    points as in the GRAD sibling.  One launch of scaml_posterior_linv_grouped_f64.  Returns dict(mu, var (T, Mq), cov (T, Ma_max, Mq):
    rows a < Ma_g of a strip are written, the rest is uninitialised -- or what ``cov_out`` held, when that buffer is given).

    ``task_base`` (G,) int32 with ``tasks_per_group``: every group owns its source tasks (scaml_posterior_linv_grouped_own_f64) -- the
    source arrays hold Tsrc = X.shape[0] tasks, slot t of group g reads task ``task_base[g] + t``, the outputs have T =
    ``tasks_per_group`` leading rows."""
    if (task_base is not None) != (tasks_per_group is not None):
        raise ValueError("task_base and tasks_per_group go together")
    if Xq.shape[0] % 16:
        raise ValueError(f"the candidates come in whole strips of 16, got Mq = {Xq.shape[0]}")
    return _source_pass_grouped(True, Xq, group, Xa, n_points_a, VA_tab, X, theta, kind, Linv, alpha, y_mean, y_std, n_points, task_base,
                                tasks_per_group, cov_out)


def target_score_batched(mu: torch.Tensor, var: torch.Tensor, cov: torch.Tensor, group: torch.Tensor, Xq: torch.Tensor, w: torch.Tensor,
                         active: torch.Tensor, Xt: torch.Tensor, theta: torch.Tensor, L: torch.Tensor, Linv_diag: torch.Tensor,
                         alpha: torch.Tensor, n_points: torch.Tensor, m_all: torch.Tensor, s_all: torch.Tensor, info: torch.Tensor,
                         acqf_param: torch.Tensor, acqf: int, kind: int, want_posterior: bool = False):
    """The acquisition value of every candidate of a table from the value-only grouped pass's outputs (``source_posteriors_grouped``:
    mu, var (T, Mq), cov (T, n_max, Mq)), ``group`` (Mq / 16,) int32 per strip of 16 candidates, and the studies' padded arrays as
    ``target_acqf_batched`` takes them.  One launch of scaml_target_score_batched_f64: a workgroup per strip, the study's factor staged
    once for its 16 candidates; per candidate the arithmetic is ``target_acqf_batched``'s, bit for bit.  No gradient.
    Returns dict(value (Mq,), mu, var (Mq,) or None)."""
    if Xq.shape[0] % 16:
        raise ValueError(f"the candidates come in whole strips of 16, got Mq = {Xq.shape[0]}")
    out = _target_pass_studies(True, mu, var, cov, group, Xq, w, active, Xt, theta, L, Linv_diag, alpha, n_points, m_all, s_all, info,
                               acqf_param, acqf, kind, False, want_posterior)
    return dict(value=out["value"], mu=out["mu"], var=out["var"])


def target_factors_batched(batch: "TargetFitBatch", w: torch.Tensor, active: torch.Tensor, theta: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The jittered Cholesky factors of the training blocks of ALL problems of a ``TargetFitBatch`` in two launches whatever their
    number: scaml_target_train_block_batched_f64 (Knn, resid per problem from the padded source terms and each problem's pruned
    ``w`` (S, T), ``active`` (S, T) uint8 and ``theta`` (S, D + 2): what the weighted task sums and the target assemble produce for one
    model's training block) and ONE ``potrf_batched(Knn, resid, n_points=..., want_linv=True)``.
    Returns its dict: L (S, n_max, n_max), alpha (S, n_max), Linv_diag, info, jitter, quad, logdet."""
    S, T, D, n_max = batch.S, batch.T, batch.D, batch.n_max
    w = _check(w, "w", (S, T))
    active = _check(active, "active", (S, T), torch.uint8)
    theta = _check(theta, "theta", (S, D + 2))
    dev = batch.device
    with torch.cuda.device(dev):
        Knn = torch.zeros(S, n_max, n_max, dtype=torch.float64, device=dev)
        resid = torch.zeros(S, n_max, dtype=torch.float64, device=dev)
        rc = _lib.lib.scaml_target_train_block_batched_f64(_ptr(batch.means_t), _ptr(batch.covs_p), _ptr(batch.X), _ptr(batch.y),
                                                           _ptr(batch.n_points), _ptr(batch.m_all), _ptr(batch.s_all), _ptr(w), _ptr(active),
                                                           _ptr(theta), S, n_max, T, D, int(batch.kind), _ptr(Knn), _ptr(resid),
                                                           _stream_handle())
    _lib.check_rc(rc, "scaml_target_train_block_batched_f64")
    out = potrf_batched(Knn, resid, n_points=batch.n_points, want_linv=True)
    out["Knn"], out["resid"] = Knn, resid
    return out


def studies_condition_block(mu: torch.Tensor, cov: torch.Tensor, strip_base: torch.Tensor, w: torch.Tensor, active: torch.Tensor,
                            Xt: torch.Tensor, theta: torch.Tensor, y: torch.Tensor, n_points: torch.Tensor, n_obs: torch.Tensor,
                            m_all: torch.Tensor, s_all: torch.Tensor, kind: int) -> Dict[str, torch.Tensor]:
    """The training blocks of the CONDITIONED models of G studies from the value-mode grouped pass's outputs at the studies' own
    X' = cat(train_X, X_pend) strips (``source_posteriors_grouped``: mu (T, Mq), cov (T, n_max, Mq); ``strip_base`` (G,) int32 the first
    strip of a study) and the studies' padded arrays: w (G, T), active (G, T) uint8, Xt (G, n_max, D), theta (G, D + 2), y (G, n_max)
    standardised targets of the observed rows, n_points (G,) int32 = n + p, n_obs (G,) int32 = n, m_all, s_all (G,).  One launch of
    scaml_studies_condition_block_f64.  Returns dict(Knn (G, n_max, n_max), resid (G, n_max): zero in the pending rows, mean_p (G, n_max):
    the prior mean at the pending rows); what lies past a study's n + p is zero."""
    if mu.dim() != 2 or Xt.dim() != 3:
        raise ValueError("mu must be (T, Mq) and Xt (G, n_max, D)")
    T, Mq = (int(v) for v in mu.shape)
    G, n_max, D = (int(v) for v in Xt.shape)
    if Mq % 16:
        raise ValueError(f"the query points come in whole strips of 16, got Mq = {Mq}")
    mu = _check(mu, "mu", (T, Mq))
    cov = _check(cov, "cov", (T, n_max, Mq))
    strip_base = _check(strip_base, "strip_base", (G,), torch.int32)
    w = _check(w, "w", (G, T))
    active = _check(active, "active", (G, T), torch.uint8)
    Xt = _check(Xt, "Xt", (G, n_max, D))
    theta = _check(theta, "theta", (G, D + 2))
    y = _check(y, "y", (G, n_max))
    n_points = _check(n_points, "n_points", (G,), torch.int32)
    n_obs = _check(n_obs, "n_obs", (G,), torch.int32)
    m_all = _check(m_all, "m_all", (G,))
    s_all = _check(s_all, "s_all", (G,))
    dev = Xt.device
    with torch.cuda.device(dev):
        Knn = torch.zeros(G, n_max, n_max, dtype=torch.float64, device=dev)
        resid = torch.zeros(G, n_max, dtype=torch.float64, device=dev)
        mean_p = torch.zeros(G, n_max, dtype=torch.float64, device=dev)
        rc = _lib.lib.scaml_studies_condition_block_f64(_ptr(mu), _ptr(cov), _ptr(strip_base), _ptr(w), _ptr(active), _ptr(Xt), _ptr(theta),
                                                        _ptr(y), _ptr(n_points), _ptr(n_obs), _ptr(m_all), _ptr(s_all), Mq, G, n_max, T, D,
                                                        int(kind), _ptr(Knn), _ptr(resid), _ptr(mean_p), _stream_handle())
    _lib.check_rc(rc, "scaml_studies_condition_block_f64")
    return dict(Knn=Knn, resid=resid, mean_p=mean_p)


def studies_fantasy_condition(L: torch.Tensor, resid: torch.Tensor, mean_p: torch.Tensor, n_points: torch.Tensor, n_obs: torch.Tensor,
                              info: torch.Tensor, eps: torch.Tensor, n_fant: torch.Tensor, m_all: torch.Tensor,
                              s_all: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The fantasies and alpha_f of G studies from the factors L (G, n_max, n_max) / info (G,) int32 that ``potrf_batched`` returns for
    ``studies_condition_block``'s Knn, its resid and mean_p, and the standard-normal draws eps (G, p_max, F_max) (row i of a study: the
    F_g = ``n_fant[g]`` values of pending point i).  One launch of scaml_studies_fantasy_condition_f64.  Returns dict(alpha_f
    (G, n_max, F_max) in ``target_fantasy_acqf_batched``'s layout, y_fant (G, p_max, F_max) the fantasy targets and mu_p (G, p_max) the
    posterior mean at the pending points, both in original units); what lies past a study's n + p, p or F_g is zero.  A study with
    ``info != 0`` or counts out of range holds NaN."""
    if L.dim() != 3 or eps.dim() != 3:
        raise ValueError("L must be (G, n_max, n_max) and eps (G, p_max, F_max)")
    G, n_max = int(L.shape[0]), int(L.shape[1])
    p_max, F_max = int(eps.shape[1]), int(eps.shape[2])
    L = _check(L, "L", (G, n_max, n_max))
    resid = _check(resid, "resid", (G, n_max))
    mean_p = _check(mean_p, "mean_p", (G, n_max))
    n_points = _check(n_points, "n_points", (G,), torch.int32)
    n_obs = _check(n_obs, "n_obs", (G,), torch.int32)
    info = _check(info, "info", (G,), torch.int32)
    eps = _check(eps, "eps", (G, p_max, F_max))
    n_fant = _check(n_fant, "n_fant", (G,), torch.int32)
    m_all = _check(m_all, "m_all", (G,))
    s_all = _check(s_all, "s_all", (G,))
    dev = L.device
    with torch.cuda.device(dev):
        alpha_f = torch.zeros(G, n_max, F_max, dtype=torch.float64, device=dev)
        y_fant = torch.zeros(G, p_max, F_max, dtype=torch.float64, device=dev)
        mu_p = torch.zeros(G, p_max, dtype=torch.float64, device=dev)
        rc = _lib.lib.scaml_studies_fantasy_condition_f64(_ptr(L), _ptr(resid), _ptr(mean_p), _ptr(n_points), _ptr(n_obs), _ptr(info), _ptr(eps),
                                                          _ptr(n_fant), _ptr(m_all), _ptr(s_all), G, n_max, p_max, F_max, _ptr(alpha_f),
                                                          _ptr(y_fant), _ptr(mu_p), _stream_handle())
    _lib.check_rc(rc, "scaml_studies_fantasy_condition_f64")
    return dict(alpha_f=alpha_f, y_fant=y_fant, mu_p=mu_p)


def mll_backward_workspace(T: int, N: int, D: int, device) -> Dict[str, torch.Tensor]:
    """Reusable buffers of ``mll_backward`` for a (T, N, D) stack: the explicit inverse factors (T N^2 doubles) and
    the per-tile partial sums.  An optimiser loop allocates them once (scaml_mll_backward_workspace_doubles)."""
    nb = (N + 15) // 16
    nt = nb * (nb + 1) // 2
    return dict(work=_empty(device, T * N * N), partials=_empty(device, T, nt, D + 2), shape=(T, N, D))


def mll_backward(
    X: torch.Tensor,
    theta: torch.Tensor,
    kind: int,
    L: torch.Tensor,
    Linv_diag: torch.Tensor,
    alpha: torch.Tensor,
    n_points: Optional[torch.Tensor] = None,
    workspace: Optional[Dict[str, torch.Tensor]] = None,
) -> torch.Tensor:
    """d mll[t] / d theta[t] (T, D+2) for the constrained hyper-parameters, from the outputs of
    ``gp_fit_fused(..., want_linv=True)``.  Launches scaml_mll_backward_f64; the final sum over the
    per-tile partials and the 1 / (2 n_t) scaling are two tiny torch ops.  ``workspace`` (from
    ``mll_backward_workspace``) is reused across calls instead of allocating T N^2 doubles each time."""
    T, N, D = X.shape
    X = _check(X, "X")
    theta = _check(theta, "theta", (T, D + 2))
    L = _check(L, "L", (T, N, N))
    Linv_diag = _check(Linv_diag, "Linv_diag", (T, (N + 15) // 16, 16, 16))
    alpha = _check(alpha, "alpha", (T, N))
    n_points = _opt(n_points, "n_points", (T,), torch.int32)
    dev = X.device
    if workspace is None:
        workspace = mll_backward_workspace(T, N, D, dev)
    elif workspace["shape"] != (T, N, D) or workspace["work"].device != dev:
        raise ValueError("workspace does not match this call's (T, N, D) / device")
    work, partials = workspace["work"], workspace["partials"]
    with torch.cuda.device(dev):
        rc = _lib.lib.scaml_mll_backward_f64(_ptr(X), _ptr(theta), _ptr(L), _ptr(Linv_diag), _ptr(alpha), _ptr(n_points),
                                             T, N, D, int(kind), _ptr(work), _ptr(partials), _stream_handle())
    _lib.check_rc(rc, "scaml_mll_backward_f64")
    n = n_points.to(torch.float64) if n_points is not None else torch.full((T,), float(N), dtype=torch.float64, device=dev)
    return partials.sum(1) / (2.0 * n.clamp_min(1.0)).unsqueeze(-1)


class FusedMLL(torch.autograd.Function):
    """mll (T,) = FusedMLL.apply(X, y, theta, kind, n_points): the marginal log-likelihood of every task of the
    stack as a differentiable torch op.  forward = one launch of scaml_gp_fit_fused_f64 (K, jittered Cholesky,
    alpha, MLL), backward = scaml_mll_backward_f64 (analytic d mll / d theta; no gradient flows to X or y).
    Replaces the autograd pass through kernel -> Cholesky -> solves that botorch's fit_gpytorch_mll runs per
    L-BFGS-B iteration (scamlgp/utils.py:175, 190).  Tasks whose factorisation fails even with jitter give
    mll = NaN and a zero gradient; ``FusedMLL.last`` keeps the last forward's outputs (info, jitter, L, alpha)."""

    last: Optional[Dict[str, torch.Tensor]] = None
    workspace: Optional[Dict[str, torch.Tensor]] = None

    @staticmethod
    def forward(ctx, X, y, theta, kind, n_points=None, out=None):
        # (N > scaml_fit_max_n() goes through the two-block composite, which allocates its own outputs)
        if out is not None and X.shape[1] > _lib.lib.scaml_fit_max_n():
            out = None
        fit = gp_fit_fused(X.detach(), y.detach(), theta.detach(), kind, n_points=n_points, want_linv=True, zero_upper=False,
                           out=out)
        ctx.kind, ctx.n_points = int(kind), n_points
        ctx.save_for_backward(X.detach(), theta.detach(), fit["L"], fit["Linv_diag"], fit["alpha"], fit["info"])
        FusedMLL.last = fit
        return fit["mll"].clone()

    @staticmethod
    def backward(ctx, grad_mll):
        X, theta, L, Linv_diag, alpha, info = ctx.saved_tensors
        ws = FusedMLL.workspace
        if ws is not None and (ws["shape"] != tuple(X.shape) or ws["work"].device != X.device):
            ws = None
        if ws is None:
            ws = FusedMLL.workspace = mll_backward_workspace(*X.shape, X.device)
        g = mll_backward(X, theta, ctx.kind, L, Linv_diag, alpha, n_points=ctx.n_points, workspace=ws)
        g = torch.where((info > 0).unsqueeze(-1), torch.zeros_like(g), g)
        return None, None, g * grad_mll.unsqueeze(-1), None, None, None


class GaussianLogProb(torch.autograd.Function):
    """log N(resid | 0, K) for ONE given covariance matrix K (n, n), n <= scaml_fit_max_n(), as a differentiable torch op on the
    library's launches: forward = scaml_potrf_batched_f64 (T = 1; psd_safe_cholesky's jitter ladder in-kernel, alpha, quad, logdet),
    backward = scaml_cho_solve_batched_f64 with the identity as right-hand side (K^-1), d/dK = (alpha alpha^T - K^-1) / 2,
    d/dresid = -alpha.  This is the MultivariateNormal.log_prob of the TARGET GP's marginal likelihood
    (scamlgp/utils.py:171-177 on the ScaMLGP model of scamlgp/model.py:359-384), whose K is not a kernel matrix of points but
    weighted source covariances + target kernel + noise.  Nothing synchronises with the host: a factorisation that fails even
    with jitter gives NaN (value and gradient), and the status of the last call is in ``GaussianLogProb.last_info``."""

    last_info: Optional[torch.Tensor] = None

    @staticmethod
    def forward(ctx, K, resid):
        n = K.shape[-1]
        f = potrf_batched(K.detach().reshape(1, n, n).contiguous(), resid.detach().reshape(1, n).contiguous(), want_linv=True)
        GaussianLogProb.last_info = f["info"]
        ctx.save_for_backward(f["L"], f["Linv_diag"], f["alpha"], f["info"])
        nan = torch.where(f["info"] > 0, float("nan"), 0.0).to(torch.float64)
        return (-0.5 * (f["quad"] + f["logdet"] + n * 1.8378770664093453) + nan).reshape(())

    @staticmethod
    def backward(ctx, g):
        L, W, alpha, info = ctx.saved_tensors
        n = L.shape[-1]
        eye = torch.eye(n, dtype=torch.float64, device=L.device).unsqueeze(0)
        Kinv = cho_solve(L, W, eye)[0]
        a = alpha[0]
        nan = torch.where(info > 0, float("nan"), 0.0).to(torch.float64)
        gK = 0.5 * (torch.outer(a, a) - Kinv) + nan
        return g * gK, g * (-a + nan)


def gaussian_log_prob(K: torch.Tensor, resid: torch.Tensor) -> torch.Tensor:
    """Functional form of ``GaussianLogProb``."""
    return GaussianLogProb.apply(K, resid)


def fused_mll(X: torch.Tensor, y: torch.Tensor, theta: torch.Tensor, kind: int,
              n_points: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
    """Functional form of ``FusedMLL``.  ``out`` (the dict ``FusedMLL.last`` of an earlier call with the same shapes)
    lets an optimiser loop reuse the factor buffers: the caller then runs backward before the next forward."""
    return FusedMLL.apply(X, y, theta, kind, n_points, out)



def _spec_host(spec, kernel: str, weights=None):
    """The host block of doubles the optimiser kernels read (include/scaml_gp.h (8), (9)): the Interval bounds and (kind, p1, p2) of
    the lengthscale / outputscale / noise priors -- 15 doubles; ``weights`` = (prior, lower bound) appends the target's four."""
    import ctypes

    from . import hyper

    def prior(pr):
        if pr is None:
            return [0.0, 0.0, 0.0]
        if isinstance(pr, hyper.GammaPrior):
            return [1.0, pr.concentration, pr.rate]
        if isinstance(pr, hyper.LogNormalPrior):
            return [2.0, pr.loc, pr.scale]
        raise TypeError(f"prior {type(pr).__name__} is not supported by the {kernel} kernel")

    vals = [spec.ls_constraint.lower, spec.ls_constraint.upper, spec.os_constraint.lower, spec.os_constraint.upper,
            spec.noise_constraint.lower, spec.noise_constraint.upper, *prior(spec.ls_prior), *prior(spec.os_prior), *prior(spec.noise_prior)]
    if weights is not None:
        vals += [*prior(weights[0]), weights[1]]
    return (ctypes.c_double * len(vals))(*[float(v) for v in vals])


# ---- (8) target GP: objective + gradient / whole refit in one launch -------------------------------------------------------
class TargetFitProblem:
    """Device-resident inputs of ``scaml_target_mll_f64`` / ``scaml_target_fit_f64`` for ONE ScaMLGP training set: the source
    terms cached at construction (scamlgp/model.py:279-289) in the kernel's layouts -- means (T, n), covariances packed lower
    (T, n (n + 1) / 2) --, the target inputs / standardised targets, the standardiser and the constraint / prior block.
    Built once per model; every objective evaluation and the refit reuse it."""

    def __init__(self, source_means: torch.Tensor, source_covs: torch.Tensor, train_X: torch.Tensor, train_targets: torch.Tensor,
                 m_all: float, s_all: float, spec, weights_prior, weights_lower_bound: float, kind: int):
        n, T = source_means.shape
        D = train_X.shape[-1]
        self.n, self.T, self.D, self.kind = int(n), int(T), int(D), int(kind)
        self.P = D + 2 + T
        self.device = train_X.device
        self.means_t = _check(source_means.transpose(0, 1), "source_means^T", (T, n))
        ia, ib = torch.tril_indices(n, n, device=self.device)
        self.covs_p = source_covs[ia, ib, :].transpose(0, 1).contiguous()          # (T, n (n + 1) / 2): plumbing, once per model
        self.X = _check(train_X, "train_X", (n, D))
        self.y = _check(train_targets, "train_targets", (n,))
        self.m_all, self.s_all = float(m_all), float(s_all)
        self.spec_host = _spec_host(spec, "target-fit", (weights_prior, weights_lower_bound))

    @staticmethod
    def supported(n: int, T: int, D: int) -> bool:
        return D <= _lib.lib.scaml_target_fit_max_d() and 1 <= n <= _lib.lib.scaml_target_fit_max_n(T, D)

    _symbol = "scaml_target_%s"   # (+ "_f64" / "_workspace_doubles"; "%s": mll or fit)

    def _problem_args(self):
        return (_ptr(self.means_t), _ptr(self.covs_p), _ptr(self.X), _ptr(self.y), self.m_all, self.s_all, self.spec_host)

    def _dims(self):
        """(leading shape of the results in front of B, the n the entry point takes)."""
        return (), self.n


def _target_launch(prob, z: torch.Tensor, fit=None) -> Dict[str, torch.Tensor]:
    """The one call path of the four wrappers below.  ``prob``: a TargetFitProblem with z (B, P), or a TargetFitBatch with z (S, B, P).
    ``fit`` None: value and gradient at z; ``fit`` = (max_iter, history, gtol, ftol): the L-BFGS runs from z, which is overwritten."""
    lead, n = prob._dims()
    B = z.shape[-2]
    dev = prob.device
    name = prob._symbol % ("mll" if fit is None else "fit")
    with torch.cuda.device(dev):
        value = _empty(dev, *lead, B)
        info = _empty(dev, *lead, B, dtype=torch.int32)
        jit = _empty(dev, *lead, B)
        head = (*prob._problem_args(), _ptr(z), *lead, B, n, prob.T, prob.D, prob.kind)
        if fit is None:
            grad = _empty(dev, *lead, B, prob.P)
            rc = getattr(_lib.lib, name + "_f64")(*head, _ptr(value), _ptr(grad), _ptr(info), _ptr(jit), _stream_handle())
            out = dict(value=value, grad=grad, info=info, jitter=jit)
        else:
            max_iter, history, gtol, ftol = fit
            stats = torch.zeros((*lead, B, 4), dtype=torch.int32, device=dev)
            nws = int(getattr(_lib.lib, name + "_workspace_doubles")(*lead, B, prob.T, prob.D, history))
            ws = _empty(dev, max(nws, 1))
            rc = getattr(_lib.lib, name + "_f64")(*head, int(max_iter), int(history), float(gtol), float(ftol), _ptr(value), _ptr(info),
                                                  _ptr(jit), _ptr(stats), _ptr(ws), nws, _stream_handle())
            ws.record_stream(torch.cuda.current_stream(dev))
            out = dict(z=z, value=value, info=info, jitter=jit, stats=stats)
    _lib.check_rc(rc, name + "_f64")
    return out


def target_mll(prob: TargetFitProblem, z: torch.Tensor) -> Dict[str, torch.Tensor]:
    """mll(z_b) and d mll / d z_b for the rows of z (B, D + 2 + T) = [raw lengthscales, raw outputscale, raw noise, weights]:
    the ScaMLGP training objective of scamlgp/model.py:360-363 + utils.py:171-177 (priors included, divided by n) with its
    analytic gradient, ONE launch of scaml_target_mll_f64.  Returns dict(value (B,), grad (B, P), info (B,), jitter (B,));
    a matrix that is not positive definite even with jitter 1e-6 gives value NaN, info > 0 and a zero gradient."""
    return _target_launch(prob, _check(z, "z", (z.shape[0], prob.P)))


def target_fit(prob: TargetFitProblem, z0: torch.Tensor, max_iter: int = 200, history: int = 10, gtol: float = 1e-5,
               ftol: float = 2.2e-9) -> Dict[str, torch.Tensor]:
    """Maximise mll from every row of z0 (B, P) on the device: ONE launch of scaml_target_fit_f64 runs all B L-BFGS
    optimisations (warm start + restarts of scamlgp/utils.py:184-199) to convergence -- no host round trip per evaluation.
    Returns dict(z (B, P) optima, value (B,) mll there, info, jitter, stats (B, 4) = [iterations, evaluations, status, 0])."""
    return _target_launch(prob, _check(z0, "z0", (z0.shape[0], prob.P)).clone(), (max_iter, history, gtol, ftol))


# ---- (8b) the same over a batch of training sets: S problems x B start points in one launch -----------------------------------
class TargetFitBatch:
    """S ``TargetFitProblem``s (anything with their attributes) in the layouts of ``scaml_target_mll_batched_f64`` /
    ``scaml_target_fit_batched_f64``: means (S, T, n_max), packed covariances (S, T, n_max (n_max + 1) / 2), inputs (S, n_max, D),
    targets (S, n_max), the counts n_s (S,) int32 and the standardisers m_all, s_all (S,) as device arrays.  The problems share T, D,
    the kernel family, the device and the constraint / prior block; they may differ in n (ragged: the packed index does not depend on
    n, so problem s fills the leading part of its slices and the rest -- zeros here -- is never read)."""

    def __init__(self, problems):
        problems = list(problems)
        if not problems:
            raise ValueError("TargetFitBatch needs at least one problem")
        p0 = problems[0]
        self.S, self.T, self.D, self.kind, self.P, self.device = len(problems), p0.T, p0.D, p0.kind, p0.P, p0.device
        self.spec_host = p0.spec_host
        for p in problems[1:]:
            if (p.T, p.D, p.kind, p.device) != (self.T, self.D, self.kind, self.device) or list(p.spec_host) != list(p0.spec_host):
                raise ValueError("the problems of a TargetFitBatch must share T, D, the kernel family, the device and the constraint / prior block")
        self.sizes = [int(p.n) for p in problems]
        self.n_max = n_max = max(self.sizes)
        dev, S, T, D = self.device, self.S, self.T, self.D
        self.means_t = torch.zeros(S, T, n_max, dtype=torch.float64, device=dev)
        self.covs_p = torch.zeros(S, T, n_max * (n_max + 1) // 2, dtype=torch.float64, device=dev)
        self.X = torch.zeros(S, n_max, D, dtype=torch.float64, device=dev)
        self.y = torch.zeros(S, n_max, dtype=torch.float64, device=dev)
        for s, p in enumerate(problems):
            n = self.sizes[s]
            self.means_t[s, :, :n].copy_(p.means_t)
            self.covs_p[s, :, :n * (n + 1) // 2].copy_(p.covs_p)
            self.X[s, :n].copy_(p.X)
            self.y[s, :n].copy_(p.y)
        self.n_points = torch.tensor(self.sizes, dtype=torch.int32).to(dev)
        self.m_all = torch.tensor([float(p.m_all) for p in problems], dtype=torch.float64).to(dev)
        self.s_all = torch.tensor([float(p.s_all) for p in problems], dtype=torch.float64).to(dev)

    @staticmethod
    def supported(n_max: int, T: int, D: int) -> bool:
        return TargetFitProblem.supported(n_max, T, D)

    _symbol = "scaml_target_%s_batched"

    def _problem_args(self):
        return (_ptr(self.means_t), _ptr(self.covs_p), _ptr(self.X), _ptr(self.y), _ptr(self.n_points), _ptr(self.m_all), _ptr(self.s_all),
                self.spec_host)

    def _dims(self):
        return (self.S,), self.n_max


def target_mll_batched(batch: TargetFitBatch, z: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``target_mll`` for every (problem, start): z (S, B, P) -> dict(value (S, B), grad (S, B, P), info (S, B), jitter (S, B)), ONE
    launch of scaml_target_mll_batched_f64 (S * B workgroups).  Row (s, b) is what ``target_mll`` gives for problem s at z[s, b]."""
    if z.dim() != 3:
        raise ValueError(f"z must have shape (S, B, P) (got {tuple(z.shape)})")
    return _target_launch(batch, _check(z, "z", (batch.S, z.shape[1], batch.P)))


def target_fit_batched(batch: TargetFitBatch, z0: torch.Tensor, max_iter: int = 200, history: int = 10, gtol: float = 1e-5,
                       ftol: float = 2.2e-9) -> Dict[str, torch.Tensor]:
    """``target_fit`` for every (problem, start): all S * B L-BFGS optimisations in ONE launch of scaml_target_fit_batched_f64.
    z0 (S, B, P) -> dict(z (S, B, P), value (S, B), info, jitter, stats (S, B, 4)); row (s, b) is what ``target_fit`` gives for
    problem s from z0[s, b]."""
    if z0.dim() != 3:
        raise ValueError(f"z0 must have shape (S, B, P) (got {tuple(z0.shape)})")
    return _target_launch(batch, _check(z0, "z0", (batch.S, z0.shape[1], batch.P)).clone(), (max_iter, history, gtol, ftol))


# ---- the L-BFGS state machine of (9) and (7h): csrc/gp_lbfgs_core.h ---------------------------------------------------------------
_LBFGS_SCALARS = 16             # LBFGS_SCALARS
# status codes of both optimisers (stats[:, 2] of stack_fit and of StudiesAcqfOpt; "padding" only in the latter)
ACQF_OPT_STATUS = ("running", "converged", "ftol", "stalled", "failed", "max_iter", "padding")


def _lbfgs_state_doubles(P: int, history: int) -> int:
    """Doubles of one problem's optimiser state at the head of the workspace: ``lbfgs_state_doubles`` of csrc/gp_lbfgs_core.h (x, g, d,
    xt, the curvature pairs, rho, the scalars; tests/test_stack_fit_emul.py and tests/test_acqf_opt_emul.py compare the two)."""
    return (4 + 2 * history) * P + history + _LBFGS_SCALARS


stack_fit_state_doubles = studies_acqf_opt_state_doubles = _lbfgs_state_doubles


def _lbfgs_state(ws: torch.Tensor, B: int, P: int, history: int) -> torch.Tensor:
    """(B, _lbfgs_state_doubles(P, history)) float64: the per-problem state that opens the workspace (include/scaml_gp.h), a view."""
    stride = _lbfgs_state_doubles(P, history)
    return ws[: B * stride * 8].view(torch.float64).reshape(B, stride)


def _lbfgs_rounds(enqueue, stats: torch.Tensor, per_call: int, budget: int, live: bool, n_eval: int = 0, n_calls: int = 0) -> Dict:
    """The chunked round loop of both optimisers: ``enqueue(k, n_calls)`` enqueues k rounds (n_calls == 0: from a reset), then the status
    column is read -- the only synchronisation -- and the loop goes on while a problem is still running and the budget of
    ``1 + max_iter * max_ls`` evaluations is not spent.  Returns dict(stats on the host, n_eval rounds enqueued, n_calls)."""
    if per_call < 1:
        raise ValueError("evals_per_call must be positive")
    host = stats.cpu()
    while live:
        k = min(per_call, budget - n_eval)
        enqueue(k, n_calls)
        n_eval += k
        n_calls += 1
        host = stats.cpu()
        if not bool((host[:, 2] == 0).any()) or n_eval >= budget:
            break
    return dict(stats=host, n_eval=n_eval, n_calls=n_calls)


# ---- (9) source stack: the whole hyper-parameter fit enqueued on the device ---------------------------------------------------
# rounds enqueued between two reads of the status.  Measured (tools/dev_stackfit_time.py, profiles/stack_fit_timings.txt): the cost per
# evaluation is flat from 4 on (the rounds are GPU-bound), and every round past the last problem's stop is a wasted evaluation of the
# whole batch, so the smallest value past the knee is the default.
STACK_FIT_EVALS_PER_CALL = 4
_STACK_FIT_MAX_LS = 20          # trials per line search inside scaml_stack_fit_f64


def stack_spec_host(spec):
    """The 15 host doubles ``scaml_stack_fit_f64`` reads: Interval bounds and (kind, p1, p2) of the three hyper-priors."""
    return _spec_host(spec, "stack-fit")


def stack_fit(X: torch.Tensor, y: torch.Tensor, n_points: Optional[torch.Tensor], spec, z0: torch.Tensor, kind: int, *,
              max_iter: int = 200, history: int = 10, gtol: float = 1e-5, ftol: float = 2.2e-9,
              evals_per_call: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Minimise -(mll + sum log p(theta) / n) from every row of z0 (B, D + 2) (raw parameters; problem b uses X[b], y[b]) with
    ``scaml_stack_fit_f64``: every call enqueues ``evals_per_call`` rounds of fit + MLL gradient + optimiser step for all B problems,
    then the status column is read -- the only synchronisation -- and the fit continues while a problem is still running (at most
    ``1 + max_iter * 20`` evaluations: then every problem has stopped).  ``hyper.batched_lbfgs`` per problem, without the host.
    Returns dict(z (B, D+2) accepted points, value (B,) mll + prior term there, grad (B, D+2) gradient of -value there,
    stats (B, 4) int32 [iterations, evaluations, status, 0] on the host, n_eval rounds enqueued, n_calls)."""
    if X.dim() != 3:
        raise ValueError("X must be (B, N, D)")
    B, N, D = X.shape
    P = D + 2
    X = _check(X, "X")
    y = _check(y, "y", (B, N))
    z = _check(z0, "z0", (B, P)).clone()
    n_points = _opt(n_points, "n_points", (B,), torch.int32)
    per_call = int(evals_per_call or STACK_FIT_EVALS_PER_CALL)
    spec_host = stack_spec_host(spec)
    dev = X.device
    with torch.cuda.device(dev):
        value = _empty(dev, B)
        stats = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        nbytes = int(_lib.lib.scaml_stack_fit_workspace_bytes(B, N, D, int(history)))
        ws = _empty(dev, max(nbytes, 16), dtype=torch.uint8)

        def enqueue(k, n_calls):
            rc = _lib.lib.scaml_stack_fit_f64(_ptr(X), _ptr(y), _ptr(n_points), spec_host, _ptr(z), B, N, D, int(kind), k,
                                              _lib.STACK_FIT_CONTINUE if n_calls else 0, int(max_iter), int(history), float(gtol),
                                              float(ftol), _ptr(value), _ptr(stats), _ptr(ws), nbytes, _stream_handle())
            _lib.check_rc(rc, "scaml_stack_fit_f64")

        out = _lbfgs_rounds(enqueue, stats, per_call, 1 + int(max_iter) * _STACK_FIT_MAX_LS, B > 0)
        grad = _lbfgs_state(ws, B, P, int(history))[:, P:2 * P].clone()
    return dict(z=z, value=value, grad=grad, **out)


# ---- (7h) the acquisition optimiser of many studies' start points enqueued on the device --------------------------------------
# rounds enqueued between two reads of the status.  Measured (tools/dev_studies_time.py --suggest --sweep 1,2,4,8,16,
# profiles/studies_suggest_device_timings.txt): the suggest time is flat within 10 % from 1 to 16 at S = 1, 8 and 32 -- a status
# read costs little next to a round, a round after the last stop evaluates no start -- and 8 is the fastest column or within 0.2 ms of it.
ACQF_OPT_EVALS_PER_CALL = 8
ACQF_OPT_MAX_LS = 20            # trials per line search (hyper.batched_lbfgs's max_ls)


class StudiesAcqfOpt:
    """One optimisation of ``scaml_studies_acqf_opt_f64``: the checked arguments, the workspace and the outputs, so that the rounds can
    be enqueued in chunks (``enqueue``; the first call resets, the later ones continue).  ``arrays``: the 22 device arrays of the C
    signature from ``x0`` to ``acqf_param``, in its order (None for the optional y_mean / y_std / n_points_s).  ``task_base`` (G,)
    int32: every study owns its source tasks (scaml_studies_acqf_opt_own_f64) -- the eight source arrays then hold ``Tsrc`` tasks and T
    is the tasks per study.  ``fantasy`` = (alpha_f (G, n_max, F_max), n_fant (G,) int32): studies may hold pending evaluations
    (scaml_studies_fantasy_acqf_opt_f64, with or without ``task_base``); the ``alpha_t`` slot of ``arrays`` is then not used (None)."""

    def __init__(self, arrays, B: int, G: int, n_max: int, T: int, N: int, D: int, kind_s: int, kind_t: int, acqf: int, lo: torch.Tensor, hi: torch.Tensor,
                 max_iter: int, history: int = 10, max_ls: int = ACQF_OPT_MAX_LS, gtol: float = 1e-5, ftol: float = 2.2e-9, c1: float = 1e-4,
                 task_base: Optional[torch.Tensor] = None, Tsrc: Optional[int] = None, fantasy=None):
        dev = arrays[0].device
        i32, u8, i64, f64, nbm = torch.int32, torch.uint8, torch.int64, torch.float64, (n_max + 15) // 16
        if (task_base is None) != (Tsrc is None):
            raise ValueError("task_base and Tsrc go together")
        Ts = T if task_base is None else int(Tsrc)   # tasks in the source arrays
        self._own = None if task_base is None else (_check(task_base, "task_base", (G,), i32), Ts)
        spec = [("x0", (B, D), f64), ("group", (B,), i32), ("VA_tab", (G,), i64), ("X", (Ts, N, D), f64), ("theta_s", (Ts, D + 2), f64),
                ("Linv", (Ts, N, N), f64), ("alpha_s", (Ts, N), f64), ("y_mean", (Ts,), f64), ("y_std", (Ts,), f64), ("n_points_s", (Ts,), i32),
                ("w", (G, T), f64), ("active", (G, T), u8), ("Xt", (G, n_max, D), f64), ("theta_t", (G, D + 2), f64),
                ("L", (G, n_max, n_max), f64), ("Linv_diag", (G, nbm, 16, 16), f64), ("alpha_t", (G, n_max), f64), ("n_points_t", (G,), i32),
                ("m_all", (G,), f64), ("s_all", (G,), f64), ("info", (G,), i32), ("acqf_param", (G,), f64)]
        if len(arrays) != len(spec):
            raise ValueError(f"expected {len(spec)} arrays, got {len(arrays)}")
        self._fantasy = fantasy is not None
        if self._fantasy:
            if fantasy[0].dim() != 3:
                raise ValueError("alpha_f must be (G, n_max, F_max)")
            F_max = int(fantasy[0].shape[2])
            arrays = list(arrays)
            arrays[16:17] = fantasy   # alpha_f and n_fant stand where alpha_t stood
            spec[16:17] = [("alpha_f", (G, n_max, F_max), f64), ("n_fant", (G,), i32)]
        arrays = [_opt(a, name, shape, dt) for a, (name, shape, dt) in zip(arrays, spec)]
        self._keep = arrays
        self._ptrs = [_ptr(a) for a in arrays]
        self._shape = (B, G, n_max, *((F_max,) if self._fantasy else ()), T, N, D, int(kind_s), int(kind_t), int(acqf))
        self._dims = (B, G, D)
        self._opts = (int(max_iter), int(history), int(max_ls), float(gtol), float(ftol), float(c1))
        self.lo, self.hi = _check(lo, "lo", (D,)), _check(hi, "hi", (D,))
        self.device, self.n_calls, self.n_eval = dev, 0, 0
        self.budget = 1 + int(max_iter) * int(max_ls)
        with torch.cuda.device(dev):
            self.x, self.f = _empty(dev, B, D), _empty(dev, B)
            self.stats = torch.zeros((B, 4), dtype=torch.int32, device=dev)
            self.nbytes = int(_lib.lib.scaml_studies_acqf_opt_workspace_bytes(B, G, n_max, T, D, int(history)))
            if self.nbytes == 0 and B > 0:
                raise ValueError("scaml_studies_acqf_opt_f64: problem size exceeds kernel limits")
            self.ws = _empty(dev, max(self.nbytes, 16), dtype=torch.uint8)

    def enqueue(self, n_evals: int) -> None:
        fn, own = ("scaml_studies_acqf_opt_f64", ()) if self._own is None else ("scaml_studies_acqf_opt_own_f64", (_ptr(self._own[0]), self._own[1]))
        if self._fantasy:   # one entry for both: task_base NULL is the shared stack
            fn, own = "scaml_studies_fantasy_acqf_opt_f64", own or (None, 0)
        with torch.cuda.device(self.device):
            rc = getattr(_lib.lib, fn)(*self._ptrs, *self._shape, _ptr(self.lo), _ptr(self.hi), *self._opts, int(n_evals),
                                       _lib.ACQF_OPT_CONTINUE if self.n_calls else 0, _ptr(self.ws), _ptr(self.x), _ptr(self.f),
                                       _ptr(self.stats), *own, _stream_handle())
        _lib.check_rc(rc, fn)
        self.n_calls += 1
        self.n_eval += int(n_evals)

    def run(self, evals_per_call: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Every call enqueues ``evals_per_call`` rounds of grouped source pass + batched acquisition + optimiser step for all B starts,
        then the status column is read -- the only synchronisation -- and the optimisation continues while a start is still running (at
        most ``1 + max_iter * max_ls`` evaluations: then every start has stopped).  Returns dict(x (B, D), f (B,) the acquisition value
        there, stats (B, 4) int32 [iterations, evaluations, status, pairs] on the host, n_eval rounds enqueued, n_calls, state)."""
        out = _lbfgs_rounds(lambda k, _: self.enqueue(k), self.stats, int(evals_per_call or ACQF_OPT_EVALS_PER_CALL), self.budget,
                            self._dims[0] > 0 and self._dims[1] > 0, self.n_eval, self.n_calls)
        return dict(x=self.x, f=self.f, state=self.state(), **out)

    def state(self) -> torch.Tensor:
        """(B, studies_acqf_opt_state_doubles(D, history)): the per-start state that opens the workspace (a view)."""
        return _lbfgs_state(self.ws, self._dims[0], self._dims[2], self._opts[1])


def studies_acqf_opt(arrays, B: int, G: int, n_max: int, T: int, N: int, D: int, kind_s: int, kind_t: int, acqf: int, lo: torch.Tensor, hi: torch.Tensor,
                     max_iter: int, evals_per_call: Optional[int] = None, **options) -> Dict[str, torch.Tensor]:
    """Maximise the studies' acquisition functions from every start with ``scaml_studies_acqf_opt_f64`` (``StudiesAcqfOpt(...).run``):
    ``arrays`` are the 22 device arrays of the C signature from ``x0`` to ``acqf_param``, ``kind_s`` / ``kind_t`` the kernel families of the source stack and of the target kernels; ``options``: history, max_ls, gtol, ftol, c1."""
    return StudiesAcqfOpt(arrays, B, G, n_max, T, N, D, kind_s, kind_t, acqf, lo, hi, max_iter, **options).run(evals_per_call)


# ---- (7s), (7t) the optimiser of the joint q-point acquisition enqueued on the device --------------------------------------------
# rounds enqueued between two reads of the status: DESIGN 4t.  A start that has stopped leaves the evaluation kernels at the next chunk
# boundary (the caller's slot table), so the smaller chunk wins where the columns of tools/dev_qacqf_time.py --opt --sweep agree.
QACQF_OPT_EVALS_PER_CALL = 4


def qacqf_opt_max_p() -> int:
    """Variables per start (q * D) of the joint acquisition's optimiser step."""
    return int(_lib.lib.scaml_qacqf_opt_max_p())


def qacqf_opt_step(state: torch.Tensor, mode: int, lo: torch.Tensor, hi: torch.Tensor, Xq: torch.Tensor, x: torch.Tensor, f: torch.Tensor,
                   stats: torch.Tensor, x0: Optional[torch.Tensor] = None, value: Optional[torch.Tensor] = None,
                   grad: Optional[torch.Tensor] = None, slots: Optional[torch.Tensor] = None, max_iter: int = 50, history: int = 10,
                   max_ls: int = ACQF_OPT_MAX_LS, gtol: float = 1e-5, ftol: float = 2.2e-9, c1: float = 1e-4) -> None:
    """One launch of scaml_qacqf_opt_step_f64 (7t), in place: a box L-BFGS step of B starts of P <= 128 variables that MAXIMISES.
    ``state`` (B, studies_acqf_opt_state_doubles(P, history)); ``mode`` 0 resets from ``x0`` (B, P), 1 consumes ``value`` (Bs,) /
    ``grad`` (Bs, P) -- the function at ``Xq`` (Bs, P), which then receives the next trial points --, 2 writes the outputs again for a
    changed ``slots`` (Bs,) int32 table (None: the identity).  ``x`` (B, P), ``f`` (B,), ``stats`` (B, 4) int32 are addressed by start."""
    B, P = x.shape
    Bs = B if slots is None else int(slots.shape[0])
    state = _check(state, "state", (B, _lbfgs_state_doubles(P, int(history))))
    lo, hi = _check(lo, "lo", (P,)), _check(hi, "hi", (P,))
    Xq, x, f = _check(Xq, "Xq", (Bs, P)), _check(x, "x", (B, P)), _check(f, "f", (B,))
    stats = _check(stats, "stats", (B, 4), torch.int32)
    x0 = _opt(x0, "x0", (B, P))
    value, grad = _opt(value, "value", (Bs,)), _opt(grad, "grad", (Bs, P))
    slots = _opt(slots, "slots", (Bs,), torch.int32)
    with torch.cuda.device(state.device):
        rc = _lib.lib.scaml_qacqf_opt_step_f64(_ptr(value), _ptr(grad), _ptr(slots), _ptr(x0), _ptr(lo), _ptr(hi), B, Bs, P, int(mode),
                                               int(max_iter), int(history), int(max_ls), float(gtol), float(ftol), float(c1), _ptr(state),
                                               _ptr(Xq), _ptr(x), _ptr(f), _ptr(stats), _stream_handle())
    _lib.check_rc(rc, "scaml_qacqf_opt_step_f64")


class QAcqfOpt:
    """One optimisation of ``scaml_qacqf_opt_f64`` (7s): the checked arguments, the workspace and the outputs, so that the rounds can be
    enqueued in chunks (``enqueue``; the first call resets, the later ones continue).  ``arrays``: the round-independent device arrays
    by the C signature's names, as ``ScaMLGP.joint_acqf_opt_inputs`` returns them (Xa, X, theta_s, Linv, alpha_s, y_mean, y_std,
    n_points_s, VA, w, active, mu_t, cov_tt, var_t, Xt, theta_t, targets, L, Linv_diag, alpha_t, info, base_samples and, with points
    pending, Xp, Zp, mu_p, Sigma_pp; the floats m_all, s_all; the ints kind_s, kind_t).  ``x0`` (B, q, D): the start batches.
    ``slots``: the starts the next call works on (all of them after construction); ``run`` rebuilds it from the starts still running
    after every status read, so that a stopped start costs the evaluation kernels nothing from the next call on."""

    def __init__(self, arrays: Dict, x0: torch.Tensor, acqf: int, acqf_param: float, lo: torch.Tensor, hi: torch.Tensor, max_iter: int,
                 history: int = 10, max_ls: int = ACQF_OPT_MAX_LS, gtol: float = 1e-5, ftol: float = 2.2e-9, c1: float = 1e-4):
        if x0.dim() != 3:
            raise ValueError("x0 must be (B, q, D)")
        B, q, D = (int(v) for v in x0.shape)
        f64, i32 = torch.float64, torch.int32
        a = dict(arrays)
        X = _check(a["X"], "X")
        T, N, _ = X.shape
        n = int(a["Xt"].shape[0])
        S, Q = (int(v) for v in a["base_samples"].shape)
        p = Q - q
        if p < 0 or (p > 0) != (a.get("Xp") is not None):
            raise ValueError("base_samples must be (S, q + p) with p = Xp.shape[0] pending points")
        nbm = (n + 15) // 16
        spec = [("Xa", (n + p, D), f64), ("X", (T, N, D), f64), ("theta_s", (T, D + 2), f64), ("Linv", (T, N, N), f64), ("alpha_s", (T, N), f64),
                ("y_mean", (T,), f64), ("y_std", (T,), f64), ("n_points_s", (T,), i32), ("VA", (T, N, n + p), f64), ("w", (T,), f64),
                ("active", (T,), torch.uint8), ("mu_t", (n,), f64), ("cov_tt", (n, n), f64), ("var_t", (n,), f64), ("Xt", (n, D), f64),
                ("theta_t", (D + 2,), f64), ("targets", (n,), f64), ("L", (1, n, n), f64), ("Linv_diag", (1, nbm, 16, 16), f64),
                ("alpha_t", (n,), f64)]
        tail = [("info", (1,), i32), ("base_samples", (S, Q), f64), ("Xp", (p, D), f64), ("Zp", (n, p), f64), ("mu_p", (p,), f64),
                ("Sigma_pp", (p, p), f64)]
        self._keep = [_opt(a.get(name), name, shape, dt) for name, shape, dt in spec + tail]
        self._head = [_ptr(t) for t in self._keep[:len(spec)]]
        self._tail = [_ptr(t) for t in self._keep[len(spec):]]
        self._scale = (float(a["m_all"]), float(a["s_all"]))
        self._shape = (n, p, q, S, T, N, D, int(a["kind_s"]), int(a["kind_t"]), int(acqf))
        self._param = float(acqf_param)
        self._dims = (B, q, D)
        self._opts = (int(max_iter), int(history), int(max_ls), float(gtol), float(ftol), float(c1))
        P = q * D
        self.x0 = _check(x0.reshape(B, P), "x0", (B, P))
        self.lo, self.hi = _check(lo, "lo", (P,)), _check(hi, "hi", (P,))
        dev = self.x0.device
        self.device, self.n_calls, self.n_eval, self.live = dev, 0, 0, []
        self.budget = 1 + int(max_iter) * int(max_ls)
        with torch.cuda.device(dev):
            self.x, self.f = _empty(dev, B, P), _empty(dev, B)
            self.stats = torch.zeros((B, 4), dtype=i32, device=dev)
            self.nbytes = int(_lib.lib.scaml_qacqf_opt_workspace_bytes(B, n, p, q, T, N, D, int(history)))
            if self.nbytes == 0:
                raise ValueError("scaml_qacqf_opt_f64: problem size exceeds kernel limits")
            self.ws = _empty(dev, max(self.nbytes, 16), dtype=torch.uint8)
            self.slots = torch.arange(B, dtype=i32, device=dev)

    def enqueue(self, n_evals: int) -> None:
        B = self._dims[0]
        Bs = int(self.slots.shape[0])
        with torch.cuda.device(self.device):
            rc = _lib.lib.scaml_qacqf_opt_f64(_ptr(self.x0), _ptr(self.slots), *self._head, *self._scale, *self._tail, B, Bs, *self._shape,
                                              self._param, _ptr(self.lo), _ptr(self.hi), *self._opts, int(n_evals),
                                              _lib.ACQF_OPT_CONTINUE if self.n_calls else 0, _ptr(self.ws), self.nbytes, _ptr(self.x),
                                              _ptr(self.f), _ptr(self.stats), _stream_handle())
        _lib.check_rc(rc, "scaml_qacqf_opt_f64")
        self.n_calls += 1
        self.n_eval += int(n_evals)
        self.live.append(Bs)

    def run(self, evals_per_call: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Every call enqueues ``evals_per_call`` rounds for the starts in ``slots``, then the status column is read -- the only
        synchronisation --, the stopped starts leave the table and the optimisation continues while a start is still running (at most
        ``1 + max_iter * max_ls`` evaluations: then every start has stopped).  Returns dict(x (B, q, D), f (B,) the acquisition value
        there, stats (B, 4) int32 [iterations, evaluations, status, pairs] on the host, n_eval rounds enqueued, n_calls, live: the
        slots of every call)."""
        per_call = int(evals_per_call or QACQF_OPT_EVALS_PER_CALL)
        if per_call < 1:
            raise ValueError("evals_per_call must be positive")
        host = self.stats.cpu()
        while self._dims[0] > 0 and self.n_eval < self.budget:
            self.enqueue(min(per_call, self.budget - self.n_eval))
            host = self.stats.cpu()
            running = torch.nonzero(host[:, 2] == 0).flatten()
            if running.numel() == 0:
                break
            self.slots = running.to(torch.int32).to(self.device)
        B, q, D = self._dims
        return dict(x=self.x.reshape(B, q, D), f=self.f, stats=host, n_eval=self.n_eval, n_calls=self.n_calls, live=list(self.live))

    def state(self) -> torch.Tensor:
        """(B, studies_acqf_opt_state_doubles(q * D, history)): the per-start state that opens the workspace (a view)."""
        B, q, D = self._dims
        return _lbfgs_state(self.ws, B, q * D, self._opts[1])


def raise_if_not_psd(info: torch.Tensor) -> None:
    """Host-side check of the per-task status (one device->host sync)."""
    if bool((info < 0).any()):
        # only the several-CUs-per-task fit reports this (csrc/gp_fit_coop.hip): its workgroups wait for each other inside one launch, with
        # bounded polls; a task given up after ~4 s means its workgroups were not resident together -- another launch (a second process
        # or stream on this GPU) held the CUs while waiting itself.  SCAML_BLOCKED_FIT_PATH=1 keeps to the sequence of launches.
        raise RuntimeError("scaml_gp_fit_blocked_f64: the one-launch fit timed out waiting for its own workgroups (the GPU is shared with "
                           "another long-running launch?); set SCAML_BLOCKED_FIT_PATH=1 to use the sequence of launches")
    bad = torch.nonzero(info > 0).flatten()
    if bad.numel():
        raise NotPSDError(
            f"Matrix not positive definite after repeatedly adding jitter up to 1.0e-06 "
            f"(tasks {bad.tolist()[:8]}{'...' if bad.numel() > 8 else ''})."
        )
