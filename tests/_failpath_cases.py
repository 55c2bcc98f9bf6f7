"""Seeded CPU inputs (and their references) for the failure and jitter-retry paths of the fused fit and the batched POTRF
(scaml_gp_fit_fused_f64 / scaml_potrf_batched_f64, csrc/gp_fit_fused.hip).

Four kinds of task:
  clean     positive definite at the first attempt
  rescued   fails below a target rung r of the ladder (1e-8, 1e-7, 1e-6) and succeeds at r.  The well-conditioned builders
            place the smallest eigenvalue of A + j I at j - r / 2 with cond(A + r I) <= 5, so the retried factor can be held to
            the tolerances of a first-attempt factor; the ill-conditioned builder (duplicated points) is the realistic case.
  hopeless  pivot k is negative at every rung while every leading minor below order k is safely positive definite: the status
            must be exactly k, as LAPACK reports it.
tests/test_failpath_inputs.py holds these properties against the oracle alone; tests/test_fit_failpath_gpu.py runs the
kernels on the same inputs.  A task's data depends on (seed, task index) only, never on the stack size.
"""
import functools
import math

import numpy as np
import torch

from oracle import gp_oracle as O
from scamlgp_amd import synthetic
from tests._dispatch import narrow_fit_tasks

F64 = torch.float64
RUNGS = (1e-8, 1e-7, 1e-6)
JITTER_IN_RETRY = 4.5e-8   # caller-side jitter on a rung-1e-7 task: attempt 0 at -5e-9, rung 1e-8 at +5e-9

# (instance, N, T): shapes that reach each kernel instance (fit_plan, csrc/gp_dispatch.h; tests/test_failpath_inputs.py holds the
# names to the plan).  T = None: the smallest stack the plan sends to the narrow instance on the device's CU count; the CPU test
# uses NARROW_T_CPU.
INSTANCES = {
    "nb2_wu1": (32, 9, 2),
    "nb4_wu3": (64, 9, 4),
    "nb8_wu7_wide": (100, 6, 8),
    "nb8_wu3_narrow": (100, None, 8),
    "nb16_wu7_n255": (255, 9, 16),
    "nb16_wu7_n256": (256, 9, 16),
}
NARROW_T_CPU = narrow_fit_tasks(256, N=INSTANCES["nb8_wu3_narrow"][0])      # MI355X: 256 CUs
RAGGED_SHORT = 5        # the ragged hopeless task has n = N - 5 valid points and fails at its last one
SMALL_PATTERN = ("clean", 1e-8, "hopeless", 1e-7, "hopeless", 1e-6, "hopeless", "clean", "hopeless")
CYCLE_PATTERN = ("clean", 1e-8, 1e-7, 1e-6, "hopeless")

RBF_LS, MATERN_LS = 0.45, 0.3                   # rescued / clean lattice fits
RBF_LS_HOPELESS, MATERN_LS_HOPELESS = 0.2, 0.1  # hopeless lattice fits: off-diagonals below 4e-6


def _eye(n):
    return torch.eye(n, dtype=F64)


def _gen(seed, t):
    return torch.Generator().manual_seed(1000003 * seed + t)


def hopeless_list(N, NB, k_min=1):
    """(k, n) of the hopeless tasks: k in {1, 16, 17, 16 (NB / 2) + 1, N - 1, N} at n = N, then the ragged one (k = n < N).
    k_min = 2 for the fit from X, whose builder fails pivot k through a copy of point 0 (k = 1 cannot fail that way)."""
    ks = []
    for k in (max(1, k_min), 16, 17, 16 * (NB // 2) + 1, N - 1, N):
        if k not in ks:
            ks.append(k)
    return [(k, N) for k in ks] + [(N - RAGGED_SHORT, N - RAGGED_SHORT)]


def plan(N, NB, T, part=0, k_min=1):
    """Task specs (what, rung, k, n) of one stack.  T <= 9: the first T entries of the interleaved SMALL_PATTERN; stack
    `part` continues in hopeless_list where the previous one stopped, so n_parts() stacks cover it.  Larger T: CYCLE_PATTERN,
    the hopeless tasks cycling through the whole list."""
    hl = hopeless_list(N, NB, k_min)
    small = T <= len(SMALL_PATTERN)
    pattern = SMALL_PATTERN if small else CYCLE_PATTERN
    out, h = [], (part * pattern[:T].count("hopeless") if small else 0)
    for t in range(T):
        what = pattern[t % len(pattern)]
        if what == "hopeless":
            k, n = hl[h % len(hl)]
            h += 1
            out.append(dict(what="hopeless", rung=None, k=k, n=n))
        elif what == "clean":
            # the second clean task of a part-1 stack is ragged too: a successful task with rows past n_t
            n = N - 3 if (small and part == 1 and t == 7) else N
            out.append(dict(what="clean", rung=None, k=0, n=n))
        else:
            out.append(dict(what="rescued", rung=what, k=0, n=N))
    return out


def n_parts(N, NB, T, k_min=1):
    """How many stacks of T <= 9 tasks it takes to place every entry of hopeless_list once."""
    if T > len(SMALL_PATTERN):
        return 1
    return -(-len(hopeless_list(N, NB, k_min)) // SMALL_PATTERN[:T].count("hopeless"))


# ---- matrices for the POTRF -------------------------------------------------------------------------------------------
def spd_matrix(n, g):
    B = torch.randn(n, n, dtype=F64, generator=g)
    return B @ B.T / n + _eye(n)


def rescued_matrix(n, rung, g):
    """A = r M - 1.5 r I with M = Q diag(lam) Q^T, lam uniform in [1, 3], lam[0] = 1: the smallest eigenvalue of A + j I is
    j - r / 2 and cond(A + r I) <= 5."""
    Q, _ = torch.linalg.qr(torch.randn(n, n, dtype=F64, generator=g))
    lam = 1.0 + 2.0 * torch.rand(n, dtype=F64, generator=g)
    lam[0] = 1.0
    M = (Q * lam) @ Q.T
    M = 0.5 * (M + M.T)
    return rung * M - 1.5 * rung * _eye(n)


def hopeless_matrix(n, k, g):
    A = spd_matrix(n, g)
    A[k - 1, k - 1] = -1.0
    return A


PAD_FILL = 7.0   # input rows / columns past n_t: never read by the kernel


@functools.lru_cache(maxsize=None)
def potrf_stack(N, NB, T, part=0, seed=1):
    """dict(A (T, N, N), y (T, N), n_points (T) int32, plan).  Read-only: clone before changing anything."""
    pl = plan(N, NB, T, part)
    A = torch.full((T, N, N), PAD_FILL, dtype=F64)
    y = torch.zeros(T, N, dtype=F64)
    for t, s in enumerate(pl):
        g, n = _gen(seed, t), s["n"]
        if s["what"] == "clean":
            M = spd_matrix(n, g)
        elif s["what"] == "rescued":
            M = rescued_matrix(n, s["rung"], g)
        else:
            M = hopeless_matrix(n, s["k"], g)
        A[t, :n, :n] = M
        y[t, :n] = torch.randn(n, dtype=F64, generator=g)
    return dict(A=A, y=y, n_points=torch.tensor([s["n"] for s in pl], dtype=torch.int32), plan=pl)


def task_matrix_potrf(case, t, jitter_in=0.0):
    n = case["plan"][t]["n"]
    return case["A"][t, :n, :n] + jitter_in * _eye(n)


# ---- fits from X on the lattice ---------------------------------------------------------------------------------------
def lattice(N):
    i = torch.arange(N)
    return torch.stack([(i % 16).to(F64), (i // 16).to(F64)], 1)


def _ls(kind, hopeless):
    if hopeless:
        return RBF_LS_HOPELESS if kind == O.KIND_RBF else MATERN_LS_HOPELESS
    return RBF_LS if kind == O.KIND_RBF else MATERN_LS


def oracle_kernel(X, theta, kind):
    """os k(X) without noise, the kernels' distance formulation."""
    D = X.shape[-1]
    return O.kernel_matrix(X, None, theta[:D], theta[D], kind, "direct")


@functools.lru_cache(maxsize=None)
def _lattice_lambda_min(N, kind):
    th = torch.tensor([_ls(kind, False)] * 2 + [1.0, 0.0], dtype=F64)
    return float(torch.linalg.eigvalsh(oracle_kernel(lattice(N), th, kind))[0])


@functools.lru_cache(maxsize=None)
def fit_stack(N, NB, T, kind, part=0, seed=2):
    """dict(X (T, N, 2), y (T, N), theta (T, 4), n_points, plan): lattice points; a rescued task has os = r and
    noise = -(lambda_min(K0) + r / 2), a hopeless one noise = -0.5 and point k a copy of point 0.  Read-only."""
    pl = plan(N, NB, T, part, k_min=2)
    X = lattice(N).repeat(T, 1, 1)
    y = torch.zeros(T, N, dtype=F64)
    theta = torch.zeros(T, 4, dtype=F64)
    for t, s in enumerate(pl):
        g, n = _gen(seed, t), s["n"]
        y[t, :n] = torch.randn(n, dtype=F64, generator=g)
        ls = _ls(kind, s["what"] == "hopeless")
        if s["what"] == "clean":
            theta[t] = torch.tensor([ls, ls, 1.0, 1e-2], dtype=F64)
        elif s["what"] == "rescued":
            r = s["rung"]
            theta[t] = torch.tensor([ls, ls, r, -(r * _lattice_lambda_min(N, kind) + 0.5 * r)], dtype=F64)
        else:
            theta[t] = torch.tensor([ls, ls, 1.0, -0.5], dtype=F64)
            X[t, s["k"] - 1] = X[t, 0]
    return dict(X=X, y=y, theta=theta, n_points=torch.tensor([s["n"] for s in pl], dtype=torch.int32), plan=pl, kind=kind)


def task_matrix_fit(case, t, jitter_in=0.0):
    """The oracle's K + (noise + jitter_in) I of task t (valid points only)."""
    n = case["plan"][t]["n"]
    th = case["theta"][t]
    return oracle_kernel(case["X"][t, :n], th, case["kind"]) + (float(th[-1]) + jitter_in) * _eye(n)


def clean_fit_stack(case, seed=3):
    """The same stack with every rescued / hopeless slot refilled with clean data: same T, hence the same kernel instance;
    the clean slots are the mixed stack's, bit for bit."""
    X, y, theta = case["X"].clone(), case["y"].clone(), case["theta"].clone()
    N = X.shape[1]
    ls = _ls(case["kind"], False)
    for t, s in enumerate(case["plan"]):
        if s["what"] != "clean":
            X[t] = lattice(N)
            y[t] = torch.randn(N, dtype=F64, generator=_gen(seed, t))
            theta[t] = torch.tensor([ls, ls, 1.0, 1e-2], dtype=F64)
    pl = [dict(what="clean", rung=None, k=0, n=s["n"] if s["what"] == "clean" else N) for s in case["plan"]]
    return dict(X=X, y=y, theta=theta, n_points=torch.tensor([s["n"] for s in pl], dtype=torch.int32), plan=pl, kind=case["kind"])


# ---- ill-conditioned rescue: duplicated points ----------------------------------------------------------------------
DUP_NOISE = {1e-8: -2e-9, 1e-7: -5e-8, 1e-6: -5e-7}
DUP_SHAPES = ((100, 6), (256, 8))   # (N, D): the wide (8, 7) instance and (16, 7)


def stack_like_fit_tests(T, N, D, seed, ls=0.5, noise=1e-3, spread=0.4):
    """The `_stack` helper of tests/test_fit_gpu.py (kept there for its own tests; restated so that this CPU-only module
    does not import a GPU test module)."""
    d = synthetic.smooth_field_task_stack(T, N, D, seed=seed)
    ys, _, _ = synthetic.standardize_rows(d["Y"])
    rng = np.random.default_rng(seed + 1)
    theta = np.concatenate([ls * (1 + spread * (rng.uniform(size=(T, D)) - 0.5)), np.full((T, 1), 1.0), np.full((T, 1), noise)], 1)
    return torch.from_numpy(d["X"]), torch.from_numpy(ys), torch.from_numpy(theta)


@functools.lru_cache(maxsize=None)
def duplicate_stack(N, D, kind, seed=40):
    """Three tasks, one per rung: the second half of the points repeats the first, os = 1, slightly negative noise."""
    X, y, theta = stack_like_fit_tests(3, N, D, seed + N)
    X = X.clone()
    X[:, N // 2:] = X[:, : N - N // 2]
    for t, r in enumerate(RUNGS):
        theta[t, D + 1] = DUP_NOISE[r]
    pl = [dict(what="rescued", rung=r, k=0, n=N) for r in RUNGS]
    return dict(X=X, y=y, theta=theta, plan=pl, kind=kind)


# ---- references -------------------------------------------------------------------------------------------------------
def ladder(A):
    """(jitter, info): what psd_safe_cholesky settles on -- (j, 0) -- or (1e-6, cholesky_ex's status at 1e-6) when it raises."""
    try:
        _, _, j = O.psd_safe_cholesky(A)
        return float(j), 0
    except O.NotPSDError:
        return RUNGS[-1], int(torch.linalg.cholesky_ex(A + RUNGS[-1] * _eye(A.shape[-1])).info)


def reference(A, y):
    """Reference results of one task from its (noise-included) matrix: dict(jitter, info, L, alpha, quad, logdet, mll)."""
    n = A.shape[-1]
    j, info = ladder(A)
    if info:
        return dict(jitter=j, info=info)
    L = torch.linalg.cholesky(A + j * _eye(n))
    alpha = torch.cholesky_solve(y[:n, None], L)[:, 0]
    quad = float(y[:n] @ alpha)
    logdet = float(2.0 * torch.log(torch.diagonal(L)).sum())
    return dict(jitter=j, info=0, L=L, alpha=alpha, quad=quad, logdet=logdet,
                mll=-0.5 * (quad + logdet + n * math.log(2.0 * math.pi)) / n)


def fit_reference(case, t, jitter_in=0.0):
    """The same dict for task t of a fit-from-X stack: O.gp_fit(dist="direct") with noise + jitter_in; the status of a task
    the oracle gives up on comes from cholesky_ex of the oracle's matrix at the last rung."""
    n = case["plan"][t]["n"]
    th = case["theta"][t].clone()
    th[-1] += jitter_in
    try:
        f = O.gp_fit(case["X"][t, :n], case["y"][t, :n], th, case["kind"], dist="direct")
    except O.NotPSDError:
        A = task_matrix_fit(case, t, jitter_in)
        return dict(jitter=RUNGS[-1], info=int(torch.linalg.cholesky_ex(A + RUNGS[-1] * _eye(n)).info))
    return dict(jitter=float(f["jitter"]), info=0, L=f["L"], alpha=f["alpha"], quad=float(f["quad"]), logdet=float(f["logdet"]),
                mll=float(f["mll"]), K=f["K"])


def pivots(A):
    """Pivots of a plain right-looking fp64 elimination, up to and including the first non-positive one."""
    S = A.clone()
    out = []
    for c in range(S.shape[0]):
        d = float(S[c, c])
        out.append(d)
        if not d > 0.0:
            break
        col = S[c + 1:, c] / d
        S[c + 1:, c + 1:] -= torch.outer(col, S[c + 1:, c])
    return out


def clean_potrf_stack(N, T, seed=5):
    """T clean matrices with right-hand sides (the caller-side jitter test)."""
    A = torch.stack([spd_matrix(N, _gen(seed, t)) for t in range(T)])
    y = torch.stack([torch.randn(N, dtype=F64, generator=_gen(seed + 1, t)) for t in range(T)])
    return dict(A=A, y=y, n_points=torch.full((T,), N, dtype=torch.int32), plan=[dict(what="clean", rung=None, k=0, n=N)] * T)


# ---- the assertions of the mixed-stack tests (on host tensors, so that the CPU suite can show that they bite) ---------
def rel(a, b):
    """The `_rel` of tests/test_fit_gpu.py."""
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


TOL_L, TOL_LOGDET, TOL_ALPHA, TOL_MLL = 1e-9, 1e-10, 1e-6, 1e-10   # a well-posed first attempt in tests/test_fit_gpu.py
TOL_QUAD = 1e-9   # quad = y . alpha of a system with condition number <= 5 (the existing rtol of that identity)


def check_outputs(out, plan_, refs, full=None, has_mll=False):
    """out: host tensors of one launch with n_points given (L, alpha zero-initialised by the front end).  refs[t]: dict(jitter, info)
    for every task, the whole reference() / fit_reference() dict for the tasks in `full` (default: all)."""
    T, N = out["L"].shape[:2]
    assert out["jitter"].tolist() == [r["jitter"] for r in refs], ("jitter_used", out["jitter"].tolist(), [r["jitter"] for r in refs])
    assert out["info"].tolist() == [r["info"] for r in refs], ("info", out["info"].tolist(), [r["info"] for r in refs])
    for t, s in enumerate(plan_):
        hopeless = s["what"] == "hopeless"
        assert (refs[t]["info"] > 0) == hopeless
        for key in ("quad", "logdet") + (("mll",) if has_mll else ()):
            v = float(out[key][t])
            assert math.isnan(v) if hopeless else math.isfinite(v), (key, t, s, v)
    L, alpha = out["L"], out["alpha"]
    assert float(torch.triu(L, diagonal=1).abs().max()) == 0.0, "strict upper triangle of L"
    for t, s in enumerate(plan_):
        n = s["n"]
        assert not L[t, n:, :].any() and not L[t, :, n:].any() and not alpha[t, n:].any(), ("rows / columns past n_t", t, s)
    for t in (range(T) if full is None else full):
        s, r = plan_[t], refs[t]
        if s["what"] == "hopeless":
            continue
        n = s["n"]
        e = dict(L=rel(L[t, :n, :n], r["L"]), alpha=rel(alpha[t, :n], r["alpha"]),
                 logdet=abs(float(out["logdet"][t]) - r["logdet"]) / abs(r["logdet"]),
                 quad=abs(float(out["quad"][t]) - r["quad"]) / abs(r["quad"]))
        if has_mll:
            e["mll"] = abs(float(out["mll"][t]) - r["mll"]) / abs(r["mll"])
        assert e["L"] < TOL_L and e["logdet"] < TOL_LOGDET and e["alpha"] < TOL_ALPHA and e["quad"] < TOL_QUAD \
            and e.get("mll", 0.0) < TOL_MLL, (t, s, e)


def outputs_from_references(plan_, refs, N):
    """What a correct launch returns, assembled from the references (host side)."""
    T = len(plan_)
    out = dict(L=torch.zeros(T, N, N, dtype=F64), alpha=torch.zeros(T, N, dtype=F64), jitter=torch.tensor([r["jitter"] for r in refs], dtype=F64),
               info=torch.tensor([r["info"] for r in refs], dtype=torch.int32))
    for key in ("quad", "logdet", "mll"):
        out[key] = torch.tensor([r.get(key, float("nan")) for r in refs], dtype=F64)
    for t, (s, r) in enumerate(zip(plan_, refs)):
        if r["info"] == 0:
            out["L"][t, :s["n"], :s["n"]] = r["L"]
            out["alpha"][t, :s["n"]] = r["alpha"]
    return out
