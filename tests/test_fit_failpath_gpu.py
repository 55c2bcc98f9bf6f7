"""GPU: the failure and in-kernel jitter-retry paths of scaml_gp_fit_fused_f64 / scaml_potrf_batched_f64 on every kernel
instance (csrc/gp_fit_fused.hip: (2, 1), (4, 3), (8, 3) narrow, (8, 7) wide, (16, 7)), against the CPU oracle.

A failed pivot restarts the task through gp_fit_retry, an out-of-line copy of the attempt that reuses the hand-managed
accumulator tiles and the LDS hand-off counters.  The inputs (tests/_failpath_cases.py; their margins are held by
tests/test_failpath_inputs.py on the CPU) make a rescued task WELL conditioned (condition number <= 5 at the rung that
succeeds), so the retried factor, alpha and scalars are held to the tolerances tests/test_fit_gpu.py applies to a first
attempt, and make a hopeless task fail at a known pivot, so the status is compared with LAPACK's.
The fit from X cannot fail at pivot 1 through a copied point; its smallest failing index is 2.
"""
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import ops
from tests import _failpath_cases as C
from tests._dispatch import narrow_fit_tasks

pytestmark = pytest.mark.gpu

KINDS = [pytest.param(O.KIND_RBF, id="rbf"), pytest.param(O.KIND_MATERN52, id="matern")]
SMALL = [name for name, (_, T, _) in C.INSTANCES.items() if T is not None]
NARROW = "nb8_wu3_narrow"
SAMPLE_MAX = 12   # tasks of the narrow-instance stack that are compared with the full reference


def _stacks(k_min):
    for name in SMALL:
        N, T, NB = C.INSTANCES[name]
        for part in range(C.n_parts(N, NB, T, k_min)):
            yield pytest.param(name, part, id=f"{name}-part{part}")


def _host(out):
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def _run_potrf(case, device, **kw):
    return ops.potrf_batched(case["A"].to(device), case["y"].to(device), n_points=case["n_points"].to(device), **kw)


def _run_fit(case, kind, device, n_points=True, **kw):
    return ops.gp_fit_fused(case["X"].to(device), case["y"].to(device), case["theta"].to(device), kind,
                            n_points=case["n_points"].to(device) if n_points else None, **kw)


def _bits(a, b):
    """Bit-for-bit equality (NaN equals NaN)."""
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def _idx(case, *what):
    return [t for t, s in enumerate(case["plan"]) if s["what"] in what]


def _narrow_T(device):
    """The smallest stack the launcher's plan sends to the four-wave (8, 3) instance on this device (asserted there)."""
    return narrow_fit_tasks(torch.cuda.get_device_properties(device).multi_processor_count, N=C.INSTANCES[NARROW][0])


def _narrow_sample(plan_):
    """At most SAMPLE_MAX tasks with every kind of task among them: the first two cycles, the last task, the ragged one."""
    ragged = next(t for t, s in enumerate(plan_) if s["n"] != plan_[0]["n"])
    sample = sorted(set(range(2 * len(C.CYCLE_PATTERN))) | {len(plan_) - 1, ragged})
    assert len(sample) <= SAMPLE_MAX
    assert {(plan_[t]["what"], plan_[t]["rung"]) for t in sample} == {("clean", None), ("hopeless", None)} | {("rescued", r) for r in C.RUNGS}
    return sample


# ---- (a) mixed stacks through the POTRF -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,part", list(_stacks(1)))
def test_potrf_mixed_stack(name, part, device):
    N, T, NB = C.INSTANCES[name]
    case = C.potrf_stack(N, NB, T, part)
    out = _host(_run_potrf(case, device))
    refs = [C.reference(C.task_matrix_potrf(case, t), case["y"][t]) for t in range(T)]
    C.check_outputs(out, case["plan"], refs)


def test_potrf_mixed_stack_narrow_instance(device):
    N, _, NB = C.INSTANCES[NARROW]
    T = _narrow_T(device)
    case = C.potrf_stack(N, NB, T, 0)
    out = _host(_run_potrf(case, device))
    sample = _narrow_sample(case["plan"])
    refs = [C.reference(C.task_matrix_potrf(case, t), case["y"][t]) if t in sample
            else dict(zip(("jitter", "info"), C.ladder(C.task_matrix_potrf(case, t)))) for t in range(T)]
    C.check_outputs(out, case["plan"], refs, full=sample)


# ---- (b) mixed stacks through the fit from X ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,part", list(_stacks(2)))
def test_fit_mixed_stack(name, part, kind, device):
    N, T, NB = C.INSTANCES[name]
    case = C.fit_stack(N, NB, T, kind, part)
    out = _host(_run_fit(case, kind, device))
    refs = [C.fit_reference(case, t) for t in range(T)]
    C.check_outputs(out, case["plan"], refs, has_mll=True)


@pytest.mark.parametrize("kind", KINDS)
def test_fit_mixed_stack_narrow_instance(kind, device):
    N, _, NB = C.INSTANCES[NARROW]
    T = _narrow_T(device)
    case = C.fit_stack(N, NB, T, kind, 0)
    out = _host(_run_fit(case, kind, device))
    sample = _narrow_sample(case["plan"])
    refs = [C.fit_reference(case, t) if t in sample
            else dict(zip(("jitter", "info"), C.ladder(C.task_matrix_fit(case, t)))) for t in range(T)]
    C.check_outputs(out, case["plan"], refs, full=sample, has_mll=True)


# ---- (c) the realistic, ill-conditioned rescue ------------------------------------------------------------------------
RESIDUAL_FACTOR = 8.0   # order of operations, not another class of algorithm


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,D", C.DUP_SHAPES)
def test_duplicated_points_rescue(N, D, kind, device):
    """Half of each task's points repeat the other half (the normal state of a BO loop); noise -2e-9 / -5e-8 / -5e-7 needs the
    rungs 1e-8 / 1e-7 / 1e-6.  The factor is held to Higham's backward-error bound for a Cholesky factorisation in any
    summation order, |L L^T - A| <= gamma_{N+1} |L| |L^T| with (|L| |L^T|)_ij <= sqrt(a_ii a_jj) / (1 - gamma_{N+1}) -- the
    factor 2 covers the denominator --, plus the 1e-12 os agreement of the kernel matrix that test_full_size_properties
    asserts.  alpha and Linv_diag (explicit inverses of 16 x 16 blocks with condition number ~1e4 here) have no derived
    bound: their residuals are compared with the residuals of torch's solve / inverse on the oracle's factor, same input.

    Measured (GPU, reference) residual pairs: to be recorded here and in profiles/failpath_notes.md from the lines this test
    prints (none measured yet).
    """
    case = C.duplicate_stack(N, D, kind)
    out = _host(ops.gp_fit_fused(case["X"].to(device), case["y"].to(device), case["theta"].to(device), kind, want_linv=True))
    refs = [C.fit_reference(case, t) for t in range(3)]
    assert out["jitter"].tolist() == [r["jitter"] for r in refs] == list(C.RUNGS)
    assert out["info"].tolist() == [0, 0, 0]
    gamma = (N + 1) * 2.0 ** -53 / (1.0 - (N + 1) * 2.0 ** -53)
    eye = torch.eye(N, dtype=C.F64)
    pad = 16 * ((N + 15) // 16)
    for t, r in enumerate(refs):
        A = r["K"] + r["jitter"] * eye        # the oracle's K already holds the noise
        y, L, alpha = case["y"][t], out["L"][t], out["alpha"][t]
        backward = float((L @ L.T - A).abs().max())
        bound = 2.0 * gamma * float(torch.diagonal(A).max()) + 1e-12 * float(case["theta"][t, D])

        def rho(a):
            return float((A @ a - y).abs().max() / (A.abs().sum(1).max() * a.abs().max() + y.abs().max()))

        def block_residual(Lm, inverse_of):
            Lp = torch.eye(pad, dtype=C.F64)
            Lp[:N, :N] = Lm
            worst = 0.0
            for b in range(pad // 16):
                blk = Lp[16 * b:16 * b + 16, 16 * b:16 * b + 16]
                worst = max(worst, float((inverse_of(b, blk) @ blk - torch.eye(16, dtype=C.F64)).abs().max()))
            return worst

        rho_gpu, rho_ref = rho(alpha), rho(torch.cholesky_solve(y[:, None], r["L"])[:, 0])
        inv_gpu = block_residual(L, lambda b, blk: out["Linv_diag"][t, b])
        inv_ref = block_residual(r["L"], lambda b, blk: torch.linalg.inv(blk))
        print(f"[failpath] N={N} kind={kind} rung={r['jitter']:.0e} backward={backward:.3e} bound={bound:.3e} "
              f"rho gpu={rho_gpu:.3e} ref={rho_ref:.3e} linv gpu={inv_gpu:.3e} ref={inv_ref:.3e}", flush=True)
        assert backward <= bound
        torch.testing.assert_close(out["logdet"][t], 2.0 * torch.log(torch.diagonal(L)).sum(), rtol=1e-12, atol=0)
        torch.testing.assert_close(out["quad"][t], y @ alpha, rtol=1e-9, atol=0)
        assert rho_gpu <= RESIDUAL_FACTOR * rho_ref
        assert inv_gpu <= RESIDUAL_FACTOR * inv_ref


# ---- (d) caller-side jitter -------------------------------------------------------------------------------------------
JITTER_IN_CLEAN = (0.0, 1e-5, 3e-4)


def _with_jitter(case, jin, run, ref_of, device, has_mll):
    T = len(case["plan"])
    out = _host(run(jitter=torch.tensor(jin, dtype=C.F64, device=device)))
    refs = [ref_of(t, jin[t]) for t in range(T)]
    C.check_outputs(out, case["plan"], refs, has_mll=has_mll)
    return out


@pytest.mark.parametrize("name", ["nb4_wu3", "nb16_wu7_n256"])
def test_jitter_in_potrf(name, device):
    N, T, NB = C.INSTANCES[name]
    # clean stack: the caller's jitter is part of the matrix, jitter_used reports the ladder's value only
    clean = C.clean_potrf_stack(N, T)
    jin = [JITTER_IN_CLEAN[t % 3] for t in range(T)]
    out = _with_jitter(clean, jin, lambda **kw: _run_potrf(clean, device, **kw),
                       lambda t, j: C.reference(C.task_matrix_potrf(clean, t, j), clean["y"][t]), device, False)
    assert out["jitter"].tolist() == [0.0] * T
    # the retry copy: a rung-1e-7 task with 4.5e-8 from the caller is rescued at 1e-8, its factor is that of A + 5.5e-8 I
    case = C.potrf_stack(N, NB, T, 0)
    t7 = next(t for t, s in enumerate(case["plan"]) if s["rung"] == 1e-7)
    jin = [C.JITTER_IN_RETRY if t == t7 else 0.0 for t in range(T)]
    out = _with_jitter(case, jin, lambda **kw: _run_potrf(case, device, **kw),
                       lambda t, j: C.reference(C.task_matrix_potrf(case, t, j), case["y"][t]), device, False)
    assert float(out["jitter"][t7]) == 1e-8
    assert C.rel(out["L"][t7], torch.linalg.cholesky(case["A"][t7] + 5.5e-8 * torch.eye(N, dtype=C.F64))) < C.TOL_L


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["nb4_wu3", "nb16_wu7_n256"])
def test_jitter_in_fit(name, kind, device):
    N, T, NB = C.INSTANCES[name]
    case = C.fit_stack(N, NB, T, kind, 0)
    clean = C.clean_fit_stack(case)
    jin = [JITTER_IN_CLEAN[t % 3] for t in range(T)]
    out = _with_jitter(clean, jin, lambda **kw: _run_fit(clean, kind, device, **kw), lambda t, j: C.fit_reference(clean, t, j), device, True)
    assert out["jitter"].tolist() == [0.0] * T
    t7 = next(t for t, s in enumerate(case["plan"]) if s["rung"] == 1e-7)
    jin = [C.JITTER_IN_RETRY if t == t7 else 0.0 for t in range(T)]
    out = _with_jitter(case, jin, lambda **kw: _run_fit(case, kind, device, **kw), lambda t, j: C.fit_reference(case, t, j), device, True)
    assert float(out["jitter"][t7]) == 1e-8
    assert C.rel(out["L"][t7], torch.linalg.cholesky(C.task_matrix_fit(case, t7, 5.5e-8))) < C.TOL_L


# ---- (e) flag combinations under a retry ------------------------------------------------------------------------------
SENTINEL = -7.25


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["nb4_wu3", "nb16_wu7_n256"])
def test_flags_under_retry(name, kind, device):
    N, T, NB = C.INSTANCES[name]
    case = C.fit_stack(N, NB, T, kind, 0)
    assert bool((case["n_points"] == N).all())    # part 0 has no ragged task: the runs below pass no n_points
    good, clean, failing = _idx(case, "clean", "rescued"), _idx(case, "clean"), _idx(case, "rescued", "hopeless")
    full = _host(_run_fit(case, kind, device, n_points=False, want_linv=True))
    # MLL-only mode through the retries
    lite = _host(_run_fit(case, kind, device, n_points=False, store_L=False, want_alpha=False))
    assert lite["L"] is None and lite["alpha"] is None
    for key in ("mll", "quad", "logdet", "info", "jitter"):
        assert _bits(full[key], lite[key]), key
    assert full["jitter"][_idx(case, "rescued")].tolist() == list(C.RUNGS) and bool((full["info"][_idx(case, "hopeless")] > 0).all())
    # single attempt
    single = _host(_run_fit(case, kind, device, n_points=False, retry=False))
    assert [t for t in range(T) if int(single["info"][t]) > 0] == failing
    assert single["jitter"].tolist() == [0.0] * T
    for key in ("L", "alpha", "mll", "quad", "logdet"):
        assert _bits(single[key][clean], full[key][clean]), key
    # zero_upper=False leaves the strict upper triangle alone, in the retries too
    buf = _run_fit(case, kind, device, n_points=False, zero_upper=False)
    buf["L"].fill_(SENTINEL)
    keep = _host(_run_fit(case, kind, device, n_points=False, zero_upper=False, out=buf))
    upper = torch.triu(torch.ones(N, N, dtype=torch.bool), diagonal=1)
    assert bool((keep["L"][:, upper] == SENTINEL).all())
    lower = ~upper
    assert _bits(keep["L"][good][:, lower], full["L"][good][:, lower])
    assert float(full["L"][good][:, upper].abs().max()) == 0.0


# ---- (f) isolation and determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SMALL)
def test_failing_neighbours_leave_clean_tasks_untouched(name, kind, device):
    N, T, NB = C.INSTANCES[name]
    case = C.fit_stack(N, NB, T, kind, C.n_parts(N, NB, T, 2) - 1)   # the last part: with the ragged tasks
    mixed = _host(_run_fit(case, kind, device))
    alone = _host(_run_fit(C.clean_fit_stack(case), kind, device))    # same T: same kernel instance
    assert not alone["info"].any() and not alone["jitter"].any()
    clean, good = _idx(case, "clean"), _idx(case, "clean", "rescued")
    for key in ("L", "alpha", "mll"):
        assert _bits(mixed[key][clean], alone[key][clean]), key
    again = _host(_run_fit(case, kind, device))
    assert _bits(again["info"], mixed["info"]) and _bits(again["jitter"], mixed["jitter"])
    assert _bits(again["L"][good], mixed["L"][good])
