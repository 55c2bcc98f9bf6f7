"""CPU: the inputs of tests/test_fit_failpath_gpu.py (tests/_failpath_cases.py) behave as their builders say, by the oracle alone
and with margins that rounding on either side cannot cross.

Ladder.  O.psd_safe_cholesky settles on the intended jitter, and at every rung it tries
    |lambda_min(A + j I)| >= 1e3 * N * 2^-53 * ||A||_2,
a thousand times the backward error of an fp64 Cholesky of order N: the outcome of each attempt is a property of the matrix,
not of the order of operations.
Hopeless index.  A plain right-looking elimination has every pivot before k at >= 1e-6 and pivot k at <= -1e-6 with the last
rung's jitter added, and cholesky_ex reports exactly k.
"""
import pytest
import torch

from oracle import gp_oracle as O
from tests import _failpath_cases as C
from tests._dispatch import fit_plan

KINDS = [O.KIND_RBF, O.KIND_MATERN52]
U = 2.0 ** -53


def _check_ladder(A, want, jitter_in=0.0):
    n = A.shape[-1]
    A = A + jitter_in * torch.eye(n, dtype=C.F64)
    j, info = C.ladder(A)
    assert info == 0 and j == want
    ev = torch.linalg.eigvalsh(A)
    margin = 1e3 * n * U * float(ev.abs().max())
    for rung in (0.0,) + C.RUNGS:
        lam = float(ev[0]) + rung      # the shift moves every eigenvalue alike
        assert abs(lam) >= margin, (rung, lam, margin)
        assert (lam > 0) == (rung >= want)
        if rung >= want:
            break


def _check_hopeless(A, k):
    n = A.shape[-1]
    Aj = A + C.RUNGS[-1] * torch.eye(n, dtype=C.F64)
    piv = C.pivots(Aj)
    assert len(piv) == k and min(piv[:-1], default=1.0) >= 1e-6 and piv[-1] <= -1e-6, (k, len(piv), piv[-3:])
    assert int(torch.linalg.cholesky_ex(Aj).info) == k
    assert int(torch.linalg.cholesky_ex(A).info) == k            # the single attempt of retry=False fails at the same place
    assert C.ladder(A) == (C.RUNGS[-1], k)


def _check_stack(case, matrix_of):
    seen = set()
    for t, s in enumerate(case["plan"]):
        A = matrix_of(case, t)
        assert A.shape[-1] == s["n"]
        if s["what"] == "hopeless":
            _check_hopeless(A, s["k"])
        else:
            _check_ladder(A, s["rung"] or 0.0)
        seen.add((s["what"], s["rung"]))
    return seen


ALL_KINDS_OF_TASK = {("clean", None), ("hopeless", None)} | {("rescued", r) for r in C.RUNGS}


def _stacks(k_min):
    for name, (N, T, NB) in C.INSTANCES.items():
        T = T or C.NARROW_T_CPU
        for part in range(C.n_parts(N, NB, T, k_min)):
            yield pytest.param(N, NB, T, part, id=f"{name}-part{part}")


@pytest.mark.parametrize("N,NB,T,part", list(_stacks(1)))
def test_potrf_stacks(N, NB, T, part):
    case = C.potrf_stack(N, NB, T, part)
    assert _check_stack(case, C.task_matrix_potrf) == ALL_KINDS_OF_TASK
    for t, s in enumerate(case["plan"]):
        if s["what"] == "rescued":    # the builder's promise that lets the retried factor be held to first-attempt tolerances
            assert float(torch.linalg.cond(C.task_matrix_potrf(case, t, s["rung"]))) < 5.0 + 1e-6


@pytest.mark.parametrize("kind", KINDS, ids=["rbf", "matern"])
@pytest.mark.parametrize("N,NB,T,part", list(_stacks(2)))
def test_fit_stacks(N, NB, T, part, kind):
    case = C.fit_stack(N, NB, T, kind, part)
    assert _check_stack(case, C.task_matrix_fit) == ALL_KINDS_OF_TASK
    for t, s in enumerate(case["plan"]):
        if s["what"] == "rescued":
            assert float(torch.linalg.cond(C.task_matrix_fit(case, t, s["rung"]))) < 5.0


@pytest.mark.parametrize("name", list(C.INSTANCES))
def test_name_is_the_instance_the_launcher_picks(name):
    """At the 256 CUs the CPU shapes are chosen for, the launcher's plan for (T, N) is the instance the name and NB say, and the narrow
    stack is one task past the last the wide instance takes."""
    N, T, NB = C.INSTANCES[name]
    p = fit_plan(T or C.NARROW_T_CPU, N, 1, 256)
    assert p.nb == NB and name.startswith(f"nb{p.nb}_wu{p.wu}"), (name, p)
    if T is None:
        assert C.NARROW_T_CPU == 257 and fit_plan(C.NARROW_T_CPU - 1, N, 1, 256)[1:3] == (8, 7)


@pytest.mark.parametrize("name", list(C.INSTANCES))
def test_every_hopeless_index_is_placed(name):
    N, T, NB = C.INSTANCES[name]
    T = T or C.NARROW_T_CPU
    for k_min in (1, 2):
        placed = [(s["k"], s["n"]) for part in range(C.n_parts(N, NB, T, k_min)) for s in C.plan(N, NB, T, part, k_min) if s["what"] == "hopeless"]
        assert set(placed) == set(C.hopeless_list(N, NB, k_min))
        assert {k for k, n in C.hopeless_list(N, NB, k_min) if n == N} == {k_min, 16, 17, 16 * (NB // 2) + 1, N - 1, N}
        assert (N - C.RAGGED_SHORT, N - C.RAGGED_SHORT) in placed


@pytest.mark.parametrize("kind", KINDS, ids=["rbf", "matern"])
@pytest.mark.parametrize("N,D", C.DUP_SHAPES)
def test_duplicate_stacks(N, D, kind):
    case = C.duplicate_stack(N, D, kind)
    assert _check_stack(case, C.task_matrix_fit) == {("rescued", r) for r in C.RUNGS}


@pytest.mark.parametrize("name", ["nb4_wu3", "nb16_wu7_n256"])
def test_jitter_in_ladders(name):
    N, T, NB = C.INSTANCES[name]
    cases = [(C.potrf_stack(N, NB, T, 0), C.task_matrix_potrf)] + [(C.fit_stack(N, NB, T, k, 0), C.task_matrix_fit) for k in KINDS]
    for case, matrix_of in cases:
        t = next(t for t, s in enumerate(case["plan"]) if s["rung"] == 1e-7)
        _check_ladder(matrix_of(case, t), 1e-8, jitter_in=C.JITTER_IN_RETRY)
        for t, s in enumerate(case["plan"]):     # a clean task stays clean with caller-side jitter on top
            if s["what"] == "clean":
                for jin in (0.0, 1e-5, 3e-4):
                    _check_ladder(matrix_of(case, t), 0.0, jitter_in=jin)


def test_the_gpu_assertions_catch_a_wrong_retry():
    """C.check_outputs (what tests/test_fit_failpath_gpu.py applies to the kernels' results) accepts the references
    themselves and rejects a retry that went wrong: a factor at the neighbouring rung, a status off by one, a jitter
    one rung up."""
    N, T, NB = C.INSTANCES["nb4_wu3"]
    case = C.potrf_stack(N, NB, T, 0)
    refs = [C.reference(C.task_matrix_potrf(case, t), case["y"][t]) for t in range(T)]
    C.check_outputs(C.outputs_from_references(case["plan"], refs, N), case["plan"], refs)

    t7 = next(t for t, s in enumerate(case["plan"]) if s["rung"] == 1e-7)
    wrong = C.outputs_from_references(case["plan"], refs, N)
    wrong["L"][t7] = torch.linalg.cholesky(C.task_matrix_potrf(case, t7, 1e-6))     # the factor of the next rung
    with pytest.raises(AssertionError, match="'L'"):
        C.check_outputs(wrong, case["plan"], refs)

    th = next(t for t, s in enumerate(case["plan"]) if s["what"] == "hopeless")
    wrong = C.outputs_from_references(case["plan"], refs, N)
    wrong["info"][th] += 1
    with pytest.raises(AssertionError, match="info"):
        C.check_outputs(wrong, case["plan"], refs)

    wrong = C.outputs_from_references(case["plan"], refs, N)
    wrong["jitter"][t7] = 1e-6
    with pytest.raises(AssertionError, match="jitter_used"):
        C.check_outputs(wrong, case["plan"], refs)
