"""GPU tests of the fused fit with the per-wave tile schedule (csrc/gf_schedule.hpp) on every kernel instance (NB 16-blocks,
WU update waves), dense and blocked, at the smallest shape that fills the instance's triangle.  Three tasks per case with
ragged point counts, so that the last 16-block holds 16, 15 and 1 valid rows; the shapes cover what the schedule has to
get right and a full-size benchmark run does not single out: update waves that own no tile of a late column, the empty
last slot of a wave, and the parked diagonal tile that the bulk update skips.

Per case: L, alpha, MLL and logdet against the oracle at the tolerances of tests/test_fit_gpu.py (its
test_fit_matches_oracle: north-star tolerances against the reference's formulation, the tight ones against the kernel's
own distance formulation); two launches agree bit for bit; fit mode and POTRF mode (the same kernel handed the matrix)
agree on the factor and are each reproducible, the checks of tools/dev_race_check.py."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import _lib, ops
from tests._dispatch import narrow_fit_tasks
from tests.test_fit_gpu import RTOL_MLL, RTOL_POST, _rel, _stack

pytestmark = pytest.mark.gpu

D = 3


def _narrow_kernel_task_count(device):
    """64 < N <= 128 runs the (8, 3) instance only when the stack has more tasks than the device has CUs; up to that
    count the launcher takes the wide (8, 7) instance.  The count is asked of the launcher's own plan (tests/_dispatch.py)
    with the device's CU count, which asserts the instance, so that the test fails, rather than silently testing (8, 7)
    twice, when the rule changes."""
    return narrow_fit_tasks(torch.cuda.get_device_properties(device).multi_processor_count, N=128, D=D)


# (instance, N, tasks, blocked): tasks None = just above the launcher's switch-over count
CASES = [((2, 1), 32, 3, False), ((4, 3), 64, 3, False), ((8, 7), 128, 3, False), ((16, 7), 256, 3, False),
         ((8, 3), 128, None, False), ((16, 7), 272, 3, True)]


@pytest.fixture
def sequence_of_launches(device):
    """256 < N <= 512: route the fit through the 2 x 2 sequence of launches, whose diagonal blocks are factored by
    gp_fit_blocked_kernel (small stacks would take the several-CUs-per-task kernel by default)."""
    was = _lib.lib.scaml_debug_blocked_fit_path(1)
    yield
    _lib.lib.scaml_debug_blocked_fit_path(was)


@pytest.mark.parametrize("kind", [O.KIND_RBF, O.KIND_MATERN52], ids=["rbf", "matern52"])
@pytest.mark.parametrize("inst,N,T,blocked", CASES, ids=[f"nb{i[0]}wu{i[1]}-N{n}{'-blocked' if b else ''}" for i, n, _, b in CASES])
def test_fit_with_schedule(inst, N, T, blocked, kind, device, sequence_of_launches):
    if T is None:
        T = _narrow_kernel_task_count(device)
    X, y, theta = _stack(T, N, D, seed=500 + N + 7 * kind + inst[1])
    npts = torch.tensor([N, N - 1, N - 15] * (T // 3 + 1), dtype=torch.int32)[:T]   # last block: 16, 15, 1 valid rows
    Xd, yd, thd, nd = X.to(device), y.to(device), theta.to(device), npts.to(device)

    def fit():
        return ops.gp_fit_fused(Xd, yd, thd, kind, n_points=nd) if blocked else ops.gp_fit_fused(Xd, yd, thd, kind, n_points=nd, want_linv=True)

    out = fit()
    assert not out["info"].cpu().any()
    assert float(out["jitter"].abs().max()) == 0.0

    # ---- the oracle, task by task on the valid points (the first three tasks: one of each raggedness)
    for t in range(3):
        n = int(npts[t])
        ref_g = O.gp_fit(X[t, :n], y[t, :n], theta[t], kind, dist="gpytorch")   # the reference's formulation
        ref_d = O.gp_fit(X[t, :n], y[t, :n], theta[t], kind, dist="direct")     # the kernel's formulation
        L, alpha = out["L"][t, :n, :n].cpu(), out["alpha"][t, :n].cpu()
        mll, logdet = out["mll"][t].cpu().reshape(1), out["logdet"][t].cpu().reshape(1)
        figs = dict(mll_g=_rel(mll, ref_g["mll"].reshape(1)), alpha_g=_rel(alpha, ref_g["alpha"]), L_d=_rel(L, ref_d["L"]),
                    mll_d=_rel(mll, ref_d["mll"].reshape(1)), logdet_d=_rel(logdet, ref_d["logdet"].reshape(1)), alpha_d=_rel(alpha, ref_d["alpha"]))
        print(f"N={N} inst={inst} blocked={blocked} kind={kind} task {t} n={n}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
        assert figs["mll_g"] < RTOL_MLL and figs["alpha_g"] < RTOL_POST
        assert figs["L_d"] < 1e-9 and figs["mll_d"] < 1e-10 and figs["logdet_d"] < 1e-10 and figs["alpha_d"] < 1e-6
        # nothing outside the valid points is written: rows / columns beyond n stay zero
        assert float(out["L"][t, n:, :].abs().max()) == 0.0 if n < N else True
    assert float(torch.triu(out["L"], diagonal=1).abs().max()) == 0.0

    # ---- two launches agree bit for bit (alpha: its back-substitution folds through LDS floating-point atomics,
    #      whose order is free; tools/dev_race_check.py holds it to rtol 1e-9 / atol 1e-12)
    again = fit()
    for k in ("L", "logdet", "mll", "quad") + (() if blocked else ("Linv_diag",)):
        assert torch.equal(out[k], again[k]), k
    assert torch.allclose(out["alpha"], again["alpha"], rtol=1e-9, atol=1e-12)

    # ---- fit mode and POTRF mode on the same matrix (blocked: on the leading 256 points, the matrix that the first
    #      diagonal block's kernel factors; POTRF mode has no blocked form)
    M = min(N, _lib.lib.scaml_fit_max_n())
    K = ops.kernel_matrix(Xd[:, :M].contiguous(), thd, kind, add_noise=True)
    nm = torch.clamp(nd, max=M)
    ym = yd[:, :M].contiguous()
    p1 = ops.potrf_batched(K, ym, n_points=nm, want_linv=True)
    p2 = ops.potrf_batched(K, ym, n_points=nm, want_linv=True)
    assert not p1["info"].cpu().any()
    for k in ("L", "logdet", "Linv_diag"):
        assert torch.equal(p1[k], p2[k]), k
    assert torch.allclose(p1["alpha"], p2["alpha"], rtol=1e-9, atol=1e-12) and torch.allclose(p1["quad"], p2["quad"], rtol=1e-11)
    dL = _rel(out["L"][:, :M, :M], p1["L"])
    print(f"N={N} inst={inst} blocked={blocked} kind={kind}: fit vs potrf rel |dL| = {dL:.2e}")
    assert dL < 1e-9   # both are held to 1e-9 against the same factor (test_fit_matches_oracle)
    if not blocked:
        assert _rel(out["logdet"], p1["logdet"]) < 1e-10
        assert _rel(out["alpha"], p1["alpha"]) < 1e-6
