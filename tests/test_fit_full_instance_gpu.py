"""GPU: the full-tile instance of the fused fit, gp_fit_fused_kernel<16, 7, kind, true> (csrc/gp_fit_fused.hip, FULL), against the
generic instance of the same class in ONE library and one process: the launcher reads the environment variable SCAML_FIT_NO_FULL
at every launch (include/scaml_gp_debug.h), and os.environ reaches the C library's environment.  Which instance a call takes is
asserted through the launcher's own rule (fit_full_instance, csrc/gp_dispatch.h, compiled for the host: tests/_fit_full.py).

FULL exists only at N = 256, so that is every case's shape; two or three tasks per case.  The instance does the generic one's
arithmetic operation for operation, so on identical inputs every output is equal bit for bit, except alpha: its back-substitution
meets in LDS floating-point atomics, and it is held to the bound tests/test_fit_schedule_gpu.py holds two launches of one
instance to (rtol 1e-9, atol 1e-12).  A call that breaks one clause of the contract (fit_full_instance, csrc/gp_dispatch.h; pinned
on the host by tests/test_fit_full_dispatch.py) must take the generic instance and reproduce what the switch set to `never` gives.
"""
import os

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import _lib, ops
from tests import _failpath_cases as C
from tests import _fit_bounds as B
from tests import _fit_full as F
from tests import test_fit_bounds_gpu as FB      # (the module, not its names: nothing of it is collected here)
from tests.test_fit_gpu import RTOL_MLL, RTOL_POST, _rel, _stack

pytestmark = pytest.mark.gpu

N = 256
NO_FULL = "SCAML_FIT_NO_FULL"
KINDS = [pytest.param(O.KIND_RBF, id="rbf"), pytest.param(O.KIND_MATERN52, id="matern")]
EXACT = ("L", "Linv_diag", "mll", "quad", "logdet", "info", "jitter")


@pytest.fixture
def switch():
    """switch(1): SCAML_FIT_NO_FULL set, the generic instance for every call; switch(0): unset, the choice by arguments.  The
    variable is put back to what it was when the test ends."""
    was = os.environ.get(NO_FULL)

    def set_mode(mode):
        if mode:
            os.environ[NO_FULL] = "1"
        else:
            os.environ.pop(NO_FULL, None)

    set_mode(0)
    yield set_mode
    if was is None:
        os.environ.pop(NO_FULL, None)
    else:
        os.environ[NO_FULL] = was


def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _equal(a, b, keys=EXACT):
    for k in keys:
        if a.get(k) is None:
            assert b.get(k) is None, k
            continue
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), equal_nan=True), k
    if a.get("alpha") is not None:
        assert torch.allclose(a["alpha"], b["alpha"], rtol=1e-9, atol=1e-12)      # tests/test_fit_schedule_gpu.py: two launches of one instance


def _filled(T, device, store_L, want_linv, fill, l_offset=0):
    """Output buffers for out=, L full of `fill` (what zero_upper = False leaves alone must be the same in both runs);
    l_offset: L starts that many doubles past an aligned allocation."""
    big = torch.full((T * N * N + l_offset,), fill, dtype=torch.float64, device=device)
    o = dict(L=big[l_offset:].view(T, N, N) if store_L else None, alpha=torch.zeros(T, N, dtype=torch.float64, device=device),
             info=torch.full((T,), -7, dtype=torch.int32, device=device),
             Linv_diag=torch.zeros(T, N // 16, 16, 16, dtype=torch.float64, device=device) if want_linv else None)
    o.update({k: torch.zeros(T, dtype=torch.float64, device=device) for k in ("quad", "logdet", "mll", "jitter")})
    return o


# ---- FULL against the generic instance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_linv", [False, True], ids=["", "linv"])
@pytest.mark.parametrize("flags", [0, 1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [1, 4, 8, 9, 20, 21])      # the steps of the MFMA k-loop; both sides of the early chain's D <= 20
def test_full_equals_generic(D, kind, flags, want_linv, device, switch):
    T = 3
    X, y, theta = (a.to(device) for a in _stack(T, N, D, seed=900 + 10 * D + kind))
    kw = dict(store_L=bool(flags & 1), zero_upper=bool(flags & 2), want_linv=want_linv)
    assert F.fit_full_of_call(T, N, D, _cus(device), stores_l=bool(flags & 1), l_addr=0)
    res = {}
    for mode in (0, 1):
        switch(mode)
        out = ops.gp_fit_fused(X, y, theta, kind, out=_filled(T, device, bool(flags & 1), want_linv, -3.5), **kw)
        torch.cuda.synchronize()
        assert F.fit_full_of_call(T, N, D, _cus(device), stores_l=bool(flags & 1), l_addr=0, mode=mode) == (mode == 0)
        res[mode] = out
    assert not res[0]["info"].cpu().any() and float(res[0]["jitter"].abs().max()) == 0.0
    _equal(res[0], res[1])
    if flags == 1:      # zero_upper off: nothing above the diagonal is written
        up = torch.triu(torch.ones(N, N, dtype=torch.bool, device=device), diagonal=1)
        assert bool((res[0]["L"][:, up] == -3.5).all())
    if flags == 3:
        assert float(torch.triu(res[0]["L"], diagonal=1).abs().max()) == 0.0


# ---- calls that break the contract take the generic instance ----------------------------------------------------------------
def _both_modes(switch, call):
    res = {}
    for mode in (0, 1):
        switch(mode)
        res[mode] = call()
        torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [255, 241])
def test_fallback_padded_rows(n, kind, device, switch):
    X, y, theta = (a.to(device) for a in _stack(2, n, 8, seed=40 + n + kind))
    assert not F.fit_full_of_call(2, n, 8, _cus(device))
    res = _both_modes(switch, lambda: ops.gp_fit_fused(X, y, theta, kind, want_linv=True))
    assert not res[0]["info"].cpu().any()
    _equal(res[0], res[1])


@pytest.mark.parametrize("kind", KINDS)
def test_fallback_n_points_given(kind, device, switch):
    X, y, theta = (a.to(device) for a in _stack(2, N, 8, seed=77 + kind))
    npts = torch.full((2,), N, dtype=torch.int32, device=device)      # every point valid -- but the kernel cannot know
    assert not F.fit_full_of_call(2, N, 8, _cus(device), ragged=True)
    res = _both_modes(switch, lambda: ops.gp_fit_fused(X, y, theta, kind, n_points=npts, want_linv=True))
    assert not res[0]["info"].cpu().any()
    _equal(res[0], res[1])
    # ... and the full-tile instance gives the same factor on the same points
    switch(0)
    full = ops.gp_fit_fused(X, y, theta, kind, want_linv=True)
    torch.cuda.synchronize()
    _equal(full, res[0])


@pytest.mark.parametrize("kind", KINDS)
def test_fallback_l_on_an_8_byte_boundary(kind, device, switch):
    T = 2
    X, y, theta = (a.to(device) for a in _stack(T, N, 8, seed=78 + kind))
    probe = _filled(T, device, True, True, 0.0, l_offset=1)
    assert probe["L"].data_ptr() % 16 == 8
    assert not F.fit_full_of_call(T, N, 8, _cus(device), l_addr=probe["L"].data_ptr())
    res = _both_modes(switch, lambda: ops.gp_fit_fused(X, y, theta, kind, want_linv=True, out=_filled(T, device, True, True, 0.0, l_offset=1)))
    assert not res[0]["info"].cpu().any()
    _equal(res[0], res[1])
    # without L the pointer does not matter: the same call in MLL-only mode takes the full-tile instance
    switch(0)
    lite = ops.gp_fit_fused(X, y, theta, kind, store_L=False, out=_filled(T, device, False, False, 0.0))
    torch.cuda.synchronize()
    _equal(lite, res[0], keys=("mll", "quad", "logdet", "info", "jitter"))


def test_fallback_potrf_mode(device, switch):
    X, y, theta = (a.to(device) for a in _stack(2, N, 8, seed=79))
    K = ops.kernel_matrix(X, theta, O.KIND_MATERN52, add_noise=True)
    assert not F.fit_full_of_call(2, N, 8, _cus(device), from_matrix=True)
    res = _both_modes(switch, lambda: ops.potrf_batched(K, y, want_linv=True))
    assert not res[0]["info"].cpu().any()
    _equal(res[0], res[1], keys=("L", "Linv_diag", "quad", "logdet", "info", "jitter"))


@pytest.mark.parametrize("kind", KINDS)
def test_fallback_blocked_entry_point(kind, device, switch):
    """N = 272 through the sequence of launches: its first diagonal block is a 256-point fit by gp_fit_blocked_kernel<16, 7>."""
    X, y, theta = (a.to(device) for a in _stack(2, 272, 8, seed=80 + kind))
    assert not F.fit_full_of_call(2, N, 8, _cus(device), blocked=True)
    was = _lib.lib.scaml_debug_blocked_fit_path(1)
    try:
        res = _both_modes(switch, lambda: ops.gp_fit_fused(X, y, theta, kind))
    finally:
        _lib.lib.scaml_debug_blocked_fit_path(was)
    assert not res[0]["info"].cpu().any()
    _equal(res[0], res[1], keys=("L", "mll", "quad", "logdet", "info", "jitter"))


# ---- numerical failure paths on FULL -------------------------------------------------------------------------------------------
def _substack(case, tasks):
    sub = {k: case[k][tasks].clone() for k in ("X", "y", "theta", "n_points")}
    sub["plan"] = [case["plan"][t] for t in tasks]
    sub["kind"] = case["kind"]
    return sub


@pytest.mark.parametrize("tasks", [(0, 1, 2), (3, 5, 7)], ids=["clean-1e-8-hopeless", "1e-7-1e-6-clean"])
@pytest.mark.parametrize("kind", KINDS)
def test_failure_paths_on_full(kind, tasks, device, switch):
    """Tasks of the nine-task stack of tests/test_fit_failpath_gpu.py at N = 256 (tests/_failpath_cases.py: a clean one, one per
    jitter rung, a hopeless one), without n_points, so that the retries run in the full-tile instance's out-of-line copy; held to
    that file's bounds (C.check_outputs).  Reported numerical outcomes, not faults."""
    name = "nb16_wu7_n256"
    n, T9, NB = C.INSTANCES[name]
    assert n == N
    case = _substack(C.fit_stack(N, NB, T9, kind, 0), list(tasks))
    assert bool((case["n_points"] == N).all())
    T = len(tasks)
    o = _filled(T, device, True, False, 0.0)      # zeroed, as the front end hands them over when n_points is given
    out = ops.gp_fit_fused(case["X"].to(device), case["y"].to(device), case["theta"].to(device), kind, out=o)
    torch.cuda.synchronize()
    host = {k: (v.cpu() if v is not None else None) for k, v in out.items()}
    refs = [C.fit_reference(case, t) for t in range(T)]
    assert {s["what"] for s in case["plan"]} >= {"clean"} and any(s["what"] != "clean" for s in case["plan"])
    C.check_outputs(host, case["plan"], refs, has_mll=True)
    # the generic instance reports the same: status, rung, and the recovered factors bit for bit
    switch(1)
    gen = ops.gp_fit_fused(case["X"].to(device), case["y"].to(device), case["theta"].to(device), kind, out=_filled(T, device, True, False, 0.0))
    torch.cuda.synchronize()
    good = [t for t, s in enumerate(case["plan"]) if s["what"] != "hopeless"]
    assert torch.equal(out["info"], gen["info"]) and torch.equal(out["jitter"], gen["jitter"])
    for k in ("L", "mll", "quad", "logdet"):
        assert torch.equal(out[k][good], gen[k][good]), k


@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_point_on_full(kind, device, switch):
    """A NaN coordinate in one task: info > 0 and NaN scalars there, the neighbours as without it."""
    T = 3
    X, y, theta = _stack(T, N, 8, seed=81 + kind)
    Xn = X.clone()
    Xn[1, 17, 3] = float("nan")
    clean = ops.gp_fit_fused(X.to(device), y.to(device), theta.to(device), kind)
    torch.cuda.synchronize()
    bad = ops.gp_fit_fused(Xn.to(device), y.to(device), theta.to(device), kind)
    torch.cuda.synchronize()
    info = bad["info"].cpu()
    assert int(info[1]) > 0 and int(info[0]) == 0 and int(info[2]) == 0
    assert float(bad["jitter"][1]) == C.RUNGS[-1]      # every rung was tried
    for k in ("mll", "quad", "logdet"):
        assert bool(torch.isnan(bad[k][1]))
    for k in ("L", "mll", "quad", "logdet"):
        assert torch.equal(bad[k][[0, 2]], clean[k][[0, 2]]), k


# ---- capture ----------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_with_the_full_instance(device, switch):
    """The choice reads pointer values on the host, nothing else: valid under stream capture."""
    kind = O.KIND_MATERN52
    X, y, th = (a.to(device) for a in _stack(3, N, 8, seed=82))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.gp_fit_fused(X, y, th, kind)          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.gp_fit_fused(X, y, th, kind)
    y2 = y.flip(1).contiguous()
    y.copy_(y2)                                   # new targets in the captured buffers
    g.replay()
    torch.cuda.synchronize()
    ref = ops.gp_fit_fused(X, y2, th, kind)
    torch.cuda.synchronize()
    assert torch.allclose(out["alpha"], ref["alpha"], rtol=1e-9, atol=1e-12)
    for k in ("L", "mll", "quad", "logdet", "info", "jitter"):
        assert torch.equal(out[k], ref[k]), k


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_full_within_the_componentwise_bounds(kind, device, switch):
    """One case per kind through tests/_fit_bounds.py with the backend of tests/test_fit_bounds_gpu.py (imported): every output
    element of every task within its a-priori bound of the long-double reference; and the first task against oracle/gp_oracle.py
    at the tolerances of tests/test_fit_gpu.py."""
    c = B._f(T=2, N=N, D=8, kind=kind)            # ragged None: no n_points
    assert B.fit_inputs(c)["n_points"] is None
    out = B.check_fit(FB.Device(device), c)
    inp = B.fit_inputs(c)
    X0, y0, th0 = (torch.from_numpy(np.ascontiguousarray(inp[k][0])) for k in ("X", "y", "theta"))
    ref_g = O.gp_fit(X0, y0, th0, kind, dist="gpytorch")
    ref_d = O.gp_fit(X0, y0, th0, kind, dist="direct")
    L, alpha, mll = torch.from_numpy(out["L"][0]), torch.from_numpy(out["alpha"][0]), torch.from_numpy(out["mll"][:1])
    assert _rel(mll, ref_g["mll"].reshape(1)) < RTOL_MLL and _rel(alpha, ref_g["alpha"]) < RTOL_POST
    assert _rel(torch.tril(L), ref_d["L"]) < 1e-9 and _rel(mll, ref_d["mll"].reshape(1)) < 1e-10 and _rel(alpha, ref_d["alpha"]) < 1e-6
