"""GPU tests of how the fused fit writes the factor L (csrc/gp_fit_fused.hip): finished tiles leave in 16-byte stores
where L's rows sit on 16-byte boundaries and in 8-byte stores elsewhere, and the strict upper triangle is zero-filled (on
request) during the kernel-matrix build, by the wave that builds the mirrored lower tile.

Every fused instance at its smallest telling shape (tests/test_fit_schedule_gpu.py's cases, plus N = 208 for a partly filled last
column of the (16, 7) instance), both kernels, the blocked kernel and the POTRF mode; an aligned L, an L that starts 8 bytes
into a larger buffer, and odd N (33, 255: every second row is off the 16-byte grid), so that both store widths run;
ragged point counts with 16, 15 and 1 valid rows in the last 16-block.  L is launched through the C ABI into pre-filled
buffers, so that every element the kernel must NOT write is checked bit for bit:
  zero_upper on  -> the strict upper triangle inside n_t is exactly 0.0,
  zero_upper off -> it is untouched (NaN fill),
  both           -> rows / columns at or past n_t and the guard elements around the buffer untouched, the lower triangle
                    bit-identical between the two settings,
  no STORE_L     -> all of L untouched.
The lower triangle is held to the oracle at the tolerance of tests/test_fit_schedule_gpu.py (1e-9 relative against the
oracle in the kernel's own distance formulation)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import _lib, ops
from tests.test_fit_gpu import _rel, _stack
from tests.test_fit_schedule_gpu import _narrow_kernel_task_count, sequence_of_launches  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D = 3
SENT = -7.25                       # a value no factor holds
GUARD = 3                          # untouched doubles in front of and behind L (the aligned view takes one more in front)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = [pytest.param(O.KIND_RBF, id="rbf"), pytest.param(O.KIND_MATERN52, id="matern52")]

# (instance, N, tasks): tasks None = just above the launcher's switch-over count to the narrow (8, 3) instance
DENSE = [((2, 1), 32, 3), ((4, 3), 64, 3), ((8, 7), 128, 3), ((8, 3), 128, None), ((16, 7), 256, 3), ((16, 7), 208, 3),
         ((4, 3), 33, 3), ((16, 7), 255, 3)]
DENSE_IDS = [f"nb{i[0]}wu{i[1]}-N{n}" for i, n, _ in DENSE]


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _buffer(T, N, fill, offset8, device):
    """L (T, N, N) as a view into a filled buffer with guard elements on both sides; offset8: the view starts 8 bytes off the
    16-byte grid (torch's allocations are at least 256-byte aligned)."""
    lead = GUARD + (GUARD % 2 == (0 if offset8 else 1))   # an even number of doubles in front: aligned; odd: 8 bytes off
    buf = torch.full((lead + T * N * N + GUARD,), fill, dtype=torch.float64, device=device)
    assert buf.data_ptr() % 16 == 0
    L = buf[lead:lead + T * N * N].view(T, N, N)
    assert L.data_ptr() % 16 == (8 if offset8 else 0)
    return buf, L, lead


def _guards_untouched(buf, lead, fill, count):
    g = torch.cat([buf[:lead], buf[lead + count:]]).cpu()
    return _same_bits(g, torch.full_like(g, fill))


def _launch_fit(X, y, theta, kind, npts, L, flags):
    T, N, Dx = X.shape
    dev = X.device
    out = dict(alpha=torch.zeros(T, N, dtype=torch.float64, device=dev), info=torch.empty(T, dtype=torch.int32, device=dev))
    for k in ("quad", "logdet", "mll", "jitter"):
        out[k] = torch.empty(T, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib.scaml_gp_fit_fused_f64(X.data_ptr(), y.data_ptr(), theta.data_ptr(), npts.data_ptr() if npts is not None else None, None,
                                             T, N, Dx, int(kind), L.data_ptr() if L is not None else None, out["alpha"].data_ptr(),
                                             out["quad"].data_ptr(), out["logdet"].data_ptr(), out["mll"].data_ptr(), out["info"].data_ptr(),
                                             out["jitter"].data_ptr(), None, flags, torch.cuda.current_stream().cuda_stream)
    _lib.check_rc(rc, "scaml_gp_fit_fused_f64")
    return out


def _launch_potrf(A, y, npts, L, flags):
    T, N, _ = A.shape
    dev = A.device
    out = dict(alpha=torch.zeros(T, N, dtype=torch.float64, device=dev), info=torch.empty(T, dtype=torch.int32, device=dev))
    for k in ("quad", "logdet", "jitter"):
        out[k] = torch.empty(T, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib.scaml_potrf_batched_f64(A.data_ptr(), y.data_ptr(), npts.data_ptr(), None, T, N, L.data_ptr(), out["alpha"].data_ptr(),
                                              out["quad"].data_ptr(), out["logdet"].data_ptr(), out["info"].data_ptr(), out["jitter"].data_ptr(),
                                              None, flags, torch.cuda.current_stream().cuda_stream)
    _lib.check_rc(rc, "scaml_potrf_batched_f64")
    return out


@functools.lru_cache(maxsize=None)
def _problem(N, T, kind, seed_extra):
    """Host tensors of one stack and the oracle's factors of its first three tasks (one of each raggedness), computed once."""
    X, y, theta = _stack(T, N, D, seed=900 + N + 7 * kind + seed_extra)
    npts = torch.tensor([N, N - 1, N - 15] * (T // 3 + 1), dtype=torch.int32)[:T]   # last block: 16, 15, 1 valid rows (N % 16 == 0)
    refs = tuple(O.gp_fit(X[t, :int(npts[t])], y[t, :int(npts[t])], theta[t], kind, dist="direct")["L"] for t in range(3))
    return X, y, theta, npts, refs


def _check_written_set(Lz, Ln, npts, sample):
    """Lz: zero_upper on, SENT fill.  Ln: zero_upper off, NaN fill.  Host tensors."""
    T, N, _ = Lz.shape
    nan_bits = _bits(torch.full((1,), float("nan"), dtype=torch.float64))[0]
    sent_bits = _bits(torch.full((1,), SENT, dtype=torch.float64))[0]
    up = torch.triu(torch.ones(N, N, dtype=torch.bool), diagonal=1)
    for t in sample:
        n = int(npts[t])
        inside = torch.zeros(N, N, dtype=torch.bool)
        inside[:n, :n] = True
        bz, bn = _bits(Lz[t]), _bits(Ln[t])
        assert bool((bz[up & inside] == 0).all()), ("strict upper triangle inside n_t must be +0.0", t, n)
        assert bool((bn[up & inside] == nan_bits).all()), ("upper triangle written without zero_upper", t, n)
        assert bool((bz[~inside] == sent_bits).all()), ("rows / columns at or past n_t written (zero_upper on)", t, n)
        assert bool((bn[~inside] == nan_bits).all()), ("rows / columns at or past n_t written (zero_upper off)", t, n)
        low = ~up & inside
        assert torch.equal(bz[low], bn[low]), ("lower triangle differs between the flag settings", t, n)
        assert bool(torch.isfinite(Lz[t][low]).all()) and bool((bz[low] != sent_bits).all()), ("lower triangle not fully written", t, n)


@pytest.mark.parametrize("offset8", [False, True], ids=["aligned", "offset8"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inst,N,T", DENSE, ids=DENSE_IDS)
def test_written_elements_and_factor(inst, N, T, kind, offset8, device):
    if T is None:
        T = _narrow_kernel_task_count(device)
    X, y, theta, npts, refs = _problem(N, T, kind, inst[1])
    Xd, yd, thd, nd = X.to(device), y.to(device), theta.to(device), npts.to(device)
    bufz, Lz, lead = _buffer(T, N, SENT, offset8, device)
    bufn, Ln, _ = _buffer(T, N, float("nan"), offset8, device)
    oz = _launch_fit(Xd, yd, thd, kind, nd, Lz, _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER)
    on = _launch_fit(Xd, yd, thd, kind, nd, Ln, _lib.FIT_STORE_L)
    assert not oz["info"].cpu().any() and not on["info"].cpu().any()
    assert float(oz["jitter"].abs().max()) == 0.0
    assert _guards_untouched(bufz, lead, SENT, T * N * N) and _guards_untouched(bufn, lead, float("nan"), T * N * N)
    sample = sorted(set(range(3)) | {T - 1})
    Lzh, Lnh = Lz.cpu(), Ln.cpu()
    if T > 3:   # the large stack of the narrow instance: every task's untouched part in one comparison, the details on the sample
        past = torch.arange(N)[None, :] >= npts[:, None]
        outside = past[:, :, None] | past[:, None, :]
        assert bool((Lzh[outside] == SENT).all())
        assert float(torch.triu(torch.where(outside, torch.zeros_like(Lzh), Lzh), diagonal=1).abs().max()) == 0.0
    _check_written_set(Lzh, Lnh, npts, sample)
    for t in range(3):
        n = int(npts[t])
        err = _rel(torch.tril(Lzh[t, :n, :n]), refs[t])
        print(f"inst={inst} N={N} kind={kind} offset8={offset8} task {t} n={n}: rel |dL| = {err:.2e}")
        assert err < 1e-9
    for k in ("mll", "logdet", "quad"):   # the scalars do not depend on how L leaves the chip
        assert torch.equal(oz[k], on[k]), k


@pytest.mark.parametrize("inst,N,T", DENSE, ids=DENSE_IDS)
def test_without_store_L_nothing_is_written(inst, N, T, device):
    if T is None:
        T = _narrow_kernel_task_count(device)
    kind = O.KIND_MATERN52
    X, y, theta, npts, _ = _problem(N, T, kind, inst[1])
    Xd, yd, thd, nd = X.to(device), y.to(device), theta.to(device), npts.to(device)
    buf, L, lead = _buffer(T, N, SENT, False, device)
    for flags in (0, _lib.FIT_ZERO_UPPER):   # the zero-fill is part of storing L: not without it
        out = _launch_fit(Xd, yd, thd, kind, nd, L, flags)
        assert not out["info"].cpu().any()
        h = buf.cpu()
        assert _same_bits(h, torch.full_like(h, SENT))
    ref = _launch_fit(Xd, yd, thd, kind, nd, L, _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER)
    for k in ("mll", "logdet", "quad"):
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("offset8", [False, True], ids=["aligned", "offset8"])
@pytest.mark.parametrize("N,T", [(32, 3), (64, 3), (128, 3), (256, 3), (208, 3), (255, 3)])
def test_potrf_mode_written_elements(N, T, offset8, device):
    """The same kernel handed the matrix (A_in): same written set, and the factor of the fit from X on the same matrix."""
    kind = O.KIND_MATERN52
    X, y, theta, npts, refs = _problem(N, T, kind, 0)
    Xd, yd, thd, nd = X.to(device), y.to(device), theta.to(device), npts.to(device)
    K = ops.kernel_matrix(Xd, thd, kind, add_noise=True)
    bufz, Lz, lead = _buffer(T, N, SENT, offset8, device)
    bufn, Ln, _ = _buffer(T, N, float("nan"), offset8, device)
    oz = _launch_potrf(K, yd, nd, Lz, _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER)
    on = _launch_potrf(K, yd, nd, Ln, _lib.FIT_STORE_L)
    assert not oz["info"].cpu().any() and not on["info"].cpu().any()
    assert _guards_untouched(bufz, lead, SENT, T * N * N) and _guards_untouched(bufn, lead, float("nan"), T * N * N)
    Lzh = Lz.cpu()
    _check_written_set(Lzh, Ln.cpu(), npts, range(T))
    for t in range(3):
        n = int(npts[t])
        err = _rel(torch.tril(Lzh[t, :n, :n]), refs[t])
        print(f"potrf N={N} offset8={offset8} task {t} n={n}: rel |dL| = {err:.2e}")
        assert err < 1e-9


def _launch_blocked(X, y, theta, kind, npts, L, flags):
    T, N, Dx = X.shape
    dev = X.device
    out = dict(alpha=torch.zeros(T, N, dtype=torch.float64, device=dev), info=torch.empty(T, dtype=torch.int32, device=dev),
               Linv_diag=torch.empty(T, N // 16, 16, 16, dtype=torch.float64, device=dev))
    for k in ("quad", "logdet", "mll", "jitter"):
        out[k] = torch.empty(T, dtype=torch.float64, device=dev)
    nbytes = int(_lib.lib.scaml_gp_fit_blocked_workspace_bytes(T, N))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    with torch.cuda.device(dev):
        rc = _lib.lib.scaml_gp_fit_blocked_f64(X.data_ptr(), y.data_ptr(), theta.data_ptr(), npts.data_ptr() if npts is not None else None, None,
                                               T, N, Dx, int(kind), L.data_ptr(), out["alpha"].data_ptr(), out["quad"].data_ptr(),
                                               out["logdet"].data_ptr(), out["mll"].data_ptr(), out["info"].data_ptr(), out["jitter"].data_ptr(),
                                               out["Linv_diag"].data_ptr(), flags, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()   # (the workspace is this function's)
    _lib.check_rc(rc, "scaml_gp_fit_blocked_f64")
    assert _lib.lib.scaml_debug_blocked_fit_path(-1) == 1   # the sequence of launches: gp_fit_blocked_kernel factors the diagonal blocks
    return out


BLOCKED_N1 = 256   # the first diagonal block of the 2 x 2 factorisation


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("offset8", [False, True], ids=["aligned", "offset8"])
@pytest.mark.parametrize("kind", KINDS)
def test_blocked_kernel(kind, offset8, ragged, device, sequence_of_launches):  # noqa: F811
    """N = 272 through the 2 x 2 sequence of launches, launched through the C ABI into pre-filled buffers: the first diagonal block
    is factored by gp_fit_blocked_kernel<16, 7> with the leading dimension (272) and the task stride of the WHOLE matrix, the only
    case where they differ from the block's own size.  Checked on block (0, 0), whose every element is that kernel's: the same
    written set as in the dense cases.  Ragged: the first block's last 16-block holds 16, 16, 16, 15 and 1 valid rows; the rows at
    or past n_t, which the strip solve of the later launches reads, are zeroed beforehand as the front end does, everything else
    carries the fill."""
    N, T, N1 = 272, 5 if ragged else 3, BLOCKED_N1
    X, y, theta = _stack(T, N, D, seed=977 + 7 * kind)
    npts = torch.tensor([272, 271, 257, 255, 241] if ragged else [N] * T, dtype=torch.int32)
    Xd, yd, thd = X.to(device), y.to(device), theta.to(device)
    nd = npts.to(device) if ragged else None
    res = {}
    for name, fill, flags in (("z", SENT, _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER), ("n", float("nan"), _lib.FIT_STORE_L)):
        buf, L, lead = _buffer(T, N, fill, offset8, device)
        for t in range(T):
            L[t, int(npts[t]):, :] = 0.0
        out = _launch_blocked(Xd, yd, thd, kind, nd, L, flags)
        assert not out["info"].cpu().any()
        assert _guards_untouched(buf, lead, fill, T * N * N)
        res[name] = L.cpu()
    n1 = torch.clamp(npts, max=N1)
    Lz, Ln = res["z"][:, :N1, :N1].contiguous(), res["n"][:, :N1, :N1].contiguous()
    nan_bits = _bits(torch.full((1,), float("nan"), dtype=torch.float64))[0]
    sent_bits = _bits(torch.full((1,), SENT, dtype=torch.float64))[0]
    up = torch.triu(torch.ones(N1, N1, dtype=torch.bool), diagonal=1)
    for t in range(T):
        n = int(n1[t])
        inside = torch.zeros(N1, N1, dtype=torch.bool)
        inside[:n, :n] = True
        right = torch.zeros(N1, N1, dtype=torch.bool)
        right[:n, n:] = True       # columns at or past n_t in the valid rows: the fill (the rows at or past n_t: the zeros put there)
        bz, bn = _bits(Lz[t]), _bits(Ln[t])
        assert bool((bz[up & inside] == 0).all()), ("strict upper triangle of block (0, 0) must be +0.0", t, n)
        assert bool((bn[up & inside] == nan_bits).all()), ("upper triangle of block (0, 0) written without zero_upper", t, n)
        assert bool((bz[right] == sent_bits).all()) and bool((bn[right] == nan_bits).all()), ("columns at or past n_t written", t, n)
        assert bool((bz[n:, :] == 0).all()) and bool((bn[n:, :] == 0).all()), ("rows at or past n_t written", t, n)
        low = ~up & inside
        assert torch.equal(bz[low], bn[low]), ("lower triangle differs between the flag settings", t, n)
    for t in range(T):   # the whole factor, all four blocks, against the oracle
        n = int(npts[t])
        ref = O.gp_fit(X[t, :n], y[t, :n], theta[t], kind, dist="direct")["L"]
        err = _rel(torch.tril(res["z"][t, :n, :n]), ref)
        print(f"blocked N={N} kind={kind} offset8={offset8} task {t} n={n}: rel |dL| = {err:.2e}")
        assert err < 1e-9


def test_jitter_retries_refill_the_same_zeros(device):
    """tests/golden/edge_duplicates_jitter_T3_N32_rbf: tasks 0 and 1 need the rungs 1e-8 and 1e-7 (each retry fills the upper
    triangle again), task 2 is clean.  With retries: the factor of tests/test_fit_gpu.py's golden comparison and exact zeros.
    Without (NO_RETRY): tasks 0 and 1 fail, and their clean neighbour is bit-identical to the run with retries."""
    g = np.load(os.path.join(GOLDEN, "edge_duplicates_jitter_T3_N32_rbf.npz"))
    kind = int(g["kind"])
    X, y, theta = (torch.from_numpy(g[k]).to(device) for k in ("X", "y", "theta"))
    T, N, _ = X.shape
    assert (g["jitter"] > 0).tolist() == [True, True, False] and (g["n_points"] == N).all()
    buf, L, lead = _buffer(T, N, SENT, False, device)
    out = _launch_fit(X, y, theta, kind, None, L, _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER)
    assert not out["info"].cpu().any()
    np.testing.assert_array_equal(out["jitter"].cpu().numpy(), g["jitter"])
    assert _guards_untouched(buf, lead, SENT, T * N * N)
    Lh = L.cpu()
    assert bool((_bits(torch.triu(Lh, diagonal=1)) == 0).all())
    for t in range(T):
        tol = (1e-9 if g["jitter"][t] == 0 else 1e-4) * np.abs(g["L"][t]).max()   # (a rescued task has condition number ~1e10)
        np.testing.assert_allclose(torch.tril(Lh[t]).numpy(), g["L"][t], rtol=0, atol=tol)
    again = ops.gp_fit_fused(X, y, theta, kind)
    assert _same_bits(again["L"].cpu(), Lh)
    buf1, L1, _ = _buffer(T, N, SENT, False, device)
    one = _launch_fit(X, y, theta, kind, None, L1, _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER | _lib.FIT_NO_RETRY)
    assert [i > 0 for i in one["info"].cpu().tolist()] == [True, True, False]
    assert _same_bits(L1[2].cpu(), Lh[2]) and _guards_untouched(buf1, lead, SENT, T * N * N)
    for k in ("mll", "logdet", "quad"):
        assert torch.equal(one[k][2], out[k][2]), k
