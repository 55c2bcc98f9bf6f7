"""GPU: the early chain of the fused fit (csrc/gp_fit_fused.hip) -- the owners of D_0, R_1 and D_1 park their tile while the
kernel matrix is still being built and the panel wave factors the first two diagonal blocks inside the build, whenever the staged
points and the tile images end in front of the panel wave's LDS outputs (`early`: N <= 128 classes D <= 44, N > 128 D <= 20).

Judged as the existing fit tests are: tests/_fit_bounds.py (long-double references, a-priori bounds, the padding rules) for the
factor, Linv_diag, alpha and the scalars of the fit from X and of the POTRF entry point; tests/_failpath_cases.py (status as LAPACK
reports it, the jitter ladder, its tolerances) for the failed pivots.  Shapes: one and two blocks in the smallest instance, the class
edges, every kernel instance at its smallest N, (16, 7) at 241 and 256 points dense and as both blocks of the blocked fit, D on
either side of the overlay gate of every instance, point counts around the first block, and a first non-positive pivot in block 0,
1 and 2."""
import numpy as np
import pytest
import torch

from scamlgp_amd import ops
from tests import _failpath_cases as C
from tests import _fit_bounds as B
from tests.test_fit_bounds_gpu import Device

pytestmark = pytest.mark.gpu

RBF, MATERN = B.KIND_RBF, B.KIND_MATERN52


def _check_fit_with_counts(be, c, n_points):
    """check_fit of tests/_fit_bounds.py on the case's inputs with the point counts given here."""
    inp = B.fit_inputs(c)
    inp["n_points"] = np.asarray(n_points, dtype=np.int32)
    for t, n in enumerate(n_points):
        inp["y"][t, n:] = 0.0
    out = be.fit(c, inp)
    assert (out["info"] == 0).all() and (out["jitter"] == 0.0).all(), (out["info"], out["jitter"])
    key = (B.fit_instance(c), B.FAMILY[c.kind])
    for t, n in enumerate(n_points):
        th = inp["theta"][t]
        A = B.kmat_reference(inp["X"][t, :n], th, c.kind, True, noise_add=th[c.D + 1]) if n else None
        B.check_factor_task(f"{B.fit_id(c)} n={n}", key, out, t, n, c.N, inp["y"][t], A, cache_key=("early", c, t))
    return out


# ---- shapes: blocks, class edges, every instance -------------------------------------------------------------------------------
# N = 16: the second block of the (2, 1) instance is identity padding; 17: its last block holds one row; 32 | 33 the class edge;
# 48: three blocks.  Then each instance at its smallest N: (4, 3) 33, (8, 7) 65, (16, 7) 129 and, with a stack larger than the CU
# count, the narrow (8, 3) at 65 (three tasks referenced).  (16, 7) again at 241 and 256.
SHAPES = [B._f(T=3, N=N, D=2, kind=kind, ragged=0) for N, kind in ((16, RBF), (17, MATERN), (32, RBF), (33, MATERN), (48, RBF), (65, MATERN), (129, RBF))]
SHAPES += [B._f(T=2, N=241, D=8, kind=MATERN), B._f(T=2, N=256, D=8, kind=RBF, ragged=1),
           B._f(T=B.CUS + 1, N=65, D=2, kind=RBF, ragged=0, refs=(0, B.CUS // 2, B.CUS))]


@pytest.mark.parametrize("case", SHAPES, ids=B.fit_id)
def test_shapes(case, device):
    B.check_fit(Device(device), case)


def test_every_instance_is_covered():
    assert {B.fit_instance(c) for c in SHAPES} == {f"fit_fused[nb{nb},wu{wu}]" for nb, wu in ((2, 1), (4, 3), (8, 7), (8, 3), (16, 7))}


# ---- the blocked fit: block 1 is the (16, 7) blocked instance from X, block 2 the blocked instance of its size in POTRF mode ----
# N = 272: block 2 is (2, 1); N = 512 with 497 and 512 points: block 2 is (16, 7) at 241 and 256 points.  path 1: the launch sequence.
def test_blocked_small_second_block(device):
    B.check_fit(Device(device), B._f(T=2, N=272, D=8, kind=MATERN, path=1))


def test_blocked_both_blocks_16_7(device):
    _check_fit_with_counts(Device(device), B._f(T=2, N=512, D=8, kind=RBF, path=1, noise=1e-3), [497, 512])


# ---- D on either side of the overlay gate -----------------------------------------------------------------------------------
# early <=> XROWS * NP + images <= 3 * NP * 17 with XROWS = D rounded up to 4, + 4 (csrc/gp_fit_fused.hip):
# NP = 256 (24 images of 256 doubles): XROWS <= 27, D <= 20 | 21 ..;  the other instances (no images): XROWS <= 51, D <= 44 | 45 ..
GATE = [(129, 20), (129, 24), (129, 21), (33, 44), (33, 45), (17, 44), (17, 48), (65, 44), (65, 45)]


@pytest.mark.parametrize("N,D", GATE)
def test_both_sides_of_the_overlay_gate(N, D, device):
    B.check_fit(Device(device), B._f(T=2, N=N, D=D, kind=MATERN if D % 2 else RBF, ragged=0))


def test_the_gate_pairs_are_the_gate():
    for N, D in GATE:
        p = B.DP.fit_plan(2, N, D, B.CUS)
        build = (((D + 3) & ~3) + 4) * p.nb * 16 + (24 * 256 if p.nb == 16 else 0)
        assert (build <= 3 * p.nb * 16 * 17) == (D <= (20 if p.nb == 16 else 44)), (N, D)


# ---- point counts around the first block ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,counts", [(48, (1, 16, 17)), (129, (15, 17, 33)), (256, (16, 17, 241))])
def test_short_point_counts(N, counts, device):
    _check_fit_with_counts(Device(device), B._f(T=3, N=N, D=3, kind=MATERN), list(counts))


# ---- POTRF mode (the matrix is given: nothing staged, the early path always) ---------------------------------------------------
@pytest.mark.parametrize("N", [16, 17, 33, 48, 129])
def test_potrf_mode(N, device):
    B.check_potrf(Device(device), B._f(T=3, N=N, D=4, kind=RBF, ragged=0))


# ---- Linv_diag: W_0 and W_1 are written during the build ---------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(48, 3), (129, 20), (129, 24), (256, 8)])
def test_first_two_inverse_blocks_against_the_oracle(N, D, device):
    """Linv_diag blocks 0 and 1 against the inverses of the diagonal blocks of the ORACLE's factor (numpy fp64 Cholesky of the
    long-double kernel matrix), not of the device's own.  Bound, to first order with a factor 2 for the rest: both factorisations
    are backward stable, L L^T = A + E with |E| <= gamma(N + 1) |L| |L^T| (Higham, Thm 10.3), the device's A carries the kernel
    matrix's own bound and the oracle's one rounding; the leading 32 x 32 factor moves by |dL| <= |L| (|L^-1| |dA| |L^-T|)
    (Higham, Sec. 10.3: the triangular part only shrinks it), a block's inverse by |W| |dL_bb| |W|, and the inversion itself
    adds gamma(20) |W| |L_bb| |W| (wblock_reference of tests/_fit_bounds.py)."""
    c = B._f(T=2, N=N, D=D, kind=MATERN)
    inp = B.fit_inputs(c)
    out = Device(device).fit(c, inp)
    assert (out["info"] == 0).all()
    u = 2.0 ** -53
    for t in range(c.T):
        th = inp["theta"][t]
        A = B.kmat_reference(inp["X"][t], th, c.kind, True, noise_add=th[D + 1])
        A64 = A.ref.astype(np.float64)
        L = np.linalg.cholesky(A64)
        Lm = np.abs(L[:32, :32])
        Wm = np.abs(np.linalg.inv(L[:32, :32]))
        dA = 2 * float(B.gamma(N + 1)) * (np.abs(L) @ np.abs(L).T)[:32, :32] + A.bound[:32, :32].astype(np.float64) + u * np.abs(A64[:32, :32])
        dL = Lm @ (Wm @ dA @ Wm.T)
        for b in (0, 1):
            s = slice(16 * b, 16 * b + 16)
            W = np.linalg.inv(L[s, s])
            aW = np.abs(W)
            bound = 2 * aW @ dL[s, s] @ aW + 2 * float(B.gamma(20)) * aW @ np.abs(L[s, s]) @ aW
            err = np.abs(out["Linv_diag"][t, b] - W)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            print(f"[early chain] N={N} D={D} task {t} block {b}: largest error / bound {ratio:.3e}, bound / scale {float(bound.max() / aW.max()):.3e}", flush=True)
            assert (err <= bound).all(), (t, b, ratio)


# ---- a first non-positive pivot in block 0, 1 and 2 --------------------------------------------------------------------------
PIVOTS = (5, 16, 17, 20, 33, 40)     # 1-based: block 0 (its last pivot too), block 1 (its first too), block 2


def _decoupled(n, k, value, g):
    """SPD but for row / column k (1-based), which is decoupled with `value` on the diagonal: the first k - 1 pivots are safely
    positive, pivot k is `value` exactly."""
    A = C.spd_matrix(n, g)
    A[k - 1, :] = 0.0
    A[:, k - 1] = 0.0
    A[k - 1, k - 1] = value
    return A


def _failing_stack(N, value):
    T = len(PIVOTS)
    A = torch.stack([_decoupled(N, k, value, C._gen(11, t)) for t, k in enumerate(PIVOTS)])
    y = torch.stack([torch.randn(N, dtype=C.F64, generator=C._gen(12, t)) for t in range(T)])
    return A, y, [dict(what="clean", rung=None, k=0, n=N)] * T


def _host(out):
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("N", [48, 129, 256])      # (4, 3), (16, 7) at its smallest N and full
def test_failed_pivot_single_attempt_and_hopeless(N, device):
    """An indefinite matrix: info is the failing pivot's index with retry=False (jitter_used 0) and after the whole ladder (1e-6)."""
    A, y, _ = _failing_stack(N, -1.0)
    n_pts = torch.full((len(PIVOTS),), N, dtype=torch.int32, device=device)
    single = _host(ops.potrf_batched(A.to(device), y.to(device), n_points=n_pts, retry=False))
    assert single["info"].tolist() == list(PIVOTS) and single["jitter"].tolist() == [0.0] * len(PIVOTS)
    ladder = _host(ops.potrf_batched(A.to(device), y.to(device), n_points=n_pts))
    refs = [dict(zip(("jitter", "info"), C.ladder(A[t]))) for t in range(len(PIVOTS))]
    assert [r["info"] for r in refs] == list(PIVOTS)
    assert ladder["info"].tolist() == list(PIVOTS) and ladder["jitter"].tolist() == [C.RUNGS[-1]] * len(PIVOTS)
    for o in (single, ladder):
        assert bool(torch.isnan(o["quad"]).all()) and bool(torch.isnan(o["logdet"]).all())


@pytest.mark.parametrize("N", [48, 129, 256])
def test_failed_pivot_rescued_at_the_next_jitter(N, device):
    """Pivot k is -5e-9: the first attempt fails there, the retry at 1e-8 succeeds; jitter, status and the outputs as
    tests/_failpath_cases.py holds a rescued task."""
    A, y, plan_ = _failing_stack(N, -5e-9)
    n_pts = torch.full((len(PIVOTS),), N, dtype=torch.int32, device=device)
    single = _host(ops.potrf_batched(A.to(device), y.to(device), n_points=n_pts, retry=False))
    assert single["info"].tolist() == list(PIVOTS)
    out = _host(ops.potrf_batched(A.to(device), y.to(device), n_points=n_pts))
    refs = [C.reference(A[t], y[t]) for t in range(len(PIVOTS))]
    assert [r["jitter"] for r in refs] == [C.RUNGS[0]] * len(PIVOTS)
    C.check_outputs(out, plan_, refs)


@pytest.mark.parametrize("N", [48, 256])
def test_nan_input(N, device):
    """A NaN on the diagonal of a given matrix fails at that pivot at every rung; a NaN coordinate of a fit from X poisons the
    diagonal (status > 0) and leaves the neighbours alone."""
    A, y, _ = _failing_stack(N, float("nan"))
    out = _host(ops.potrf_batched(A.to(device), y.to(device)))
    assert out["info"].tolist() == list(PIVOTS) and out["jitter"].tolist() == [C.RUNGS[-1]] * len(PIVOTS)
    B.check_fit(Device(device), B._f(T=3, N=N, D=2, kind=RBF, ragged=0, nan_task=1))
