"""CPU half of the target-fit bounds (tests/_target_fit_bounds.py): the reference's formulas against torch autograd through the
oracle, then every column-path input set, the ragged batch and the refit through the single-threaded host build of
csrc/gp_target_fit.hip (tests/host_emul/target_fit_batched_emul.cpp, which carries the single-problem entry too), and every
matrix-core input set through a plain numpy fp64 stand-in of that path's formulation (blocked factor on 16 x 16 tiles with explicit
inverses of the diagonal tiles, X = L^-1 by block columns, K^-1 = X^T X, the packed doubled G) -- all held to the bounds and caps the
MI355X is held to in tests/test_target_fit_bounds_gpu.py.  The stand-in also carries the planted faults, each of which must be
rejected; the assertion text of each is printed (profiles/target_fit_bounds_notes.md records it)."""
import ctypes
import math

import numpy as np
import pytest
import scipy.linalg
import torch

torch.set_num_threads(1)

from tests import _target_fit_bounds as TF
from tests._host_emul import DP, IP, build, ptr as _p
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF, SENTINEL, _kernel
from tests._target_bounds import potrf_reference
from tests._target_problem import oracle_mll_and_grad

LDS_LIMIT = 160 * 1024


def _buffers(rows, P):
    r = rows + TF.GUARD
    return dict(value=np.full(r, SENTINEL), grad=np.full((r, P), SENTINEL), info=np.full(r, -7, dtype=np.int32), jitter=np.full(r, SENTINEL))


class Emul:
    """The backend interface of tests/_target_fit_bounds.py on the host build: column-by-column elimination only, one thread."""
    name, arith = "emul", TF.SERIAL_ARITH

    def __init__(self, lib):
        self.lib = lib

    def max_n(self, T, D):
        n = 0
        while self.lib.emul_target_fit_problem_lds_doubles(n + 1, T, D, 8, 0) * 8 <= LDS_LIMIT:
            n += 1
        return n

    def path_of(self, n, T, D, forced):
        return "col"

    def _single(self, prob, z, mode, max_iter, o, stats):
        B = z.shape[0]
        mt, cp, X, y = (np.ascontiguousarray(prob[k]) for k in ("means_t", "covs_p", "X", "y"))
        rc = self.lib.emul_target_fit_single(_p(mt), _p(cp), _p(X), _p(y), prob["m_all"], prob["s_all"], _p(prob["spec"]), _p(z), B, prob["n"], prob["T"], prob["D"],
                                             prob["kind"], mode, max_iter, 10, 1e-5, 2.2e-9, _p(o["value"]), _p(o["grad"]), _p(o["info"]), _p(o["jitter"]), _p(stats))
        assert rc == 0

    def _batched(self, b, z, mode, max_iter, o, stats):
        S, B, _ = z.shape
        rc = self.lib.emul_target_fit_batched(_p(b["means_t"]), _p(b["covs_p"]), _p(b["X"]), _p(b["y"]), _p(b["n_points"]), _p(b["m_all"]), _p(b["s_all"]),
                                              _p(b["spec"]), _p(z), S, B, b["n_max"], b["T"], b["D"], b["kind"], mode, max_iter, 10, 1e-5, 2.2e-9, _p(o["value"]),
                                              _p(o["grad"]), _p(o["info"]), _p(o["jitter"]), _p(stats))
        assert rc == 0

    def mll(self, prob, z, forced):
        o = _buffers(z.shape[0], z.shape[1])
        self._single(prob, np.ascontiguousarray(z.copy()), 0, 0, o, np.zeros((z.shape[0], 4), dtype=np.int32))
        return o

    def mll_batched(self, b, z, forced):
        S, B, P = z.shape
        o = _buffers(S * B, P)
        self._batched(b, np.ascontiguousarray(z.copy()), 0, 0, o, np.zeros((S * B, 4), dtype=np.int32))
        return o

    def fit(self, prob, z0, forced, max_iter):
        B, P = z0.shape
        o, z, stats = _buffers(B, P), np.ascontiguousarray(z0.copy()), np.zeros((B, 4), dtype=np.int32)
        self._single(prob, z, 1, max_iter, o, stats)
        return dict(z=z, value=o["value"][:B], info=o["info"][:B], jitter=o["jitter"][:B], stats=stats)

    def fit_batched(self, b, z0, forced, max_iter):
        S, B, P = z0.shape
        o, z, stats = _buffers(S * B, P), np.ascontiguousarray(z0.copy()), np.zeros((S, B, 4), dtype=np.int32)
        self._batched(b, z, 1, max_iter, o, stats)
        return dict(z=z, value=o["value"][:S * B].reshape(S, B), info=o["info"][:S * B].reshape(S, B), jitter=o["jitter"][:S * B].reshape(S, B), stats=stats)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "target_fit_batched_emul")
    lib.emul_target_fit_batched.restype = ctypes.c_int
    lib.emul_target_fit_batched.argtypes = [DP, DP, DP, DP, IP, DP, DP, DP, DP] + [ctypes.c_int] * 9 + [ctypes.c_double, ctypes.c_double, DP, DP, IP, DP, IP]
    lib.emul_target_fit_single.restype = ctypes.c_int
    lib.emul_target_fit_single.argtypes = [DP, DP, DP, DP, ctypes.c_double, ctypes.c_double, DP, DP] + [ctypes.c_int] * 8 + [ctypes.c_double, ctypes.c_double, DP, DP, IP,
                                                                                                                    DP, IP]
    lib.emul_target_fit_problem_lds_doubles.restype, lib.emul_target_fit_problem_lds_doubles.argtypes = ctypes.c_longlong, [ctypes.c_int] * 5
    return Emul(lib)


# ------------------------------------------------------------------------------------------------------------------
# the numpy fp64 stand-in of the matrix-core formulation (and the planted faults)
def _logp(pr, x):
    kind, p1, p2 = int(pr[0]), pr[1], pr[2]
    if kind == 1:
        return p1 * math.log(p2) - math.lgamma(p1) + (p1 - 1.0) * np.log(x) - p2 * x
    if kind == 2:
        u = (np.log(x) - p1) / p2
        return -math.log(p2) - 0.9189385332046727 - np.log(x) - 0.5 * u * u
    return np.zeros_like(x)


def _dlogp(pr, x):
    kind, p1, p2 = int(pr[0]), pr[1], pr[2]
    if kind == 1:
        return (p1 - 1.0) / x - p2
    if kind == 2:
        return -(1.0 + (np.log(x) - p1) / (p2 * p2)) / x
    return np.zeros_like(x)


def standin_eval(prob, z, fault=None):
    """(value, grad, info, jitter) at one z in fp64, in the matrix-core path's formulation.  fault: one of FAULTS."""
    n, T, D, kind, spec = prob["n"], prob["T"], prob["D"], prob["kind"], prob["spec"]
    P = D + 2 + T
    lo, hi = np.array([spec[0]] * D + [spec[2], spec[4]]), np.array([spec[1]] * D + [spec[3], spec[5]])
    with np.errstate(all="ignore"):
        sg = 1.0 / (1.0 + np.exp(-z[:D + 2]))
        th, dth = lo + (hi - lo) * sg, (hi - lo) * sg * (1.0 - sg)
        if fault == "dth_neighbour":
            dth[0] = dth[1]
        invl, os_, noise = 1.0 / th[:D], th[D], th[D + 1]
        w = z[D + 2:]
        inv_s = 1.0 / prob["s_all"]
        inv_s2 = inv_s * inv_s
        w2 = w * w * inv_s2
        ia, ib = np.tril_indices(n)
        cp, M = prob["covs_p"][:, :ia.size], prob["means_t"][:, :n]
        off = ia != ib
        df2 = ((prob["X"][ia] - prob["X"][ib]) * invl) ** 2
        d2 = df2.sum(-1)
        kk, dk = _kernel(d2, kind)
        kk = kk + (d2 - d2)       # (a non-finite distance gives NaN in both families)
        acc = w2 @ cp
        Tm = T - 1 if (fault == "mean_tail" and T % 4) else T
        r = np.zeros(16 * ((n + 15) // 16))
        r[:n] = prob["y"][:n] - (w[:Tm] @ M[:Tm] - prob["m_all"]) * inv_s
        nb = (n + 15) // 16
        blk = [slice(16 * i, 16 * i + 16) for i in range(nb)]
        info, jit = 0, 0.0
        for jit in (0.0, 1e-8, 1e-7, 1e-6):
            info = 0
            A = np.eye(16 * nb)
            A[ia, ib] = acc + np.where(off, os_ * kk, os_ + (noise if fault == "no_jitter" else noise + jit))
            W = [None] * nb
            for K in range(nb):
                Akk = np.tril(A[blk[K], blk[K]])
                Akk = Akk + np.tril(Akk, -1).T
                try:
                    if not np.isfinite(Akk).all():
                        raise np.linalg.LinAlgError
                    Lkk = np.linalg.cholesky(Akk)
                except np.linalg.LinAlgError:
                    info = 16 * K + 1
                    break
                W[K] = scipy.linalg.solve_triangular(Lkk, np.eye(16), lower=True)
                A[blk[K], blk[K]] = Lkk
                for i in range(K + 1, nb):
                    A[blk[i], blk[K]] = A[blk[i], blk[K]] @ W[K].T
                for i in range(K + 1, nb):
                    for j in range(K + 1, i + 1):
                        A[blk[i], blk[j]] -= A[blk[i], blk[K]] @ A[blk[j], blk[K]].T
            if not info:
                break
        if info:
            return np.nan, np.zeros(P), info, jit
        Xi = np.zeros((16 * nb, 16 * nb))
        for k in range(nb):
            Xi[blk[k], blk[k]] = W[k]
            for i in range(k + 1, nb):
                sacc = np.zeros((16, 16))
                for j in range(k, i):
                    sacc += A[blk[i], blk[j]] @ Xi[blk[j], blk[k]]
                Xi[blk[i], blk[k]] = -W[i] @ sacc
        v = Xi @ r
        quad = v[:n] @ v[:n]
        logdet = (2.0 * np.log(np.diagonal(A)[:n])).sum()
        alpha = (Xi.T @ v)[:n]
        Xk = Xi.copy()
        if fault == "kinv_row":
            Xk[n - 1] = 0.0
        Kinv = (Xk.T @ Xk)[:n, :n]
        G2 = 0.5 * (alpha[ia] * alpha[ib] - Kinv[ia, ib])
        dbl = off & ~((ia // 16 == 1) & (ib // 16 == 0)) if fault == "tile_not_doubled" else off
        G2 = np.where(dbl, 2.0 * G2, G2)
        lp = _logp(spec[6:9], th[:D]).sum() + _logp(spec[9:12], th[D]) + _logp(spec[12:15], th[D + 1]) + _logp(spec[15:18], w).sum()
        value = (-0.5 * (quad + logdet + n * 1.8378770664093453) + lp) / n
        inv_n = 1.0 / n
        g = np.zeros(P)
        fac = 2.0 * w * inv_s2
        if fault == "w_factor2":
            fac[0] = w[0] * inv_s2
        g[D + 2:] = ((cp @ G2) * fac + (M @ alpha) * inv_s + _dlogp(spec[15:18], w)) * inv_n
        dkg = dk.copy()
        if fault == "slope":
            dkg[np.argmax(np.where(off, np.abs(G2), -1.0))] *= 1.0 + 1e-7
        if fault == "matern_rbf_slope":
            dkg = -0.5 * kk
        h = np.where(off, -2.0 * G2 * os_ * dkg, 0.0)
        ssum = np.zeros(D + 2)
        for d in range(D):
            terms = h * df2[:, d]
            if fault == "invl_one_wave" and d == 0:
                ssum[d] = terms[0::8].sum() * invl[d] + sum(terms[v::8].sum() for v in range(1, 8))
            else:
                ssum[d] = terms.sum() * invl[d]
        ssum[D] = (G2 * np.where(off, kk, 1.0)).sum()
        ssum[D + 1] = G2[~off].sum()
        dpr = np.concatenate([_dlogp(spec[6:9], th[:D]), _dlogp(spec[9:12], th[D:D + 1]), _dlogp(spec[12:15], th[D + 1:])])
        g[:D + 2] = (ssum + dpr) * dth * inv_n
    return value, g, 0, jit


FAULTS = ("w_factor2", "mean_tail", "kinv_row", "tile_not_doubled", "slope", "no_jitter", "dth_neighbour", "invl_one_wave", "matern_rbf_slope")


class StandIn:
    name, arith = "standin", TF.SERIAL_ARITH

    def __init__(self, fault=None):
        self.fault = fault

    def path_of(self, n, T, D, forced):
        return "mfma"

    def max_n(self, T, D):
        return 112

    def _rows(self, o, row, prob, z):
        for b in range(z.shape[0]):
            o["value"][row + b], o["grad"][row + b], o["info"][row + b], o["jitter"][row + b] = standin_eval(prob, z[b], self.fault)

    def mll(self, prob, z, forced):
        o = _buffers(z.shape[0], z.shape[1])
        self._rows(o, 0, prob, z)
        return o

    def mll_batched(self, b, z, forced):
        S, B, P = z.shape
        o = _buffers(S * B, P)
        for s in range(S):
            n = int(b["n_points"][s])
            prob = dict(means_t=b["means_t"][s], covs_p=b["covs_p"][s], X=b["X"][s, :n], y=b["y"][s, :n], m_all=b["m_all"][s], s_all=b["s_all"][s], n=n, T=b["T"],
                        D=b["D"], kind=b["kind"], spec=b["spec"])
            self._rows(o, s * B, prob, z[s])
        return o


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52])
def test_reference_formulas_match_oracle_autograd(kind):
    """Pins the reference's formulas (not a tolerance for any kernel): 1e-9 relative on the value and on every gradient entry, the
    tiny weight and the weight on its bound included; and the reference's own factor reproduces K in long double."""
    prob = TF.make_problem(12, 4, 3, kind)
    z = TF.starts(prob, 2)
    n, T = prob["n"], prob["T"]
    C = TF.unpack(prob["covs_p"], n).astype(np.float64)
    tp = dict(X=torch.from_numpy(prob["X"]), y=torch.from_numpy(prob["y"]), source_means=torch.from_numpy(np.ascontiguousarray(prob["means_t"].T)),
              source_covs=torch.from_numpy(np.ascontiguousarray(C.transpose(1, 2, 0))), m_all=prob["m_all"], s_all=prob["s_all"], n=n, T=T, D=prob["D"], kind=kind)
    for b in range(2):
        ref = TF.reference(prob, z[b], "col")
        val, g = oracle_mll_and_grad(tp, torch.from_numpy(z[b]))
        assert abs(float(ref.value) - float(val)) <= 1e-9 * abs(float(val))
        err = np.abs(ref.grad.astype(np.float64) - g.numpy())
        assert (err <= 1e-9 * np.abs(g.numpy())).all(), (err / np.abs(g.numpy()), g.numpy())
        L = ref.parts["L"]
        LLt, q = potrf_reference(L.astype(np.float64), ref.parts["K"], 0.0)
        assert (np.abs(L @ L.T - ref.parts["K"]) <= 1e-17 * np.abs(ref.parts["K"]).max()).all() and (np.abs(LLt - q.ref) <= q.bound).all()


@pytest.mark.parametrize("case", TF.COLUMN_CASES, ids=TF.case_id)
def test_column_path_host_build_within_bounds(emul, case):
    TF.check_mll(emul, case)


@pytest.mark.parametrize("case", [c for c in TF.CASES if c.path == "mfma"], ids=TF.case_id)
def test_matrix_core_standin_within_bounds(case):
    TF.check_mll(StandIn(), case)


def test_dispatch_by_shape_is_by_n_alone_on_these_sets(emul):
    """target_fit_mfma_shape (csrc/gp_target_params.h) for a workgroup of 8 waves: every n <= 112 of the input sets fits the matrix-core
    footprint at its (T, D) -- the two footprints differ exactly where the matrix cores are taken."""
    f = emul.lib.emul_target_fit_problem_lds_doubles
    shapes = [(c.n, c.T, c.D) for c in TF.CASES + TF.NAN_CASES + TF.REFIT_CASES if c.n] + [(n, TF.RAGGED["T"], TF.RAGGED["D"]) for n in TF.RAGGED["sizes"]]
    for n, T, D in shapes:
        path = TF.device_path(n, T, D)
        assert (path == "mfma") == (n <= 112), (n, T, D)
        assert (f(n, T, D, 8, 1) != f(n, T, D, 8, 0)) == (path == "mfma"), (n, T, D)
        assert f(n, T, D, 8, 1) * 8 <= LDS_LIMIT


def test_caps_hold_for_the_device_on_every_input_set(emul):
    """The conditions on the inputs, with the device's chains and the path its dispatch takes: the shapes, the ragged batch (whose
    n <= 112 problems take the matrix cores there, the columns in the host build) and the sets around the non-finite inputs."""
    for c in TF.CASES + TF.NAN_CASES:
        c = TF.resolve(emul, c)
        prob = TF.make_problem(c.n, c.T, c.D, c.kind)
        for b, z in enumerate(TF.starts(prob, 3)):
            TF.assert_caps(f"{TF.case_id(c)} start {b}", TF.reference(prob, z, c.path, TF.DEVICE_ARITH))
    for kind in (KIND_RBF, KIND_MATERN52):
        for s, n in enumerate(TF.RAGGED["sizes"]):
            prob = TF.make_problem(n, TF.RAGGED["T"], TF.RAGGED["D"], kind, seed=5 + s)
            for b, z in enumerate(TF.starts(prob, 2, seed=5)):
                TF.assert_caps(f"ragged n{n} kind {kind} start {b}", TF.reference(prob, z, TF.device_path(n, TF.RAGGED["T"], TF.RAGGED["D"]), TF.DEVICE_ARITH))


@pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52])
def test_ragged_batch_host_build_within_bounds(emul, kind):
    TF.check_ragged(emul, kind)


@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
@pytest.mark.parametrize("case", TF.REFIT_CASES[1:], ids=TF.case_id)
def test_refit_value_within_bound_at_returned_point(emul, case, batched):
    """(the host build has the columns only: the matrix-core shape runs through them here, with the column path's bound)"""
    TF.check_refit(emul, case, batched)


def test_jitter_set(emul):
    for be in (emul, StandIn()):
        TF.check_jitter(be, False)


@pytest.mark.parametrize("case", TF.NAN_CASES, ids=TF.case_id)
@pytest.mark.parametrize("what", ["weight", "ls", float("nan"), float("inf")], ids=["weight", "lengthscale", "x-nan", "x-inf"])
def test_non_finite_inputs_fail_alone(emul, case, what):
    be = emul if case.path == "col" else StandIn()
    if isinstance(what, str):
        TF.check_nan_start(be, case, what)
    else:
        TF.check_nan_point(be, case, what)


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_rejected(fault):
    be = StandIn(fault)
    with pytest.raises(AssertionError) as e:
        if fault == "no_jitter":
            TF.check_jitter(be, False)
        else:
            TF.check_mll(be, TF.FAULT_CASE)
    print(f"\n{fault}: {e.value}")


def test_zz_ratio_table():
    """Module-level summary (runs last): the largest error / bound and bound / scale per backend path, family and output."""
    lines = TF.report()
    assert lines, "no comparison was made"
    print("\n" + "\n".join(lines))
