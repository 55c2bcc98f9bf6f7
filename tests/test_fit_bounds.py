"""The error bounds of tests/_fit_bounds.py, checked without a device: they admit honest fp64 arithmetic in the kernels' own
formulation (expanded distances, a blocked right-looking Cholesky with 16 x 16 diagonal-block inverses, the strip substitutions,
the tile-partial gradient sum) on every input set of tests/test_fit_bounds_gpu.py, every cap holds on every set, and every planted
fault below is rejected by the assertion it names -- faults of the size the blanket tolerances of tests/test_fit_gpu.py and
tests/test_mll_grad_gpu.py let through."""
import numpy as np
import pytest

from tests import _fit_bounds as B
from tests._fit_bounds import FAMILY, KIND_MATERN52, KIND_RBF, U, _kernel


def _inv_lower64(Lkk):
    """The inverse of a 16 x 16 lower-triangular block by forward substitution against the identity, fp64 (the kernels apply the
    factorisation's row operations to a second accumulator: the same operations per entry in another order)."""
    X = np.zeros((16, 16))
    for i in range(16):
        X[i] = (np.eye(16)[i] - Lkk[i, :i] @ X[:i]) / Lkk[i, i]
    return X


class Host:
    """The backend interface of tests/_fit_bounds.py in plain fp64 numpy; `fault` plants one of the faults of the tests below."""
    name = "host"

    def __init__(self, fault=None):
        self.fault = fault
        if fault:
            self.name = "host-" + fault

    # ---- fit family
    def _factor(self, A, y, n, N):
        """Blocked right-looking Cholesky of the identity-padded A with inverted diagonal blocks, v = L^-1 y, alpha = L^-T v."""
        NB = (N + 15) // 16
        NP = NB * 16
        A = A.copy()
        L, W = np.zeros((NP, NP)), np.zeros((NB, 16, 16))
        sl = [slice(16 * b, 16 * b + 16) for b in range(NB)]
        for k in range(NB):
            L[sl[k], sl[k]] = np.linalg.cholesky(A[sl[k], sl[k]])
            W[k] = _inv_lower64(L[sl[k], sl[k]])
            for i in range(k + 1, NB):
                L[sl[i], sl[k]] = A[sl[i], sl[k]] @ W[k].T
            for j in range(k + 1, NB):
                for i in range(j, NB):
                    if self.fault == "skip_tile" and (k, i, j) == (0, NB - 1, NB - 1):
                        continue
                    A[sl[i], sl[j]] -= L[sl[i], sl[k]] @ L[sl[j], sl[k]].T
        yp = np.zeros(NP)
        yp[:n] = y[:n]
        v, al = np.zeros(NP), np.zeros(NP)
        for k in range(NB):
            v[sl[k]] = W[k] @ (yp[sl[k]] - L[sl[k], :16 * k] @ v[:16 * k])
        for k in range(NB - 1, -1, -1):
            al[sl[k]] = W[k].T @ (v[sl[k]] - L[16 * k + 16:, sl[k]].T @ al[16 * k + 16:])
        q, ld = float(v @ v), float(2.0 * np.log(np.diagonal(L)[:n]).sum()) if n else 0.0
        mll = -0.5 * (q + ld + n * 1.8378770664093454836) / n if n else 0.0
        return L, W, al, q, ld, mll

    def _pack(self, T, N, res, ns, store_L, want_alpha, zero_upper, fill):
        NB = (N + 15) // 16
        out = dict(L=np.full((T, N, N), fill) if store_L else None, alpha=np.zeros((T, N)) if want_alpha else None, quad=np.zeros(T), logdet=np.zeros(T),
                   mll=np.zeros(T), info=np.zeros(T, dtype=np.int32), jitter=np.zeros(T), Linv_diag=np.zeros((T, NB, 16, 16)), fill=fill)
        for t, (r, n) in enumerate(zip(res, ns)):
            if r is None:
                out["info"][t] = 1
                continue
            L, W, al, q, ld, mll = r
            if self.fault == "perturb_L_8u" and t == 0:
                L = L.copy()
                L[n - 1, 0] *= 1 + 8 * U
            if store_L:
                low = np.tril_indices(n)
                out["L"][t][low] = L[:n, :n][low]
                if zero_upper:
                    out["L"][t][:n, :n][np.triu_indices(n, 1)] = 0.0
            if want_alpha:
                out["alpha"][t, :n] = al[:n]
                if self.fault == "alpha_past_n" and n < N:
                    out["alpha"][t, n] = 1e-300
            out["quad"][t], out["logdet"][t], out["mll"][t] = q, ld, mll
            out["Linv_diag"][t] = W
            if self.fault == "w_prev_block" and n > 16:
                out["Linv_diag"][t, 1] = W[0]
        return out

    def fit(self, c, inp, store_L=True, want_alpha=True, zero_upper=True):
        T, N, D, kind = c.T, c.N, c.D, c.kind
        NP = (N + 15) // 16 * 16
        ns = B.counts(c, inp)
        res = []
        for t, n in enumerate(ns):
            th = inp["theta"][t]
            xs = np.zeros((NP, D))
            xs[:n] = inp["X"][t, :n] * (1.4142135623730951 / th[:D])
            h = -0.5 * (xs * xs).sum(-1)
            if not np.isfinite(h).all():      # the poisoned diagonal: every attempt fails
                res.append(None)
                continue
            d2 = -(xs @ xs.T + h[:, None] + h[None, :])
            i = np.arange(NP)
            d2[i, i] = 0.0
            K = th[D] * _kernel(np.fmax(d2, 0.0 if kind == KIND_RBF else 1e-30), kind)[0]
            add = np.full(NP, th[D + 1] + 0.0 + (inp["jitter_in"][t] if inp["jitter_in"] is not None else 0.0))
            if self.fault == "jitter_first_256" and inp["jitter_in"] is not None:
                add[256:] = th[D + 1]
            K[i, i] += add
            K[n:, :], K[:, n:] = 0.0, 0.0
            K[i[n:], i[n:]] = 1.0
            res.append(self._factor(K, inp["y"][t], n, N))
        fill = (B.SENTINEL if N <= 256 else 0.0) if zero_upper else np.nan
        return self._pack(T, N, res, ns, store_L, want_alpha, zero_upper, fill)

    fit_for_grad = fit

    def potrf(self, c, inp):
        N = c.N
        NP = (N + 15) // 16 * 16
        ns = B.counts(c, inp)
        res = []
        for t, n in enumerate(ns):
            A = np.eye(NP)
            A[:n, :n] = np.tril(inp["A"][t, :n, :n]) + np.tril(inp["A"][t, :n, :n], -1).T
            res.append(self._factor(A, inp["y"][t], n, N))
        return self._pack(c.T, N, res, ns, True, True, True, B.SENTINEL)

    def kmat(self, X, X2, theta, kind, add_noise):
        T, N1, D = X.shape
        out = []
        for t in range(T):
            x2 = X[t] if X2 is None else (X2 if X2.ndim == 2 else X2[t])
            df = (X[t][:, None, :] - x2[None, :, :]) / theta[t, :D]
            K = theta[t, D] * _kernel(np.fmax((df * df).sum(-1), 0.0 if kind == KIND_RBF else 1e-30), kind)[0]
            if add_noise:
                K[np.arange(N1), np.arange(N1)] += theta[t, D + 1]
            out.append(K)
        return np.stack(out)

    # ---- gradient
    def grad(self, c, inp, fit, form):
        if form == "default":
            form = "single" if "fused" in B.grad_instance(c) else "two"
        T, N, D, kind = c.T, c.N, c.D, c.kind
        NB = (N + 15) // 16
        NP = NB * 16
        sl = [slice(16 * b, 16 * b + 16) for b in range(NB)]
        hs = 1.0 if kind == KIND_RBF else 5.0 / 3.0
        out = np.zeros((T, D + 2))
        for t, n in enumerate(B.counts(c, inp)):
            if n == 0:
                continue
            th = inp["theta"][t]
            il, os_ = 1.0 / th[:D], th[D]
            Lp = np.eye(NP)
            Lp[:n, :n] = np.tril(fit["L"][t, :n, :n])
            W = fit["Linv_diag"][t]
            alp, xs = np.zeros(NP), np.zeros((NP, D))
            alp[:n], xs[:n] = fit["alpha"][t, :n], inp["X"][t, :n] * il
            nrm = (xs * xs).sum(-1)
            ok = np.arange(NP) < n
            V, Z = np.zeros((NP, NP)), np.zeros((NP, NP))      # strips of L^-1, of K^-1 (blocks at or below the strip's first)
            for cs in range(NB):
                for kb in range(cs, NB):
                    rhs = np.eye(16) if kb == cs else np.zeros((16, 16))
                    V[sl[kb], sl[cs]] = W[kb] @ (rhs - Lp[sl[kb], 16 * cs:16 * kb] @ V[16 * cs:16 * kb, sl[cs]])
                if form == "single":
                    for kb in range(NB - 1, cs - 1, -1):
                        Z[sl[kb], sl[cs]] = W[kb].T @ (V[sl[kb], sl[cs]] - Lp[16 * kb + 16:, sl[kb]].T @ Z[16 * kb + 16:, sl[cs]])
                    if self.fault == "strip_forward_only" and cs == 0:
                        Z[:, sl[cs]] = V[:, sl[cs]]
            Kinv = Z if form == "single" else V.T @ V
            tot, sd = np.zeros(D + 2), np.zeros(D)
            for tc in range(NB):
                Q, Q2, CS = np.zeros((D, 16)), np.zeros((D, 16)), np.zeros(16)
                for ta in range(tc, NB):
                    wgt = 1.0 if ta == tc or (self.fault == "tile_weight_1" and (ta, tc) == (1, 0)) else 2.0
                    Gt = wgt * (np.outer(alp[sl[ta]], alp[sl[tc]]) - Kinv[sl[ta], sl[tc]]) * (ok[sl[ta]][:, None] & ok[sl[tc]][None, :])
                    if form == "single":
                        d2 = np.fmax(-2.0 * (xs[sl[ta]] @ xs[sl[tc]].T) + nrm[sl[ta]][:, None] + nrm[sl[tc]][None, :], 0.0)
                    else:
                        d2 = ((xs[sl[ta]][:, None, :] - xs[sl[tc]][None, :, :]) ** 2).sum(-1)
                    if ta == tc:
                        d2[np.arange(16), np.arange(16)] = 0.0
                    k, dk = _kernel(np.fmax(d2, 0.0 if kind == KIND_RBF else 1e-30), kind)
                    GH = (Gt * (os_ * hs)) * (-2.0 * dk / hs)
                    tot[D] += (Gt * k).sum()
                    if ta == tc:
                        tot[D + 1] += np.trace(Gt)
                    if form == "single":
                        Q += xs[sl[ta]].T @ GH
                        Q2 += (xs[sl[ta]] ** 2).T @ GH
                        CS += GH.sum(0)
                    else:
                        for d in range(D):
                            df = xs[sl[ta], d][:, None] - xs[sl[tc], d][None, :]
                            sd[d] += (GH * (df * df)).sum()
                if form == "single":
                    xc = xs[sl[tc]].T
                    sd += (Q2 - 2.0 * xc * Q + xc * xc * CS).sum(-1)
            tot[:D] = sd * il
            if self.fault == "l2_for_l3":
                tot[0] = sd[0]
            out[t] = tot / (2.0 * n)
        return out


HOST = Host()
_FITS = {}


def _host_fit(fc):
    if fc not in _FITS:
        _FITS[fc] = HOST.fit(fc, B.fit_inputs(fc))
    return _FITS[fc]


# ---- the bounds admit honest fp64 arithmetic, and the caps hold, on every input set of the GPU file ----------------------------------
@pytest.mark.parametrize("case", B.FIT_CASES, ids=B.fit_id)
def test_fit_bounds_admit_fp64_arithmetic(case):
    B.check_fit(HOST, case)


@pytest.mark.parametrize("case", B.FLAG_CASES, ids=B.fit_id)
def test_fit_flags(case):
    B.check_flags(HOST, case)


@pytest.mark.parametrize("case", B.POTRF_CASES, ids=B.potrf_id)
def test_potrf_bounds_admit_fp64_arithmetic(case):
    B.check_potrf(HOST, case)


@pytest.mark.parametrize("case", B.KMAT_CASES, ids=B.kmat_id)
def test_kernel_matrix_bound_admits_fp64_arithmetic(case):
    B.check_kmat(HOST, case)


@pytest.mark.parametrize("case", B.GRAD_CASES, ids=B.grad_id)
def test_gradient_bounds_admit_fp64_arithmetic(case):
    B.check_grad(HOST, case, fit=_host_fit(B.grad_fit_case(case)))


def test_every_dispatchable_instance_is_named_in_both_families():
    """The case ids name the instance the dispatch of csrc/scaml_host.cpp sends each case to: all five fused-fit variants, both blocked
    paths, and for the gradient every (size class, kind, staging) of the single-launch kernel, the two-workgroup split and the
    two-launch kernel -- each in both families."""
    for fam in ("rbf", "matern"):
        fit = {B.fit_instance(c) for c in B.FIT_CASES if FAMILY[c.kind] == fam}
        assert fit == {"fit_fused[nb2,wu1]", "fit_fused[nb4,wu3]", "fit_fused[nb8,wu3]", "fit_fused[nb8,wu7]", "fit_fused[nb16,wu7]", "fit_blocked[launches]",
                       "fit_blocked[coop]"}
        grad = {B.grad_instance(c) for c in B.GRAD_CASES if FAMILY[c.kind] == fam and c.path != "default"}
        want = {f"mllgrad_fused[{sc}][{fam}][{dma}]" for sc in range(4) for dma in (0, 1)} | {f"mllgrad_split[1][{fam}][0]", f"mllgrad[{fam}]"}
        assert grad == want, grad ^ want
        assert {B.grad_instance(c) for c in B.GRAD_CASES if FAMILY[c.kind] == fam and c.path == "default"} == \
            {f"default->mllgrad_fused[1][{fam}][1]", f"default->mllgrad[{fam}]"}


# ---- planted faults: each is rejected, by the named assertion (never by the cap: "ill-chosen" is not in the message) ---------------------
def _find(cases, **kw):
    return next(c for c in cases if all(getattr(c, k) == v for k, v in kw.items()))


def _rejected(check, fault, *args, **kw):
    with pytest.raises(AssertionError) as e:
        check(Host(fault), *args, **kw)
    msg = str(e.value)
    assert "ill-chosen" not in msg, msg
    return msg


def test_rejects_a_skipped_trailing_update_tile():
    """Panel 0's update of the last diagonal tile (2, 2) is skipped (the matrix stays positive definite: the factorisation goes through):
    the first failing element of the packed lower triangle is (32, 32)."""
    msg = _rejected(B.check_fit, "skip_tile", _find(B.FIT_CASES, N=33, D=9, kind=KIND_RBF))
    assert f" L L^T[{32 * 33 // 2 + 32}]" in msg and "task 0" in msg


def test_rejects_linv_diag_of_the_previous_block():
    msg = _rejected(B.check_fit, "w_prev_block", _find(B.FIT_CASES, N=33, D=9, kind=KIND_MATERN52))
    assert " Linv_diag[1, " in msg


def test_rejects_a_nonzero_alpha_entry_past_n():
    """alpha[n_t] = 1e-300 on the first ragged task."""
    msg = _rejected(B.check_fit, "alpha_past_n", _find(B.FIT_CASES, N=65, T=9, kind=KIND_RBF))
    assert "alpha is not exactly zero at or past n_t" in msg


def test_rejects_jitter_on_the_first_256_rows_only():
    """jitter_in = 1e-4 reaches rows 0 .. 255 of a 272-point task only: the first failing element is the diagonal entry (256, 256)."""
    c = _find(B.FIT_CASES, N=272, path=1, jit=1e-4, kind=KIND_MATERN52)
    msg = _rejected(B.check_fit, "jitter_first_256", c)
    assert f" L L^T[{256 * 257 // 2 + 256}]" in msg and "task 0" in msg


def test_rejects_8u_on_one_entry_of_the_last_block_row():
    """L[n - 1, 0] (1 + 8 u).  The factor bound's own coefficient is g_{n+4} (+ E_K for a fit): it is below 8 u only for n <= 3 of a given
    matrix, so the fault is planted where the bound is sharpest -- the POTRF of two points 0.02 apart (L_10^2 >> L_11^2): element
    (1, 0) of L L^T moves by 8 u |L_10 L_00| against g_6 |L_10 L_00|, element (1, 1) by 16 u L_10^2 against g_6 (L_10^2 + L_11^2)."""
    c = B._f(T=1, N=2, D=1, kind=KIND_RBF)
    inp = B.potrf_inputs(c)
    inp["X"][0, :, 0] = (0.40, 0.42)
    inp["theta"][0] = (0.2, 1.3, 1e-2)
    inp["A"][0] = Host().kmat(inp["X"], None, inp["theta"], KIND_RBF, True)[0]
    B.check_potrf(Host(), c, inp)
    msg = _rejected(B.check_potrf, "perturb_L_8u", c, inp)
    assert " L L^T[1]" in msg and "(2 of 3 elements)" in msg


def _grad_rejected(fault, **kw):
    c = _find(B.GRAD_CASES, **kw)
    return _rejected(B.check_grad, fault, c, fit=_host_fit(B.grad_fit_case(c)))


def test_rejects_an_off_diagonal_gradient_tile_weighted_once():
    for path, N in (("single", 33), ("two", 48)):
        assert " g[" in _grad_rejected("tile_weight_1", path=path, N=N, kind=KIND_RBF)


def test_rejects_l_squared_for_l_cubed():
    """d K / d l_0 without its last division by l_0: entry 0 alone."""
    for path, N in (("single", 64), ("two", 48)):
        msg = _grad_rejected("l2_for_l3", path=path, N=N, kind=KIND_MATERN52)
        assert " g[0]" in msg and "(1 of " in msg


def test_rejects_a_strip_of_the_inverse_left_at_its_forward_value():
    """Strip 0 of K^-1 keeps V = L^-1 E_0 (the backward substitution is skipped)."""
    assert " g[" in _grad_rejected("strip_forward_only", path="single", N=128, kind=KIND_RBF)


def test_zz_ratio_table():
    """The largest error / bound and bound / scale the fp64 stand-ins reached (run after the tests above)."""
    lines = B.report()
    assert lines
    print("\n".join(lines))
