"""The error bounds of tests/_posterior_bounds.py, checked without a device: they admit honest fp64 arithmetic in the kernels'
own formulation on every input set of tests/test_posterior_bounds_gpu.py (with a wide margin: the largest error / bound is in
profiles/posterior_bounds_notes.md), and they reject every planted fault below -- the kind of fault the old 1e-4 comparison
with the oracle let through."""
import numpy as np
import pytest

from tests import _posterior_bounds as B
from tests._posterior_bounds import CASES, KIND_RBF, OS, SENTINEL


# ---- plain numpy fp64 stand-ins, one per kernel, in the kernel's formulation ----------------------------------------------
def _k64(d2, kind, restore_nan):
    """os k and os dk/dd2 from a squared distance the way the kernels clamp it: RBF max(d2, 0), Matern max(d2, 1e-30), both with
    the bare v_max that drops a NaN (np.fmax); restore_nan: the `d2 - d2` of kernel_from_sqdist puts it back."""
    dd = np.fmax(d2, 0.0 if kind == KIND_RBF else 1e-30)
    k, dk = B._kernel(dd, kind)
    if restore_nan:
        k = k + (d2 - d2)
    return OS * k, OS * dk


def _columns64(P, il, kind, xq, grad, expanded):
    """fp64 right-hand-side columns against the points P.  expanded: |a|^2 + |q|^2 - 2 a.q (the explicit-inverse pass); else
    coordinate differences (the substitution kernel, the covariance's kernel term)."""
    a, q = P * il, np.atleast_2d(xq) * il
    if expanded:
        d2 = (a * a).sum(-1)[:, None] + (q * q).sum(-1)[None, :] - 2.0 * (a @ q.T)
    else:
        d2 = ((a[:, None, :] - q[None, :, :]) ** 2).sum(-1)
    k, dk = _k64(d2, kind, restore_nan=not expanded and not grad)
    if not grad:
        return k
    C = np.zeros((P.shape[0], 16))
    C[:, 0] = k[:, 0] + (0.0 if expanded else d2[:, 0] - d2[:, 0])
    for d in range(P.shape[1]):
        C[:, 1 + d] = 2.0 * dk[:, 0] * (q[0, d] - a[:, d]) * il[d]
    return C


def _subst64(L, W, n, N, Cn):
    """V = L^-1 C by row blocks against the inverted diagonal blocks W, as gp_posterior_kernel / gp_linv_kernel do."""
    NB = (N + 15) // 16
    Lp, Cp = np.zeros((NB * 16, NB * 16)), np.zeros((NB * 16, Cn.shape[1]))
    Lp[:n, :n], Cp[:n] = L[:n, :n], Cn
    V = np.zeros_like(Cp)
    for kb in range(NB):
        r = slice(16 * kb, 16 * kb + 16)
        V[r] = W[kb] @ (Cp[r] - Lp[r, :16 * kb] @ V[:16 * kb])
    return V[:N]


def standin(c, arr, t, fault=None):
    """The outputs of case c's kernel for task t in plain fp64 numpy; `fault` plants one of the faults of the tests below."""
    N, D, M = c.N, c.D, c.M
    n = B.counts(c, arr)[t]
    if c.kern.startswith("linvmat"):
        out = np.eye(N)
        out[:n, :n] = np.tril(_subst64(arr["L"][t], arr["Linv_diag"][t], n, N, np.eye(n))[:n])
        if fault == "linv_neighbour_block":
            out[16:32, 0:16] = standin(c, arr, t + 1)["Linv"][16:32, 0:16]
        if c.kern == "linvmat_lower":
            blk = np.arange(N) // 16
            out[blk[:, None] < blk[None, :]] = SENTINEL
        return dict(Linv=out)
    th = arr["theta"][t]
    l = th[:D].copy()
    if fault == "ls_prev":
        l[D - 1] = l[D - 2]
    il = 1.0 / l
    ym = 0.0 if arr["y_mean"] is None else arr["y_mean"][t]
    ys = 1.0 if arr["y_std"] is None else arr["y_std"][t]
    if fault == "n_round_up":
        n = min(N, 16 * ((n + 15) // 16))
    P, al = arr["X"][t, :n], arr["alpha"][t, :n]
    Xq = arr["Xq"][t] if c.per_task else arr["Xq"]
    grad, family_linv = c.kern == "grad", c.kern in ("linv", "linv_cov", "grad")
    if c.kern == "cov":
        V = arr["V"][t]
        kv = _columns64(Xq[:c.Ma], il, c.kind, Xq, False, False)
        return dict(cov=ys * ys * (kv - V[:, :c.Ma].T @ V))
    res = {k: [] for k in ("mu", "var", "V", "cov")}
    for xq in (Xq if grad else [Xq]):
        C = _columns64(P, il, c.kind, xq, grad, family_linv)
        if fault == "kstar_1e-7":
            i = int(np.argmax(np.abs(al)))
            C[i, int(np.argmax(C[i]))] *= 1.0 + 1e-7
        q = np.atleast_2d(xq) * il
        nq = (q * q).sum(-1)
        poison = (nq - nq) if not grad else np.full(16, nq[0] - nq[0])      # a non-finite query point: NaN in all its outputs
        value = np.ones(C.shape[1]) if not grad else np.eye(16)[0]
        mu = ys * (C.T @ al) + ym * value + poison
        if fault == "sign_flip":
            mu[D] = -mu[D]
        res["mu"].append(mu)
        if c.kern == "subst_mean":
            continue
        V = np.zeros((N, C.shape[1]))
        if family_linv:
            V[:n] = np.tril(arr["Linv"][t, :n, :n]) @ C
        else:
            V = _subst64(arr["L"][t], arr["Linv_diag"][t], n, N, C)
        res["V"].append(V)
        V2 = V * (V[:, :1] if grad else V)
        s = V2.sum(0)
        if fault == "drop_block":
            s[M // 2] -= V2[16:32, M // 2].sum()
        var = ys * ys * (OS - s) + poison
        if grad:
            var[1:] = (-1.0 if fault == "dvar_factor2" else -2.0) * ys * ys * s[1:] + poison[1:]
        if fault == "strip_col0":
            var[M - 1] = var[0]
        res["var"].append(var)
        if c.Ma and c.kern in ("linv_cov", "grad"):
            Xa = arr["Xa"] if grad else Xq[:c.Ma]
            kv = _columns64(Xa, il, c.kind, xq, grad, False)
            cov = ys * ys * (kv - arr["VA"][t, :n].T @ V[:n]) + poison
            if fault == "ma_round_down":
                cov[16 * (c.Ma // 16):] = SENTINEL
            res["cov"].append(cov)
    out = {}
    for name, parts in res.items():
        if parts:
            out[name] = parts[0] if not grad else (np.stack(parts, 0) if name in ("mu", "var") else np.concatenate(parts, 1))
    if grad:
        del out["V"]      # (the GRAD pass has no V output)
    if c.kern == "linv_cov":
        del out["V"]
    return out


_HOST = {}


def host_arrays(c):
    """The case's inputs with the host stand-in of the device fit, and the V / VA the covariance kernels are handed."""
    if c in _HOST:
        return _HOST[c]
    arr = B.make_inputs(c)
    arr.update(B.host_fit(c, arr))
    if c.kern == "cov":
        arr["V"] = np.stack([standin(c._replace(kern="subst"), arr, t)["V"] for t in range(c.T)])
    if c.Ma and c.kern in ("linv_cov", "grad"):
        lead = c._replace(kern="linv", M=c.Ma, nanq=False, per_task=False)
        xa = dict(arr, Xq=arr["Xa"] if c.kern == "grad" else arr["Xq"][:c.Ma])
        arr["VA"] = np.stack([standin(lead, xa, t)["V"] for t in range(c.T)])
    _HOST[c] = arr
    return arr


def find(kern, **kw):
    return next(c for c in CASES if c.kern == kern and all(getattr(c, k) == v for k, v in kw.items()))


@pytest.mark.parametrize("case", CASES, ids=B.case_id)
def test_bound_admits_fp64_arithmetic(case):
    """Honest fp64 in the kernel's formulation is inside the bound on every input set of the GPU file, and every bound is within
    the cap of 1e-8 of its quantity's scale."""
    arr = host_arrays(case)
    for t in range(case.T):
        B.check_task(case, arr, arr, t, standin(case, arr, t), v_nan=case.kern == "subst")


def _rejected(case, t, fault):
    arr = host_arrays(case)
    B.check_task(case, arr, arr, t, standin(case, arr, t))            # the unfaulted stand-in passes
    with pytest.raises(AssertionError) as e:
        B.check_task(case, arr, arr, t, standin(case, arr, t, fault))
    return str(e.value)


def test_rejects_a_dropped_row_block():
    """One row block's (rows 16 .. 31) contribution to one query's variance is dropped.
    linv-T3-N255-M33-D15-rbf-std-ragged0 task 0 var[16]: got 0.44124440180187446, reference 0.19964470471030582, error 2.416e-01 >
    bound 1.242e-11 (1 of 33 elements)."""
    assert " var[16]" in _rejected(find("linv", N=255), 0, "drop_block")


def test_rejects_n_rounded_up_to_the_block():
    """n_t = 254 treated as 256: the padding rows' points contribute to V (alpha is zero there: the mean does not notice).
    linv-T3-N255-M33-D15-rbf-std-ragged0 task 1 var[0]: got 0.2617195944490343, reference 0.4309621418176418, error 1.692e-01 >
    bound 9.430e-12 (33 of 33 elements)."""
    assert " var[0]" in _rejected(find("linv", N=255), 1, "n_round_up")


def test_rejects_the_previous_coordinates_lengthscale():
    """The last coordinate scaled with the lengthscale of the one before it.
    linv-T9-N129-M17-D5-rbf-std-ragged0 task 0 mu[0]: got -0.31566590440566356, reference -0.7568737313012165, error 4.412e-01 >
    bound 9.592e-11 (17 of 17 elements)."""
    assert " mu[0]" in _rejected(find("linv", N=129, T=9), 0, "ls_prev")


def test_rejects_column_0_in_the_last_lane_of_a_partial_strip():
    """The last query of a partial strip (query 16 of M = 17, the only live lane of strip 1) gets column 0's variance.
    linv-T9-N129-M17-D5-rbf-std-ragged0 task 0 var[16]: got 0.0002694177857159638, reference 0.00039719276666362623, error
    1.278e-04 > bound 2.846e-12 (1 of 17 elements)."""
    assert " var[16]" in _rejected(find("linv", N=129, T=9), 0, "strip_col0")


def test_rejects_ma_rounded_down_to_a_multiple_of_16():
    """Ma = 17 handled as 16: row 16 of cov is left unwritten and keeps the sentinel.
    linv_cov-T3-N255-M33-D15-rbf-Ma17-std-ragged1 task 0 cov[16, 0]: got -7.25e+77, reference 0.0026450920407449074, error
    7.250e+77 > bound 5.353e-12 (33 of 561 elements)."""
    assert " cov[16, 0]" in _rejected(find("linv_cov", N=255), 0, "ma_round_down")


def test_rejects_one_cross_kernel_entry_off_by_1e_7():
    """K*[i, q] (1 + 1e-7) at the training point i with the largest |alpha| and the query that sees it best.
    linv-T9-N129-M17-D5-rbf-std-ragged0 task 0 mu[1]: got -2.1417345651892363, reference -2.1417515702447356, error 1.701e-05 >
    bound 9.866e-11 (1 of 17 elements)."""
    assert " mu[1]" in _rejected(find("linv", N=129, T=9), 0, "kstar_1e-7")


def test_rejects_a_flipped_derivative_sign():
    """d mu / d x_{D-1} with the wrong sign (GRAD strips side by side: element 4 is column 1 + 3 of query 0).
    grad-T3-N144-M3-D4-rbf-Ma17-std-ragged0 task 0 mu[4]: got -0.6785400843006466, reference 0.6785400843004383, error 1.357e+00 >
    bound 7.098e-11 (3 of 48 elements)."""
    assert " mu[4]" in _rejected(find("grad", N=144, T=3), 0, "sign_flip")


def test_rejects_d_var_without_its_factor_2():
    """d var = -ys^2 V_0 . V_d.
    grad-T3-N144-M3-D4-rbf-Ma17-std-ragged0 task 0 var[1]: got 0.0007632126107600234, reference 0.0015264252215140767, error
    7.632e-04 > bound 1.612e-11 (12 of 48 elements)."""
    assert " var[1]" in _rejected(find("grad", N=144, T=3), 0, "dvar_factor2")


def test_rejects_a_block_of_the_neighbouring_tasks_inverse():
    """Block (1, 0) of task 0's Linv taken from task 1.
    linvmat-T3-N129-M0-D5-matern-ragged0 task 0 Linv[16, 0]: got -0.07045681512801291, reference -0.7458202485802632, error
    6.754e-01 > bound 3.498e-13 (256 of 16641 elements)."""
    assert " Linv[16, 0]" in _rejected(find("linvmat", N=129), 0, "linv_neighbour_block")
