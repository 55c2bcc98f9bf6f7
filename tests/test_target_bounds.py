"""The error bounds of tests/_target_bounds.py, checked without a device: they admit honest fp64 arithmetic in the kernels' own
formulation (the 8-wide fma chains of the weighted sum and the finish, block substitution against the inverted diagonal blocks, one
lane per training point and a tree sum in the target gradient) on every input set of tests/test_target_bounds_gpu.py, and they
reject every planted fault below -- each of them invisible to the 1e-4 comparison with the oracle.  The measured ratios are in
profiles/target_bounds_notes.md."""
import numpy as np
import pytest

from tests import _posterior_bounds as P
from tests import _target_bounds as B
from tests import test_posterior_bounds as SP
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF, SENTINEL


def _chain8(terms, acc):
    """acc + sum of terms (k, ...) the way the kernels' unrolled loops add them: in order, eight at a time."""
    for x in terms:
        acc = acc + x
    return acc


def _tree(x):
    """Sum over axis 0 (a power of two long) by halving."""
    while x.shape[0] > 1:
        x = x[0::2] + x[1::2]
    return x[0]


class Numpy:
    """Plain numpy fp64 stand-ins of the kernels, behind the backend interface of tests/_target_bounds.py; `fault` plants one of the
    faults of the tests below."""
    name = "numpy"

    def __init__(self, fault=None):
        self.fault = fault

    # ---- scaml_weighted_task_sum_kernel: wave q sums the q-th quarter of the tasks, the four partial sums meet in a fixed order
    def wsum(self, inp, w, active, power):
        T, length = inp.shape
        chunk = (T + 3) // 4
        part = np.zeros((4, length))
        for q in range(4):
            for t in range(q * chunk, min(q * chunk + chunk, T)):
                if self.fault == "mask_times_zero":
                    c = (w[t] if power == 1 else w[t] * w[t]) * (1.0 if active is None or active[t] else 0.0)
                    part[q] = part[q] + c * inp[t]
                    continue
                if active is not None and not active[t]:
                    continue
                c = w[t] if power == 1 or (self.fault == "weight_not_squared" and t == T - 1) else w[t] * w[t]
                part[q] = part[q] + c * inp[t]
        return (part[0] + part[1]) + (part[2] + part[3])

    def prior_reduce(self, mu, cov, w, active):
        T = w.shape[0]
        return (None if mu is None else self.wsum(mu, w, active, 1),
                None if cov is None else self.wsum(cov.reshape(T, -1), w, active, 2).reshape(cov.shape[1:]))

    # ---- scaml_target_assemble_kernel: one element per thread
    def assemble(self, a):
        n, M, D, kind = a["n"], a["M"], a["D"], a["kind"]
        th, s, m = a["theta"], a["s"], a["m"]
        s2 = s * s
        with np.errstate(invalid="ignore"):
            df = (a["Xall"][:n, None, :] - a["Xall"][None, :, :]) / th[:D]
            d2 = (df * df).sum(-1)
            k = SP._k64(d2, kind, restore_nan=True)[0] * (th[D] / P.OS)
        v = a["cov_s"] / (s if self.fault == "cov_over_s" else s2) + k
        Knn = v[:, :n] + th[D + 1] * (np.ones((n, n)) if self.fault == "noise_everywhere" else np.eye(n))
        return dict(Knn=Knn, resid=a["y"] - (a["mean_s"][:n] - m) / s, Knq=v[:, n:], mean_q=(a["mean_s"][n:] - m) / s,
                    var_q=a["var_s"][n:] / s2 + th[D])

    # ---- the POTRF: LAPACK's factor, the inverted diagonal blocks, alpha by the solve stand-in
    def potrf(self, Knn, resid):
        n = Knn.shape[0]
        L = np.linalg.cholesky(Knn)
        NB = (n + 15) // 16
        Lp = np.eye(NB * 16)
        Lp[:n, :n] = L
        W = np.stack([np.linalg.inv(Lp[16 * b:16 * b + 16, 16 * b:16 * b + 16]) for b in range(NB)])
        alpha = self.solve(L[None], W[None], resid[None, :, None], None, False)[0, :, 0]
        return dict(L=L, W=W, alpha=alpha, info=0, jitter=0.0)

    # ---- gp_cho_solve_kernel: Y_kb = W_kb (B_kb - sum_{j<kb} L_kb,j Y_j), X_kb = W_kb^T (Y_kb - sum_{j>kb} L_j,kb^T X_j)
    def solve(self, L, W, Bs, n_points, lt):
        T, N, R = Bs.shape
        NB = (N + 15) // 16
        out = np.zeros((T, N, R))
        for t in range(T):
            n = N if n_points is None else int(n_points[t])
            Lp, Y = np.zeros((NB * 16, NB * 16)), np.zeros((NB * 16, R))
            Lp[:n, :n] = np.tril(L[t, :n, :n])
            Y[:n] = Bs[t, :n]
            if self.fault == "strip_col0" and R % 16:
                Y[:, R - 1] = Y[:, 0]
            if not lt:
                for kb in range(NB):
                    r = slice(16 * kb, 16 * kb + 16)
                    Y[r] = W[t, kb] @ (Y[r] - Lp[r, :16 * kb] @ Y[:16 * kb])
            X = np.zeros_like(Y)
            for kb in range(NB - 1, -1, -1):
                r = slice(16 * kb, 16 * kb + 16)
                X[r] = W[t, kb].T @ (Y[r] - Lp[16 * kb + 16:, r].T @ X[16 * kb + 16:])
                if self.fault == "bwd_block_from_fwd" and kb == 0:
                    X[r] = Y[r]
            out[t, :n] = X[:n]
        return out

    def fit(self, fc, inp):
        return P.host_fit(fc, inp)

    # ---- scaml_target_finish_kernel: eight rows at a time, one fma chain per query
    def finish(self, a, info):
        n, M = a["n"], a["M"]
        if info is not None and info > 0:
            return np.full(M, np.nan), np.full(M, np.nan)
        rows = 8 * ((n + 7) // 8) if self.fault == "n_round_up_8" else n
        pad = lambda x: np.concatenate([x[:n], np.full((rows - n, *x.shape[1:]), 0.37)])   # noqa: E731  (what lies behind the arrays)
        Knq, Z, al = pad(a["Knq"]), pad(a["Z"]), pad(a["alpha"])
        acc = _chain8(Knq * al[:, None], a["mean_q"].copy())
        v = _chain8(-Knq * Z, a["var_q"].copy())
        return a["s"] * acc + a["m"], a["s"] * a["s"] * (v + a["noise_add"])

    # ---- scaml_target_grad_kernel: a lane per training point (a = lane, lane + 64, ...), the slope once per (a, q), a tree sum
    def tgrad(self, a, info):
        n, Mq, D, kind = a["n"], a["Mq"], a["D"], a["kind"]
        if D > 15:
            return B.E_TOOLARGE, np.full((Mq, 15), SENTINEL), np.full((Mq, 15), SENTINEL)
        if info is not None and info > 0:
            return 0, np.full((Mq, D), np.nan), np.full((Mq, D), np.nan)
        th, s = a["theta"], a["s"]
        il, inv_s2 = 1.0 / th[:D], 1.0 / (s * s)
        mu_g, var_g = a["mu_g"].reshape(Mq, 16)[:, 1:1 + D], a["var_g"].reshape(Mq, 16)[:, 1:1 + D]
        rounds = (n + 63) // 64
        with np.errstate(invalid="ignore"):
            df = (a["Xq"][None, :, :] - a["Xt"][:n, None, :]) * il                     # (n, Mq, D)
            d2 = (df * df).sum(-1)
            slope_kind = (KIND_RBF + KIND_MATERN52 - kind) if self.fault == "wrong_family_slope" else kind
            dk = SP._k64(d2, slope_kind, restore_nan=False)[1] * (th[D] / P.OS)
            if self.fault == "k_1e-7":
                dk[int(np.argmax(np.abs(a["alpha"][:n])))] *= 1.0 + 1e-7
            dkn = a["cov_g"][:n].reshape(n, Mq, 16)[:, :, 1:1 + D] * inv_s2 + 2.0 * dk[:, :, None] * (df * il)
            lanes = np.zeros((rounds * 64, Mq, D, 2))
            lanes[:n, ..., 0], lanes[:n, ..., 1] = a["alpha"][:n, None, None] * dkn, a["Z"][:n, :, None] * dkn
            tot = _tree(_chain8(lanes.reshape(rounds, 64, Mq, D, 2), np.zeros((64, Mq, D, 2)))) if n else np.zeros((Mq, D, 2))
            bad = (a["Xq"] - a["Xq"]).sum(-1)[:, None]      # 0, or NaN for a non-finite query: every entry of it
            dmu = np.where(bad == 0.0, mu_g + s * tot[..., 0], np.nan)
            dvar = np.where(bad == 0.0, var_g - (1.0 if self.fault == "dvar_factor2" else 2.0) * s * s * tot[..., 1], np.nan)
        return 0, dmu, dvar

    # ---- the source passes of the chain: the stand-ins of tests/test_posterior_bounds.py on the host stand-in of the fit
    def source_passes(self, val, inp, grad, ginp):
        arr = dict(inp)
        arr.update(P.host_fit(val, inp))
        lead = val._replace(kern="linv", M=val.Ma)
        arr["VA"] = np.stack([SP.standin(lead, dict(arr, Xq=inp["Xq"][:val.Ma]), t)["V"] for t in range(val.T)])
        garr = dict(arr, Xq=ginp["Xq"], Xa=ginp["Xa"])
        stack = lambda c, x: {k: np.stack([SP.standin(c, x, t)[k] for t in range(c.T)]) for k in ("mu", "var", "cov")}   # noqa: E731
        return dict(arr=arr, value=stack(val, arr), grad=stack(grad, garr))


CLEAN = Numpy()


# ---- honest fp64 is inside every bound, every bound inside the cap -------------------------------------------------------------
@pytest.mark.parametrize("T", B.WSUM_T)
def test_weighted_sum_standin_within_bound(T):
    B.check_wsum(CLEAN, T)


@pytest.mark.parametrize("case", B.ASSEMBLE_CASES, ids=B.assemble_id)
def test_assemble_potrf_solve_standins_within_bound(case):
    B.check_assemble(CLEAN, case)


@pytest.mark.parametrize("case", B.SOLVE_CASES, ids=B.solve_id)
def test_solve_standin_within_bound(case):
    B.check_solve(CLEAN, case)


@pytest.mark.parametrize("shape", B.FINISH_SHAPES, ids=lambda s: f"n{s[0]}-M{s[1]}")
def test_finish_standin_within_bound(shape):
    B.check_finish(CLEAN, *shape)


@pytest.mark.parametrize("case", B.TGRAD_CASES, ids=B.tgrad_id)
def test_target_gradient_standin_within_bound(case):
    B.check_tgrad(CLEAN, case)


def test_target_gradient_standin_refuses_d_16():
    B.check_tgrad_toolarge(CLEAN)


@pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])
def test_chain_standins_within_bound(kind):
    B.check_chain(CLEAN, kind)


def test_print_the_ratio_table():
    """(after the tests above: the table of the stand-ins as profiles/target_bounds_notes.md records it -- pytest -s shows it)"""
    print()
    for line in B.report():
        print("  " + line)


# ---- every planted fault is rejected, on a named element ---------------------------------------------------------------------
def _rejected(check, fault, *args):
    check(CLEAN, *args)
    with pytest.raises(AssertionError) as e:
        check(Numpy(fault), *args)
    print(f"\n  [{fault}] {e.value}")
    return str(e.value)


def test_rejects_a_weight_not_squared_at_power_2():
    """The last task's coefficient is w_t instead of w_t^2.
    wsum-T33-len1-p2-all out_p2[0]: got 15.33412142209869, reference 14.95060583010295, error 3.835e-01 > bound 1.966e-13 (1 of 1
    elements)."""
    assert "-p2-all out_p2[0]" in _rejected(B.check_wsum, "weight_not_squared", 1)
    assert "-p2-all out_p2[0]" in _rejected(B.check_wsum, "weight_not_squared", 33)


def test_rejects_a_masked_task_multiplied_by_zero():
    """0 * NaN: the masked task's NaN values leak into every element.
    wsum-T3-len1-p1-mask out_p1[0]: got nan, reference 0.009710344937025477, error nan > bound 1.458e-17 (1 of 1 elements)."""
    assert "-p1-mask out_p1[0]: got nan" in _rejected(B.check_wsum, "mask_times_zero", 3)


def test_rejects_noise_added_off_the_diagonal():
    """The noise 1e-2 on every entry of Knn.
    assemble-n16-M17-D6-rbf Knn[0, 1]: got 1.7100000000000002, reference 1.7000000000000002, error 1.000e-02 > bound 8.993e-16 (240 of
    256 elements)."""
    assert " Knn[0, 1]" in _rejected(B.check_assemble, "noise_everywhere", (16, 17, 6, KIND_RBF, False), False)


def test_rejects_cov_s_divided_by_s():
    """cov_s / s instead of cov_s / s^2 (s = 1.9): every entry of Knn and Knq.
    assemble-n16-M17-D6-matern Knn[0, 0]: got 2.07, reference 1.71, error 3.600e-01 > bound 1.089e-15 (256 of 256 elements)."""
    assert " Knn[0, 0]" in _rejected(B.check_assemble, "cov_over_s", (16, 17, 6, KIND_MATERN52, False), False)


def test_rejects_a_backward_block_taken_from_the_forward_result():
    """Rows 0 .. 15 of X (the last block of the backward substitution) are those of Y = L^-1 B.
    solve-cho-T1-N144-R16-D5-matern task 0 X[0, 0]: got 0.06292461073049993, reference -0.8619824402216609, error 9.249e-01 > bound
    1.086e-11 (256 of 2304 elements)."""
    assert " X[0, 0]" in _rejected(B.check_solve, "bwd_block_from_fwd", B.SOLVE_CASES[2])


def test_rejects_column_0_in_the_last_partial_strip():
    """The last right-hand side (column 16 of R = 17, the only live lane of strip 1) is read from column 0.
    solve-cho-T9-N129-R17-D5-matern-ragged0 task 0 X[0, 16]: got -4.29774403967808, reference 3.3605171572820396, error 7.658e+00 > bound
    4.636e-11 (129 of 2193 elements)."""
    assert " X[0, 16]" in _rejected(B.check_solve, "strip_col0", B.SOLVE_CASES[0])


def test_rejects_n_rounded_up_to_8_in_the_finish_loop():
    """n = 7 summed as 8 rows, n = 9 as 16: what lies behind Knq / Z / alpha enters every query.
    finish-n7-M127-rbf-noise0.0-infoNone mu[0]: got -1.995307048414367, reference -2.255417048414368, error 2.601e-01 > bound 6.298e-14
    (127 of 127 elements)."""
    assert " mu[0]" in _rejected(B.check_finish, "n_round_up_8", 7, 127)
    assert " mu[0]" in _rejected(B.check_finish, "n_round_up_8", 9, 129)


def test_rejects_d_var_without_its_factor_2():
    """tgrad-n65-Mq3-D6-rbf dvar[0, 0]: got 2.0412877384245744, reference 3.835470744358992, error 1.794e+00 > bound 4.731e-13 (18 of 18
    elements)."""
    assert " dvar[0, 0]" in _rejected(B.check_tgrad, "dvar_factor2", (65, 3, 6, KIND_RBF))


def test_rejects_the_slope_of_the_wrong_family():
    """tgrad-n65-Mq3-D6-matern dmu[0, 0]: got -19.984862238231766, reference -18.25029493396854, error 1.735e+00 > bound 1.391e-12 (18 of 18
    elements)."""
    assert " dmu[0, 0]" in _rejected(B.check_tgrad, "wrong_family_slope", (65, 3, 6, KIND_MATERN52))
    assert " dmu[" in _rejected(B.check_tgrad, "wrong_family_slope", (65, 3, 6, KIND_RBF))


def test_rejects_one_kernel_slope_off_by_1e_7():
    """os dk (1 + 1e-7) at the training point with the largest |alpha|, n = 96: one term of 96, seven digits down.
    tgrad-n96-Mq3-D15-rbf dmu[0, 0]: got 7.939853230932911, reference 7.939853278021995, error 4.709e-08 > bound 1.499e-12 (45 of 45
    elements)."""
    assert " dmu[" in _rejected(B.check_tgrad, "k_1e-7", (96, 3, 15, KIND_RBF))
    assert " dmu[" in _rejected(B.check_tgrad, "k_1e-7", (96, 3, 15, KIND_MATERN52))


def test_the_chain_rejects_a_fault_in_any_stage():
    """The same faults planted in the pipeline: the stage that carries the fault fails, named."""
    assert " cov_s[" in _rejected(B.check_chain, "weight_not_squared", KIND_RBF)
    assert " Knn[" in _rejected(B.check_chain, "cov_over_s", KIND_MATERN52)
    assert " dvar[" in _rejected(B.check_chain, "dvar_factor2", KIND_MATERN52)
