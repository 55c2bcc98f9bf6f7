"""The error bounds of tests/_fantasy_bounds.py, checked without a device: they admit honest fp64 arithmetic in the fantasy kernel's own
formulation (a lane per training point and a tree sum for Knq . Z, one sequential fma chain per fantasy for mu_f, 64 lanes of which
the first F are live, a sequential chain over the fantasies for abar, a lane per training point and a tree sum for the gradient) on
every input set of tests/test_fantasy_bounds_gpu.py, the caps hold on every set, the long-double erf is good to 16 eps_LD, and every
planted fault below is rejected on a named element.  The measured ratios are in profiles/fantasy_bounds_notes.md."""
import math

import numpy as np
import pytest

from tests import _fantasy_bounds as FB
from tests import _posterior_bounds as P
from tests import _target_bounds as B
from tests import test_posterior_bounds as SP
from tests import test_target_bounds as TB
from tests._fantasy_bounds import E_BADARG, EI, UCB
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, SENTINEL

_erf = np.vectorize(math.erf, otypes=[np.float64])


def _lanes(x, rounds):
    """x (n, ...) -> the per-lane chain over a = lane, lane + 64, ..., then the tree over the 64 lanes."""
    pad = np.zeros((rounds * 64, *x.shape[1:]))
    pad[:x.shape[0]] = x
    return TB._tree(TB._chain8(pad.reshape(rounds, 64, *x.shape[1:]), np.zeros((64, *x.shape[1:]))))


class Numpy(TB.Numpy):
    """tests/test_target_bounds.Numpy with a plain fp64 stand-in of scaml_target_fantasy_acqf_f64 (launcher and kernel); `fault` plants one
    of the faults of the tests below."""

    def fantasy(self, a, info):
        n, M, F, D, acqf, s = a["n"], a["M"], a["F"], a["D"], a["acqf"], a["s"]
        want_grad = bool(a.get("grad"))
        value = np.full(a["mean_q"].shape[0], SENTINEL)
        grad = np.full((a["mean_q"].shape[0], a["Xq"].shape[1]), SENTINEL) if want_grad else None
        # ---- the launcher's checks, in its order
        if n < 1 or M < 0 or F < 1 or acqf not in (0, 1) or not s > 0.0:
            return E_BADARG, value, grad
        if want_grad and (D < 1 or a["kind"] not in (KIND_RBF, KIND_MATERN52)):
            return E_BADARG, value, grad
        if F > 64 or n > 256 or (want_grad and (n > 96 or D > 15)):
            return B.E_TOOLARGE, value, grad
        if M == 0:
            return 0, value, grad
        if info is not None and info > 0:
            return 0, np.full(M, np.nan), (np.full((M, D), np.nan) if want_grad else None)
        fault = self.fault
        Knq, al, s2 = a["Knq"][:n], a["alpha"][:n], s * s
        Z = a["Z"][:n]
        if fault == "z_stride_n":
            Z = a["Z"].ravel()[(np.arange(n)[:, None] * n + np.arange(M)[None, :]) % a["Z"].size]
        rounds = (n + 63) // 64
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            # (1) lanes = training points
            kz = _lanes(Knq * Z, rounds)
            v = s2 * (a["var_q"] - kz + (0.0 if fault == "noise_dropped" else a["noise_add"]))
            # (2) lanes = fantasies: 64 of them, lane f >= F reads what lies behind its row of alpha (and is zeroed after the transform)
            flat = np.concatenate([a["alpha"].ravel(), np.full(64, 0.37)])
            al64 = flat[np.arange(n)[:, None] * F + np.arange(64)[None, :]]
            rows = n - 1 if fault == "row_guard" and n % 8 == 1 else n
            mu = np.repeat(a["mean_q"][:, None], 64, axis=1)
            for r in range(rows):
                mu = mu + Knq[r][:, None] * al64[r][None, :]
            mu = s * mu + a["m"]
            vv = v[:, None]
            par = a["param"]
            if acqf == UCB:
                sd = np.sqrt(par * np.where(vv > 0.0, vv, 0.0))
                A = sd - mu
                Amu = -np.ones_like(mu)
                Av = 0.5 * par / np.where(sd > 1e-300, sd, 1e-300)
                Av = np.broadcast_to(Av if fault == "av_live" else np.where(vv > 0.0, Av, 0.0), mu.shape)
            else:
                sigma = np.sqrt(np.where(vv > 1e-9, vv, 1e-9))
                u = -(mu - par) / sigma
                pdf = np.exp(-0.5 * u * u) * 0.39894228040143267794
                cdf = 0.5 * (1.0 + _erf(u * 0.70710678118654752440))
                A, Amu = sigma * (pdf + u * cdf), -cdf
                Av = 0.5 * pdf / sigma
                Av = Av if fault == "av_live" else np.where(vv > 1e-9, Av, 0.0)
            dead = np.arange(64) >= (F + 1 if fault == "lane_F" and F < 64 else F)
            A, Amu, Av = (np.where(dead, 0.0, x) for x in (A, Amu, Av))
            invF = 1.0 / (64 if fault == "inv64" else F)
            val = TB._tree(A.T)
            value = val * invF
            if not want_grad:
                return 0, value, None
            sAmu, sAv = TB._tree(Amu.T), TB._tree(Av.T)
            # (3) lanes = training points
            ab = np.zeros((M, n))
            for g in range(F):
                ab = ab + Amu[:, g][:, None] * al[:, g][None, :]
            th = a["theta"]
            il, inv_s2 = 1.0 / th[:D], 1.0 / s2
            df = (a["Xq"][None, :, :D] - a["Xt"][:n, None, :D]) * il                     # (n, M, D)
            d2 = np.zeros((n, M))
            for d in range(D):
                d2 = d2 + df[..., d] * df[..., d]
            kind = a["kind"]
            slope_kind = (KIND_RBF + KIND_MATERN52 - kind) if fault == "wrong_family_slope" else kind
            dk = SP._k64(d2, slope_kind, restore_nan=False)[1] * (th[D] / P.OS)
            if fault == "slope_1e-7":
                dk[int(np.argmax(np.abs(ab).max(0)))] *= 1.0 + 1e-7
            c0 = 0 if fault == "cov_col0" else 1
            cg = a["cov_g"][:n].reshape(n, M, 16)[:, :, c0:c0 + D]
            dkn = cg * inv_s2 + 2.0 * dk[:, :, None] * (df * il)
            tot = _lanes(np.stack([ab.T[:, :, None] * dkn, Z[:, :, None] * dkn], -1), rounds)      # (M, D, 2)
            mu_g, var_g = a["mu_g"].reshape(M, 16)[:, 1:1 + D], a["var_g"].reshape(M, 16)[:, 1:1 + D]
            gmu = sAmu[:, None] * mu_g + s * tot[..., 0]
            gvar = var_g - (1.0 if fault == "dvar_factor2" else 2.0) * s2 * tot[..., 1]
            bad = ((a["Xq"][:, :D] - a["Xq"][:, :D]).sum(-1) + (val - val))[:, None]
            grad = np.where(bad == 0.0, (sAv[:, None] * gvar + gmu) * invF, np.nan)
        return 0, value, grad


CLEAN = Numpy()
FAMILIES = pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])


# ---- the reference's own erf -----------------------------------------------------------------------------------------------------
def test_long_double_erf_against_mpmath():
    """The series of tests/_fantasy_bounds.erf_ld over [-6.5, 6.5] (and +-1 beyond) against mpmath at 40 digits: <= 16 eps_LD."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    xs = np.concatenate([np.linspace(-6.5, 6.5, 2001), 10.0 ** np.linspace(-300, 0, 301), [6.5000001, -7.0, 30.0, -30.0]])
    got = FB.erf_ld(xs)
    eps = mpmath.mpf(float(np.finfo(LD).eps))
    worst = 0.0
    for x, y in zip(xs, got):
        t = mpmath.erf(mpmath.mpf(float(x)))
        if t == 0:
            assert y == 0
            continue
        y = mpmath.mpf(np.format_float_scientific(y, precision=24, unique=False))
        worst = max(worst, float(abs(y - t) / abs(t) / eps))
    print(f"\n  erf_ld: largest relative error {worst:.2f} eps_LD")
    assert worst <= 16.0
    assert FB.erf_ld(np.array([0.0]))[0] == 0 and np.isnan(FB.erf_ld(np.array([np.nan]))[0])


# ---- the caps and the smoothness conditions hold on every set, without any kernel --------------------------------------------------
def _all_sets():
    for c in FB.GRAD_CASES:
        for acqf in (UCB, EI):
            yield f"{FB.grad_id(c)}-{FB.ACQ[acqf]}", FB.inputs(*c, acqf), None
    for (n, F, M) in FB.VALUE_SHAPES:
        for acqf in (UCB, EI):
            yield f"value-n{n}-F{F}-M{M}-{FB.ACQ[acqf]}", FB.inputs(n, F, M, 0, KIND_RBF, acqf, grad=False), None
    for kind in (KIND_RBF, KIND_MATERN52):
        for mode, acqf in FB.CLAMP_MODES:
            yield f"clamp-{mode}-{FB.ACQ[acqf]}-{kind}", FB.clamp_inputs(mode, acqf, kind), None
        yield f"tail-span-{kind}", FB.tail_inputs("span", kind), None
        yield f"tail-deep-{kind}", FB.tail_inputs("deep", kind), "sigma"


def test_caps_and_conditions_hold_on_every_set():
    """Every bound at most CAP of its output's scale, eps <= 1e-6, v at least 1e3 E_v from its clamp; and the planned magnitudes:
    E_mu, E_v / v four orders inside the cap at n = 96 and n = 256."""
    worst = {}
    for label, a, scale in _all_sets():
        ref = FB.fantasy_reference(a)
        FB.conditions(label, ref)
        for name in ("value", "grad") if a.get("grad") else ("value",):
            q = ref[name]
            sc = ref["sigma"] if scale == "sigma" else q.scale
            assert sc > 0 and float(q.bound.max()) <= CAP * sc, f"{label} {name}: bound {float(q.bound.max()):.3e} against scale {sc:.3e}"
            worst[name] = max(worst.get(name, 0.0), float(q.bound.max()) / sc)
    print(f"\n  largest bound / scale over all sets: {worst}")
    for n, F, M in ((96, 64, 3), (256, 64, 130)):
        a = FB.inputs(n, F, M, 0, KIND_RBF, UCB, grad=False)
        ref = FB.fantasy_reference(a)
        assert float(ref["eps"].max()) <= 1e-12, f"n = {n}: E_v / v = {float(ref['eps'].max()):.3e}"


# ---- honest fp64 is inside every bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FB.GRAD_CASES, ids=FB.grad_id)
def test_standin_within_bound(case):
    FB.check_grad_case(CLEAN, case)


@pytest.mark.parametrize("shape", FB.VALUE_SHAPES, ids=lambda s: f"n{s[0]}-F{s[1]}-M{s[2]}")
def test_standin_value_only_within_bound(shape):
    FB.check_value_only(CLEAN, shape)


@FAMILIES
@pytest.mark.parametrize("mode,acqf", FB.CLAMP_MODES, ids=lambda x: FB.ACQ.get(x, x) if isinstance(x, int) else x)
def test_standin_clamps(mode, acqf, kind):
    FB.check_clamp(CLEAN, mode, acqf, kind)


@FAMILIES
@pytest.mark.parametrize("mode", ["span", "deep"])
def test_standin_ei_tails(mode, kind):
    FB.check_tails(CLEAN, mode, kind)


@FAMILIES
@pytest.mark.parametrize("what", [np.nan, np.inf, "col", "knq"], ids=["nan", "inf", "nan-column", "nan-knq"])
@pytest.mark.parametrize("shape", [FB.CLAMP_SHAPE, FB.EDGE_SHAPE], ids=["n9", "n65"])
def test_standin_non_finite_query(shape, what, kind):
    for acqf in (UCB, EI):
        FB.check_nonfinite(CLEAN, shape, kind, acqf, what)


def test_standin_refusals():
    FB.check_refusals(CLEAN)


@pytest.mark.parametrize("case", [c for c in FB.GRAD_CASES if c[1] == 1], ids=FB.grad_id)
def test_standin_f1_ucb_against_finish_and_gradient(case):
    FB.check_against_finish_and_gradient(CLEAN, case)


@FAMILIES
def test_chain_standins_within_bound(kind):
    FB.check_chain(CLEAN, kind)


def test_print_the_ratio_table():
    """(after the tests above: the table of the stand-in as profiles/fantasy_bounds_notes.md records it -- pytest -s shows it)"""
    print()
    for line in FB.report():
        print("  " + line)


# ---- every planted fault is rejected, on a named element -------------------------------------------------------------------------
def _rejected(check, fault, *args):
    check(CLEAN, *args)
    with pytest.raises(AssertionError) as e:
        check(Numpy(fault), *args)
    print(f"\n  [{fault}] {e.value}")
    return str(e.value)


def test_rejects_lane_f_counted():
    """Lane F (dead, F < 64: it reads what lies behind its row of alpha) counted in the sums.
    fantasy-n8-F63-M3-D6-rbf-ucb-infoNone value[0]: got 8.543618689931957, reference 8.419932733835928, error 1.237e-01 > bound 2.085e-14 (3
    of 3 elements); F = 2: got 12.433266601240524, reference 8.347509190173913."""
    assert " value[0]" in _rejected(FB.check_grad_case, "lane_F", (8, 63, 3, 6, KIND_RBF))
    assert " value[0]" in _rejected(FB.check_grad_case, "lane_F", (7, 2, 3, 6, KIND_MATERN52))


def test_rejects_one_over_64_in_place_of_one_over_f():
    """fantasy-n8-F63-M3-D6-rbf-ucb-infoNone value[0]: got 8.288371284869742, reference 8.419932733835928, error 1.316e-01 > bound 2.085e-14
    (3 of 3 elements)."""
    assert " value[0]" in _rejected(FB.check_grad_case, "inv64", (8, 63, 3, 6, KIND_RBF))


@pytest.mark.parametrize("mode,acqf", FB.CLAMP_MODES[:5], ids=lambda x: FB.ACQ.get(x, x) if isinstance(x, int) else x)
def test_rejects_av_live_on_a_clamp(mode, acqf):
    """d A / d v computed without its clamp condition, on each clamp set (queries 0 and 2).
    fantasy-clamp-neg-ucb-matern-infoNone grad[0, 0]: got 3.1990301137396784e+300, reference -0.49022736631781544 (v = 0 exactly: the same);
    fantasy-clamp-neg-ei-matern-infoNone grad[0, 0]: got 3797.7563234467157, reference -0.14319352741076888, error 3.798e+03 > bound
    1.816e-12 (30 of 45 elements; v = 5e-10: the same; v = 0: got 3880.7362245676554, reference -0.1448283776008872)."""
    assert " grad[0, 0]" in _rejected(FB.check_clamp, "av_live", mode, acqf, KIND_MATERN52)


def test_rejects_the_row_guard_off_by_one():
    """Row n - 1 of alpha dropped when n % 8 == 1.
    fantasy-n9-F64-M3-D15-rbf-ucb-infoNone value[0]: got 6.920246605899972, reference 6.930257124937023, error 1.001e-02 > bound 1.787e-14 (3
    of 3 elements); n = 65: value[0] got 1.1031811997901388, reference 1.1096738724578856 (130 of 130 elements)."""
    assert " value[0]" in _rejected(FB.check_grad_case, "row_guard", (9, 64, 3, 15, KIND_RBF))
    assert " value[0]" in _rejected(FB.check_grad_case, "row_guard", (65, 63, 130, 6, KIND_MATERN52))


def test_rejects_z_strided_by_n():
    """Z[a * n + q] in place of Z[a * M + q] (n = 9, M = 3).
    fantasy-n9-F64-M3-D15-rbf-ucb-infoNone value[0]: got 6.948757315133586, reference 6.930257124937023, error 1.850e-02 > bound 1.787e-14 (3
    of 3 elements)."""
    assert " value[" in _rejected(FB.check_grad_case, "z_stride_n", (9, 64, 3, 15, KIND_RBF))


def test_rejects_cov_g_read_at_column_0():
    """cov_g read at 16 q instead of 16 q + 1 (every column of the sets holds data).
    fantasy-n9-F64-M3-D15-matern-ucb-infoNone grad[0, 0]: got 0.37277014802557806, reference 0.36581719474143365, error 6.953e-03 > bound
    5.930e-14 (45 of 45 elements)."""
    assert " grad[0, 0]" in _rejected(FB.check_grad_case, "cov_col0", (9, 64, 3, 15, KIND_MATERN52))


def test_rejects_dvar_without_its_factor_2():
    """fantasy-n64-F64-M3-D6-rbf-ucb-infoNone grad[0, 0]: got 1.1579317895952326, reference 1.2712448563628298, error 1.133e-01 > bound
    5.197e-14 (18 of 18 elements)."""
    assert " grad[0, 0]" in _rejected(FB.check_grad_case, "dvar_factor2", (64, 64, 3, 6, KIND_RBF))


def test_rejects_noise_add_dropped():
    """noise_add = 1e-3 (the sets with odd n) left out of v.
    fantasy-n9-F64-M3-D15-rbf-ucb-infoNone value[0]: got 6.928073135677473, reference 6.930257124937023, error 2.184e-03 > bound 1.787e-14 (3
    of 3 elements)."""
    assert " value[0]" in _rejected(FB.check_grad_case, "noise_dropped", (9, 64, 3, 15, KIND_RBF))


def test_rejects_the_slope_of_the_wrong_family():
    """fantasy-n64-F64-M3-D6-matern-ucb-infoNone grad[0, 0]: got 2.7556589099661757, reference 2.765534151577122, error 9.875e-03 > bound
    3.822e-13 (18 of 18 elements); rbf: got 1.2214534048833203, reference 1.2712448563628298."""
    assert " grad[0, 0]" in _rejected(FB.check_grad_case, "wrong_family_slope", (64, 64, 3, 6, KIND_MATERN52))
    assert " grad[" in _rejected(FB.check_grad_case, "wrong_family_slope", (64, 64, 3, 6, KIND_RBF))


def test_rejects_one_kernel_slope_off_by_1e_7():
    """os dk (1 + 1e-7) at the training point with the largest |abar|, n = 96: one term of 96, seven digits down.
    fantasy-n96-F64-M3-D15-rbf-ucb-infoNone grad[0, 0]: got 1.3925567530889607, reference 1.39255675362653, error 5.376e-10 > bound 4.067e-14
    (45 of 45 elements); matern: got -1.8765717774297064, reference -1.8765717774198047, error 9.902e-12 > bound 8.959e-14."""
    assert " grad[" in _rejected(FB.check_grad_case, "slope_1e-7", (96, 64, 3, 15, KIND_RBF))
    assert " grad[" in _rejected(FB.check_grad_case, "slope_1e-7", (96, 64, 3, 15, KIND_MATERN52))
