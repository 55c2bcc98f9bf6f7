"""The error bounds of tests/_studies_bounds.py, checked without a device.  Two backends run every input set of that module through its
drivers: the kernel's own text compiled for the host (tests/host_emul/studies_acqf_emul.cpp, studies_score_emul.cpp,
studies_fantasy_emul.cpp: sa_block<1> and sa_block<16> with both argument blocks) -- the bounds admit the real statements on every
set and every cap and margin holds -- and a plain fp64 numpy stand-in of sa_block in the kernel's formulation (task sums in chunks
of eight, the blocked substitution with the block inverses W, one contraction per output), which carries the planted faults: each is
rejected on a named element, and the stand-in passes without it.  For each fault the largest error / bound and the largest error
against 1e-10 of max |ref| (the device tolerance of tests/test_studies_acqf_gpu.py) are printed; profiles/studies_bounds_notes.md
records them."""
import ctypes
import math

import numpy as np
import pytest

from tests import _studies_bounds as SB
from tests._host_emul import BP, DP, IP, build, ptr as _p
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF, LD, SENTINEL
from tests._studies_bounds import ACQ, ACQS, EI, FAMILY, KINDS, LOGEI, UCB

ORDER = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha", "n_points", "m_all", "s_all", "info", "acqf_param")
ORDER_F = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha_f", "n_fant", "n_points", "m_all", "s_all",
           "info", "acqf_param")
COMMON = [DP, DP, DP, IP, DP, DP, BP, DP, DP, DP, DP, DP, IP, DP, DP, IP, DP]


def _buf(*shape):
    return np.full((shape[0] + 1, *shape[1:]), SENTINEL)


def _take(buf):
    assert (buf[-1] == SENTINEL).all(), "the call wrote past the end of its output"
    return buf[:-1].copy()


class Host:
    """The backend interface of tests/_studies_bounds.py on the host builds of sa_block."""
    name = "host"

    def __init__(self, tmp_path_factory):
        self.q = build(tmp_path_factory, "studies_acqf_emul")
        self.q.emul_studies_acqf.restype = ctypes.c_int
        self.q.emul_studies_acqf.argtypes = COMMON + [ctypes.c_int] * 7 + [DP] * 4
        self.s = build(tmp_path_factory, "studies_score_emul")
        self.s.emul_studies_score.restype = ctypes.c_int
        self.s.emul_studies_score.argtypes = COMMON + [ctypes.c_int] * 7 + [DP] * 3
        self.f = build(tmp_path_factory, "studies_fantasy_emul")
        self.f.emul_studies_fantasy.restype = ctypes.c_int
        self.f.emul_studies_fantasy.argtypes = [ctypes.c_int] + COMMON[:11] + [DP, IP, IP, DP, DP, IP, DP] + [ctypes.c_int] * 8 + [DP, DP]

    def run(self, entry, a, grad, post):
        Mq, D = a["Xq"].shape
        strips = entry in ("score", "fantasy_score")
        value = _buf(Mq)
        gr = _buf(Mq, D) if grad and not strips else None
        mu, var = (_buf(Mq), _buf(Mq)) if post else (None, None)
        o = lambda x: None if x is None else _p(x)   # noqa: E731
        dims = (Mq, a["G"], a["n_max"])
        tail = (a["T"], D, a["kind"], a["acqf"])
        if entry == "acqf":
            rc = self.q.emul_studies_acqf(*[_p(a[k]) for k in ORDER], *dims, *tail, _p(value), o(gr), o(mu), o(var))
        elif entry == "score":
            rc = self.s.emul_studies_score(*[_p(a[k]) for k in ORDER], *dims, *tail, _p(value), o(mu), o(var))
        else:
            assert not post
            rc = self.f.emul_studies_fantasy(int(strips), *[_p(a[k]) for k in ORDER_F], *dims, a["F_max"], *tail, _p(value), o(gr))
        assert rc == 0, f"{entry}: return code {rc}"
        return dict(value=_take(value), grad=None if gr is None else _take(gr), mu=None if mu is None else _take(mu),
                    var=None if var is None else _take(var))


# ---- the stand-in -----------------------------------------------------------------------------------------------------------------
def _log_ei_terms(u):
    if u < -2.0:
        t = -u
        N = 112 if t < 3.0 else 72 if t < 5.0 else 36 if t < 8.0 else 20 if t < 16.0 else 12
        x = 0.5 * (math.sqrt(t * t + 4.0 * (N + 1)) - t)
        for k in range(N, 0, -1):
            x = k / (t + x)
        tk = t + x
        return (-0.5 * t * t - 0.91893853320467274178) + math.log(x / tk), 1.0 / x, tk / x
    pdf = math.exp(-0.5 * u * u) * 0.39894228040143267794
    cdf = 0.5 * math.erfc(-u * 0.70710678118654752440)
    h = u * cdf + pdf
    return math.log(h), cdf / h, pdf / h


def _acquisition(acqf, par, mu, vr, av_live):
    """sa_acquisition of csrc/gp_studies_formulas.h on scalars; av_live: the planted fault, d A / d var without its clamp condition."""
    if math.isnan(mu) or math.isnan(vr):
        return math.nan, math.nan, math.nan
    if acqf == UCB:
        sd = math.sqrt(par * (vr if vr > 0.0 else 0.0))
        return sd - mu, -1.0, (0.5 * par / max(sd, 1e-300) if vr > 0.0 or av_live else 0.0)
    sigma = math.sqrt(vr if vr > 1e-9 else 1e-9)
    uu = -(mu - par) / sigma
    if acqf == EI:
        pdf = math.exp(-0.5 * uu * uu) * 0.39894228040143267794
        cdf = 0.5 * (1.0 + math.erf(uu * 0.70710678118654752440))
        return sigma * (pdf + uu * cdf), -cdf, (0.5 * pdf / sigma if vr > 1e-9 or av_live else 0.0)
    g, gp, om = _log_ei_terms(uu)
    return math.log(sigma) + g, -gp / sigma, (0.5 * om / (sigma * sigma) if vr > 1e-9 or av_live else 0.0)


_acq = np.vectorize(_acquisition, otypes=[np.float64] * 3)


def _slope(kind, d2, os_):
    if kind == KIND_RBF:
        k = os_ * np.exp(-0.5 * d2)
        return k, -0.5 * k
    s5 = 2.2360679774997896964
    r = np.sqrt(np.maximum(d2, 1e-30))
    ex = os_ * np.exp(-s5 * r)
    lin = 1.0 + s5 * r
    return (lin + (5.0 / 3.0) * r * r) * ex, (-5.0 / 6.0) * lin * ex


FAULTS = ("drop_chunk2", "w_float32", "kz_early", "gradcol_shift", "av_live", "alpha_stride", "div_fmax", "w_unnormalised", "slope_1e-7",
          "slope_last_dim", "rf_row_guard")


class Numpy:
    """A plain fp64 stand-in of sa_block<R, Params> in the kernel's formulation; `fault` plants one of FAULTS."""
    name = "numpy"

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def run(self, entry, a, grad, post):
        Mq, D = a["Xq"].shape
        strips, fant = entry in ("score", "fantasy_score"), entry.startswith("fantasy")
        R = 16 if strips else 1
        assert not (fant and post) and Mq % R == 0
        out = dict(value=_buf(Mq), grad=_buf(Mq, D) if grad and not strips else None, mu=_buf(Mq) if post else None, var=_buf(Mq) if post else None)
        with np.errstate(all="ignore"):
            for blk in range(Mq // R):
                self._block(a, blk, R, fant, out)
        return {k: None if x is None else _take(x) for k, x in out.items()}

    def _block(self, a, blk, R, fant, out):
        fault = self.fault
        T, D, n_max, kind, acqf = a["T"], a["D"], a["n_max"], a["kind"], a["acqf"]
        g = int(a["group"][blk])
        rows = slice(blk * R, blk * R + R)

        def put(x):
            for k in ("value", "mu", "var", "grad"):
                if out[k] is not None:
                    out[k][rows] = x

        if g < 0 or g >= a["G"]:
            return put(0.0)
        n = int(a["n_points"][g])
        F = int(a["n_fant"][g]) if fant else 1
        if a["info"][g] != 0 or n < 1 or n > n_max or (fant and not 1 <= F <= a["F_max"]):
            return put(np.nan)
        s, m = a["s_all"][g], a["m_all"][g]
        s2 = s * s
        inv_s2 = 1.0 / s2
        th = a["theta"][g]
        os_ = th[D]
        # phase 1: the task sums, tasks ascending in chunks of eight
        nc = 16 if R == 16 else 1 + D
        if R == 16:
            mu_c, var_c, cov_c = a["mu"][:, rows], a["var"][:, rows], a["cov"][:, :n, rows]
        else:
            mu_c, var_c = a["mu"][:, blk, :nc], a["var"][:, blk, :nc]
            cov_c = a["cov"].reshape(T, n_max, -1, 16)[:, :n, blk, :nc]
        Smu, Svar, C = np.zeros(nc), np.zeros(nc), np.zeros((n, nc))
        for t0 in range(0, T, 8):
            if fault == "drop_chunk2" and t0 == 8 and T == 9:
                continue
            for t in range(t0, min(t0 + 8, T)):
                if not a["active"][g, t]:
                    continue
                wt = a["w"][g, t]
                Smu = Smu + wt * mu_c[t]
                Svar = Svar + (wt * wt) * var_c[t]
                C = C + (wt * wt) * cov_c[t]
        C = C * inv_s2
        Ls = np.tril(a["L"][g, :n, :n])
        W = a["Linv_diag"][g]
        if fault == "w_float32":
            W = W.astype(np.float32).astype(np.float64)
        # phase 1b
        xa = a["Xt"][g, :n]
        for c in range(R):
            xq = a["Xq"][blk * R + c]
            d2 = np.zeros(n)
            for d in range(D):
                df = (xq[d] - xa[:, d]) / th[d]
                d2 = d2 + df * df
            k0, dk = _slope(kind, d2, os_)
            if fault == "slope_1e-7":
                dk[int(np.argmax(d2))] *= 1.0 + 1e-7
            C[:, c] += k0
            if R == 1:
                for d in range(D - 1 if fault == "slope_last_dim" and D == 15 else D):
                    C[:, 1 + d] += 2.0 * dk * ((xq[d] - xa[:, d]) / (th[d] * th[d]))
        u = C[:, :R].copy()
        v = np.zeros_like(u)
        # phase 2: the blocked substitution with the block inverses
        nb = (n + 15) // 16
        for kb in range(nb):
            r0, cnt = 16 * kb, min(16, n - 16 * kb)
            v[r0:r0 + cnt] = np.tril(W[kb, :cnt, :cnt]) @ u[r0:r0 + cnt]
            if r0 + 16 < n:
                u[r0 + 16:] = u[r0 + 16:] - Ls[r0 + 16:, r0:r0 + 16] @ v[r0:r0 + 16]
        for kb in range(nb - 1, -1, -1):
            r0, cnt = 16 * kb, min(16, n - 16 * kb)
            u[r0:r0 + cnt] = np.tril(W[kb, :cnt, :cnt]).T @ v[r0:r0 + cnt]
            v[:r0] = v[:r0] - Ls[r0:r0 + cnt, :r0].T @ u[r0:r0 + cnt]
        z = u
        # phases 3 and 4
        last = n - 1 if fault == "kz_early" and n > 1 else n
        kz = (z[:last] * C[:last, :R]).sum(0)
        mean_q, var_q = (Smu[:R] - m) / s, Svar[:R] * inv_s2 + os_
        vr = s2 * (var_q - kz)
        par = a["acqf_param"][g]
        bad = (a["Xq"][rows] - a["Xq"][rows]).sum(1)
        if fant:
            if fault == "alpha_stride" and F > 1:
                flat = a["alpha_f"][g].ravel()
                al = flat[np.arange(n)[:, None] * F + np.arange(F)[None, :]]
            else:
                al = a["alpha_f"][g, :n, :F]
        else:
            al = a["alpha"][g, :n, None]
        rf_rows = n - 1 if fault == "rf_row_guard" and F > 1 and n % 8 == 1 else n
        mu = m + s * (mean_q[:, None] + C[:rf_rows, :R].T @ al[:rf_rows])                      # (R, F)
        A, Amu, Av = _acq(acqf, par, mu, np.broadcast_to(vr[:, None], mu.shape), fault == "av_live")
        shift = 0 if fault == "gradcol_shift" and D == 15 else 1
        if F == 1:
            value = A[:, 0]
            if out["mu"] is not None:
                out["mu"][rows] = np.where(bad == 0.0, mu[:, 0], np.nan)
                out["var"][rows] = np.where(bad == 0.0, vr, np.nan)
            if out["grad"] is not None:
                dK = C[:, shift:shift + D]
                dmu = Smu[1:1 + D] + s * (al[:, 0] @ dK)
                dvar = Svar[1:1 + D] - 2.0 * s2 * (z[:, 0] @ dK)
                out["grad"][blk] = (Av[0, 0] * dvar + Amu[0, 0] * dmu) if bad[0] == 0.0 else np.nan
        else:
            Fdiv = float(a["F_max"] if fault == "div_fmax" else F)
            if acqf == LOGEI:
                mx = A.max(1, keepdims=True) + (A - A).sum(1, keepdims=True)
                e = np.exp(A - mx)
                S = e.sum(1, keepdims=True)
                wf = e if fault == "w_unnormalised" else e / S
                Amu, Av = Amu * wf, Av * wf
                value = (mx + np.log(S) - math.log(F))[:, 0]
                Fdiv = 1.0
            else:
                value = A.sum(1) / Fdiv
            if out["grad"] is not None:
                dK = C[:, shift:shift + D]
                abar = al @ Amu[0]
                gmu = Amu[0].sum() * Smu[1:1 + D] + s * (abar @ dK)
                dvar = Svar[1:1 + D] - 2.0 * s2 * (z[:, 0] @ dK)
                out["grad"][blk] = ((Av[0].sum() * dvar + gmu) / Fdiv) if bad[0] == 0.0 else np.nan
        out["value"][rows] = np.where(bad == 0.0, value, np.nan)


CLEAN = Numpy()
FAM = pytest.mark.parametrize("kind", KINDS, ids=["rbf", "matern"])
ACQF = pytest.mark.parametrize("acqf", ACQS, ids=[ACQ[x] for x in ACQS])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return Host(tmp_path_factory)


@pytest.fixture(params=["host", "numpy"])
def be(request, host):
    return host if request.param == "host" else CLEAN


# ---- every set through both backends -------------------------------------------------------------------------------------------------
@FAM
@ACQF
@pytest.mark.parametrize("name", sorted(SB.ORDINARY_SETS))
def test_ordinary_sets_within_bound(be, name, kind, acqf):
    a = SB.ORDINARY_SETS[name](kind, acqf)
    SB.check_set(be, a, f"studies-{name}-{FAMILY[kind]}-{ACQ[acqf]}", tag="clean")
    if acqf == UCB:
        SB.check_junk_columns(be, a, f"studies-{name}-{FAMILY[kind]}")


@FAM
@ACQF
@pytest.mark.parametrize("name", sorted(SB.FANTASY_SETS))
def test_fantasy_sets_within_bound(be, name, kind, acqf):
    a = SB.FANTASY_SETS[name](kind, acqf)
    SB.check_set(be, a, f"studies-{name}-{FAMILY[kind]}-{ACQ[acqf]}", tag="clean")
    if acqf == UCB:
        SB.check_junk_columns(be, a, f"studies-{name}-{FAMILY[kind]}")


@FAM
@ACQF
def test_clamps(be, kind, acqf):
    SB.check_clamp(be, kind, acqf)


@FAM
@pytest.mark.parametrize("acqf", [EI, LOGEI], ids=["ei", "logei"])
@pytest.mark.parametrize("mode", ["span", "deep"])
def test_ei_tails(be, mode, kind, acqf):
    SB.check_tail(be, mode, kind, acqf)


@FAM
def test_refusals_and_non_finite_queries(be, kind):
    a = SB.set_T8(kind, EI)
    SB.check_refusals(be, a, f"studies-T8-{FAMILY[kind]}", victim=2)
    SB.check_nonfinite(be, a, f"studies-T8-{FAMILY[kind]}-nanq", q=3)
    f = SB.set_FB(kind, LOGEI)
    SB.check_refusals(be, f, f"studies-FB-{FAMILY[kind]}", victim=0)
    SB.check_nonfinite(be, f, f"studies-FB-{FAMILY[kind]}-nanq", q=1)


def test_the_sets_are_what_they_claim():
    """The masked task holds NaN and a NaN weight in one group only, one group has every task masked, NaN lies where nothing may be read,
    the small weight is 1e-4 of the others, and the irrelevant dimension's gradient is ten orders under the largest."""
    a = SB.set_T9(KIND_RBF, UCB)
    g, t = SB.T9_MASKED
    assert np.isnan(a["w"][g, t]) and np.isnan(a["mu"][t, a["group"] == g]).all() and not a["active"][SB.T9_ALL_MASKED].any()
    assert np.isfinite(a["mu"][t, a["group"] == 0]).all() and a["w"][0, 8] == 1e-4 * a["w"][0, 0]
    for g, n in enumerate(a["n_points"]):
        assert np.isnan(a["Xt"][g, n:]).all() and np.isnan(a["L"][g, n:]).all() and np.isnan(a["alpha"][g, n:]).all()
        assert np.isnan(a["L"][g, :n, :n][np.triu_indices(n, 1)]).all() and np.isnan(a["Linv_diag"][g, (n + 15) // 16:]).all()
        if n % 16:
            assert np.isnan(a["Linv_diag"][g, n // 16, n % 16:]).all() and np.isnan(a["Linv_diag"][g, n // 16, :, n % 16:]).all()
        rows = a["group"] == g
        assert np.isnan(a["cov"].reshape(9, 96, -1, 16)[:, n:, rows]).all()
    ref = SB.reference(a)
    gr = np.abs(ref["ref"]["grad"][a["group"] == 2])
    assert float(gr[:, 14].max()) < 1e-9 * float(gr.max())
    f = SB.set_FA(KIND_RBF, UCB)
    for g, (n, F) in enumerate(SB.FA_GROUPS):
        assert np.isnan(f["alpha_f"][g, :n, F:]).all() and np.isnan(f["alpha_f"][g, n:]).all() and np.isfinite(f["alpha_f"][g, :n, :F]).all()


def test_print_the_ratio_table():
    """(after the tests above: the table as profiles/studies_bounds_notes.md records it -- pytest -s shows it)"""
    print()
    for line in SB.report():
        print("  " + line)


# ---- every planted fault is rejected, on a named element ----------------------------------------------------------------------------
def _effect(fault, a, entry="acqf", post=True):
    """The fault's largest error / bound and its largest error against 1e-10 of max |ref| per output of the call."""
    ref = SB.reference(a)
    got = Numpy(fault).run(entry, a, grad=True, post=post)
    live = ref["state"] == "live"
    out = {}
    for k in ref["names"]:
        if got.get(k) is None:
            continue
        r, b = ref["ref"][k][live], ref["bound"][k][live]
        with np.errstate(all="ignore"):
            err = np.where(np.isnan(got[k][live]), np.inf, np.abs(LD(got[k][live]) - r))      # (a NaN where the reference is finite: infinitely wrong)
            out[k] = (float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0))), float(np.max(err) / np.abs(r).max()))
    return out


def _rejected(fault, a, label, named, under_tolerance=None):
    SB.check_set(CLEAN, a, label)
    with pytest.raises(AssertionError) as e:
        SB.check_set(Numpy(fault), a, label)
    fant = "alpha_f" in a
    eff = _effect(fault, a, "fantasy" if fant else "acqf", post=not fant)
    print(f"\n  [{fault}] {e.value}\n  [{fault}] (largest error / bound, largest error / max |ref|): " + ", ".join(f"{k} ({x:.3e}, {y:.3e})" for k, (x, y) in eff.items()))
    assert named in str(e.value), str(e.value)
    under = all(y <= 1e-10 for _, y in eff.values())
    if under_tolerance is not None:
        assert under == under_tolerance, f"{fault}: under the 1e-10 max-norm tolerance: {under}"
    return str(e.value)


def test_rejects_the_second_chunks_task_dropped():
    """T = 9: the ninth task, the one with 1e-4 of the others' weight, left out of every sum."""
    _rejected("drop_chunk2", SB.set_T9(KIND_MATERN52, UCB), "T9-matern-ucb", "group 0 value[0]", under_tolerance=False)


def test_rejects_block_inverses_rounded_to_float32():
    _rejected("w_float32", SB.set_T8(KIND_RBF, UCB), "T8-rbf-ucb", "group 0 value[0]")


def test_rejects_the_variance_contraction_stopping_one_point_early():
    """Knq . z without its last training point, which lies far from every query: the term is under the 1e-10 max-norm tolerance."""
    _rejected("kz_early", SB.set_FAR(KIND_RBF, UCB), "FAR-rbf-ucb", "group 1 value[1]", under_tolerance=True)


def test_rejects_the_row_guard_of_the_fantasy_means_off_by_one():
    """F > 1: row n - 1 of alpha_f dropped from r_f when n % 8 == 1 (n = 9, 17), the last training point far from every query."""
    _rejected("rf_row_guard", SB.set_FARF(KIND_MATERN52, UCB), "FARF-matern-ucb", "group 0 value[0]", under_tolerance=True)


def test_rejects_gradient_column_read_one_to_the_left():
    _rejected("gradcol_shift", SB.set_T9(KIND_RBF, EI), "T9-rbf-ei", "group 0 grad[0, 0]", under_tolerance=False)


@pytest.mark.parametrize("acqf", [EI, LOGEI, UCB], ids=["ei", "logei", "ucb"])
def test_rejects_av_live_on_the_floor(acqf):
    a, clamped = SB.set_CLAMP(KIND_MATERN52, acqf)
    label = f"CLAMP-matern-{ACQ[acqf]}"
    SB.check_clamp(CLEAN, KIND_MATERN52, acqf)
    with pytest.raises(AssertionError) as e:
        SB.check_clamp(Numpy("av_live"), KIND_MATERN52, acqf)
    print(f"\n  [av_live] {e.value}")
    assert "group 0 grad[0, 0]" in str(e.value), str(e.value)
    assert clamped[0] == 0 and label


def test_rejects_alpha_f_read_with_row_stride_f():
    _rejected("alpha_stride", SB.set_FA(KIND_RBF, UCB), "FA-rbf-ucb", "group 1 value[0]", under_tolerance=False)


def test_rejects_the_fantasy_mean_divided_by_f_max():
    _rejected("div_fmax", SB.set_FA(KIND_MATERN52, EI), "FA-matern-ei", "group 1 value[0]", under_tolerance=False)


def test_rejects_unnormalised_log_domain_weights():
    _rejected("w_unnormalised", SB.set_FA(KIND_RBF, LOGEI), "FA-rbf-logei", "group 1 grad[0, 0]", under_tolerance=False)


def test_rejects_one_kernel_slope_off_by_1e_7_at_the_far_point():
    """os dk (1 + 1e-7) at the training point farthest from the query: one term of n, seven digits down."""
    _rejected("slope_1e-7", SB.set_GEO(KIND_MATERN52, UCB), "GEO-matern-ucb", "group 0 grad[0, 0]")


def test_rejects_the_last_dimensions_slope_left_out():
    """D = 15: the kernel's part of gradient column 15 missing.  The dimension is an irrelevant one, its gradient component ten orders under
    the largest: a max-norm tolerance cannot see it."""
    _rejected("slope_last_dim", SB.set_T9(KIND_RBF, UCB), "T9-rbf-ucb", ", 14]", under_tolerance=True)
