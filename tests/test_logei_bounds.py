"""CPU checks of LogEI (acquisition code 17) through host builds of the kernels' own source:
  - the scalar function sa_log_ei_terms / sa_log_ei_core and sa_acquisition (tests/host_emul/logei_emul.cpp) against the 50-digit table
    tests/golden/logei/logei_scalar_table.npz, inside the a-priori budgets of tests/_logei_bounds.py, which themselves stay under the
    contract's cap of 256 u; exp(LogEI) against the EI branch; NaN; the refused codes;
  - the log-domain average over fantasies in sa_block<R> (tests/host_emul/studies_fantasy_emul.cpp, code 17) against a torch-fp64
    restatement: tests/test_studies_fantasy_emul.py's posterior, LogEI from torch.special.erfcx, torch.logsumexp, autograd.  The
    restatement's 1 - t R(t) loses t^2 eps (2.3e-13 at t = 45), so that module's tolerances hold here: value rtol 1e-9 (absolute 1e-9
    below 1), gradient rtol 1e-6, atol 1e-9 relative to the gradient's largest entry.
Every test of code 17 fails on a library that refuses or ignores the code."""
import ctypes
import math

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests import _fantasy_bounds as FB
from tests import _logei_bounds as LB
from tests._host_emul import DP, IP, BP, build, ptr as _p
from tests._posterior_bounds import LD, U, gamma
from tests.test_studies_acqf_emul import T, _kernel
from tests.test_studies_fantasy_emul import ORDER, Problem, _strip_arrays

LOGEI = LB.LOGEI


@pytest.fixture(scope="module")
def scalar(tmp_path_factory):
    lib = build(tmp_path_factory, "logei_emul")
    lib.emul_log_ei_core.argtypes = [DP, ctypes.c_int, DP, DP, DP]
    lib.emul_log_ei_core3.argtypes = [DP, ctypes.c_int, DP, DP]
    lib.emul_acquisition.argtypes = [ctypes.c_int, ctypes.c_double, DP, DP, ctypes.c_int, DP, DP, DP]
    lib.emul_acqf_valid.restype, lib.emul_acqf_valid.argtypes = ctypes.c_int, [ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def fantasy(tmp_path_factory):
    lib = build(tmp_path_factory, "studies_fantasy_emul")
    lib.emul_studies_fantasy.restype = ctypes.c_int
    lib.emul_studies_fantasy.argtypes = ([ctypes.c_int] + [DP, DP, DP, IP, DP, DP, BP, DP, DP, DP, DP, DP, IP, IP, DP, DP, IP, DP] + [ctypes.c_int] * 8
                                         + [DP, DP])
    return lib


def _acq(lib, code, par, mu, var):
    mu, var = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(var, dtype=np.float64)
    out = [np.full(mu.size, 7.0) for _ in range(3)]
    lib.emul_acquisition(code, par, _p(mu), _p(var), mu.size, *[_p(o) for o in out])
    return out


def test_the_table_covers_the_contract():
    t = LB.table()
    u = t["u"]
    assert u.size <= 2048 and u.min() == -1e8 and u.max() == 40.0
    assert tuple(t["edges"]) == LB.EDGES
    for e in LB.EDGES:
        for x in (np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)):
            assert x in u, f"branch edge {e}: {x!r} is missing"
    for x in (-1e8, -1e5, -1e3, -200, -40, -38.5, -9, -1, -0.5, 0, 0.5, 9, 40):
        assert float(x) in u
    # the long-double function used away from the table agrees with it to a few eps_LD-scaled units
    g, gp, _ = LB.g_ld(u)
    assert float((np.abs(g - t["g"]) / (1 + np.abs(t["g"]))).max()) < 2.0 ** -58
    assert float((np.abs(gp - t["gp"]) / t["gp"]).max()) < 2.0 ** -58


def test_the_stated_budgets_stay_under_the_cap():
    t = LB.table()
    bg, bgp, _ = LB.budgets(t["u"])
    rg, rgp = bg / (1 + np.abs(t["g"]).astype(np.float64)), bgp
    print(f"budget_g / (1 + |g|) at most {rg.max():.1f} (u = {t['u'][rg.argmax()]!r}), budget_g' at most {rgp.max():.1f} (u = {t['u'][rgp.argmax()]!r})")
    assert rg.max() <= LB.CAP_UNITS and rgp.max() <= LB.CAP_UNITS


def test_scalar_function_on_the_table(scalar):
    t = LB.table()
    u = np.ascontiguousarray(t["u"])
    g, gp, om = (np.full(u.size, 7.0) for _ in range(3))
    scalar.emul_log_ei_core(_p(u), u.size, _p(g), _p(gp), _p(om))
    bg, bgp, bom = LB.budgets(u)
    eg = np.abs(LD(g) - t["g"]) / U
    egp = np.abs(LD(gp) - t["gp"]) / (U * t["gp"])
    om_ref = LB.g_ld(u)[2]
    eom = (np.abs(LD(om) - om_ref) - LD(2) ** -1022) / (U * np.maximum(om_ref, LD(1e-300)))
    print(f"error / budget: g {float((eg / bg).max()):.3f}, g' {float((egp / bgp).max()):.3f}, om {float((eom / bom).max()):.3f}; "
          f"in units of u: g / (1 + |g|) {float((eg / (1 + np.abs(t['g']))).max()):.2f}, g' {float(egp.max()):.2f}")
    assert np.isfinite(g).all() and np.isfinite(gp).all() and (gp > 0).all()
    assert (eg <= bg).all() and (egp <= bgp).all() and (eom <= bom).all()
    g3, gp3 = np.full(u.size, 7.0), np.full(u.size, 7.0)
    scalar.emul_log_ei_core3(_p(u), u.size, _p(g3), _p(gp3))
    assert np.array_equal(g3, g) and np.array_equal(gp3, gp)


@pytest.mark.parametrize("v", [0.37, 1e-9, 5e-10, 0.0, -0.01], ids=["above", "on", "tiny", "zero", "negative"])
def test_acquisition_on_the_table(scalar, v):
    """A, Amu, Av at (mu, v) with u = the table's points: v above, on and below the 1e-9 floor (Av exactly 0 there)."""
    t = LB.table()
    par = 0.25
    sigma = math.sqrt(max(v, 1e-9))
    sel = np.ones(t["u"].size, dtype=bool)   # the whole table, u = -1e8 included (LB.transform takes u from (mu, v) as the code does)
    mu = par - t["u"][sel] * sigma
    A, Amu, Av = _acq(scalar, LOGEI, par, mu, np.full(mu.size, v))
    r = LB.transform(par, mu, v)
    for name, got in (("A", A), ("Amu", Amu), ("Av", Av)):
        err, bound = np.abs(LD(got) - r[name]), r["E_" + name]
        print(f"v = {v}: {name} error / bound {float((err / np.where(bound > 0, bound, 1)).max()):.3f}")
        assert np.isfinite(got).all() and (err <= bound).all(), name
    assert (Amu < 0).all()
    assert (Av == 0.0).all() if v <= 1e-9 else (Av > 0)[t["u"][sel] < 30].all()


def test_exp_of_logei_is_ei(scalar):
    u = np.linspace(-9.0, 9.0, 721)
    par, v = -0.4, 0.81
    mu = par - u * 0.9
    Al, Amul, Avl = _acq(scalar, LOGEI, par, mu, np.full(u.size, v))
    Ae, Amue, Ave = _acq(scalar, 1, par, mu, np.full(u.size, v))
    rl = LB.transform(par, mu, v)
    re_ = FB.transform(FB.EI, par, LD(mu), LD(v), 0.0, 0.0)
    ei = np.exp(LD(Al))
    # exp(A +- E) = exp(A) (1 +- E): LogEI's bound scaled by EI, plus EI's own bound
    tol = np.exp(rl["A"]) * rl["E_A"] * FB.GUARD + re_["E_A"]
    assert (np.abs(ei - LD(Ae)) <= tol).all()
    # the chain-rule factors: d EI = EI d LogEI
    assert (np.abs(ei * LD(Amul) - LD(Amue)) <= np.exp(rl["A"]) * (rl["E_Amu"] + np.abs(rl["Amu"]) * rl["E_A"]) * FB.GUARD + re_["E_Amu"]).all()
    assert (np.abs(ei * LD(Avl) - LD(Ave)) <= np.exp(rl["A"]) * (rl["E_Av"] + np.abs(rl["Av"]) * rl["E_A"]) * FB.GUARD + re_["E_Av"]).all()


def test_nan_and_the_existing_codes(scalar):
    for out in _acq(scalar, LOGEI, 0.1, [float("nan"), float("nan")], [1.0, 0.0]):   # a NaN mean, above and on the floor
        assert np.isnan(out[0]) and (np.isnan(out[1]) or out[1] == 0.0)
    assert all(np.isnan(out[0]) for out in _acq(scalar, LOGEI, 0.1, [float("nan")], [1.0]))
    # UCB and EI: the statements they had (restated in numpy fp64: bit for bit with the same libm is not claimed, 4 ulp is)
    mu, var = np.array([0.3, -0.2, 5.0]), np.array([0.5, 2.0, 1e-12])
    A, Amu, Av = _acq(scalar, 0, 9.0, mu, var)
    assert np.allclose(A, np.sqrt(9.0 * var) - mu, rtol=1e-15) and (Amu == -1.0).all()
    A, _, Av = _acq(scalar, 1, 0.1, mu, var)
    assert Av[2] == 0.0 and A[2] == 0.0 and A[0] > 0


def test_refused_codes(scalar):
    for code in (0, 1, 17):
        assert scalar.emul_acqf_valid(code) == 1
    for code in (0x10, 0x12, 0x13, 2, 3, -1, 33):
        assert scalar.emul_acqf_valid(code) == 0
        for out in _acq(scalar, code, 0.1, [0.3], [1.0]):
            assert np.isnan(out).all()


def test_refused_codes_at_the_entry_points():
    """SCAML_ACQF_LOG alone, LOG | 2 and LOG | 3 at every entry point that takes `acqf` (the argument checks answer before any HIP call)."""
    from scamlgp_amd import _lib
    from tests import test_acqf_opt_abi, test_fantasy_abi, test_studies_acqf_abi, test_studies_fantasy_abi, test_studies_own_abi, test_studies_score_abi

    calls = (test_fantasy_abi._call, test_studies_acqf_abi._acqf, test_studies_score_abi._score, test_studies_fantasy_abi._acqf,
             test_studies_fantasy_abi._score, test_studies_fantasy_abi._opt, test_acqf_opt_abi._opt, test_studies_own_abi._opt)
    for fn in calls:
        for code in (0x10, 0x12, 0x13, 33):
            assert fn(acqf=code) == _lib.E_BADARG, (fn.__module__, fn.__name__, code)
    for code in (0x10, 0x12, 0x13, 2, 3, -1):
        assert _lib.lib.scaml_acqf_transform_f64(None, None, 0.1, 0, code, None, None, None, None) == _lib.E_BADARG
    assert _lib.lib.scaml_acqf_transform_f64(None, None, 0.1, 0, LOGEI, None, None, None, None) == 0      # M == 0 enqueues nothing
    assert _lib.lib.scaml_acqf_transform_f64(None, None, 0.1, -1, LOGEI, None, None, None, None) == _lib.E_BADARG


# ---- the log-domain average over fantasies in sa_block -------------------------------------------------------------------------
GROUPS = ((1, 1), (9, 2), (17, 64), (9, 64), (17, 2), (1, 2), (1, 64))   # n in {1, 9, 17} x F in {1, 2, 64}
NO_INFO = (0,) * 7


_log_ei_torch = LB.log_ei_torch


def _reference(prob, q, par):
    """tests/test_studies_fantasy_emul.Problem.reference with LogEI and the log of the mean EI."""
    s_ = int(prob.group[q])
    F = prob.FS[s_]
    x = prob.Xq[q:q + 1].clone().requires_grad_(True)
    act = [t for t in range(T) if prob.active[s_][t]]
    w, m, s, th = prob.w[s_], prob.m[s_], prob.s[s_], prob.theta[s_]
    mu_s = sum(w[t] * prob.mu_fn(t, x) for t in act).squeeze(0)
    var_s = sum(w[t] ** 2 * (prob.var_fn(t, x) + prob.off[q]) for t in act).squeeze(0)
    cov_s = sum(w[t] ** 2 * prob.cov_fn(t, s_, x) for t in act).squeeze(-1)
    Knq = cov_s / s ** 2 + _kernel(prob.Xt[s_], x, th, prob.kind).squeeze(-1)
    z = torch.cholesky_solve(Knq.unsqueeze(-1), prob.Lc[s_]).squeeze(-1)
    mu = m + s * ((mu_s - m) / s + Knq @ prob.alpha_f[s_][:, :F])
    var = s ** 2 * (var_s / s ** 2 + th[-2] - Knq @ z)
    l, u = _log_ei_torch(mu, var.expand_as(mu), par[s_])
    val = torch.logsumexp(l, 0) - math.log(F)
    (g,) = torch.autograd.grad(val, x)
    return float(val.detach()), g.squeeze(0).numpy(), l.detach().numpy(), u.detach().numpy(), mu.detach().numpy(), float(var.detach())


def _problem(case, kind, D=6):
    prob = Problem(D, kind, seed=500 + kind, groups=GROUPS)
    for s_, (n, F) in enumerate(GROUPS):
        a0 = prob.alpha_f[s_][:, :1]
        if case == "equal":
            c = torch.ones(F, dtype=torch.float64)
        elif case == "ahead":     # fantasy 0 against F - 1 identical others far away: on one side of it or the other, per query
            c = torch.cat([torch.ones(1, dtype=torch.float64), torch.full((F - 1,), 1e5, dtype=torch.float64)])
        else:                     # spread
            c = torch.linspace(-30.0, 30.0, F, dtype=torch.float64) if F > 1 else torch.ones(1, dtype=torch.float64)
        prob.alpha_f[s_] = (a0 * c).contiguous()
    return prob


def _run(lib, prob, a, strips=False, code=LOGEI):
    Mq, D = a["Xq"].shape
    out = dict(value=np.full(Mq, 7.0), grad=np.full((Mq, D), 7.0))
    rc = lib.emul_studies_fantasy(int(strips), *[_p(a[k]) for k in ORDER], Mq, prob.G, prob.n_max, a["alpha_f"].shape[2], T, D, prob.kind, code,
                                  _p(out["value"]), None if strips else _p(out["grad"]))
    assert rc == 0
    return out


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("case", ["equal", "ahead", "spread"])
def test_log_domain_average_over_fantasies(fantasy, case, kind):
    prob = _problem(case, kind)
    par = [prob.m[s_] + 0.2 for s_ in range(prob.G)]
    prob.param[LOGEI] = par
    a = prob.arrays(LOGEI, info=NO_INFO)
    out = _run(fantasy, prob, a)
    prob.param[FB.EI] = par
    out_ei = _run(fantasy, prob, prob.arrays(FB.EI, info=NO_INFO), code=FB.EI)   # the same statements up to sa_acquisition: the same mu_f, v
    seen = set()
    gaps, us = [], []
    ratio = 0.0
    for q in range(len(prob.group) - 1):
        s_ = int(prob.group[q])
        val, gr, l, u, mu_f, var_q = _reference(prob, q, par)
        F = prob.FS[s_]
        # the value to its counted bound, through the EI code on the same block: exp(log mean EI) is the mean EI.  Bounds at the
        # block's (mu_f, v) taken as exact -- both codes see the same ones --: LogEI's per-fantasy E_A through the weights plus the
        # average's own statements, scaled by the mean EI (exp(x +- E) = exp(x) (1 +- E)); EI's E_A and its F ordered additions.
        rl = LB.transform(par[s_], mu_f, var_q)
        ref_v, w, E_avg = LB.average(rl["A"])
        re_ = FB.transform(FB.EI, par[s_], LD(mu_f), LD(var_q), 0.0, 0.0)
        mean_ei = re_["A"].sum() / F
        if float(mean_ei) > 1e-290:   # (below, the EI code underflows; the torch comparison further down covers those queries)
            tol = np.exp(ref_v) * ((w * rl["E_A"]).sum() + E_avg) * FB.GUARD + (re_["E_A"].sum() + gamma(F) * np.abs(re_["A"]).sum()) / F + 2 * U * mean_ei
            err = np.abs(np.exp(LD(out["value"][q])) - LD(out_ei["value"][q]))
            ratio = max(ratio, float(err / tol))
            assert err <= tol, f"q={q} group {s_}: exp(LogEI value) {float(np.exp(LD(out['value'][q])))!r} against the EI code's {out_ei['value'][q]!r}, bound {float(tol):.3e}"
        if F > 1:
            top = np.sort(l)[::-1]
            gaps.append((top[0] - top[1], s_))
            us.append(u)
        assert np.isfinite(out["value"][q]) and np.isfinite(out["grad"][q]).all()
        np.testing.assert_allclose(out["value"][q], val, rtol=1e-9, atol=1e-9, err_msg=f"value q={q} group {s_}")
        np.testing.assert_allclose(out["grad"][q], gr, rtol=1e-6, atol=1e-9 * max(1.0, np.abs(gr).max()), err_msg=f"gradient q={q} group {s_}")
        if case == "equal":   # F equal fantasies: the value and gradient of one of them, to the roundings of the average
            one = dict(a, n_fant=np.ones_like(a["n_fant"]))
            if s_ not in seen:
                seen.add(s_)
                ref1 = _run(fantasy, prob, one)
            np.testing.assert_allclose(out["value"][q], ref1["value"][q], rtol=0, atol=float(LB.average(np.full(F, ref1["value"][q]))[2]) + 1e-300)
    print(f"{case} kind {kind}: exp(value) against the EI code, largest error / bound {ratio:.3f}")
    if case == "ahead":   # the others' weights are exactly 0 (exp underflows past 745) on queries of F = 2 and of F = 64 studies
        lead = {GROUPS[s_][1] for gap, s_ in gaps if gap > 745.0}
        assert lead == {2, 64}, sorted(lead)
    if case == "spread":
        allu = np.concatenate(us)
        assert allu.min() < -9.0 and allu.max() > 9.0
    # the strip layout (R = 16): the same values, bit for bit
    b, qs = _strip_arrays(a, prob.group)
    strip = _run(fantasy, prob, b, strips=True)
    assert np.array_equal(strip["value"], out["value"][qs], equal_nan=True)


def test_one_fantasy_is_the_ordinary_value_bit_for_bit(fantasy):
    """F_g = 1 takes the ordinary block's statements: sa_acquisition's LogEI at the block's own posterior, no average."""
    prob = Problem(6, 1, seed=41, groups=tuple((n, 1) for n, _ in GROUPS))
    prob.param[LOGEI] = [prob.m[s_] + 0.2 for s_ in range(prob.G)]
    a = prob.arrays(LOGEI, info=NO_INFO)
    out = _run(fantasy, prob, a)
    b = prob.arrays(LOGEI, info=NO_INFO, F_max=1)
    assert np.array_equal(_run(fantasy, prob, b)["value"], out["value"]) and np.isfinite(out["value"]).all()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("which", ["(8, 63, 3, 6)", "(96, 64, 3, 15)", "deep", "tiny"])
def test_long_double_reference_of_the_fantasy_kernel(which, kind):
    """tests/_logei_bounds.fantasy_reference (what the GPU tests hold (7f) to) against the independent torch-fp64 composition: they
    agree to the composition's own error (t^2 eps in 1 - t R(t): 2.3e-13 at t = 45; 1e-9 is asked), the reference's bounds are far
    below that, and a value without the log F term or a gradient whose Av_f are not weighted lies far outside the bound."""
    a = {"deep": lambda: FB.tail_inputs("deep", kind), "tiny": lambda: FB.clamp_inputs("tiny", FB.EI, kind)}.get(
        which, lambda: FB.inputs(*eval(which), kind, FB.EI))()
    ref = LB.fantasy_reference(a)
    FB.conditions(which, ref)
    value, grad, u = LB.composition(a)
    value, grad = value.numpy(), grad.numpy()
    assert np.abs(u.numpy() - ref["u"].astype(np.float64)).max() <= 1e-9 * (1 + np.abs(u.numpy()).max())
    for name, got in (("value", value), ("grad", grad)):
        q = ref[name]
        assert float((q.bound / q.scale).max()) <= 1e-10
        assert float(np.abs(LD(got) - q.ref).max()) <= 1e-9 * q.scale, name
    F = a["F"]
    if F > 1:
        assert (np.abs(math.log(F)) > 1e3 * ref["value"].bound).all()                      # the log F term omitted
        plain = dict(a, var_g=a["var_g"] + 1.0)                                              # the gradient's sAv, seen through var_g
        d = LB.fantasy_reference(plain)["grad"].ref - ref["grad"].ref                        # = sum_f w_f Av_f per query
        live = np.abs(d) > 0
        assert (np.abs(d[live]) * (F - 1) > 1e3 * ref["grad"].bound[live]).all()             # unweighted: F times as much
