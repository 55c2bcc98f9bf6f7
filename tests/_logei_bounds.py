"""Reference and a-priori error budget of LogEI (sa_log_ei_terms / sa_acquisition with code 17, csrc/gp_studies_formulas.h).

Reference: tests/golden/logei/logei_scalar_table.npz (tests/golden/make_logei_table.py: mpmath, 50 digits, (hi, lo) float64 pairs) for the
scalar function at the table's points; anywhere else `g_ld`, long double: u >= -1 the direct formula (phi + u Phi loses at most a
factor 5 of eps_LD there, erf by tests/_fantasy_bounds.erf_ld), u < -1 the FACTORED form with the continued fraction of the Mills
ratio evaluated backwards with 4,000 terms (its truncation at t = 1 is below 1e-30).  No long-double pdf + u cdf past |u| = 1.

Budget, first order, in units of u = 2^-53, counted from the statements (x_k: the recurrence, K = x_1, r = K / (t + K)):
  u < -2   e_K(t): e_k = 2 + c_k e_{k+1}, c_k = x_{k+1} / (t + x_{k+1}) < 1 (the sum t + x, the quotient; (double)k is exact), from
           e_{N+1} = 4 (the tail: fma, root, difference, halving) + TRUNC, TRUNC = 1/16 (the truncation left by the term counts, below
           2^-57 K: measured against the table at each range's lower end, where it is largest);  computed here by the same recurrence.
           g:  t^2 / 2 (the product) + (t^2 / 2 + c) (the difference) + c / 2 (the constant) + 2 e_K + 2 (r) + LOG_U |log r| + |g|
           g' = 1 / K:  e_K + 1;    om = (t + K) / K:  2 e_K + 2
  u >= -2  pdf:  e_pdf = u^2 / 2 + EXP_U + 3/2;   cdf:  e_cdf = 3/2 kappa(y) + ERFC_U, y = -u / sqrt 2, kappa = |y erfc'(y) / erfc(y)|
           h = fma(u, cdf, pdf):  e_h = (pdf e_pdf + |u| cdf e_cdf) / h + 1  -- the cancellation (phi + |u| Phi) / (phi + u Phi) for u < 0
           g = log h:  e_h + LOG_U |g|;    g' = cdf / h:  e_cdf + e_h + 1;    om = pdf / h:  e_pdf + e_h + 1 (and 2^-1022 / h absolute:
           pdf underflows past u = 37.6)
The contract: budget_g <= 256 (1 + |g|) and budget_gp <= 256 |g'| on [-1e8, 40] (asserted on the table by tests/test_logei_bounds.py).
EXP_U as tests/_fantasy_bounds.py; ERFC_U, LOG_U by the same rule from tools/libm_ulp_probe.hip in its "logei" mode
(profiles/logei_bounds_notes.md)."""
from __future__ import annotations

import math
import os

import numpy as np

from tests import _fantasy_bounds as FB
from tests._posterior_bounds import LD, U

LOGEI = 17
EXP_U = FB.EXP_U
ERFC_U = 6     # erfc: 2.7031 ulp at worst over [-29, 1.4143] (at x = 1.324), measured on the MI355X: profiles/logei_bounds_notes.md
LOG_U = 2      # log: 0.6265 ulp at worst over [1e-20, 100]
TRUNC = 1.0 / 16
CAP_UNITS = 256.0
EDGES = (-2.0, -3.0, -5.0, -8.0, -16.0)
TERMS = (112, 72, 36, 20, 12)
LOG_SQRT_2PI = LD(0.5) * np.log(LD(2) * FB.PI)
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logei", "logei_scalar_table.npz")


def table():
    t = np.load(TABLE)
    return dict(u=t["u"], g=LD(t["g"][:, 0]) + LD(t["g"][:, 1]), gp=LD(t["gp"][:, 0]) + LD(t["gp"][:, 1]), edges=t["edges"], named=t["named"])


def g_ld(u):
    """(g, g', om = 1 - u g') in long double; NaN passes through."""
    u = np.asarray(u, dtype=LD)
    with np.errstate(all="ignore"):
        t = np.where(u < -1, -u, LD(1))
        x = np.zeros_like(t)
        for k in range(4000, 0, -1):
            x = k / (t + x)
        tk = t + x
        g_cf, gp_cf, om_cf = -t * t / 2 - LOG_SQRT_2PI + np.log(x / tk), 1 / x, tk / x
        ud = np.where(u < -1, LD(0), u)
        pdf = np.exp(-ud * ud / 2) * FB._INV_SQRT_2PI
        cdf = (1 + FB.erf_ld(ud / FB._SQRT2)) / 2
        h = pdf + ud * cdf
        cf = u < -1
        return np.where(cf, g_cf, np.log(h)), np.where(cf, gp_cf, cdf / h), np.where(cf, om_cf, pdf / h)


def _terms(t):
    return np.select([t < 3, t < 5, t < 8, t < 16], TERMS[:4], TERMS[4])


def budgets(u):
    """(budget_g, budget_gp, budget_om) in units of 2^-53: absolute for g, relative for g' and om (om also has 2^-1022 / h absolute)."""
    u = np.asarray(u, dtype=np.float64)
    bg, bgp, bom = np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    g, gp, _ = g_ld(u)
    g, gp = np.abs(g).astype(np.float64), gp.astype(np.float64)
    cfm = u < -2
    if cfm.any():
        t = -u[cfm]
        N = _terms(t)
        x = 0.5 * (np.sqrt(t * t + 4.0 * (N + 1)) - t)
        e = np.full_like(t, 4.0 + TRUNC)
        for k in range(int(N.max()), 0, -1):
            on = k <= N
            e = np.where(on, 2.0 + x / (t + x) * e, e)
            x = np.where(on, k / (t + x), x)
        c = float(LOG_SQRT_2PI)
        logr = np.abs(np.log(x / (t + x)))
        bg[cfm] = t * t / 2 + (t * t / 2 + c) + c / 2 + 2 * e + 2 + LOG_U * logr + g[cfm]
        bgp[cfm] = e + 1
        bom[cfm] = 2 * e + 2
    d = ~cfm
    if d.any():
        ud = u[d]
        y = -ud / math.sqrt(2.0)
        pdf = np.exp(-ud * ud / 2) / math.sqrt(2 * math.pi)
        erfc = np.array([math.erfc(v) for v in y])
        kappa = np.abs(y) * (2 / math.sqrt(math.pi)) * np.exp(-y * y) / erfc
        cdf = erfc / 2
        e_pdf, e_cdf = ud * ud / 2 + EXP_U + 1.5, 1.5 * kappa + ERFC_U
        h = pdf + ud * cdf
        e_h = (pdf * e_pdf + np.abs(ud) * cdf * e_cdf) / h + 1
        bg[d] = e_h + LOG_U * g[d]
        bgp[d] = e_cdf + e_h + 1
        bom[d] = e_pdf + e_h + 1
    return bg, bgp, bom


def transform(par, mu, v):
    """sa_acquisition with code 17 at exact (mu, v) in long double: A, Amu, Av with their first-order bounds (absolute).  sigma: the
    root (1 u); uu = -(mu - par) / sigma: 3 u relative (difference, sigma, quotient) -> E_u = 3 u |uu|, which reaches g through g' and
    g', om through their slopes (|g''| <= 1, |om'| <= |g'| + |u g''|: bounded with |g'| (1 + |u|) + 1 for both);  A = log sigma + g:
    LOG_U u |log sigma| + u / 2 (sigma's error through the logarithm) + the budget of g + u |A|;  Amu = -g' / sigma: budget + 2 u;
    Av = (om / 2) / sigma^2: budget + 3 u, exactly 0 on the floor."""
    mu, v = np.broadcast_arrays(LD(mu), LD(v))
    live = v > LD(1e-9)
    with np.errstate(all="ignore"):
        sigma = np.sqrt(np.where(live, v, LD(1e-9)))
        uu = -(mu - LD(par)) / sigma
        g, gp, om = g_ld(uu)
        bg, bgp, bom = budgets(np.nan_to_num(uu.astype(np.float64), nan=0.0))
        E_u = 3 * U * np.abs(uu)
        slope = np.abs(gp) * (1 + np.abs(uu)) + 1
        A = np.log(sigma) + g
        E_A = U * (LOG_U * np.abs(np.log(sigma)) + 0.5 + bg + np.abs(A)) + np.abs(gp) * E_u
        Amu = -gp / sigma
        E_Amu = (U * (bgp + 2) * np.abs(gp) + slope * E_u) / sigma
        Av = np.where(live, om / (2 * sigma * sigma), 0)
        E_Av = np.where(live, (U * (bom + 3) * np.abs(om) + slope * E_u + LD(2) ** -1022) / (2 * sigma * sigma), 0)
    return dict(A=A, Amu=Amu, Av=Av, E_A=FB.GUARD * E_A, E_Amu=FB.GUARD * E_Amu, E_Av=FB.GUARD * E_Av, u=uu)


def average(l):
    """The log-domain average over the last axis in long double, log(mean exp l), the weights, and the bound of the value the
    kernels' statements leave for EXACT l: F differences and exponentials (EXP_U + 1 each, relative in S), F - 1 additions, two
    logarithms, two additions:  u ((EXP_U + F + 1) + LOG_U (|log S| + log F) + 2 |value| + |mx|)."""
    l = LD(l)
    F = l.shape[-1]
    mx = l.max(-1, keepdims=True)
    e = np.exp(l - mx)
    S = e.sum(-1, keepdims=True)
    value = (mx + np.log(S) - np.log(LD(F)))[..., 0]
    E = U * ((EXP_U + F + 1) + LOG_U * (np.abs(np.log(S[..., 0])) + math.log(F)) + 2 * np.abs(value) + np.abs(mx[..., 0]))
    return value, e / S, FB.GUARD * E


# ---- (7f) with code 17: scaml_target_fantasy_acqf_f64 fed exactly its arrays ------------------------------------------------------
def transform_e(par, mu, v, E_mu, E_v):
    """`transform` at a posterior that carries the errors E_mu, E_v of the kernel's own mu_f and v (tests/_fantasy_bounds.py: the
    finish's chains), first order.  sigma and u_f as EI has them there:  E_sigma = sigma (E_v / (2 v) + u), on the floor sigma u;
    E_u = (E_mu + u |mu - best_f|) / sigma + |u_f| (E_sigma / sigma + u).  E_u reaches g through g', and g', om through their slopes:
    g'' = om - g'^2 lies in (-1, 0) (EI is log-concave), so |g''| <= 1 and |om'| = |g' + u g''| <= |g'| + |u|.
      A = log sigma + g:   u (LOG_U |log sigma| + budget_g + |A|) + E_sigma / sigma + |g'| E_u
      Amu = -g' / sigma:   (u (budget_g' + 2) |g'| + E_u) / sigma + |Amu| E_sigma / sigma
      Av = (om / 2) / sigma^2:  (u (budget_om + 3) |om| + (|g'| + |u_f|) E_u + 2^-1022) / (2 sigma^2) + 2 Av E_sigma / sigma, 0 on the floor
    eps (the second-order measure of tests/_fantasy_bounds.conditions): max(E_v / v, E_sigma / sigma, E_u)."""
    mu, v, E_mu, E_v = np.broadcast_arrays(LD(mu), LD(v), LD(E_mu), LD(E_v))
    thr = LD(1e-9)
    with np.errstate(all="ignore"):
        live = v > thr
        rel_v = np.where(live, E_v / np.where(live, v, 1), 0)
        margin = np.where(E_v > 0, np.abs(v - thr) / np.where(E_v > 0, E_v, 1), np.inf)
        sigma = np.sqrt(np.where(live, v, thr))
        rel_sig = rel_v / 2 + U
        d = mu - LD(par)
        uu = -d / sigma
        au = np.abs(uu)
        E_u = (E_mu + U * np.abs(d)) / sigma + au * (rel_sig + U)
        g, gp, om = g_ld(uu)
        bg, bgp, bom = budgets(np.nan_to_num(uu.astype(np.float64), nan=0.0))
        A = np.log(sigma) + g
        E_A = U * (LOG_U * np.abs(np.log(sigma)) + bg + np.abs(A)) + rel_sig + np.abs(gp) * E_u
        Amu = -gp / sigma
        E_Amu = (U * (bgp + 2) * np.abs(gp) + E_u) / sigma + np.abs(Amu) * rel_sig
        Av = np.where(live, om / (2 * sigma * sigma), 0)
        E_Av = np.where(live, (U * (bom + 3) * np.abs(om) + (np.abs(gp) + au) * E_u + LD(2) ** -1022) / (2 * sigma * sigma) + 2 * Av * rel_sig, 0)
        eps = np.maximum(np.maximum(rel_v, rel_sig), E_u)
    return dict(A=A, Amu=Amu, Av=Av, E_A=FB.GUARD * E_A, E_Amu=FB.GUARD * E_Amu, E_Av=FB.GUARD * E_Av, eps=eps, margin=margin, u=uu)


def fantasy_reference(a: dict) -> dict:
    """tests/_fantasy_bounds.fantasy_reference for code 17 (a["acqf"] is not read; a["param"] is best_f): the same long-double
    posterior, kernel slopes and contractions with their counted bounds, and in place of the mean over the fantasies
      l_f = A_f,  value = log(mean_f exp l_f) by `average`:  E_value = sum_f w_f E_A_f (d value / d l_f = w_f) + average's own bound
      w_f = exp(l_f - mx) / S:  d w_f = w_f (d l_f - sum_j w_j d l_j), the exponential (EXP_U + 1), S (EXP_U + 1 + F: the exponentials
            and the additions, wave or sequential), the quotient (1), and 2^-1074 / S where the exponential is subnormal:
            E_w_f = w_f (E_A_f + sum_j w_j E_A_j + u (2 EXP_U + F + 4)) + 2^-1074 / S
      Amu_f w_f, Av_f w_f:  E = E_A. w_f + |A.| E_w_f + u |A. w_f|
    and from there on sAmu, sAv, abar, gm, gv and grad as there, with these weighted factors and the divisor 1."""
    from tests import _target_bounds as B
    from tests._posterior_bounds import Quantity, _kernel, _S, gamma

    n, M, F = a["n"], a["M"], a["F"]
    s, m, noise = LD(a["s"]), LD(a["m"]), LD(a["noise_add"])
    s2 = s * s
    Knq, Z, al = LD(a["Knq"][:n]), LD(a["Z"][:n]), LD(a["alpha"][:n])
    mean_q, var_q = LD(a["mean_q"]), LD(a["var_q"])
    g = gamma(n + 3)
    aK, aZ, aal = np.abs(Knq), np.abs(Z), np.abs(al)
    with np.errstate(all="ignore"):
        v = s2 * (var_q - (Knq * Z).sum(0) + noise)
        E_v = s2 * g * (np.abs(var_q) + (aK * aZ).sum(0) + np.abs(noise)) + 3 * U * np.abs(v)
        mu = m + s * (mean_q[:, None] + Knq.T @ al)
        E_mu = s * g * (np.abs(mean_q)[:, None] + aK.T @ aal) + 2 * U * np.abs(mu)
        t = transform_e(a["param"], mu, v[:, None], E_mu, E_v[:, None])
        value, w, E_avg = average(t["A"])
        E_value = FB.GUARD * (w * t["E_A"]).sum(1) + E_avg
        S = np.exp(t["A"] - t["A"].max(1, keepdims=True)).sum(1, keepdims=True)
        E_w = FB.GUARD * (w * (t["E_A"] + (w * t["E_A"]).sum(1, keepdims=True) + U * (2 * EXP_U + F + 4)) + FB._TINY / S)
        Amu, Av = t["Amu"] * w, t["Av"] * w
        E_Amu = t["E_Amu"] * w + np.abs(t["Amu"]) * E_w + U * np.abs(Amu)
        E_Av = t["E_Av"] * w + np.abs(t["Av"]) * E_w + U * np.abs(Av)
    sig = np.sqrt(np.maximum(v[np.isfinite(v)], 1e-9))
    out = dict(value=Quantity(value, E_value, B._scale(value)), eps=t["eps"], margin=t["margin"], u=t["u"], v=v, w=w,
               sigma=float(sig.max()) if sig.size else 0.0)
    if not a.get("grad"):
        return out
    D, kind = a["D"], a["kind"]
    th = a["theta"]
    l, os_ = LD(th[:D]), LD(th[D])
    S1 = _S[kind][1]
    with np.errstate(all="ignore"):
        sAmu, sAv = Amu.sum(1), Av.sum(1)
        E_sAmu = E_Amu.sum(1) + gamma(max(6, F)) * np.abs(Amu).sum(1)
        E_sAv = E_Av.sum(1) + gamma(max(6, F)) * np.abs(Av).sum(1)
        ab = Amu @ al.T
        E_ab = E_Amu @ aal.T + gamma(F) * (np.abs(Amu) @ aal.T)
        df = (LD(a["Xq"])[None, :, :] - LD(a["Xt"][:n])[:, None, :]) / l
        d2 = (df * df).sum(-1)
        dk = _kernel(d2, kind)[1]
        E_dk = os_ * (S1 * gamma(D + 6) * d2 + 4 * U * np.abs(dk))
        c = 2 * os_ * dk[:, :, None] * df / l
        E_c = 2 * E_dk[:, :, None] * np.abs(df / l) + 7 * U * np.abs(c)
        cg = LD(a["cov_g"][:n]).reshape(n, M, 16)[:, :, 1:1 + D] / s2
        dkn = cg + c
        E_dkn = E_c + 2 * U * np.abs(cg) + U * np.abs(dkn)
        adkn = np.abs(dkn)
        gch = gamma((n + 63) // 64 + 8)
        gm, gv = np.einsum("qa,aqd->qd", ab, dkn), np.einsum("aq,aqd->qd", Z, dkn)
        E_gm = np.einsum("qa,aqd->qd", np.abs(ab), E_dkn) + np.einsum("qa,aqd->qd", E_ab, adkn) + gch * np.einsum("qa,aqd->qd", np.abs(ab), adkn)
        E_gv = np.einsum("aq,aqd->qd", aZ, E_dkn) + gch * np.einsum("aq,aqd->qd", aZ, adkn)
        mu_g = LD(a["mu_g"]).reshape(M, 16)[:, 1:1 + D]
        var_g = LD(a["var_g"]).reshape(M, 16)[:, 1:1 + D]
        t1 = sAmu[:, None] * mu_g
        gmu = t1 + s * gm
        E_gmu = E_sAmu[:, None] * np.abs(mu_g) + s * E_gm + 2 * U * (np.abs(t1) + s * np.abs(gm))
        gvar = var_g - 2 * s2 * gv
        E_gvar = 2 * s2 * E_gv + 3 * U * (np.abs(var_g) + 2 * s2 * np.abs(gv))
        t2 = sAv[:, None] * gvar
        grad = gmu + t2
        E_grad = FB.GUARD * (E_gmu + E_sAv[:, None] * np.abs(gvar) + np.abs(sAv)[:, None] * E_gvar + U * (np.abs(gmu) + np.abs(t2))
                             + 2 * U * np.abs(grad))
    out["grad"] = Quantity(grad, E_grad, B._scale(grad))
    return out


def hold(label, a, ref, value, grad, gmask=None):
    """tests/_fantasy_bounds._hold for code 17: the conditions on the inputs, then every element inside its bound (the bound itself at
    most CAP of the output's largest reference magnitude); the ratios go to the table of tests/_target_bounds.report."""
    from tests._target_bounds import FAMILY, within

    FB.conditions(label, ref)
    fam = FAMILY[a["kind"]]
    within(label, ("fantasy_acqf", f"{fam}/logei", "value"), value, ref["value"])
    within(label, ("fantasy_acqf", f"{fam}/logei", "grad"), grad, ref["grad"], gmask)


# ---- a second, independent statement in torch fp64 (it checks the long-double reference above, not the kernels) --------------------
def log_ei_torch(mu, var, par):
    """LogEI and u in torch fp64, differentiable: u < -1 by the scaled complementary error function, log1p(-t sqrt(pi / 2)
    erfcx(t / sqrt 2)), whose own error grows like t^2 eps; the direct formula above."""
    import torch

    sigma = var.clamp_min(1e-9).sqrt()
    u = -(mu - par) / sigma
    t = (-u).clamp_min(1.0)
    tail = -0.5 * t * t - 0.5 * math.log(2 * math.pi) + torch.log1p(-t * math.sqrt(math.pi / 2) * torch.special.erfcx(t / math.sqrt(2.0)))
    uc = u.clamp_min(-1.0)
    direct = torch.log(torch.exp(-0.5 * uc * uc) / math.sqrt(2 * math.pi) + uc * 0.5 * torch.erfc(-uc / math.sqrt(2.0)))
    return torch.log(sigma) + torch.where(u < -1.0, tail, direct), u


def composition(a):
    """(7f)'s formulas in torch fp64 on the CPU: log of the mean EI over the fantasies, the weighted chain-rule factors by autograd
    through (mu_f, v), the input gradient from them as the kernel forms it.  -> value (M), grad (M, D), u (M, F)."""
    import torch

    T_ = lambda x: torch.from_numpy(np.ascontiguousarray(x))   # noqa: E731
    Knq, Z, alpha, s, m = T_(a["Knq"]), T_(a["Z"]), T_(a["alpha"]), a["s"], a["m"]
    n, M, F, D = a["n"], a["M"], a["F"], a["D"]
    mu = (m + s * (T_(a["mean_q"]).unsqueeze(1) + Knq.T @ alpha)).requires_grad_(True)
    v = (s * s * (T_(a["var_q"]) - (Knq * Z).sum(0) + a["noise_add"])).requires_grad_(True)
    l, u = log_ei_torch(mu, v.unsqueeze(1).expand_as(mu), a["param"])
    value = torch.logsumexp(l, 1) - math.log(F)
    value.sum().backward()
    th = T_(a["theta"])
    Xq, Xt = T_(a["Xq"]), T_(a["Xt"])
    diff = (Xq.unsqueeze(0) - Xt.unsqueeze(1)) / th[:D] ** 2
    r2 = (((Xq.unsqueeze(0) - Xt.unsqueeze(1)) / th[:D]) ** 2).sum(-1)
    if a["kind"] == 0:
        dk = -th[D] * torch.exp(-0.5 * r2).unsqueeze(-1) * diff
    else:
        r = r2.sqrt()
        dk = -th[D] * (5.0 / 3.0) * ((1 + math.sqrt(5.0) * r) * torch.exp(-math.sqrt(5.0) * r)).unsqueeze(-1) * diff
    dkn = T_(a["cov_g"]).reshape(n, M, 16)[:, :, 1:1 + D] / (s * s) + dk
    dmu = T_(a["mu_g"]).reshape(M, 16)[:, 1:1 + D].unsqueeze(1) + s * torch.einsum("af,aqd->qfd", alpha, dkn)
    dvar = T_(a["var_g"]).reshape(M, 16)[:, 1:1 + D] - 2 * s * s * torch.einsum("aq,aqd->qd", Z, dkn)
    grad = (mu.grad.unsqueeze(-1) * dmu).sum(1) + v.grad.unsqueeze(-1) * dvar
    return value.detach(), grad, u.detach()
