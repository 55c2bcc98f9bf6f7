"""Long-double reference, a-priori forward error bound, input sets and shared assertions for scaml_target_fantasy_acqf_f64 ((7f) in
include/scaml_gp.h, csrc/gp_fantasy.hip): the acquisition value averaged over F fantasies and its input gradient.

Same construction as tests/_target_bounds.py (whose helpers are used here).  The reference is numpy long double on plain (M, F) and
(n, M, D) tensors, fed exactly the arrays the entry point is handed; long-double erf by the all-positive series
erf(x) = 2 / sqrt(pi) exp(-x^2) sum_k 2^k x^(2k+1) / (2k+1)!!  (400 terms on [-6.5, 6.5], +-1 beyond: erfc(6.5) = 3.8e-20 < eps_LD).
Only `value` and `grad` leave the kernel, so the bound is first order through the acquisition transform, every term evaluated from
the reference's own quantities, every constant counted from the kernel's statements.  With u = 2^-53, g_k = k u / (1 - k u), per query:

  kz, v, mu_f    E_v, E_mu of the finish (tests/_target_bounds.py), E_v once per query, E_mu per fantasy: their g_{n+3} chains
                 cover this kernel's (kz: ceil(n/64) fmas and at most min(6, n - 1) rounding levels of the wave sum, then the
                 subtraction and the sum; mu_f: n sequential fmas from mean_q, then one fma with s and m)
  UCB            sd = sqrt(beta max(v, 0)):  E_sd = sd (E_v / (2 v) + 2 u)   (the product, the root)
                 A = sd - mu:  E_A = E_sd + E_mu + u |A|;   Amu = -1 exactly;   Av = (beta / 2) / max(sd, 1e-300) where v > 0, else
                 exactly 0:  E_Av = Av (E_sd / sd + 3 u)
  EI             sigma = sqrt(max(v, 1e-9)):  E_sigma = sigma (E_v / (2 v) + u), on the floor sigma u
                 u_f = -(mu - best_f) / sigma:  E_u = (E_mu + u |mu - best_f|) / sigma + |u_f| (E_sigma / sigma + u)
                 pdf = exp(-u_f^2 / 2) c:  E_pdf = pdf (|u_f| E_u + u (u_f^2 / 2 + 2)) + EXP_U u pdf + 2^-1074
                 cdf = (1 + erf(u_f / sqrt 2)) / 2:  E_cdf = pdf (E_u + 2 u |u_f|) + ERF_U u |erf| / 2 + u (1 + |erf|) / 2
                 A = sigma (pdf + u_f cdf), the bound taken in the formulation (the tail cancellation belongs to the formula):
                 E_A = sigma (E_pdf + |u_f| E_cdf + cdf E_u + g_2 (pdf + |u_f cdf|)) + E_sigma |pdf + u_f cdf| + u |A|
                 Amu = -cdf: E_Amu = E_cdf;   Av = pdf / (2 sigma) above the floor, else exactly 0:
                 E_Av = E_pdf / (2 sigma) + Av (E_sigma / sigma + 3 u)
  value          (sum_f E_A + g_8 sum_f |A_f|) / F + 2 u |value|
  sAmu, sAv      sum_f E + g_6 sum_f |.|   (the wave sums)
  abar_a         sum_f E_Amu_f |alpha[a, f]| + g_F sum_f |Amu_f alpha[a, f]|
  dkn            df = (x_q - x_a) il (il = 1 / l: three roundings), d2 = sum_d df^2 by D fmas: E_d2 = g_{D+6} d2;
                 E_dk = os (S1 E_d2 + 4 u |dk|) (S1, the 4 u of the evaluation: tests/_posterior_bounds.py);  c = 2 dk (df il): six
                 roundings besides dk's own: E_c = 2 E_dk |df il| + 7 u |c|;  dkn = fma(cov_g, 1 / s^2, c): E_dkn = E_c + 2 u |cov_g / s^2|
                 + u |dkn|
  gm, gv         sum_a (|ab| E_dkn + E_ab |dkn|) + g_{ceil(n/64)+8} sum_a |ab dkn|;  gv with z in place of ab, E_z = 0
  grad           gmu = sAmu mu_g + s gm:  E_gmu = E_sAmu |mu_g| + s E_gm + 2 u (|sAmu mu_g| + s |gm|)
                 gvar = var_g - 2 s^2 gv:  E_gvar = 2 s^2 E_gv + 3 u (|var_g| + 2 s^2 |gv|)
                 grad = (gmu + sAv gvar) / F:  (E_gmu + E_sAv |gvar| + |sAv| E_gvar + u (|gmu| + |sAv gvar|)) / F + 2 u |grad|

Second order: every bound is multiplied by 1 / (1 - 1e-6), and eps = max(E_v / v, (1 + min(|u_f|, 40)) E_u, E_sigma / sigma) <= 1e-6 is asserted
on the inputs.  Math library: sqrt 1 u; EXP_U and ERF_U are measured on the device library itself (tools/libm_ulp_probe.hip, read by
tools/libm_ulp_read.py; figures in profiles/fantasy_bounds_notes.md), ERF_U = max(2, ceil(2 x largest observed ulp error)).

Conditions on the inputs, asserted with every comparison: each bound at most CAP = 1e-8 of the output's largest reference magnitude
in the call, and v at least 1e3 E_v away from the clamp (0 for UCB, 1e-9 for EI) on whichever side it lies.  (One set has an
all-zero reference -- EI with every u_f <= -40 --: its cap is taken against sigma, the magnitude of A's factor.)

Input sets (shapes read off the kernel: phases (1) and (3) stride by 64 lanes, phase (2) reads alpha in chunks of 8 rows with an
a0 + u < n guard, lanes >= F are zeroed after the transform):
  value + gradient, both families, both acquisition functions: (n, F, M, D) in GRAD_SHAPES; on (65, 63, 130, 6) query 0 ON a training
  point, query 1 1e-7 from one, two identical training rows;  value only: VALUE_SHAPES
  clamps on (9, 64, 3, 15): v = -0.01, v = 5e-10 (EI), v == 0 exactly, beta = 0 (UCB) for queries 0 and 2 -- the clamped partial
  exactly absent (the gradient does not change by a bit when var_g does)
  EI tails: u_f spanning -9 .. +9 within one call (65, 63, 130, 6); every u_f <= -40 (9, 64, 3, 15)
  info NULL / 0 / 2; the refusals of REFUSALS; non-finite queries (a NaN / infinite coordinate; a NaN column of Knq and Z; of Knq alone)
  chain: tests/_target_bounds.check_chain extended by the solve with R = F for alpha (n, F) and the fantasy kernel on the
  backend's own upstream outputs (n = 17 = 14 observed + 3 pending, F = 5)
"""
from __future__ import annotations

import numpy as np

from tests import _target_bounds as B
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, SENTINEL, U, Quantity, _kernel, _S, gamma
from tests._target_bounds import E_TOOLARGE, FAMILY, within

E_BADARG = -1
UCB, EI = 0, 1
ACQ = {UCB: "ucb", EI: "ei"}
# measured on the MI355X's device library (profiles/fantasy_bounds_notes.md, "The math library"): the constants are
# max(2, ceil(2 x largest observed ulp error)), the factor 2 because the sweep samples the domain
EXP_U = 2      # exp: 0.8613 ulp at worst over [-745, 0] (subnormal results within 0.85 x 2^-1074)
ERF_U = 3      # erf: 1.0205 ulp at worst over [-6.5, 6.5]
SECOND_ORDER = 1e-6
GUARD = 1.0 / (1.0 - SECOND_ORDER)
MARGIN = 1e3

PI = LD(4) * np.arctan(LD(1))
_TWO_OVER_SQRT_PI = LD(2) / np.sqrt(PI)
_INV_SQRT_2PI = LD(1) / np.sqrt(LD(2) * PI)
_SQRT2 = np.sqrt(LD(2))
_TINY = LD(2) ** -1074
ERF_TERMS = 400


def erf_ld(x):
    """erf in long double (relative error a few eps_LD; NaN passes through)."""
    x = np.asarray(x, dtype=LD)
    with np.errstate(invalid="ignore"):
        xc = np.clip(x, -6.5, 6.5)
        x2 = xc * xc
        term, tot = xc.copy(), xc.copy()
        for k in range(ERF_TERMS):
            term = term * (2 * x2 / (2 * k + 3))
            tot = tot + term
        r = _TWO_OVER_SQRT_PI * np.exp(-x2) * tot
        return np.where(np.abs(x) > 6.5, np.sign(x), r)


def transform(acqf, par, mu, v, E_mu, E_v):
    """The acquisition transform of csrc/gp_fantasy.hip / csrc/gp_studies_formulas.h in long double with its first-order bound:
    mu, v, E_mu, E_v broadcastable long-double arrays -> dict of A, Amu, Av, their bounds, eps (the second-order measure) and margin
    (|v - clamp| / E_v, inf where E_v is 0)."""
    mu, v, E_mu, E_v = np.broadcast_arrays(LD(mu), LD(v), LD(E_mu), LD(E_v))
    par = LD(par)
    thr = LD(0.0) if acqf == UCB else LD(1e-9)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        live = v > thr
        vc = np.where(live, v, thr)
        rel_v = np.where(live, E_v / np.where(live, v, 1), 0)
        margin = np.where(E_v > 0, np.abs(v - thr) / np.where(E_v > 0, E_v, 1), np.inf)
        if acqf == UCB:
            sd = np.sqrt(par * vc)
            rel_sd = rel_v / 2 + 2 * U
            A = sd - mu
            E_A = sd * rel_sd + E_mu + U * np.abs(A)
            Amu, E_Amu = -np.ones_like(mu), np.zeros_like(mu)
            Av = np.where(live, par / 2 / np.maximum(sd, LD(1e-300)), 0)
            E_Av = Av * (rel_sd + 3 * U)
            eps, uu = rel_v, np.zeros_like(mu)
        else:
            sigma = np.sqrt(vc)
            rel_sig = rel_v / 2 + U
            E_sig = sigma * rel_sig
            d = mu - par
            uu = -d / sigma
            au = np.abs(uu)
            E_u = (E_mu + U * np.abs(d)) / sigma + au * (rel_sig + U)
            pdf = np.exp(-uu * uu / 2) * _INV_SQRT_2PI
            erf = erf_ld(uu / _SQRT2)
            cdf = (1 + erf) / 2
            E_pdf = pdf * (au * E_u + U * (uu * uu / 2 + 2)) + EXP_U * U * pdf + _TINY
            E_cdf = pdf * (E_u + 2 * U * au) + ERF_U * U * np.abs(erf) / 2 + U * (1 + np.abs(erf)) / 2
            core = pdf + uu * cdf
            A = sigma * core
            E_A = sigma * (E_pdf + au * E_cdf + cdf * E_u + gamma(2) * (pdf + np.abs(uu * cdf))) + E_sig * np.abs(core) + U * np.abs(A)
            Amu, E_Amu = -cdf, E_cdf
            Av = np.where(live, pdf / (2 * sigma), 0)
            E_Av = np.where(live, E_pdf / (2 * sigma) + Av * (rel_sig + 3 * U), 0)
            eps = np.maximum(np.maximum(rel_v, (1 + np.minimum(au, 40)) * E_u), rel_sig)   # (|u_f| E_u: the exponent of pdf, 0 past 40)
    return dict(A=A, Amu=Amu, Av=Av, E_A=GUARD * E_A, E_Amu=GUARD * E_Amu, E_Av=GUARD * E_Av, eps=eps, margin=margin, u=uu)


def fantasy_reference(a: dict) -> dict:
    """a: the arguments of scaml_target_fantasy_acqf_f64 (numpy; a["grad"]: with the gradient) -> value / grad Quantities, and the
    conditions eps / margin / u of the transform."""
    n, M, F = a["n"], a["M"], a["F"]
    s, m, noise = LD(a["s"]), LD(a["m"]), LD(a["noise_add"])
    s2 = s * s
    Knq, Z, al = LD(a["Knq"][:n]), LD(a["Z"][:n]), LD(a["alpha"][:n])
    mean_q, var_q = LD(a["mean_q"]), LD(a["var_q"])
    g = gamma(n + 3)
    aK, aZ, aal = np.abs(Knq), np.abs(Z), np.abs(al)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = s2 * (var_q - (Knq * Z).sum(0) + noise)                                       # (M)
        E_v = s2 * g * (np.abs(var_q) + (aK * aZ).sum(0) + np.abs(noise)) + 3 * U * np.abs(v)
        mu = m + s * (mean_q[:, None] + Knq.T @ al)                                       # (M, F)
        E_mu = s * g * (np.abs(mean_q)[:, None] + aK.T @ aal) + 2 * U * np.abs(mu)
        t = transform(a["acqf"], a["param"], mu, v[:, None], E_mu, E_v[:, None])
        A, Amu, Av = t["A"], t["Amu"], t["Av"]
        value = A.sum(1) / F
        E_value = GUARD * ((t["E_A"].sum(1) + gamma(8) * np.abs(A).sum(1)) / F + 2 * U * np.abs(value))
    sig = np.sqrt(np.maximum(v[np.isfinite(v)], 1e-9))
    out = dict(value=Quantity(value, E_value, B._scale(value)), eps=t["eps"], margin=t["margin"], u=t["u"], v=v,
               sigma=float(sig.max()) if sig.size else 0.0)
    if not a.get("grad"):
        return out
    D, kind = a["D"], a["kind"]
    th = a["theta"]
    l, os_ = LD(th[:D]), LD(th[D])
    S1 = _S[kind][1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sAmu, sAv = Amu.sum(1), Av.sum(1)
        E_sAmu = t["E_Amu"].sum(1) + gamma(6) * np.abs(Amu).sum(1)
        E_sAv = t["E_Av"].sum(1) + gamma(6) * np.abs(Av).sum(1)
        ab = Amu @ al.T                                                                   # (M, n)
        E_ab = t["E_Amu"] @ aal.T + gamma(F) * (np.abs(Amu) @ aal.T)
        df = (LD(a["Xq"])[None, :, :] - LD(a["Xt"][:n])[:, None, :]) / l                   # (n, M, D)
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
        grad = (gmu + t2) / F
        E_grad = GUARD * ((E_gmu + E_sAv[:, None] * np.abs(gvar) + np.abs(sAv)[:, None] * E_gvar + U * (np.abs(gmu) + np.abs(t2))) / F
                          + 2 * U * np.abs(grad))
    out["grad"] = Quantity(grad, E_grad, B._scale(grad))
    return out


def conditions(label, ref):
    """The conditions on the inputs: first order is enough (eps), and no v within 1e3 E_v of its clamp."""
    eps = ref["eps"][np.isfinite(ref["eps"])]
    assert eps.size == 0 or float(eps.max()) <= SECOND_ORDER, f"{label}: eps = {float(eps.max()):.3e} > {SECOND_ORDER} -- the input set is ill-chosen"
    mg = ref["margin"][~np.isnan(ref["margin"])]
    assert mg.size == 0 or float(mg.min()) >= MARGIN, f"{label}: v within {float(mg.min()):.3e} E_v of its clamp -- the input set is ill-chosen"


def key(a, name):
    fam = FAMILY[a["kind"]] if a.get("grad") else "-"
    return ("fantasy_acqf", f"{fam}/{ACQ[a['acqf']]}", name)


def report():
    return B.report("fantasy_acqf") + B.report("fantasy_chain") + B.report("acqf_batched") + B.report("fantasy_vs_finish")


# ------------------------------------------------------------------------------------------------------------------
# input sets
GRAD_SHAPES = ((1, 1, 1, 1), (7, 2, 3, 6), (8, 63, 3, 6), (9, 64, 3, 15), (63, 1, 3, 1), (64, 64, 3, 6), (65, 63, 130, 6), (96, 64, 3, 15))
VALUE_SHAPES = ((97, 64, 3), (255, 2, 3), (256, 64, 130))
GRAD_CASES = [(*sh, kind) for sh in GRAD_SHAPES for kind in (KIND_RBF, KIND_MATERN52)]
CLAMP_SHAPE = (9, 64, 3, 15)
EDGE_SHAPE = (65, 63, 130, 6)
M_ALL, S_ALL, BETA, BEST_F = 0.3, 1.7, 9.0, 0.1
PARAM = {UCB: BETA, EI: BEST_F}


def grad_id(c):
    return f"n{c[0]}-F{c[1]}-M{c[2]}-D{c[3]}-{FAMILY[c[4]]}"


def _rng(*seed):
    return np.random.default_rng([20261020, *seed])


def inputs(n, F, M, D, kind, acqf, grad=True) -> dict:
    """Xt, Xq uniform in the unit cube, theta = (l in 0.3 .. 1.3, os 1.3, noise 1e-3), Knq = 0.3 randn, Z = 0.01 randn,
    alpha = randn / sqrt(n) (mu_f of order 1, EI's u_f mostly within +-4), mean_q = randn, var_q in 0.5 .. 1.5, cov_g = 0.1 randn, mu_g,
    var_g = randn in ALL 16 columns of a query (the kernel may read columns 1 .. D only); noise_add = 1e-3 for odd n, else 0.  On
    EDGE_SHAPE: query 0 on training point 0, query 1 1e-7 from training point 3, training points 0 and 1 identical."""
    rng = _rng(1, n, F, M, D, kind)
    Xt, Xq = rng.uniform(size=(n, max(D, 1))), rng.uniform(size=(M, max(D, 1)))
    if (n, F, M, D) == EDGE_SHAPE:
        Xt[1] = Xt[0]
        Xq[0] = Xt[0]
        Xq[1] = Xt[3] + 1e-7
    a = dict(Knq=0.3 * rng.normal(size=(n, M)), Z=0.01 * rng.normal(size=(n, M)), alpha=rng.normal(size=(n, F)) / np.sqrt(n),
             mean_q=rng.normal(size=M), var_q=rng.uniform(0.5, 1.5, size=M), m=M_ALL, s=S_ALL, noise_add=1e-3 if n % 2 else 0.0,
             acqf=acqf, param=PARAM[acqf], n=n, M=M, F=F, D=D, kind=kind, grad=grad,
             cov_g=0.1 * rng.normal(size=(n, M * 16)), mu_g=rng.normal(size=M * 16), var_g=rng.normal(size=M * 16), Xt=Xt, Xq=Xq,
             theta=np.concatenate([rng.uniform(0.3, 1.3, size=max(D, 1)), [1.3, 1e-3]]))
    return a


def _v64(a):
    return a["s"] * a["s"] * (a["var_q"] - (a["Knq"] * a["Z"]).sum(0) + a["noise_add"])


CLAMP_MODES = (("neg", UCB), ("neg", EI), ("tiny", EI), ("zero", UCB), ("zero", EI), ("beta0", UCB))
CLAMPED_Q = (0, 2)


def clamp_inputs(mode, acqf, kind) -> dict:
    """CLAMP_SHAPE with queries 0 and 2 on the clamp: v = -0.01 ('neg'), 5e-10 ('tiny', EI's floor), exactly 0 ('zero': var_q = 0, a zero
    column of Knq, noise_add = 0); 'beta0': beta = 0, every query (the sd > 1e-300 guard)."""
    a = inputs(*CLAMP_SHAPE, kind, acqf)
    if mode == "beta0":
        a["param"] = 0.0
        return a
    for q in CLAMPED_Q:
        if acqf == EI:      # on the floor sigma = 3.2e-5: mu_f within a few sigma of best_f, or pdf underflows and Av is 0 clamp or no clamp
            a["Knq"][:, q] *= 1e-5
            a["mean_q"][q] = (a["param"] - a["m"]) / a["s"] + 1e-5
        if mode == "zero":
            a["noise_add"] = 0.0
            a["Knq"][:, q] = 0.0
            a["var_q"][q] = 0.0
        else:
            target = -0.01 if mode == "neg" else 5e-10
            a["var_q"][q] += (target - _v64(a)[q]) / (a["s"] * a["s"])
    return a


def tail_inputs(mode, kind) -> dict:
    """EI: 'span' on EDGE_SHAPE, mean_q placed so that u_f runs from -9 to +9 over the queries of one call; 'deep' on CLAMP_SHAPE, every
    u_f <= -40 (pdf and cdf underflow: value and gradient are 0 within the absolute term)."""
    a = inputs(*(EDGE_SHAPE if mode == "span" else CLAMP_SHAPE), kind, EI)
    sigma = np.sqrt(_v64(a))
    t = np.linspace(-9.0, 9.0, a["M"]) if mode == "span" else np.full(a["M"], -45.0)
    a["mean_q"] = (a["param"] - a["m"] - t * sigma) / a["s"]
    return a


def nonfinite_inputs(shape, kind, acqf, what) -> dict:
    """The last query with a NaN / infinite last coordinate (source columns finite), or -- 'col', the real-pipeline form -- with a NaN
    column of Knq and Z, or -- 'knq' -- a NaN column of Knq next to a finite one of Z (UCB: A_mu = -1 and A_v = 0 whatever v holds, so
    nothing but the value carries the NaN)."""
    a = inputs(*shape, kind, acqf)
    q = a["M"] - 1
    if what in ("col", "knq"):
        a["Knq"][:, q] = np.nan
        if what == "col":
            a["Z"][:, q] = np.nan
    else:
        a["Xq"][q, a["D"] - 1] = what
    return a


# ------------------------------------------------------------------------------------------------------------------
# drivers.  Backend: be.fantasy(a, info) -> (rc, value (M), grad (M, D) or None), every output through a guarded buffer of SENTINEL
def _hold(label, a, ref, value, grad, vmask=None, gmask=None, value_scale=None):
    conditions(label, ref)
    qv = ref["value"] if value_scale is None else ref["value"]._replace(scale=value_scale)
    within(label, key(a, "value"), value, qv, vmask)
    if a.get("grad"):
        qg = ref["grad"] if value_scale is None else ref["grad"]._replace(scale=value_scale)
        within(label, key(a, "grad"), grad, qg, gmask)


def check_set(be, a, label, infos=(None, 0, 2), **kw):
    ref = fantasy_reference(a)
    for info in infos:
        rc, value, grad = be.fantasy(a, info)
        assert rc == 0, f"{label}: return code {rc}"
        if info:
            assert np.isnan(value).all() and (grad is None or np.isnan(grad).all()), f"{label}: info = {info} must give NaN everywhere"
        else:
            _hold(f"{label}-info{info}", a, ref, value, grad, **kw)
    return ref


def check_grad_case(be, c):
    for acqf in (UCB, EI):
        check_set(be, inputs(*c, acqf), f"fantasy-{grad_id(c)}-{ACQ[acqf]}")


def check_value_only(be, shape):
    """The value path beyond the gradient's limits; `kind` is not read there: kind = 7 gives the values of a valid kind, bit for bit."""
    n, F, M = shape
    for acqf in (UCB, EI):
        a = inputs(n, F, M, 0, KIND_RBF, acqf, grad=False)
        check_set(be, a, f"fantasy-n{n}-F{F}-M{M}-value-{ACQ[acqf]}")
        v0 = be.fantasy(a, None)[1]
        rc, v7, _ = be.fantasy(dict(a, kind=7), None)
        assert rc == 0 and np.array_equal(v0, v7), "value only: kind = 7 must be accepted and change nothing"


def check_clamp(be, mode, acqf, kind):
    """Within the bounds (the reference has Av = 0 on the clamp: a live partial is far outside), and the clamped queries' gradient
    does not move by a bit when var_g does -- the partial is exactly absent."""
    a = clamp_inputs(mode, acqf, kind)
    label = f"fantasy-clamp-{mode}-{ACQ[acqf]}-{FAMILY[kind]}"
    ref = check_set(be, a, label, infos=(None,))
    clamped = list(range(a["M"])) if mode == "beta0" else list(CLAMPED_Q)
    thr = 0.0 if acqf == UCB else 1e-9
    assert mode == "beta0" or (ref["v"][clamped] <= thr).all(), f"{label}: the set does not clamp"
    g1 = be.fantasy(a, None)[2]
    g2 = be.fantasy(dict(a, var_g=3.0 * a["var_g"] + 1.0), None)[2]
    assert np.array_equal(g1[clamped], g2[clamped]), f"{label}: the clamped partial d A / d v is live in the gradient"
    if mode != "beta0":
        assert (g1[1] != g2[1]).all(), f"{label}: the unclamped query must depend on var_g"


def check_tails(be, mode, kind):
    a = tail_inputs(mode, kind)
    label = f"fantasy-tail-{mode}-{FAMILY[kind]}"
    if mode == "span":
        ref = check_set(be, a, label, infos=(None,))
        assert float(ref["u"].min()) < -8.5 and float(ref["u"].max()) > 8.5, f"{label}: u spans {float(ref['u'].min())} .. {float(ref['u'].max())}"
    else:
        pre = fantasy_reference(a)
        assert float(pre["u"].max()) <= -40.0, f"{label}: u up to {float(pre['u'].max())}"
        assert float(np.abs(pre["value"].ref).max()) < 1e-300 and float(np.abs(pre["grad"].ref).max()) < 1e-300
        check_set(be, a, label, infos=(None,), value_scale=pre["sigma"])     # (a zero reference: the cap against sigma)


def check_nonfinite(be, shape, kind, acqf, what):
    """The rule of (7f): NaN in EVERY entry of that query's gradient (and in its value when a column of Knq / Z is NaN); the other
    queries within their bounds."""
    a = nonfinite_inputs(shape, kind, acqf, what)
    M, D = a["M"], a["D"]
    gmask = np.zeros((M, D), dtype=bool)
    gmask[M - 1] = True
    vmask = None
    if what in ("col", "knq"):
        vmask = np.zeros(M, dtype=bool)
        vmask[M - 1] = True
    check_set(be, a, f"fantasy-{grad_id((*shape, kind))}-{ACQ[acqf]}-bad={what}", infos=(None,), vmask=vmask, gmask=gmask)


# (what to change in a legal call, the return code, with the gradient?)
REFUSALS = (
    ("n = 257", dict(n=257), E_TOOLARGE, False), ("F = 65", dict(F=65), E_TOOLARGE, False), ("grad with n = 97", dict(n=97), E_TOOLARGE, True),
    ("grad with D = 16", dict(D=16), E_TOOLARGE, True), ("n = 0", dict(n=0), E_BADARG, True), ("F = 0", dict(F=0), E_BADARG, True),
    ("s_all = 0", dict(s=0.0), E_BADARG, True), ("s_all = NaN", dict(s=float("nan")), E_BADARG, True), ("acqf = 2", dict(acqf=2), E_BADARG, True),
    ("grad with kind = 7", dict(kind=7), E_BADARG, True), ("M = 0", dict(M=0), 0, True),
)


def check_refusals(be):
    """Each call brings the buffers of the legal shape (7, 2, 3, 6): nothing may be written, whatever the scalars say."""
    for what, change, want, with_grad in REFUSALS:
        a = inputs(7, 2, 3, 6, KIND_MATERN52, UCB, grad=with_grad)
        a["param"] = PARAM[UCB]
        a.update(change)
        rc, value, grad = be.fantasy(a, None)
        assert rc == want, f"{what}: return code {rc}, expected {want}"
        assert (value == SENTINEL).all() and (grad is None or (grad == SENTINEL).all()), f"{what}: the call wrote to its outputs"


def check_against_finish_and_gradient(be, c):
    """F = 1 with UCB: value = -mu + sqrt(beta var) and grad = -dmu + Av dvar of scaml_target_finish_f64 / scaml_target_posterior_grad_f64
    on the same arrays, within the sum of the kernels' bounds (the composition of the two in long double, their bounds propagated
    to first order)."""
    n, F, M, D, kind = c
    assert F == 1
    a = inputs(*c, UCB)
    ref = fantasy_reference(a)
    conditions("F = 1", ref)
    rc, value, grad = be.fantasy(a, None)
    fa = dict(Knq=a["Knq"], Z=a["Z"], alpha=np.ascontiguousarray(a["alpha"][:, 0]), mean_q=a["mean_q"], var_q=a["var_q"], m=a["m"], s=a["s"],
              noise_add=a["noise_add"], n=n, M=M)
    mu, var = be.finish(fa, None)
    fr = B.finish_reference(fa)
    ga = dict(cov_g=a["cov_g"], mu_g=a["mu_g"], var_g=a["var_g"], Xt=a["Xt"], Xq=a["Xq"], theta=a["theta"], alpha=fa["alpha"], Z=a["Z"], s=a["s"],
              n=n, Mq=M, D=D, kind=kind)
    rc2, dmu, dvar = be.tgrad(ga, None)
    gr = B.tgrad_reference(ga)
    assert rc == 0 and rc2 == 0
    beta = LD(BETA)
    sd = np.sqrt(beta * LD(var))
    Av = beta / (2 * sd)
    comp_v = sd - LD(mu)
    tol_v = fr["mu"].bound + sd * fr["var"].bound / (2 * LD(var))
    comp_g = -LD(dmu) + Av[:, None] * LD(dvar)
    tol_g = gr["dmu"].bound + Av[:, None] * gr["dvar"].bound + np.abs(Av[:, None] * LD(dvar)) * (fr["var"].bound / (2 * LD(var)))[:, None]
    label = f"fantasy-vs-finish-{grad_id(c)}"
    within(label, ("fantasy_vs_finish", FAMILY[kind], "value"), value, Quantity(comp_v, GUARD * tol_v + ref["value"].bound, ref["value"].scale))
    within(label, ("fantasy_vs_finish", FAMILY[kind], "grad"), grad, Quantity(comp_g, GUARD * tol_g + ref["grad"].bound, ref["grad"].scale))


CHAIN_F, CHAIN_PENDING = 5, 3


def check_chain(be, kind):
    """tests/_target_bounds.check_chain, then on ITS outputs: the solve with R = F for alpha in its (n, F) layout (the fantasised
    outcomes of the 3 pending points differ per column), and the fantasy kernel for both acquisition functions, its reference fed the
    backend's own Knq / Z / alpha / mean_q / var_q and GRAD sums."""
    fam = FAMILY[kind]
    ch = B.check_chain(be, kind)["ctx"]
    n, M, D = B.CHAIN["n"], B.CHAIN["Mq"], B.CHAIN["D"]
    rng = _rng(2, kind)
    R = np.repeat(ch["resid"][:, None], CHAIN_F, axis=1)
    R[n - CHAIN_PENDING:] += 0.3 * rng.normal(size=(CHAIN_PENDING, CHAIN_F))
    alpha = be.solve(ch["L"][None], ch["W"][None], R[None], None, False)[0]
    within(f"chain-{fam}", ("fantasy_chain", fam, "alpha"), alpha, B.solve_reference(ch["L"], R, n))
    out = {}
    for acqf in (UCB, EI):
        a = dict(Knq=ch["Knq"], Z=ch["Z"], alpha=alpha, mean_q=ch["mean_q"], var_q=ch["var_q"], m=ch["m"], s=ch["s"], noise_add=0.0, acqf=acqf,
                 param=PARAM[acqf], n=n, M=M, F=CHAIN_F, D=D, kind=kind, grad=True, cov_g=ch["cov_g"], mu_g=ch["mu_g"], var_g=ch["var_g"],
                 Xt=ch["Xall"][:n], Xq=ch["Xall"][n:], theta=ch["theta"])
        ref = fantasy_reference(a)
        conditions(f"chain-{fam}-{ACQ[acqf]}", ref)
        rc, value, grad = be.fantasy(a, ch["info"])
        assert rc == 0
        within(f"chain-{fam}-{ACQ[acqf]}", ("fantasy_chain", fam, f"value/{ACQ[acqf]}"), value, ref["value"])
        within(f"chain-{fam}-{ACQ[acqf]}", ("fantasy_chain", fam, f"grad/{ACQ[acqf]}"), grad, ref["grad"])
        out[acqf] = (value, grad)
    return out


def batched_value_reference(acqf, par, mu_out, var_out):
    """scaml_target_acqf_batched_f64's value from ITS OWN mu_out / var_out (E_mu = E_v = 0): the transform bound alone.  par (Mq)."""
    t = transform(acqf, LD(par), LD(mu_out), LD(var_out), 0.0, 0.0)
    return Quantity(t["A"], t["E_A"], B._scale(t["A"]))


def ulp_errors(x, got, ref):
    """|got - ref| in units of the fp64 spacing at ref (subnormal spacing 2^-1074 below 2^-1022)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sp = np.spacing(np.abs(ref).astype(np.float64))
        return np.abs(LD(got) - ref) / LD(sp)
