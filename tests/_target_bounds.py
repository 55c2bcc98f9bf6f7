"""Long-double reference, a-priori forward error bound, input sets and shared assertions for the kernels downstream of the source
pass: scaml_weighted_task_sum_f64 / scaml_weighted_prior_reduce_f64, scaml_target_assemble_f64, the POTRF at T = 1,
scaml_cho_solve_batched_f64 / scaml_solve_lt_batched_f64, scaml_target_finish_f64 and scaml_target_posterior_grad_f64.

Same construction as tests/_posterior_bounds.py (whose helpers are used here): the reference consumes exactly the arrays the
kernel is handed -- a downstream stage the DEVICE's own upstream outputs --, so each stage is judged on its own arithmetic and the
conditioning of Knn enters only through the solve's own bound.  With u = 2^-53, g_k = k u / (1 - k u):

  weighted sum   E = g_{T+2} sum_t |c_t| |in_t|,  c_t = w_t or w_t^2 (the square is one rounding, inside g); a masked task contributes
                 nothing whatever it holds, every task masked gives exact zeros
  assemble       d2 from coordinate differences (no cancellation): E_d2 = g_{D+5} d2
                 E_K  = os (S E_d2 + 4 u |k|),  S = 1/2 (RBF), 5/6 (Matern-5/2)              (tests/_posterior_bounds.py)
                 Knn / Knq entry v = cov_s / s^2 + os k:  E = E_K + 3 u |cov_s / s^2| + u |v|,  + u |v + noise| on the diagonal
                 resid  = y - (mean_s - m) / s:           E = g_2 |(mean_s - m) / s| (1 + u) + u |resid|   (subtraction, division,
                                                                                               then the last subtraction)
                 mean_q = (mean_s - m) / s:               E = g_2 |mean_q|
                 var_q  = var_s / s^2 + os:               E = g_2 |var_s / s^2| (1 + u) + u |var_q|   (s * s, the division, the sum)
  POTRF, T = 1   residual form |L L^T - (Knn + jitter I)| <= g_{n+4} |L| |L^T| componentwise; alpha under the solve bound, R = 1
  solve          the reference is the long-double inverse of the device's L alone (never Linv_diag: a wrong W is an error)
                 forward   E_Y = g_{N+4} |L^-1| |L| |Y|
                 backward  E_X = |L^-T| (E_Y + g_{N+4} |L^T| |X|);   scaml_solve_lt_batched_f64: the backward half with E_Y = 0
                 rows at or past n_t are exactly zero
  finish         E_mu  = s g_{n+3} (|mean_q| + |Knq|^T |alpha|) + 2 u |mu|
                 E_var = s^2 g_{n+3} (|var_q| + |Knq|^T |Z| + |noise_add|) + 3 u |var|
  target grad    slope term c = 2 os dk (x_q - x_a)_d / l_d^2: the "GRAD col" bound of tests/_posterior_bounds.py with E_d2 = g_{D+5} d2
                 dkn  = cov_g / s^2 + c:  E_dkn = E_c + 2 u |cov_g / s^2| + u |dkn|
                 E_dmu  = s (|alpha|^T E_dkn + g_{n+8} |alpha|^T |dkn|) + 2 u (|mu_g| + |dmu - mu_g|)
                 E_dvar = 2 s^2 (|Z|^T E_dkn + g_{n+8} |Z|^T |dkn|) + 3 u (|var_g| + |dvar - var_g|)

Terms added to the issue's model: the (1 + u) on the first terms of resid and var_q (the last statement rounds the COMPUTED
operand, second order), nothing else.  No constant here is fitted to what a kernel returns.

Every bound is capped at CAP = 1e-8 of the quantity's largest reference magnitude in the call (a condition on the INPUTS, asserted
with every comparison).  A non-finite query coordinate: NaN in exactly that column of Knq from the assemble, NaN in every entry of
that query's mu / var (finish, through Knq and Z) and dmu / dvar (target gradient); the other queries stay within their bounds.

Input sets (the smallest shapes at which the kernels branch; read off the kernels):
  weighted sum   T in {1, 3, 4, 5, 9, 33} (quarter-per-wave split: empty quarters, a partial group of eight, two groups), len in
                 {1, 63, 64, 65, 275}, powers 1 and 2, active NULL / one masked task holding NaN values and a NaN weight / all masked
  prior reduce   mu alone, cov alone, both; Ma * M = 91 (no multiple of 64)
  assemble       (n, M, D) in {(1, 1, 1), (1, 0, 3), (16, 17, 6), (17, 1, 15), (15, 300, 2), (96, 127, 6)}: a query on a training point, one
                 1e-7 away, two identical training points (d2 = 0 off the diagonal); (16, 17, 6) and (15, 300, 2) again with a NaN query
                 coordinate.  Each finite set goes on through the POTRF (T = 1) and the solve (R = M) on the device's own Knn / Knq
  solve          N = 129, 255 (odd: the scalar-load path), 144 (even), 320 / 336 (either side of the 4 -> 2 waves-per-workgroup
                 switch of strip_solve_waves: 4 waves x 320 x 16 doubles = 160 KiB = kLdsLimit exactly, 336 is the next multiple of
                 16), 512; R in {1, 16, 17, 65}; T in {1, 2, 9}; ragged counts {N, N - 1, a multiple of 16, 1, 0}
  finish         (n, M) in {(1, 1), (7, 127), (8, 128), (9, 129), (96, 129), (96, 1)}, noise_add 0 and > 0, info NULL / 0 / 2
  target grad    (n, Mq, D) in {(0, 1, 1), (1, 3, 6), (63, 1, 15), (64, 3, 1), (65, 3, 6), (96, 3, 15), (130, 1, 6)}: a query on a
                 training point and one 1e-7 away; info > 0; D = 16 (SCAML_E_TOOLARGE, nothing written); a NaN and an infinite query coordinate
  chain          per family the real pipeline: source stack T = 3, N = 48, ragged, target n = 17, Mq = 3, D = 6 -- source value and GRAD
                 passes, weighted sums, assemble, POTRF, solve, finish, gradient, each reference fed the upstream outputs

The drivers below (`check_*`) run a set through a BACKEND -- the C ABI on the device (tests/test_target_bounds_gpu.py) or the plain
fp64 numpy stand-ins in the kernels' formulation (tests/test_target_bounds.py) -- and hold every output to its bound.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import _posterior_bounds as P
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, OS, SENTINEL, U, Quantity, _kernel, _S, gamma, inverse_lower

E_TOOLARGE = -2
FAMILY = {KIND_RBF: "rbf", KIND_MATERN52: "matern"}
RATIOS = P.Ratios()      # (kernel, family or "-", output) -> [largest error / bound, largest bound / scale]


def _scale(x):
    return P._scale(np.asarray(x, dtype=LD))


def _up(x):
    """A bound factor computed in fp64 from nonnegative fp64 products (relative error <= N u): rounded up generously."""
    return x * (1 + 1e-9)


def within(label, key, got, q: Quantity, nan_mask=None):
    """|got - ref| <= bound elementwise, the bound at most CAP of the scale; entries under nan_mask must be NaN.  The first failing
    element is quoted as `<label> <output>[i, j]`."""
    name = key[2]
    got = np.asarray(got)
    assert got.shape == q.ref.shape, f"{label} {name}: shape {got.shape} against {q.ref.shape}"
    live = np.ones(got.shape, dtype=bool) if nan_mask is None else ~np.broadcast_to(nan_mask, got.shape)
    if nan_mask is not None:
        assert np.isnan(got[~live]).all(), f"{label} {name}: a non-finite query must give NaN, got {got[~live].ravel()[:4]}"
    bound = np.broadcast_to(q.bound, got.shape)
    over = live & ~(bound <= CAP * q.scale)
    assert not over.any(), (f"{label} {name}: the bound {float(bound[over].max()):.3e} exceeds {CAP} of the scale {q.scale:.3e} -- the input "
                            f"set is ill-chosen")
    with np.errstate(invalid="ignore"):
        err = np.abs(LD(got) - q.ref)
        bad = live & ~(err <= bound)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{label} {name}{list(i)}: got {float(got[i])!r}, reference {float(q.ref[i])!r}, error {float(err[i]):.3e} > bound "
                             f"{float(bound[i]):.3e} ({int(bad.sum())} of {bad.size} elements)")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(live & (bound > 0), err / np.where(bound > 0, bound, 1), 0)
    RATIOS.note(key, float(r.max()) if r.size else 0.0, float(bound[live].max() / q.scale) if live.any() and q.scale > 0 else 0.0)


def report(prefix=None):
    """The ratio table so far, one line per (kernel, family, output)."""
    return [f"{k[0]} {k[1]} {k[2]}: largest error / bound {e:.3e}, largest bound / scale {c:.3e}" for k, (e, c) in sorted(RATIOS.items())
            if prefix is None or k[0] == prefix]


# ------------------------------------------------------------------------------------------------------------------
# references and bounds, one per stage
def wsum_reference(inp, w, active, power):
    """inp (T, len), w (T), active (T) or None -> Quantity over (len)."""
    T = inp.shape[0]
    ref, mag = np.zeros(inp.shape[1], dtype=LD), np.zeros(inp.shape[1], dtype=LD)
    for t in range(T):
        if active is not None and not active[t]:
            continue
        c = LD(w[t]) if power == 1 else LD(w[t]) * LD(w[t])
        ref += c * LD(inp[t])
        mag += np.abs(c) * np.abs(LD(inp[t]))
    return Quantity(ref, gamma(T + 2) * mag, _scale(ref))


def _sqdist(Xa, Xb, l):
    diff = (LD(Xa)[:, None, :] - LD(Xb)[None, :, :]) / LD(l)
    return diff, (diff * diff).sum(-1)


def assemble_reference(a: dict) -> dict:
    """a: the arguments of scaml_target_assemble_f64 (numpy) -> name -> Quantity."""
    n, M, D, kind = a["n"], a["M"], a["D"], a["kind"]
    th, s, m = a["theta"], LD(a["s"]), LD(a["m"])
    os_, noise = LD(th[D]), LD(th[D + 1])
    s2 = s * s
    with np.errstate(invalid="ignore"):
        _, d2 = _sqdist(a["Xall"][:n], a["Xall"], th[:D])
        k = _kernel(d2, kind)[0]
        E_K = os_ * (_S[kind][0] * gamma(D + 5) * d2 + 4 * U * np.abs(k))
        cs = LD(a["cov_s"]) / s2
        v = cs + os_ * k
        E = E_K + 3 * U * np.abs(cs) + U * np.abs(v)
    Knn, E_nn = v[:, :n].copy(), E[:, :n].copy()
    idx = np.arange(n)
    Knn[idx, idx] += noise
    E_nn[idx, idx] += U * np.abs(Knn[idx, idx])
    qm = (LD(a["mean_s"]) - m) / s
    resid = LD(a["y"]) - qm[:n]
    qv = LD(a["var_s"][n:]) / s2
    out = dict(Knn=Quantity(Knn, E_nn, _scale(Knn)),
               resid=Quantity(resid, gamma(2) * np.abs(qm[:n]) * (1 + U) + U * np.abs(resid), _scale(resid)))
    if M:
        out.update(Knq=Quantity(v[:, n:], E[:, n:], _scale(v[:, n:])),
                   mean_q=Quantity(qm[n:], gamma(2) * np.abs(qm[n:]), _scale(qm[n:])),
                   var_q=Quantity(qv + os_, gamma(2) * np.abs(qv) * (1 + U) + U * np.abs(qv + os_), _scale(qv + os_)))
    return out


def potrf_reference(L, Knn, jitter):
    """(what to compare, Quantity): L L^T in long double against Knn + jitter I under g_{n+4} |L| |L^T|."""
    n = L.shape[0]
    Ll = LD(np.tril(L))
    A = LD(Knn) + LD(jitter) * np.eye(n, dtype=LD)
    A = np.tril(A) + np.tril(A, -1).T          # (the factorisation reads the lower triangle)
    return Ll @ Ll.T, Quantity(A, gamma(n + 4) * (np.abs(Ll) @ np.abs(Ll).T), _scale(A))


_LINV = {}


def solve_reference(L, B, n, lt=False, cache_key=None):
    """X = (L L^T)^-1 B (lt: L^-T B) for one task: L (N, N), B (N, R), n live rows -> Quantity over (N, R); rows >= n: 0 +- 0."""
    N, R = B.shape
    ref, bound = np.zeros((N, R), dtype=LD), np.zeros((N, R), dtype=LD)
    if n:
        if cache_key is None or cache_key not in _LINV:
            Li = inverse_lower(np.tril(L[:n, :n]))
            if cache_key is not None:
                _LINV[cache_key] = Li
        else:
            Li = _LINV[cache_key]
        g = gamma(N + 4)
        aLi, aL = np.abs(Li.astype(np.float64)), np.abs(np.tril(L[:n, :n]))
        Y = LD(B[:n]) if lt else Li @ LD(B[:n])
        X = Li.T @ Y
        E_Y = np.zeros((n, R)) if lt else _up(g * (aLi @ (aL @ np.abs(Y.astype(np.float64)))))
        ref[:n] = X
        bound[:n] = _up(aLi.T @ (E_Y + g * (aL.T @ np.abs(X.astype(np.float64)))))
    return Quantity(ref, bound, _scale(ref))


def finish_reference(a: dict) -> dict:
    n, s, m = a["n"], LD(a["s"]), LD(a["m"])
    Knq, Z, al = LD(a["Knq"][:n]), LD(a["Z"][:n]), LD(a["alpha"][:n])
    g = gamma(n + 3)
    with np.errstate(invalid="ignore"):
        mu = m + s * (LD(a["mean_q"]) + Knq.T @ al)
        E_mu = s * g * (np.abs(LD(a["mean_q"])) + np.abs(Knq).T @ np.abs(al)) + 2 * U * np.abs(mu)
        var = s * s * (LD(a["var_q"]) - (Knq * Z).sum(0) + LD(a["noise_add"]))
        E_var = s * s * g * (np.abs(LD(a["var_q"])) + (np.abs(Knq) * np.abs(Z)).sum(0) + abs(a["noise_add"])) + 3 * U * np.abs(var)
    return dict(mu=Quantity(mu, E_mu, _scale(mu)), var=Quantity(var, E_var, _scale(var)))


def tgrad_reference(a: dict) -> dict:
    """a: the arguments of scaml_target_posterior_grad_f64 -> dmu / dvar Quantities (Mq, D)."""
    n, Mq, D, kind = a["n"], a["Mq"], a["D"], a["kind"]
    th, s = a["theta"], LD(a["s"])
    l, os_ = LD(th[:D]), LD(th[D])
    s2 = s * s
    S1 = _S[kind][1]
    mu_g = LD(a["mu_g"]).reshape(Mq, 16)[:, 1:1 + D]
    var_g = LD(a["var_g"]).reshape(Mq, 16)[:, 1:1 + D]
    dmu, dvar = mu_g.copy(), var_g.copy()
    E_mu, E_var = np.zeros((Mq, D), dtype=LD), np.zeros((Mq, D), dtype=LD)
    if n:
        with np.errstate(invalid="ignore"):
            al, Z = LD(a["alpha"][:n]), LD(a["Z"][:n])
            cg = (LD(a["cov_g"][:n]).reshape(n, Mq, 16)[:, :, 1:1 + D]) / s2          # (n, Mq, D)
            diff, d2 = _sqdist(a["Xt"][:n], a["Xq"], th[:D])                         # diff = a' - q'
            df = -diff                                                              # q' - a'
            dk = _kernel(d2, kind)[1]
            E_dk = os_ * (S1 * gamma(D + 5) * d2 + 4 * U * np.abs(dk))
            ap, qp = np.abs(LD(a["Xt"][:n]) / l), np.abs(LD(a["Xq"]) / l)
            c = 2 * os_ * dk[:, :, None] * df / l
            E_c = (2 / l) * (E_dk[:, :, None] * np.abs(df) + os_ * np.abs(dk)[:, :, None] * (2 * U * (qp[None] + ap[:, None]) + U * np.abs(df))) \
                + 5 * U * np.abs(c)
            dkn = cg + c
            E_dkn = E_c + 2 * U * np.abs(cg) + U * np.abs(dkn)
            g = gamma(n + 8)
            sm, sv = np.einsum("a,aqd->qd", al, dkn), np.einsum("aq,aqd->qd", Z, dkn)
            dmu = mu_g + s * sm
            dvar = var_g - 2 * s2 * sv
            E_mu = s * (np.einsum("a,aqd->qd", np.abs(al), E_dkn) + g * np.einsum("a,aqd->qd", np.abs(al), np.abs(dkn)))
            E_var = 2 * s2 * (np.einsum("aq,aqd->qd", np.abs(Z), E_dkn) + g * np.einsum("aq,aqd->qd", np.abs(Z), np.abs(dkn)))
    with np.errstate(invalid="ignore"):
        E_mu = E_mu + 2 * U * (np.abs(mu_g) + np.abs(dmu - mu_g))
        E_var = E_var + 3 * U * (np.abs(var_g) + np.abs(dvar - var_g))
    return dict(dmu=Quantity(dmu, E_mu, _scale(dmu)), dvar=Quantity(dvar, E_var, _scale(dvar)))


# ------------------------------------------------------------------------------------------------------------------
# input sets
def _rng(*seed):
    return np.random.default_rng([20261019, *seed])


def _theta(rng, D, noise=1e-2, c=0.5):
    return np.concatenate([c * np.sqrt(D) * rng.uniform(0.5, 1.5, size=D), [OS, noise]])


def _k64(Xa, Xb, th, kind):
    D = Xa.shape[1]
    d2 = (((Xa[:, None, :] - Xb[None, :, :]) / th[:D]) ** 2).sum(-1)
    return th[D] * _kernel(d2, kind)[0]


WSUM_T = (1, 3, 4, 5, 9, 33)
WSUM_LEN = (1, 63, 64, 65, 275)


def wsum_inputs(T, length, mode):
    """mode: 'all' (active NULL), 'mask' (task T // 2 masked, holding NaN values and a NaN weight), 'none' (every task masked)."""
    rng = _rng(1, T, length)
    inp, w = rng.normal(size=(T, length)) * 2.0, rng.normal(size=T)
    if mode == "all":
        return inp, w, None
    act = np.ones(T, dtype=np.uint8)
    if mode == "none":
        act[:] = 0
    else:
        act[T // 2] = 0
        inp[T // 2], w[T // 2] = np.nan, np.nan
    return inp, w, act


ASSEMBLE_SHAPES = ((1, 1, 1), (1, 0, 3), (16, 17, 6), (17, 1, 15), (15, 300, 2), (96, 127, 6))
ASSEMBLE_NAN = ((16, 17, 6), (15, 300, 2))
ASSEMBLE_CASES = [(n, M, D, kind, False) for (n, M, D) in ASSEMBLE_SHAPES for kind in (KIND_RBF, KIND_MATERN52)] \
    + [(n, M, D, kind, True) for (n, M, D) in ASSEMBLE_NAN for kind in (KIND_RBF, KIND_MATERN52)]


def assemble_id(c):
    n, M, D, kind, nanq = c
    return f"n{n}-M{M}-D{D}-{FAMILY[kind]}" + ("-nanq" if nanq else "")


def assemble_inputs(c) -> dict:
    """Xall in the unit cube: training points 0 and 1 identical (n >= 3), query 0 ON training point 0, query 1 1e-7 from training point
    min(3, n - 1); the weighted source sums smooth functions of realistic magnitude (cov_s = s^2 0.4 exp(-|x - x'|^2): Knn stays
    positive definite); nanq: the last coordinate of query M - 2 is NaN."""
    n, M, D, kind, nanq = c
    rng = _rng(2, n, M, D, kind)
    Xall = rng.uniform(size=(n + M, D))
    if n >= 3:
        Xall[1] = Xall[0]
    if M >= 1:
        Xall[n] = Xall[0]
    if M >= 2:
        Xall[n + 1] = Xall[min(3, n - 1)] + 1e-7
    m, s = 0.7, 1.9
    d2 = ((Xall[:n, None, :] - Xall[None, :, :]) ** 2).sum(-1)
    cov_s = s * s * 0.4 * np.exp(-d2)
    mean_s = m + s * np.sin(3.0 * Xall.sum(-1) / np.sqrt(D))
    var_s = s * s * (0.05 + 0.4 * rng.uniform(size=n + M))
    y = np.sin(3.0 * Xall[:n].sum(-1) / np.sqrt(D)) + 0.3 * rng.normal(size=n)
    if nanq:
        Xall[n + M - 2, D - 1] = np.nan
    return dict(cov_s=cov_s, mean_s=mean_s, var_s=var_s, Xall=Xall, theta=_theta(rng, D), y=y, m=m, s=s, n=n, M=M, D=D, kind=kind)


# kern: "cho" (scaml_cho_solve_batched_f64) / "lt" (scaml_solve_lt_batched_f64); the fit's inputs are those of tests/_posterior_bounds.py
SolveCase = namedtuple("SolveCase", "kern T N R D kind ragged noise")
SOLVE_CASES = [
    SolveCase("cho", 9, 129, 17, 5, KIND_MATERN52, 0, 1e-2),      # odd N, second XCD round, two waves, partial last strip, n_t down to 1 and 0
    SolveCase("cho", 2, 255, 65, 4, KIND_RBF, 1, 1e-3),           # odd N, five strips on four waves: a second workgroup with one live wave
    SolveCase("cho", 1, 144, 16, 5, KIND_MATERN52, None, 1e-2),   # even N (vector loads), a single full strip: one wave
    SolveCase("cho", 2, 320, 65, 4, KIND_MATERN52, 0, 1e-2),      # the last N with four waves per workgroup (160 KiB exactly)
    SolveCase("cho", 2, 336, 65, 4, KIND_RBF, 2, 1e-2),           # the first N with two: three workgroups, the last with one live wave
    SolveCase("cho", 1, 512, 17, 5, KIND_MATERN52, None, 1e-3),   # the limit
    SolveCase("cho", 2, 512, 1, 4, KIND_RBF, 1, 1e-2),            # R = 1: one wave, one live lane column
    SolveCase("lt", 2, 255, 17, 5, KIND_MATERN52, 1, 1e-2),
    SolveCase("lt", 1, 336, 65, 4, KIND_RBF, None, 1e-2),
    SolveCase("lt", 9, 144, 1, 4, KIND_MATERN52, 0, 1e-3),
]


def solve_id(c):
    return f"{c.kern}-T{c.T}-N{c.N}-R{c.R}-D{c.D}-{FAMILY[c.kind]}" + ("" if c.ragged is None else f"-ragged{c.ragged}")


def solve_fit_case(c: SolveCase) -> P.Case:
    return P._c("solve", c.T, c.N, c.R, c.D, c.kind, ragged=c.ragged, noise=c.noise)


def solve_inputs(c: SolveCase):
    """(fit case, its inputs, B (T, N, R)): right-hand sides = kernel columns at random query points, roughened by 30 %; rows at or
    past n_t hold NaN (never read)."""
    fc = solve_fit_case(c)
    inp = P.make_inputs(fc)
    rng = _rng(3, c.T, c.N, c.R)
    B = np.full((c.T, c.N, c.R), np.nan)
    for t, n in enumerate(P.counts(fc, inp)):
        B[t, :n] = _k64(inp["X"][t, :n], rng.uniform(size=(c.R, c.D)), inp["theta"][t], c.kind) * (1 + 0.3 * rng.normal(size=(n, c.R)))
    return fc, inp, B


FINISH_SHAPES = ((1, 1), (7, 127), (8, 128), (9, 129), (96, 129), (96, 1))


def finish_inputs(n, M, kind):
    """Synthetic inputs of realistic magnitude: Knq, Z = Knn^-1 Knq and alpha = Knn^-1 y of a target kernel matrix, in plain fp64."""
    D = 4
    rng = _rng(4, n, M, kind)
    Xt, Xq, th = rng.uniform(size=(n, D)), rng.uniform(size=(M, D)), _theta(rng, D)
    Knn = _k64(Xt, Xt, th, kind) + th[D + 1] * np.eye(n)
    Knq = _k64(Xt, Xq, th, kind)
    y = np.sin(3.0 * Xt.sum(-1)) + 0.2 * rng.normal(size=n)
    return dict(Knq=Knq, Z=np.linalg.solve(Knn, Knq), alpha=np.linalg.solve(Knn, y), mean_q=0.3 * rng.normal(size=M),
                var_q=OS + 0.2 * rng.uniform(size=M), m=0.7, s=1.9, noise_add=0.0, n=n, M=M)


TGRAD_SHAPES = ((0, 1, 1), (1, 3, 6), (63, 1, 15), (64, 3, 1), (65, 3, 6), (96, 3, 15), (130, 1, 6))
TGRAD_CASES = [(n, Mq, D, kind) for (n, Mq, D) in TGRAD_SHAPES for kind in (KIND_RBF, KIND_MATERN52)]


def tgrad_id(c):
    return f"n{c[0]}-Mq{c[1]}-D{c[2]}-{FAMILY[c[3]]}"


def tgrad_inputs(c, nanq=None) -> dict:
    """Synthetic weighted GRAD sums (columns 1 .. D live, the rest zero), alpha and Z of realistic magnitude; query 0 ON training point 0,
    query 1 1e-7 from training point min(3, n - 1); nanq (NaN or inf): the first coordinate of the last query, everything else finite."""
    n, Mq, D, kind = c
    rng = _rng(5, n, Mq, D, kind)
    Xt, Xq = rng.uniform(size=(n, D)), rng.uniform(size=(Mq, D))
    if n:
        Xq[0] = Xt[0]
        if Mq >= 2:
            Xq[1] = Xt[min(3, n - 1)] + 1e-7
    s = 1.9
    live = np.zeros(16)
    live[1:1 + D] = 1.0
    cov_g = (s * s * 0.3 * rng.normal(size=(n, Mq, 16)) * live).reshape(n, Mq * 16)
    a = dict(cov_g=cov_g, mu_g=(rng.normal(size=(Mq, 16)) * live).reshape(-1), var_g=(0.5 * rng.normal(size=(Mq, 16)) * live).reshape(-1),
             Xt=Xt, Xq=Xq, theta=_theta(rng, D), alpha=3.0 * rng.normal(size=n), Z=0.3 * rng.normal(size=(n, Mq)), s=s, n=n, Mq=Mq, D=D, kind=kind)
    if nanq is not None:
        a["Xq"][Mq - 1, 0] = nanq
    return a


# ------------------------------------------------------------------------------------------------------------------
# drivers: one input set through a backend, every output against its reference
def check_wsum(be, T):
    """All lengths, powers and masks for one T; the prior reduce at T == 5."""
    for length in WSUM_LEN:
        for power in (1, 2):
            for mode in ("all", "mask", "none"):
                inp, w, act = wsum_inputs(T, length, mode)
                got = be.wsum(inp, w, act, power)
                label = f"wsum-T{T}-len{length}-p{power}-{mode}"
                if mode == "none" or (mode == "mask" and T == 1):
                    assert (got == 0).all() and not np.signbit(got).any(), f"{label}: every task masked must give exact zeros, got {got[:3]}"
                within(label, ("weighted_task_sum", "-", f"out_p{power}"), got, wsum_reference(inp, w, act, power))
    if T == 5:
        M, Ma = 13, 7
        rng = _rng(6)
        mu, cov, w = rng.normal(size=(T, M)), rng.normal(size=(T, Ma, M)), rng.uniform(0.1, 1.0, size=T)
        act = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
        mu[2], cov[2], w[2] = np.nan, np.nan, np.nan
        for want_mu, want_cov in ((True, False), (False, True), (True, True)):
            mu_s, cov_s = be.prior_reduce(mu if want_mu else None, cov if want_cov else None, w, act)
            label = f"prior_reduce-mu{int(want_mu)}-cov{int(want_cov)}"
            if want_mu:
                within(label, ("weighted_prior_reduce", "-", "mu_s"), mu_s, wsum_reference(mu, w, act, 1))
            if want_cov:
                within(label, ("weighted_prior_reduce", "-", "cov_s"), cov_s.reshape(-1), wsum_reference(cov.reshape(T, -1), w, act, 2))


def check_assemble(be, c, then_solve=True):
    """The assemble on one set; for a finite set then the POTRF (T = 1) on the backend's own Knn / resid and the solve (R = M) on its own
    L / Linv_diag / Knq.  Returns the backend's outputs."""
    n, M, D, kind, nanq = c
    a = assemble_inputs(c)
    got = be.assemble(a)
    refs = assemble_reference(a)
    label, fam = "assemble-" + assemble_id(c), FAMILY[kind]
    mask = None
    if nanq:
        mask = np.zeros(M, dtype=bool)
        mask[M - 2] = True
    for name, q in refs.items():
        within(label, ("target_assemble", fam, name), got[name], q, mask if name == "Knq" else None)
    if not then_solve:
        return got
    f = check_potrf(be, "potrf-" + assemble_id(c), fam, got["Knn"], got["resid"])
    if M:
        Z = be.solve(f["L"][None], f["W"][None], got["Knq"][None], None, False)[0]
        within("solve-" + assemble_id(c), ("cho_solve(target)", fam, "Z"), Z, solve_reference(f["L"], np.nan_to_num(got["Knq"]), n), mask)
        got["Z"] = Z
        if nanq:      # the rule of (7): NaN in that query's mu and var, the other queries within the finish's bound
            fa = dict(Knq=got["Knq"], Z=Z, alpha=f["alpha"], mean_q=got["mean_q"], var_q=got["var_q"], m=a["m"], s=a["s"], noise_add=0.0, n=n, M=M)
            mu, var = be.finish(fa, None)
            fr = finish_reference(fa)
            within("finish-" + assemble_id(c), ("target_finish", fam, "mu"), mu, fr["mu"], mask)
            within("finish-" + assemble_id(c), ("target_finish", fam, "var"), var, fr["var"], mask)
    got.update(f)
    return got


def check_potrf(be, label, fam, Knn, resid):
    n = Knn.shape[0]
    f = be.potrf(Knn, resid)
    assert f["info"] == 0 and f["jitter"] == 0.0, f"{label}: info {f['info']}, jitter {f['jitter']} on a well-conditioned Knn"
    assert (np.triu(f["L"], 1) == 0).all(), f"{label}: L is not zero above the diagonal"
    LLt, q = potrf_reference(f["L"], Knn, f["jitter"])
    within(label, ("potrf(T=1)", fam, "L L^T"), LLt, q)
    within(label, ("potrf(T=1)", fam, "alpha"), f["alpha"], _col(solve_reference(f["L"], resid[:, None], n)))
    return f


def _col(q: Quantity):
    return Quantity(q.ref[:, 0], q.bound[:, 0], q.scale)


def check_solve(be, c: SolveCase, fit=None):
    fc, inp, B = solve_inputs(c)
    fit = be.fit(fc, inp) if fit is None else fit
    got = be.solve(fit["L"], fit["Linv_diag"], B, inp["n_points"], c.kern == "lt")
    for t, n in enumerate(P.counts(fc, inp)):
        label = f"solve-{solve_id(c)} task {t}"
        assert (got[t, n:] == 0).all(), f"{label}: rows at or past n_t = {n} are not exactly zero"
        q = solve_reference(fit["L"][t], np.nan_to_num(B[t]), n, c.kern == "lt", cache_key=(be.name, c, t))
        within(label, ("cho_solve" if c.kern == "cho" else "solve_lt", FAMILY[c.kind], "X"), got[t], q)
    return got


def check_finish(be, n, M):
    for kind in (KIND_RBF, KIND_MATERN52):
        a = finish_inputs(n, M, kind)
        for noise_add in (0.0, 0.0125):
            a["noise_add"] = noise_add
            refs = finish_reference(a)
            for info in (None, 0):
                mu, var = be.finish(a, info)
                label = f"finish-n{n}-M{M}-{FAMILY[kind]}-noise{noise_add}-info{info}"
                within(label, ("target_finish", FAMILY[kind], "mu"), mu, refs["mu"])
                within(label, ("target_finish", FAMILY[kind], "var"), var, refs["var"])
        mu, var = be.finish(a, 2)
        assert np.isnan(mu).all() and np.isnan(var).all(), f"finish-n{n}-M{M}: info = 2 must give NaN everywhere"


def check_tgrad(be, c):
    n, Mq, D, kind = c
    fam, label = FAMILY[kind], "tgrad-" + tgrad_id(c)
    a = tgrad_inputs(c)
    refs = tgrad_reference(a)
    for info in (None, 0):
        rc, dmu, dvar = be.tgrad(a, info)
        assert rc == 0
        within(label, ("target_posterior_grad", fam, "dmu"), dmu, refs["dmu"])
        within(label, ("target_posterior_grad", fam, "dvar"), dvar, refs["dvar"])
    rc, dmu, dvar = be.tgrad(a, 3)
    assert rc == 0 and np.isnan(dmu).all() and np.isnan(dvar).all(), f"{label}: info = 3 must give NaN everywhere"
    for bad in ((np.nan, -np.inf) if Mq >= 2 else ()):      # the rule: NaN in every entry of that query, the others within their bounds
        b = tgrad_inputs(c, nanq=bad)
        refs = tgrad_reference(b)
        mask = np.zeros((Mq, D), dtype=bool)
        mask[Mq - 1] = True
        rc, dmu, dvar = be.tgrad(b, None)
        assert rc == 0
        within(f"{label}-xq={bad}", ("target_posterior_grad", fam, "dmu"), dmu, refs["dmu"], mask)
        within(f"{label}-xq={bad}", ("target_posterior_grad", fam, "dvar"), dvar, refs["dvar"], mask)


def check_tgrad_toolarge(be):
    a = tgrad_inputs((9, 2, 15, KIND_RBF))
    a["D"] = 16          # (the buffers are those of D = 15: nothing may be read or written)
    rc, dmu, dvar = be.tgrad(a, None)
    assert rc == E_TOOLARGE, f"D = 16: return code {rc}"
    assert (dmu == SENTINEL).all() and (dvar == SENTINEL).all(), "D = 16 wrote to its outputs"


CHAIN = dict(T=3, N=48, n=17, Mq=3, D=6)


def chain_cases(kind):
    """The two source passes of the chain as cases of tests/_posterior_bounds.py, sharing one set of inputs: the value pass at
    cat(Xt, Xq) with the covariance block of the n leading points, the GRAD pass at Xq against the same leading points."""
    n, Mq = CHAIN["n"], CHAIN["Mq"]
    val = P._c("linv_cov", CHAIN["T"], CHAIN["N"], n + Mq, CHAIN["D"], kind, Ma=n, ragged=0, std=True)
    inp = P.make_inputs(val)
    grad = val._replace(kern="grad", M=Mq)
    ginp = dict(inp, Xq=inp["Xq"][n:].copy(), Xa=inp["Xq"][:n].copy())
    return val, inp, grad, ginp


def check_chain(be, kind):
    """The real pipeline end to end, every stage's reference fed the backend's own upstream outputs."""
    T, N, n, Mq, D = (CHAIN[k] for k in ("T", "N", "n", "Mq", "D"))
    fam = FAMILY[kind]
    val, inp, grad, ginp = chain_cases(kind)
    src = be.source_passes(val, inp, grad, ginp)      # arr (inputs + L / Linv / alpha / VA), value outputs, GRAD outputs, all (T, ...)
    arr, v, g = src["arr"], src["value"], src["grad"]
    for t in range(T):      # stage 1: the source passes under the bounds of tests/_posterior_bounds.py
        P.check_task(val, inp, arr, t, {k: x[t] for k, x in v.items()})
        P.check_task(grad, ginp, dict(arr, Xq=ginp["Xq"], Xa=ginp["Xa"]), t, {k: x[t] for k, x in g.items()})
    # stage 2: the weighted sums -- the layout contracts: cov (T, n, n + Mq) -> cov_s (n, n + Mq), GRAD cov (T, n, Mq * 16) -> cov_g
    w = np.array([0.6, 0.3, 0.45])
    label = f"chain-{fam}"
    mean_s, cov_s = be.prior_reduce(v["mu"], v["cov"], w, None)
    var_s = be.wsum(v["var"], w, None, 2)
    mu_g = be.wsum(g["mu"].reshape(T, -1), w, None, 1)
    var_g = be.wsum(g["var"].reshape(T, -1), w, None, 2)
    cov_g = be.wsum(g["cov"].reshape(T, -1), w, None, 2).reshape(n, Mq * 16)
    for name, got, x, power in (("mean_s", mean_s, v["mu"], 1), ("cov_s", cov_s.reshape(-1), v["cov"].reshape(T, -1), 2), ("var_s", var_s, v["var"], 2),
                                ("mu_g", mu_g, g["mu"].reshape(T, -1), 1), ("var_g", var_g, g["var"].reshape(T, -1), 2),
                                ("cov_g", cov_g.reshape(-1), g["cov"].reshape(T, -1), 2)):
        within(label, ("chain", fam, name), got, wsum_reference(x, w, None, power))
    # stage 3: assemble on those sums
    rng = _rng(7, kind)
    Xall = inp["Xq"]
    m, s = 0.4, 1.7
    y = (np.sin(3.0 * Xall[:n].sum(-1) / np.sqrt(D)) + 0.2 * rng.normal(size=n) - 0.1) / 1.1
    a = dict(cov_s=cov_s.reshape(n, n + Mq), mean_s=mean_s, var_s=var_s, Xall=Xall, theta=_theta(rng, D), y=y, m=m, s=s, n=n, M=Mq, D=D, kind=kind)
    asm = be.assemble(a)
    for name, q in assemble_reference(a).items():
        within(label, ("chain", fam, name), asm[name], q)
    # stages 4, 5: POTRF and solve on the assembled block
    f = check_potrf(be, label, fam, asm["Knn"], asm["resid"])
    Z = be.solve(f["L"][None], f["W"][None], asm["Knq"][None], None, False)[0]
    within(label, ("chain", fam, "Z"), Z, solve_reference(f["L"], asm["Knq"], n))
    # stage 6: finish
    fa = dict(Knq=asm["Knq"], Z=Z, alpha=f["alpha"], mean_q=asm["mean_q"], var_q=asm["var_q"], m=m, s=s, noise_add=0.0, n=n, M=Mq)
    mu, var = be.finish(fa, int(f["info"]))
    refs = finish_reference(fa)
    within(label, ("chain", fam, "mu"), mu, refs["mu"])
    within(label, ("chain", fam, "var"), var, refs["var"])
    # stage 7: the target gradient
    ga = dict(cov_g=cov_g, mu_g=mu_g, var_g=var_g, Xt=Xall[:n], Xq=Xall[n:], theta=a["theta"], alpha=f["alpha"], Z=Z, s=s, n=n, Mq=Mq, D=D, kind=kind)
    rc, dmu, dvar = be.tgrad(ga, int(f["info"]))
    assert rc == 0
    refs = tgrad_reference(ga)
    within(label, ("chain", fam, "dmu"), dmu, refs["dmu"])
    within(label, ("chain", fam, "dvar"), dvar, refs["dvar"])
    # ctx: what a further stage on the same pipeline needs (tests/_fantasy_bounds.check_chain)
    ctx = dict(Knq=asm["Knq"], mean_q=asm["mean_q"], var_q=asm["var_q"], resid=asm["resid"], L=f["L"], W=f["W"], info=int(f["info"]), Z=Z, cov_g=cov_g,
               mu_g=mu_g, var_g=var_g, theta=a["theta"], Xall=Xall, m=m, s=s)
    return dict(mu=mu, var=var, dmu=dmu, dvar=dvar, ctx=ctx)
