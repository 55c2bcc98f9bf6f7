"""Long-double reference and a-priori forward error bounds for the two kernels of the studies' batched fantasy set-up
(include/scaml_gp.h (7m) scaml_studies_condition_block_f64, (7n) scaml_studies_fantasy_condition_f64; csrc/gp_studies_condition.h).

Same construction as tests/_target_bounds.py (whose helpers are used here): the reference consumes exactly the arrays the kernel is
handed -- (7m) the source pass's mu / cov, (7n) the SAME L', resid, mean_p and eps --, so each stage is judged on its own arithmetic and
the conditioning of K' enters only through the substitutions' own bounds.  With u = 2^-53, g_k = k u / (1 - k u):

  (7m) weighted sums  (6')'s bound: E_ws = g_{T+2} sum_t |c_t| |in_t|, c_t = w_t or w_t^2; a masked task contributes nothing
       K' entry v = cov_s / s^2 + os k(d2):   E = E_ws / s^2 + 3 u |cov_s / s^2| + E_K + u |v|   (+ u |v + noise| on the diagonal)
                      d2 from coordinate differences (no cancellation): E_d2 = g_{D+5} d2
                      E_K = os (S E_d2 + (10 + 2 a) u |k|),  S = 1/2 (RBF), 5/6 (Matern-5/2) the largest slope, a = d2 / 2 (RBF), sqrt(5 d2)
                      (Matern) the exponential's argument: libm's exp within one ulp of a rounded argument (a u relative), and at most
                      nine further roundings in the Matern polynomial, the outputscale and the products
       mean = (mean_s - m) / s:               E_mean = E_ws / s + g_2 |mean|
       resid = y - mean:                      E = E_mean (1 + u) + u |resid|;   the pending rows are exactly zero
  (7n) v = L_nn^-1 resid, forward substitution, row i: i FMAs and one division, i + 1 <= n_obs roundings:
                      E_v = g_{n_obs+2} |L_nn^-1| |L_nn| |v|                                 (the form of tests/_target_bounds.py)
       mu~ = mean_p + L_pn v, n_obs FMAs and one addition:
                      E_mu~ = g_{n_obs+1} (|L_pn| |v| + |mean_p|) + |L_pn| E_v               (dot product + the propagated bound on v)
       mu_p = fma(s, mu~, m), one rounding:   E = s E_mu~ + u |mu_p|
       y_fant = fma(s, mu~ + L_pp eps_f, m), row i: i + 1 <= p FMAs, one addition, one rounding:
                      E = s (E_mu~ + g_{p+1} (|L_pp| |eps_f| + |mu~|)) + u |y_fant|
       alpha_f = L'^-T [v ; eps_f], backward substitution, row i: n' - 1 - i FMAs and one division:
                      E = |L'^-T| ([E_v ; 0] + g_{n'+2} |L'^T| |alpha_f|)

No constant here is fitted to what a kernel returns.  Every bound is capped at CAP = 1e-8 of the quantity's largest reference magnitude
(tests/_target_bounds.within asserts it: a condition on the INPUTS)."""
from __future__ import annotations

import numpy as np

from tests._posterior_bounds import LD, U, Quantity, _kernel, _S, gamma, inverse_lower
from tests._target_bounds import _scale, _up, within  # noqa: F401  (within: re-exported for the tests)

FAMILY = {0: "rbf", 1: "matern"}


def block_reference(mu, cov, w, active, X, theta, y, n_obs, m, s, kind) -> dict:
    """(7m) for one study: mu (T, n') and cov (T, n', n') its columns / rows of the pass (cov[t][i][c]: row of point i, column of point c),
    w, active (T), X (n', D) = X', theta (D + 2), y (n_obs) -> Knn (n', n'), resid (n'), mean (n') as Quantities (the kernel writes mean
    at the pending rows only)."""
    T, n = mu.shape
    D = X.shape[1]
    m, s = LD(m), LD(s)
    os_, noise = LD(theta[D]), LD(theta[D + 1])
    cs, mag, ms, mmag = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for t in range(T):
        if not active[t]:
            continue
        wt = LD(w[t])
        cs += wt * wt * LD(cov[t])
        mag += wt * wt * np.abs(LD(cov[t]))
        ms += wt * LD(mu[t])
        mmag += np.abs(wt) * np.abs(LD(mu[t]))
    g = gamma(T + 2)
    low = np.tril(np.ones((n, n), dtype=bool))
    cs = np.where(low, cs, cs.T)          # element (i, c), c <= i, is fed by cov[t][i][c]; (c, i) is its copy
    mag = np.where(low, mag, mag.T)
    s2 = s * s
    diff = (LD(X)[:, None, :] - LD(X)[None, :, :]) / LD(theta[:D])
    d2 = (diff * diff).sum(-1)
    k = _kernel(d2, kind)[0]
    arg = 0.5 * d2 if kind == 0 else np.sqrt(5.0 * d2)
    E_K = os_ * (_S[kind][0] * gamma(D + 5) * d2 + (10 + 2 * arg) * U * np.abs(k))
    c2 = cs / s2
    v = c2 + os_ * k
    E = g * mag / s2 + 3 * U * np.abs(c2) + E_K + U * np.abs(v)
    idx = np.arange(n)
    v[idx, idx] += noise
    E[idx, idx] += U * np.abs(v[idx, idx])
    mean = (ms - m) / s
    E_mean = g * mmag / s + gamma(2) * np.abs(mean)
    resid, E_r = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    resid[:n_obs] = LD(y[:n_obs]) - mean[:n_obs]
    E_r[:n_obs] = E_mean[:n_obs] * (1 + U) + U * np.abs(resid[:n_obs])
    return dict(Knn=Quantity(v, E, _scale(v)), resid=Quantity(resid, E_r, max(_scale(resid), _scale(mean))),
                mean=Quantity(mean, E_mean, _scale(mean)))


def fantasy_reference(L, resid, mean_p, eps, n_obs, m, s) -> dict:
    """(7n) for one study: L (n', n') (the lower triangle is read), resid (n'), mean_p (n': the pending rows are read), eps (p, F) -- F = 1
    and no rows for an ordinary study -> alpha_f (n', F), and with p > 0 y_fant (p, F), mu_p (p), as Quantities."""
    n, no = L.shape[0], int(n_obs)
    p = n - no
    F = eps.shape[1] if p else 1
    m, s = LD(m), LD(s)
    Ll = LD(np.tril(L))
    Li = inverse_lower(Ll)
    aL, aLi = np.abs(Ll.astype(np.float64)), np.abs(Li.astype(np.float64))
    v = Li[:no, :no] @ LD(resid[:no])
    av = np.abs(v.astype(np.float64))
    E_v = _up(gamma(no + 2) * (aLi[:no, :no] @ (aL[:no, :no] @ av)))
    out = {}
    b, E_b = np.zeros((n, F), dtype=LD), np.zeros((n, F))
    b[:no], E_b[:no] = v[:, None], E_v[:, None]
    if p:
        Lpn, Lpp, e = Ll[no:, :no], Ll[no:, no:], LD(eps)
        mt = LD(mean_p[no:n]) + Lpn @ v
        E_mt = _up(gamma(no + 1) * (aL[no:, :no] @ av + np.abs(mean_p[no:n])) + aL[no:, :no] @ E_v)
        mu_p = m + s * mt
        out["mu_p"] = Quantity(mu_p, float(s) * E_mt + U * np.abs(mu_p), _scale(mu_p))
        yt = mt[:, None] + Lpp @ e
        y = m + s * yt
        E_y = float(s) * (E_mt[:, None] + _up(gamma(p + 1) * (aL[no:, no:] @ np.abs(eps) + np.abs(mt.astype(np.float64))[:, None]))) + U * np.abs(y)
        out["y_fant"] = Quantity(y, E_y, _scale(y))
        b[no:] = e
    x = Li.T @ b
    E_x = _up(aLi.T @ (E_b + gamma(n + 2) * (aL.T @ np.abs(x.astype(np.float64)))))
    out["alpha_f"] = Quantity(x, E_x, _scale(x))
    return out


def check_study(label, kind, got_block, got_fant, ref_block, ref_fant, n_obs):
    """One study's outputs of (7m) (Knn (n', n'), resid (n'), mean_p (n')) and (7n) (alpha_f (n', F), y_fant (p, F), mu_p (p)) within
    their bounds; ``got_fant`` / ``ref_fant`` None: (7m) alone."""
    fam = FAMILY[kind]
    n = got_block["Knn"].shape[0]
    within(label, ("condition_block", fam, "Knn"), got_block["Knn"], ref_block["Knn"])
    within(label, ("condition_block", fam, "resid"), got_block["resid"], ref_block["resid"])
    assert (np.asarray(got_block["resid"])[n_obs:] == 0.0).all(), f"{label}: the pending rows of resid are exactly zero"
    if n > n_obs:
        q = ref_block["mean"]
        within(label, ("condition_block", fam, "mean_p"), got_block["mean_p"][n_obs:], Quantity(q.ref[n_obs:], q.bound[n_obs:], q.scale))
    if ref_fant is None:
        return
    for name, q in ref_fant.items():
        within(label, ("fantasy_condition", fam, name), got_fant[name], q)
