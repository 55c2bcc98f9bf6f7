"""Generates tests/golden/logei/logei_scalar_table.npz (a directory of its own: tests/test_oracle.py takes every tests/golden/*.npz for a stack): g(u) = log(phi(u) + u Phi(u)) and g'(u) = Phi(u) / (phi(u) + u Phi(u)) at 50 digits
(mpmath, working precision 120 digits), each stored as a float64 (hi, lo) pair, for at most 2,048 values of u in [-1e8, 40]:
the branch edges of sa_log_ei_terms (csrc/gp_studies_formulas.h) at -1, 0 and +1 ulp, the points the accuracy contract names,
and a log-spaced fill on both sides of 0.  Run from the repository root:  python tests/golden/make_logei_table.py

For u < 0 the factored form is used, with t = -u and the Mills ratio R(t) = sqrt(pi / 2) exp(t^2 / 2) erfc(t / sqrt 2):
g = -t^2 / 2 - log sqrt(2 pi) + log(1 - t R),  g' = R / (1 - t R);  1 - t R cancels to about 1 / t^2 (1e-16 at t = 1e8), which 120 digits
cover with 50 to spare.  The tests read only the table: mpmath is not needed to run them."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 120
EDGES = (-2.0, -3.0, -5.0, -8.0, -16.0)   # sa_log_ei_terms: direct formula | continued fraction with 112, 72, 36, 20, 12 terms
NAMED = (-1e8, -1e5, -1e3, -200.0, -40.0, -38.5, -9.0, -1.0, -0.5, 0.0, 0.5, 9.0, 40.0)


def g_and_slope(u):
    u = mp.mpf(u)
    if u < 0:
        t = -u
        R = mp.sqrt(mp.pi / 2) * mp.exp(t * t / 2) * mp.erfc(t / mp.sqrt(2))
        om = 1 - t * R
        return -t * t / 2 - mp.log(mp.sqrt(2 * mp.pi)) + mp.log(om), R / om
    pdf, cdf = mp.npdf(u), mp.ncdf(u)
    h = pdf + u * cdf
    return mp.log(h), cdf / h


def hi_lo(x):
    hi = float(x)
    return hi, float(x - mp.mpf(hi))


def main():
    us = set(NAMED)
    for e in EDGES:
        us.update((float(np.nextafter(e, -np.inf)), e, float(np.nextafter(e, np.inf))))
    us.update((-np.logspace(-6, 8, 1200)).tolist())     # the left tail, through every branch
    us.update(np.logspace(-6, np.log10(40.0), 400).tolist())
    us.update(np.linspace(-20.0, 9.0, 400).tolist())
    u = np.array(sorted(x for x in us if -1e8 <= x <= 40.0))
    assert u.size <= 2048
    g, gp = np.empty((u.size, 2)), np.empty((u.size, 2))
    for i, x in enumerate(u):
        a, b = g_and_slope(x)
        g[i], gp[i] = hi_lo(a), hi_lo(b)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "logei", "logei_scalar_table.npz")
    np.savez_compressed(out, u=u, g=g, gp=gp, edges=np.array(EDGES), named=np.array(NAMED))
    print(f"{out}: {u.size} points, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
