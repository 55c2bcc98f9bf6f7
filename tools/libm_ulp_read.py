"""Reader of tools/libm_ulp_probe.hip's output: the device library's erf and exp against the long-double reference of
tests/_fantasy_bounds.py, in units of the fp64 spacing at the reference value, and the constants the bound takes from them:
max(2, ceil(2 x largest observed ulp error)) -- the factor 2 because the sweep samples the domain rather than exhausting it.

    python tools/libm_ulp_read.py /tmp/libm_ulp.bin
    python tools/libm_ulp_read.py /tmp/libm_ulp_logei.bin logei     (the probe run with a third argument "logei")
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _fantasy_bounds as FB  # noqa: E402


def _line(name, x, ulp, sel):
    if not sel.any():
        print(f"{name}: no arguments")
        return 0.0
    u = np.where(sel, ulp, 0)
    i = int(np.argmax(u))
    print(f"{name}: {int(sel.sum())} arguments, largest error {float(u[i]):.4f} ulp at x = {float(x[i])!r}, mean {float(ulp[sel].mean()):.4f} ulp")
    return float(u[i])


def main_logei(xe, ye, xx, yx):
    """The "logei" mode of the probe: erfc and log for ERFC_U / LOG_U of tests/_logei_bounds.py.  Reference erfc = 1 - erf in long
    double: over [-29, 1.4143] erfc >= 0.0455, so the subtraction loses at most a factor 22 of eps_LD (0.01 ulp of fp64)."""
    from tests import _logei_bounds as LB
    ulp_c = FB.ulp_errors(xe, ye, 1 - FB.erf_ld(xe))
    worst_c = _line("erfc, [-29, 1.4143] grid and 1e-300 .. 1 log-spaced", xe, ulp_c, np.ones(xe.size, dtype=bool))
    ulp_l = FB.ulp_errors(xx, yx, np.log(FB.LD(xx)))
    worst_l = _line("log, [1e-20, 100] log-spaced", xx, ulp_l, np.ones(xx.size, dtype=bool))
    print(f"ERFC_U = max(2, ceil(2 x {worst_c:.4f})) = {max(2, math.ceil(2 * worst_c))}")
    print(f"LOG_U = max(2, ceil(2 x {worst_l:.4f})) = {max(2, math.ceil(2 * worst_l))}")
    print(f"module constants: ERFC_U = {LB.ERFC_U}, LOG_U = {LB.LOG_U}")


def main(path, mode=""):
    raw = np.fromfile(path, dtype=np.float64)
    assert raw.size % 4 == 0 and raw.size, f"{path}: {raw.size} doubles"
    xe, ye, xx, yx = raw.reshape(4, -1)
    if mode == "logei":
        return main_logei(xe, ye, xx, yx)
    n = xe.size
    nu = n - n // 8
    grid = np.arange(n) < nu
    ref_e = FB.erf_ld(xe)
    ulp_e = FB.ulp_errors(xe, ye, ref_e)
    worst_erf = max(_line("erf, [-6.5, 6.5] grid", xe, ulp_e, grid), _line("erf, 1e-300 .. 1 log-spaced", xe, ulp_e, ~grid))
    ref_x = np.exp(FB.LD(xx))
    ulp_x = FB.ulp_errors(xx, yx, ref_x)
    normal = ref_x >= FB.LD(2) ** -1022
    worst_exp = max(_line("exp, [-745, 0] grid, normal results", xx, ulp_x, grid & normal), _line("exp, -1 .. -1e-300 log-spaced", xx, ulp_x, ~grid))
    worst_sub = _line("exp, [-745, 0] grid, subnormal results (units of 2^-1074)", xx, ulp_x, grid & ~normal)
    erf_u, exp_u = max(2, math.ceil(2 * worst_erf)), max(2, math.ceil(2 * worst_exp))
    print(f"ERF_U = max(2, ceil(2 x {worst_erf:.4f})) = {erf_u}")
    print(f"EXP_U = max(2, ceil(2 x {worst_exp:.4f})) = {exp_u}   (EXP_U = 2 {'confirmed' if exp_u == 2 else 'NOT confirmed'})")
    print(f"subnormal exp results within {worst_sub:.4f} x 2^-1074   (the bound's absolute term on pdf takes 1 x 2^-1074 after the product with "
          f"0.3989: needs <= {1 / 0.39894228 - 0.5 / 0.39894228:.3f})")
    print(f"module constants: ERF_U = {FB.ERF_U}, EXP_U = {FB.EXP_U}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
