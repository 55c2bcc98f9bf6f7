"""The joint q-point acquisition body (csrc/gp_qacqf.h: qa_batch / qa_tail, the arithmetic of scaml_target_qacqf_f64 (7p),
scaml_target_qacqf_pending_f64 (7q) and scaml_target_qacqf_value_f64 (7r)) through its host builds (tests/host_emul/qacqf_emul.cpp,
qacqf_pending_emul.cpp, qacqf_value_emul.cpp) against the long-double reference of tests/_qacqf_bounds.py, value and gradient held
element by element to its a-priori bound, on the input sets that module lists.  tests/test_qacqf_bounds_gpu.py runs the same sets
through the C ABI on the device.

That the bound DISCRIMINATES is shown here, on the CPU only: for each planted arithmetic error the header is copied to a temporary
directory, one textual substitution is applied (the pattern must occur exactly once), the host build is compiled against the copy and
the shared check must reject it on a named set.  Every mutant changes a number only; none is built or run for the GPU.
profiles/qacqf_bounds_notes.md records the ratios and the mutants' first failing elements."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _qacqf_bounds as QB
from tests._host_emul import CSRC, DP, IP, ROOT, ptr as _ptr
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF, SENTINEL
from tests._qacqf_bounds import EI, UCB

_I, _F = ctypes.c_int, ctypes.c_double
FAMILIES = pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])
CODES = pytest.mark.parametrize("acqf", [UCB, EI], ids=["qucb", "qei"])
HEADER = os.path.join(CSRC, "gp_qacqf.h")


def _build(out_dir, name, first_include=None):
    so = os.path.join(str(out_dir), name + ".so")
    inc = (["-I", str(first_include)] if first_include else []) + ["-I", CSRC]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", *inc, os.path.join(ROOT, "tests", "host_emul", name + ".cpp"), "-o", so],
                   check=True)
    return ctypes.CDLL(so)


def _p(x):
    return None if x is None or x.size == 0 else _ptr(x)


class Host:
    """The backend of tests/_qacqf_bounds.py on the host builds: every output through a buffer full of the sentinel with one guard row."""

    def __init__(self, out_dir, first_include=None):
        self.libs = {"7p": _build(out_dir, "qacqf_emul", first_include), "7q": _build(out_dir, "qacqf_pending_emul", first_include),
                     "7r": _build(out_dir, "qacqf_value_emul", first_include)}
        self.libs["7p"].emul_qacqf.restype = _I
        self.libs["7p"].emul_qacqf.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 7 + [_I, _F] + [_I] * 6 + [DP, DP, DP, IP]
        self.libs["7p"].emul_qacqf_tail.restype = _I
        self.libs["7p"].emul_qacqf_tail.argtypes = [DP, DP, DP, _I, _I, _I, _F, DP, DP, DP, DP, IP]
        self.libs["7q"].emul_qacqf_pending.restype = _I
        self.libs["7q"].emul_qacqf_pending.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 11 + [_I, _F] + [_I] * 7 + [DP, DP, DP, IP]
        self.libs["7r"].emul_qacqf_value.restype = _I
        self.libs["7r"].emul_qacqf_value.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 8 + [_I, _F] + [_I] * 8 + [DP, DP, IP]

    def run(self, a, info):
        c = {k: (None if a.get(k) is None else np.ascontiguousarray(a[k], dtype=np.float64)) for k in
             ("Knq", "Z", "alpha", "mean_q", "var_q", "cov", "mu_g", "var_g", "Xt", "Xq", "theta", "eps", "Xp", "Zp", "mu_p", "Sigma_pp")}
        n, q, p, S, D, Bn = a["n"], a["q"], a["p"], a["S"], a["D"], a["B"]
        Mq = c["Knq"].shape[1]
        inf = None if info is None else np.array([info], dtype=np.int32)
        value, jitter = np.full(Bn + 1, SENTINEL), np.full(Bn + 1, SENTINEL)
        info_out = np.full(Bn + 1, QB.ISENTINEL, dtype=np.int32)
        grad = None if a["layout"] == "value" else np.full((Bn * q + 1, D), SENTINEL)
        head = [_p(c[k]) for k in ("Knq", "Z", "alpha", "mean_q", "var_q")] + [a["m"], a["s"], _p(inf)]
        pend = [_p(c[k]) for k in ("Xp", "Zp", "mu_p", "Sigma_pp")]
        if a["entry"] == "7p":
            assert p == 0
            rc = self.libs["7p"].emul_qacqf(*head, *[_p(c[k]) for k in ("cov", "mu_g", "var_g", "Xt", "Xq", "theta", "eps")], a["acqf"], a["param"],
                                            n, Mq, q, S, D, a["kind"], _p(value), _p(grad), _p(jitter), _p(info_out))
        elif a["entry"] == "7q":
            rc = self.libs["7q"].emul_qacqf_pending(*head, *[_p(c[k]) for k in ("cov", "mu_g", "var_g", "Xt", "Xq", "theta", "eps")], *pend, a["acqf"],
                                                    a["param"], n, Mq, q, p, S, D, a["kind"], _p(value), _p(grad), _p(jitter), _p(info_out))
        else:
            rc = self.libs["7r"].emul_qacqf_value(*head, *[_p(c[k]) for k in ("cov", "Xq", "theta", "eps")], *pend, a["acqf"], a["param"], n, Mq, Bn,
                                                  q, p, S, D, a["kind"], _p(value), _p(jitter), _p(info_out))
        assert value[-1] == SENTINEL and jitter[-1] == SENTINEL and info_out[-1] == QB.ISENTINEL and (grad is None or (grad[-1] == SENTINEL).all()), \
            "the call wrote past the end of an output"
        if rc == 0:
            assert not (value[:-1] == SENTINEL).any() and not (jitter[:-1] == SENTINEL).any() and not (info_out[:-1] == QB.ISENTINEL).any() \
                and (grad is None or not (grad[:-1] == SENTINEL).any()), "an output entry was not written"
        return rc, value[:-1], (None if grad is None else grad[:-1]), jitter[:-1], info_out[:-1]

    def tail(self, mu, Sigma, eps, acqf, par):
        q, S = len(mu), eps.shape[0]
        Sg, m, e = (np.ascontiguousarray(x, dtype=np.float64) for x in (Sigma, mu, eps))
        value, jit, mubar, Sbar = np.full(1, 7.0), np.full(1, 7.0), np.full(q, 7.0), np.full((q, q), 7.0)
        info = np.full(1, 7, dtype=np.int32)
        assert self.libs["7p"].emul_qacqf_tail(_ptr(Sg), _ptr(m), _ptr(e), q, S, acqf, par, _ptr(value), _ptr(mubar), _ptr(Sbar), _ptr(jit), _ptr(info)) == 0
        return float(value[0]), mubar, Sbar, float(jit[0]), int(info[0])


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    return Host(tmp_path_factory.mktemp("qacqf_bounds"))


def _show():
    for line in QB.report():
        print(line)


ALL_SHAPES = [("7p", s) for s in QB.SETS_7P] + [("7q", s) for s in QB.SETS_7Q]
_ids = [f"{e}-{QB.set_id(s)}" for e, s in ALL_SHAPES]


def _every_set():
    """Every finite set of the module, by name."""
    for kind in QB.KINDS:
        for acqf in QB.CODES:
            for entry, shape in ALL_SHAPES:
                yield QB.make(entry, shape, kind, acqf), QB.CAP
            for shape in QB.SETS_7R:
                yield QB.to_value_layout(QB.make("7q" if shape[2] else "7p", shape, kind, acqf)), QB.CAP
            for cond in QB.CONDS:
                yield QB.make("7p", QB.COND_SHAPE, kind, acqf, cond=cond), QB.CAP
            yield QB.ladder_inputs(kind, acqf), QB.NORTH_STAR
            yield QB.make("7q", QB.NONFINITE_SHAPE, kind, acqf), QB.CAP
        yield QB.make("7p", (17, 3, 0, 5, 2, 5), kind, EI, best="below"), QB.CAP
        yield QB.make("7p", (17, 3, 0, 5, 2, 5), kind, UCB, beta=0.0), QB.CAP


def test_caps_and_conditions_hold_on_every_set_from_the_reference_alone():
    """No kernel runs here: the reference's own bounds meet the caps (1e-8 of the scale; the ladder sets 1e-4) and its own quantities
    the conditions -- first order suffices, every pivot, winner and clamp is MARGIN bounds away from changing.  No sample and no set
    is left out."""
    count = 0
    for a, cap in _every_set():
        ref = QB.reference(a)
        QB.conditions(a["name"], ref)
        for name in ("value", "grad"):
            if name in ref:
                qn = ref[name]
                worst = float(qn.bound[np.isfinite(qn.bound)].max())
                assert worst <= cap * qn.scale, f"{a['name']} {name}: bound {worst:.3e} over {cap} x {qn.scale:.3e}"
        count += 1
    print(f"{count} sets")


@FAMILIES
@pytest.mark.parametrize("entry,shape", ALL_SHAPES, ids=_ids)
def test_value_and_gradient_within_their_bounds(be, entry, shape, kind):
    """(7p) and (7q), both codes (qEI with best_f in the bulk), info NULL / 0 / 2; sentinel-filled outputs."""
    QB.check_shape(be, entry, shape, kind)
    _show()


@FAMILIES
@pytest.mark.parametrize("shape", QB.SETS_7R, ids=QB.set_id)
def test_value_layout_within_its_bound_and_bit_equal_to_the_grad_layout(be, shape, kind):
    QB.check_value_layout(be, shape, kind)
    _show()


@FAMILIES
@pytest.mark.parametrize("cond", QB.CONDS, ids=lambda c: f"cond{c:.0e}")
def test_conditioning(be, cond, kind):
    """q = 8 with cond(Sigma) = 1e2 and 1e6."""
    QB.check_cond(be, cond, kind)
    _show()


@FAMILIES
def test_best_f_below_every_sample_gives_exact_zeros(be, kind):
    QB.check_below(be, kind)


@FAMILIES
def test_qucb_with_beta_zero(be, kind):
    QB.check_beta0(be, kind)


@CODES
@FAMILIES
def test_ladder(be, kind, acqf):
    """jitter exactly 0, 1e-8, 1e-7, 1e-6, NaN; info (0, 0, 0, 0, 1); batch 4 NaN; batches 0 .. 3 within their bounds and bit-equal to a
    call without batch 4."""
    QB.check_ladder(be, kind, acqf)
    _show()


@CODES
@pytest.mark.parametrize("what", sorted(QB.NONFINITE))
def test_non_finite_inputs(be, what, acqf):
    QB.check_nonfinite(be, what, KIND_MATERN52 if acqf == EI else KIND_RBF, acqf)


@pytest.mark.parametrize("entry", ["7p", "7q", "7r"])
def test_two_calls_bit_for_bit(be, entry):
    QB.check_twice(be, entry, KIND_RBF, EI)


# ---- exact bit patterns: only the tail entry can be handed them -------------------------------------------------------------------
@CODES
def test_an_exact_tie_takes_the_lowest_index(be, acqf):
    """Sigma = I (C = I exactly), equal means: a sample with eps_0 == eps_1 ties the two utilities exactly; the weight goes to point 0.
    Samples 4 .. 7 are won by point 1 strictly (S = 8: 1 / S is exact)."""
    eps = np.array([[0.5, 0.5], [-1.25, -1.25], [2.0, 2.0], [0.0, 0.0], [0.5, -3.0], [1.0, -2.0], [-0.5, -1.5], [0.25, -4.0]])
    par = 8.0 if acqf == EI else 4.0
    value, mubar, Sbar, jit, info = be.tail(np.array([0.25, 0.25]), np.eye(2), eps, acqf, par)
    assert info == 0 and jit == 0.0
    assert mubar[0] == -0.5 and mubar[1] == -0.5, f"mubar {mubar}"
    # and with the points swapped in the samples that are not tied, point 0 takes them too
    value, mubar, _, _, _ = be.tail(np.array([0.25, 0.25]), np.eye(2), eps[:, ::-1].copy(), acqf, par)
    assert mubar[0] == -1.0 and mubar[1] == 0.0, f"mubar {mubar}"


def test_the_slope_is_exactly_zero_on_the_kinks(be):
    one = np.ones((1, 1))
    # qEI: best == 0 exactly (best_f - (mu + z) = 1 - (0 + 1)): no improvement, no weight
    value, mubar, Sbar, _, info = be.tail(np.zeros(1), one, one, EI, 1.0)
    assert info == 0 and value == 0.0 and mubar[0] == 0.0 and Sbar[0, 0] == 0.0
    value, mubar, Sbar, _, _ = be.tail(np.zeros(1), one, 0.5 * one, EI, 1.0)
    assert value == 0.5 and mubar[0] == -1.0 and Sbar[0, 0] == -0.25          # d value / d Sigma = -eps / (2 C)
    # qUCB: z_b == 0 exactly: the value is -mu, the slope on C is 0
    value, mubar, Sbar, _, info = be.tail(np.array([0.75]), one, 0.0 * one, UCB, 4.0)
    assert info == 0 and value == -0.75 and mubar[0] == -1.0 and Sbar[0, 0] == 0.0
    value, mubar, Sbar, _, _ = be.tail(np.array([0.75]), one, -0.5 * one, UCB, 4.0)
    assert Sbar[0, 0] > 0.0


# ---- the bound discriminates ----------------------------------------------------------------------------------------------------
# (name, pattern, replacement, the set it must be rejected on: entry, shape, kind, code, and the output that fails first)
MUTANTS = [
    ("mate weight without its factor 2", "u = k == j ? 0.0 : 2.0 * s2 * Sb[j * 8 + k];", "u = k == j ? 0.0 : s2 * Sb[j * 8 + k];",
     ("7p", (17, 3, 0, 5, 2, 5), KIND_RBF, UCB)),
    ("the point's own mate row weighted", "u = k == j ? 0.0 : 2.0 * s2 * Sb[j * 8 + k];", "u = 2.0 * s2 * Sb[j * 8 + k];",
     ("7p", (17, 3, 0, 5, 2, 5), KIND_MATERN52, EI)),
    ("diagonal of Phi not halved", "T1[e] = i == j ? 0.5 * acc : acc;", "T1[e] = acc;", ("7p", (17, 3, 0, 5, 2, 5), KIND_RBF, EI)),
    ("1 / S from 4 * chunk", "const double invS = 1.0 / (double)S;", "const double invS = 1.0 / (double)(4 * chunk);",
     ("7p", (9, 5, 0, 257, 6, 2), KIND_RBF, EI)),
    ("last sample dropped", "s_hi = s_lo + chunk < S ? s_lo + chunk : S;", "s_hi = s_lo + chunk < S ? s_lo + chunk : S - 1;",
     ("7p", (9, 5, 0, 257, 6, 2), KIND_MATERN52, UCB)),
    ("ucb_c without pi / 2", "sqrt(par * 1.5707963267948966192)", "sqrt(par)", ("7p", (20, 4, 0, 2, 6, 3), KIND_RBF, UCB)),
    ("pending weight read at Sb[j * 8 + k]", "sz = fma(Sb[j * 8 + q + k], Zpl[a * 8 + k], sz);", "sz = fma(Sb[j * 8 + k], Zpl[a * 8 + k], sz);",
     ("7q", (17, 2, 3, 300, 2, 5), KIND_RBF, EI)),
    ("mate row read at n + k under pending", "prior = p.cov_g[(size_t)(n + P + k) * W", "prior = p.cov_g[(size_t)(n + k) * W",
     ("7q", (20, 7, 1, 64, 6, 3), KIND_MATERN52, UCB)),
    ("slope scaled by 1 + 1e-7", "SL[j * R + a] = 2.0 * u * dk;", "SL[j * R + a] = 2.0 * u * dk * (1.0 + 1e-7);",
     ("7p", (17, 3, 0, 5, 2, 5), KIND_RBF, UCB)),
]


@pytest.mark.parametrize("name,pattern,replacement,where", MUTANTS, ids=[m[0].replace(" ", "-") for m in MUTANTS])
def test_the_bound_rejects_a_planted_error(be, tmp_path, name, pattern, replacement, where):
    with open(HEADER) as f:
        text = f.read()
    assert text.count(pattern) == 1, f"`{pattern}` occurs {text.count(pattern)} times in csrc/gp_qacqf.h"
    (tmp_path / "gp_qacqf.h").write_text(text.replace(pattern, replacement))
    with open(os.path.join(CSRC, "gp_dispatch.h")) as f:          # (includes the header by name: next to the copy it takes the copy)
        (tmp_path / "gp_dispatch.h").write_text(f.read())
    mutant = Host(tmp_path, first_include=tmp_path)
    entry, shape, kind, acqf = where
    a = QB.make(entry, shape, kind, acqf)
    ref = QB.reference(a)
    QB.hold(a["name"], a, ref, be.run(a, None))                  # (the header as it is passes on the same set)
    with pytest.raises(AssertionError, match=r"error .* > bound") as exc:
        QB.hold(a["name"], a, ref, mutant.run(a, None))
    msg = str(exc.value)
    m = re.search(r"error (\S+) > bound (\S+)", msg)
    print(f"mutant `{name}` on {a['name']}: {msg}  [error / bound = {float(m.group(1)) / float(m.group(2)):.3e}]")
