"""scaml_target_qacqf_pending_f64 (7q), the joint q-point acquisition with evaluations pending: exported, and every argument check and
size limit answers before any HIP call -- no GPU needed."""
import ctypes

from scamlgp_amd import _lib, ops

one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
NAMES = ("Knq", "Z", "alpha", "mean_q", "var_q", "cov_g", "mu_g", "var_g", "Xt", "Xq", "theta", "base_samples", "value")
PENDING = ("Xp", "Zp", "mu_p", "Sigma_pp")


def _call(n=8, Mq=6, q=3, p=2, S=16, D=3, kind=0, acqf=1, s_all=1.0, grad=True, null=()):
    a = {k: (None if k in null else one) for k in NAMES + PENDING}
    return _lib.lib.scaml_target_qacqf_pending_f64(a["Knq"], a["Z"], a["alpha"], a["mean_q"], a["var_q"], 0.0, s_all, None, a["cov_g"], a["mu_g"],
                                                   a["var_g"], a["Xt"], a["Xq"], a["theta"], a["base_samples"], a["Xp"], a["Zp"], a["mu_p"],
                                                   a["Sigma_pp"], acqf, 0.5, n, Mq, q, p, S, D, kind, a["value"], one if grad else None, None,
                                                   None, None)


def test_symbol():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert "scaml_target_qacqf_pending_f64" in _lib.EXPORTED_SYMBOLS and hasattr(dll, "scaml_target_qacqf_pending_f64")
    assert hasattr(ops, "target_qacqf_pending")


def test_bad_arguments():
    for k in NAMES + PENDING:
        assert _call(null=(k,)) == _lib.E_BADARG, k
    assert _call(p=-1) == _lib.E_BADARG
    assert _call(Mq=7, q=3) == _lib.E_BADARG            # Mq is not a multiple of q
    for code in (17, 0x10, 2, 3, 0x12, -1):             # LogEI and the log flag alone are refused, like every unknown code
        assert _call(acqf=code) == _lib.E_BADARG, code
    assert _call(n=0) == _lib.E_BADARG
    assert _call(q=0, Mq=0) == _lib.E_BADARG
    assert _call(S=0) == _lib.E_BADARG
    assert _call(D=0) == _lib.E_BADARG
    assert _call(Mq=-1) == _lib.E_BADARG
    assert _call(s_all=0.0) == _lib.E_BADARG
    assert _call(kind=5) == _lib.E_BADARG
    # bad arguments answer before size limits
    assert _call(q=3, p=6, Mq=6, acqf=17) == _lib.E_BADARG
    assert _call(q=3, p=6, Mq=6, null=("Zp",)) == _lib.E_BADARG
    assert _call(S=513, Mq=7, q=3) == _lib.E_BADARG


def test_size_limits():
    assert _call(q=3, p=6, Mq=6) == _lib.E_TOOLARGE              # q + p = 9
    assert _call(q=1, p=8, Mq=6) == _lib.E_TOOLARGE
    assert _call(n=92, q=3, p=2) == _lib.E_TOOLARGE              # n + p + q = 97
    assert _call(S=513) == _lib.E_TOOLARGE
    assert _call(D=16) == _lib.E_TOOLARGE
    assert _call(q=2 ** 30, p=2 ** 30, Mq=0) == _lib.E_TOOLARGE  # (no overflow in the sums)
    # at the limits, no batches: a no-op
    assert _call(n=88, q=3, p=5, Mq=0, S=512, D=15) == 0
    assert _call(n=88, q=1, p=7, Mq=0, S=512, D=15, grad=False, acqf=0) == 0
    # no pending points: their arrays may be NULL
    assert _call(n=88, q=8, p=0, Mq=0, S=512, D=15, null=PENDING) == 0
