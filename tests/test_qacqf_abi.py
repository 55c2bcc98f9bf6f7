"""scaml_posterior_linv_grad_joint_f64 (5g) and scaml_target_qacqf_f64 (7p), the joint q-point acquisition entry points: exported, and
every argument check and size limit answers before any HIP call -- no GPU needed."""
import ctypes

from scamlgp_amd import _lib, ops

one = ctypes.c_void_p(16)   # never dereferenced: validation fails first


def _joint(T=2, N=64, Mq=6, Ma=4, q=3, D=3, kind=0, flags=0, null=()):
    a = dict(Xq=one, Xa=one, X=one, theta=one, Linv=one, alpha=one, VA=one, VQ=one, cov=one)
    for k in null:
        a[k] = None
    return _lib.lib.scaml_posterior_linv_grad_joint_f64(a["Xq"], a["Xa"], a["X"], a["theta"], a["Linv"], a["alpha"], None, None, None, a["VA"],
                                                        a["VQ"], T, N, Mq, Ma, q, D, kind, one, one, a["cov"], flags, None)


def _qacqf(n=8, Mq=6, q=3, S=16, D=3, kind=0, acqf=1, s_all=1.0, grad=True, null=()):
    names = ("Knq", "Z", "alpha", "mean_q", "var_q", "cov_g", "mu_g", "var_g", "Xt", "Xq", "theta", "base_samples", "value")
    a = {k: (None if k in null else one) for k in names}
    return _lib.lib.scaml_target_qacqf_f64(a["Knq"], a["Z"], a["alpha"], a["mean_q"], a["var_q"], 0.0, s_all, None, a["cov_g"], a["mu_g"],
                                           a["var_g"], a["Xt"], a["Xq"], a["theta"], a["base_samples"], acqf, 0.5, n, Mq, q, S, D, kind,
                                           a["value"], one if grad else None, None, None, None)


def test_symbols_and_limits():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("scaml_posterior_linv_grad_joint_f64", "scaml_target_qacqf_f64", "scaml_qacqf_max_q", "scaml_qacqf_max_samples"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name)
    assert _lib.lib.scaml_qacqf_max_q() == ops.qacqf_max_q() == 8
    assert _lib.lib.scaml_qacqf_max_samples() == ops.qacqf_max_samples() == 512


def test_joint_pass_bad_arguments():
    for k in ("Xq", "Xa", "X", "theta", "Linv", "alpha", "VA", "VQ", "cov"):
        assert _joint(null=(k,)) == _lib.E_BADARG, k
    assert _joint(q=0) == _lib.E_BADARG
    assert _joint(Mq=7, q=3) == _lib.E_BADARG          # Mq is not a multiple of q
    assert _joint(Ma=0) == _lib.E_BADARG
    assert _joint(Mq=-3) == _lib.E_BADARG
    assert _joint(D=0) == _lib.E_BADARG
    assert _joint(N=0) == _lib.E_BADARG
    assert _joint(T=-1) == _lib.E_BADARG
    assert _joint(kind=5) == _lib.E_BADARG
    assert _joint(flags=_lib.POST_MEAN_ONLY) == _lib.E_BADARG
    assert _joint(q=9, Mq=7) == _lib.E_BADARG          # bad arguments answer before size limits


def test_joint_pass_size_limits():
    assert _joint(q=9, Mq=9) == _lib.E_TOOLARGE
    assert _joint(D=16) == _lib.E_TOOLARGE
    assert _joint(N=128, Ma=89, q=8, Mq=8) == _lib.E_TOOLARGE    # Ma + q > 96
    assert _joint(N=32, Ma=30, q=3, Mq=3) == _lib.E_TOOLARGE     # Ma + q > N
    assert _joint(N=100000) == _lib.E_TOOLARGE
    assert _joint(N=96, Ma=88, q=8, Mq=0, D=15) == 0             # at the limits, no query points: a no-op
    assert _joint(T=0) == 0


def test_qacqf_bad_arguments():
    for k in ("Knq", "Z", "alpha", "mean_q", "var_q", "cov_g", "mu_g", "var_g", "Xt", "Xq", "theta", "base_samples", "value"):
        assert _qacqf(null=(k,)) == _lib.E_BADARG, k
    for code in (17, 0x10, 2, 3, 0x12, -1):            # LogEI and the log flag alone are refused here, like every unknown code
        assert _qacqf(acqf=code) == _lib.E_BADARG, code
    assert _qacqf(n=0) == _lib.E_BADARG
    assert _qacqf(q=0) == _lib.E_BADARG
    assert _qacqf(S=0) == _lib.E_BADARG
    assert _qacqf(D=0) == _lib.E_BADARG
    assert _qacqf(Mq=-1) == _lib.E_BADARG
    assert _qacqf(Mq=7, q=3) == _lib.E_BADARG
    assert _qacqf(s_all=0.0) == _lib.E_BADARG
    assert _qacqf(kind=5) == _lib.E_BADARG
    assert _qacqf(q=9, Mq=9, acqf=17) == _lib.E_BADARG   # bad arguments answer before size limits


def test_qacqf_size_limits():
    assert _qacqf(q=9, Mq=9) == _lib.E_TOOLARGE
    assert _qacqf(S=513) == _lib.E_TOOLARGE
    assert _qacqf(n=94, q=3) == _lib.E_TOOLARGE          # n + q > 96
    assert _qacqf(D=16) == _lib.E_TOOLARGE
    assert _qacqf(n=88, q=8, Mq=0, S=512, D=15) == 0    # at the limits, no batches: a no-op
    assert _qacqf(n=88, q=8, Mq=0, S=512, D=15, grad=False, acqf=0) == 0
