"""scaml_posterior_linv_cov_joint_f64 (5h), scaml_target_qacqf_value_f64 (7r) and scaml_qacqf_value_columns, the value-only route of
the joint q-point acquisition: exported, and every argument check and size limit answers before any HIP call -- no GPU needed."""
import ctypes

from scamlgp_amd import _lib, ops

one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
SYMBOLS = ("scaml_posterior_linv_cov_joint_f64", "scaml_target_qacqf_value_f64", "scaml_qacqf_value_columns")
SRC = ("Xq", "Xa", "X", "theta", "Linv", "alpha", "VA", "cov")
NAMES = ("Knq", "Z", "alpha", "mean_q", "var_q", "cov_s", "Xq", "theta", "base_samples", "value")
PENDING = ("Xp", "Zp", "mu_p", "Sigma_pp")
cols = _lib.lib.scaml_qacqf_value_columns


def _src(T=2, N=64, Mp=None, Ma=8, B=6, q=3, D=3, kind=0, flags=0, null=()):
    a = {k: (None if k in null else one) for k in SRC}
    Mp = cols(B, q) if Mp is None else Mp
    return _lib.lib.scaml_posterior_linv_cov_joint_f64(a["Xq"], a["Xa"], a["X"], a["theta"], a["Linv"], a["alpha"], None, None, None, a["VA"],
                                                       T, N, Mp, Ma, B, q, D, kind, None, None, a["cov"], flags, None)


def _acq(n=8, Mp=None, B=6, q=3, p=2, S=16, D=3, kind=0, acqf=1, s_all=1.0, null=()):
    a = {k: (None if k in null else one) for k in NAMES + PENDING}
    Mp = cols(B, q) if Mp is None else Mp
    return _lib.lib.scaml_target_qacqf_value_f64(a["Knq"], a["Z"], a["alpha"], a["mean_q"], a["var_q"], 0.0, s_all, None, a["cov_s"], a["Xq"],
                                                 a["theta"], a["base_samples"], a["Xp"], a["Zp"], a["mu_p"], a["Sigma_pp"], acqf, 0.5, n, Mp, B,
                                                 q, p, S, D, kind, a["value"], None, None, None)


def test_symbols():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(dll, s), s
    for f in ("source_posteriors_cov_joint", "target_qacqf_value", "qacqf_value_columns"):
        assert hasattr(ops, f), f


def test_columns():
    # bps = 16 // q whole batches per strip of 16 columns
    assert [cols(1, q) for q in range(1, 9)] == [16] * 8
    assert cols(0, 4) == 0 and cols(4, 4) == 16 and cols(5, 4) == 32 and cols(1024, 4) == 4096
    assert cols(5, 3) == 16 and cols(6, 3) == 32 and cols(17, 1) == 32 and cols(2, 7) == 16 and cols(3, 7) == 32
    for B, q in ((-1, 2), (3, 0), (3, 9), (3, -1), (2 ** 26 + 1, 1)):
        assert cols(B, q) == -1, (B, q)
    assert ops.qacqf_value_columns(6, 3) == 32


def test_source_pass_bad_arguments():
    for k in SRC:
        assert _src(null=(k,)) == _lib.E_BADARG, k
    for kw in (dict(T=-1), dict(N=0), dict(Mp=-16), dict(Ma=0), dict(B=-1, Mp=0), dict(q=0, Mp=16), dict(D=0), dict(kind=5),
               dict(flags=_lib.POST_MEAN_ONLY)):
        assert _src(**kw) == _lib.E_BADARG, kw
    # Mp is not scaml_qacqf_value_columns(B, q)
    assert _src(B=6, q=3, Mp=16) == _lib.E_BADARG
    assert _src(B=6, q=3, Mp=18) == _lib.E_BADARG
    assert _src(B=0, q=3, Mp=16) == _lib.E_BADARG
    # bad arguments answer before size limits
    assert _src(Ma=95, null=("VA",)) == _lib.E_BADARG
    assert _src(N=513, kind=5) == _lib.E_BADARG
    assert _src(q=9, Mp=16, null=("cov",)) == _lib.E_BADARG
    assert _src(Ma=95, B=6, q=3, Mp=16) == _lib.E_BADARG


def test_source_pass_size_limits():
    assert _src(q=9, Mp=16) == _lib.E_TOOLARGE
    assert _src(q=2 ** 30, Mp=16) == _lib.E_TOOLARGE
    assert _src(N=128, Ma=94, q=3) == _lib.E_TOOLARGE            # Ma + q = 97
    assert _src(N=128, Ma=2 ** 31 - 1, q=3) == _lib.E_TOOLARGE   # (no overflow in the sum)
    assert _src(N=32, Ma=30, q=3) == _lib.E_TOOLARGE             # Ma + q > N
    assert _src(N=513) == _lib.E_TOOLARGE
    assert _src(N=512, D=4000) == _lib.E_TOOLARGE                # the LDS footprint
    assert _src(B=2 ** 26 + 1, q=1, Mp=16) == _lib.E_TOOLARGE
    # at the limits, nothing to do: a no-op (no HIP call)
    assert _src(N=96, Ma=89, q=7, B=0, Mp=0) == 0
    assert _src(N=32, Ma=17, q=3, B=0, Mp=0) == 0
    assert _src(T=0, N=512, Ma=88, q=8, B=2, Mp=16) == 0


def test_acquisition_bad_arguments():
    for k in NAMES + PENDING:
        assert _acq(null=(k,)) == _lib.E_BADARG, k
    for kw in (dict(p=-1), dict(n=0), dict(q=0, Mp=16), dict(S=0), dict(D=0), dict(B=-1, Mp=0), dict(Mp=-16), dict(s_all=0.0), dict(kind=5)):
        assert _acq(**kw) == _lib.E_BADARG, kw
    for code in (17, 0x10, 2, 3, 0x12, -1):             # LogEI and the log flag alone are refused, like every unknown code
        assert _acq(acqf=code) == _lib.E_BADARG, code
    assert _acq(B=6, q=3, Mp=16) == _lib.E_BADARG       # Mp is not scaml_qacqf_value_columns(B, q)
    assert _acq(B=6, q=3, Mp=48) == _lib.E_BADARG
    # bad arguments answer before size limits
    assert _acq(q=3, p=6, acqf=17) == _lib.E_BADARG
    assert _acq(q=3, p=6, null=("Zp",)) == _lib.E_BADARG
    assert _acq(S=513, B=6, q=3, Mp=16) == _lib.E_BADARG
    assert _acq(D=16, null=("cov_s",)) == _lib.E_BADARG


def test_acquisition_size_limits():
    assert _acq(q=3, p=6) == _lib.E_TOOLARGE              # q + p = 9
    assert _acq(q=1, p=8) == _lib.E_TOOLARGE
    assert _acq(q=9, p=0, Mp=16) == _lib.E_TOOLARGE
    assert _acq(n=92, q=3, p=2) == _lib.E_TOOLARGE        # n + p + q = 97
    assert _acq(S=513) == _lib.E_TOOLARGE
    assert _acq(D=16) == _lib.E_TOOLARGE
    assert _acq(q=2 ** 30, p=2 ** 30, Mp=16) == _lib.E_TOOLARGE   # (no overflow in the sums)
    # at the limits, no batches: a no-op
    assert _acq(n=88, q=3, p=5, B=0, S=512, D=15) == 0
    assert _acq(n=88, q=1, p=7, B=0, S=512, D=15, acqf=0) == 0
    # no pending points: their arrays may be NULL
    assert _acq(n=88, q=8, p=0, B=0, S=512, D=15, null=PENDING) == 0
