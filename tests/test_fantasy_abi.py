"""scaml_target_fantasy_acqf_f64 (the fantasy-model acquisition kernel): exported, and its argument checks and size limits answer
before any HIP call -- no GPU needed."""
import ctypes

from scamlgp_amd import _lib, ops


def _call(n=8, M=4, F=16, D=6, grad=True, acqf=1, s_all=1.0, kind=0, null_knq=False, null_cov_g=False):
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    return _lib.lib.scaml_target_fantasy_acqf_f64(
        None if null_knq else one, one, one, one, one, 0.0, s_all, 0.0, None, acqf, 0.5,
        None if null_cov_g else one, one, one, one, one, one, n, M, F, D, kind, one, one if grad else None, None)


def test_symbol_is_declared_and_bound():
    assert "scaml_target_fantasy_acqf_f64" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "scaml_target_fantasy_acqf_f64")
    assert ops.ACQF_UCB == 0 and ops.ACQF_EI == 1


def test_size_limits_answer_without_a_gpu():
    assert _call(F=65) == _lib.E_TOOLARGE                      # more fantasies than lanes
    assert _call(F=65, grad=False) == _lib.E_TOOLARGE
    assert _call(n=97) == _lib.E_TOOLARGE                      # gradient: the GRAD pass's covariance block
    assert _call(n=96, D=16) == _lib.E_TOOLARGE                # gradient: 16 columns per query point
    assert _call(n=257, grad=False) == _lib.E_TOOLARGE         # value: scaml_fit_max_n()
    assert _call(n=96, F=64, D=15, M=0) == 0                  # at the limits, no query points: a no-op
    assert _call(n=256, F=64, M=0, grad=False) == 0


def test_bad_arguments_answer_without_a_gpu():
    assert _call(null_knq=True) == _lib.E_BADARG
    assert _call(null_cov_g=True) == _lib.E_BADARG             # gradient inputs missing
    assert _call(null_cov_g=True, grad=False, M=0) == 0        # ... not needed for the value
    assert _call(acqf=2) == _lib.E_BADARG
    assert _call(s_all=0.0) == _lib.E_BADARG
    assert _call(kind=5) == _lib.E_BADARG
    assert _call(n=0) == _lib.E_BADARG
    assert _call(F=0) == _lib.E_BADARG
    assert _call(D=0) == _lib.E_BADARG
    # bad arguments answer before size limits
    assert _call(F=65, acqf=7) == _lib.E_BADARG
