"""The entry points of the batched stage 1 (include/scaml_gp.h (5f), (5f'), (7i), (7j)): exported, declared and bound with the header's
argument lists; every bad size is SCAML_E_BADARG, every limit + 1 SCAML_E_TOOLARGE, a candidate count that is no multiple of 16 is
rejected, NULL required pointers are rejected, and Mq = 0 at the limits is a no-op -- all before any HIP call (never-dereferenced
pointers, no GPU)."""
import ctypes
import re

from scamlgp_amd import _lib
from tests.test_studies_acqf_abi import ACQF_PTRS, GROUPED_PTRS, ONE, ROOT, _header_argtypes

L = _lib.lib
GROUPED, GROUPED_OWN = "scaml_posterior_linv_grouped_f64", "scaml_posterior_linv_grouped_own_f64"
SCORE, BLOCK = "scaml_target_score_batched_f64", "scaml_target_train_block_batched_f64"
NAMES = (GROUPED, GROUPED_OWN, SCORE, BLOCK)
BLOCK_PTRS = ("means_t", "covs_packed", "X", "y", "n_points", "m_all", "s_all", "w", "active", "theta")
OPTIONAL = ("y_mean", "y_std", "n_points")


def _grouped(T=3, N=32, Mq=32, G=2, Ma_max=8, D=2, kind=0, mu=ONE, var=ONE, cov=ONE, own=False, task_base=ONE, Tsrc=6, **ptrs):
    args = [ptrs.get(k, ONE) for k in GROUPED_PTRS]
    if own:
        return L.scaml_posterior_linv_grouped_own_f64(*args, T, N, Mq, G, Ma_max, D, kind, mu, var, cov, task_base, Tsrc, None)
    return L.scaml_posterior_linv_grouped_f64(*args, T, N, Mq, G, Ma_max, D, kind, mu, var, cov, None)


def _score(Mq=32, G=2, n_max=8, T=3, D=2, kind=0, acqf=0, value=ONE, mu_out=None, var_out=None, **ptrs):
    args = [ptrs.get(k, ONE) for k in ACQF_PTRS]
    return L.scaml_target_score_batched_f64(*args, Mq, G, n_max, T, D, kind, acqf, value, mu_out, var_out, None)


def _block(G=2, n_max=8, T=3, D=2, kind=0, Knn=ONE, resid=ONE, **ptrs):
    args = [ptrs.get(k, ONE) for k in BLOCK_PTRS]
    return L.scaml_target_train_block_batched_f64(*args, G, n_max, T, D, kind, Knn, resid, None)


def test_symbols_are_exported_declared_and_bound():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/scaml_gp.h").read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        restype, argtypes = _header_argtypes(name)
        assert _lib.SIGNATURES[name][0] is restype, name
        assert list(_lib.SIGNATURES[name][1]) == argtypes, name
    # the value-only passes take their GRAD counterparts' arguments
    assert _lib.SIGNATURES[GROUPED][1] == _lib.SIGNATURES["scaml_posterior_linv_grad_grouped_f64"][1]
    assert _lib.SIGNATURES[GROUPED_OWN][1] == _lib.SIGNATURES["scaml_posterior_linv_grad_grouped_own_f64"][1]
    assert len(_lib.SIGNATURES[SCORE][1]) == len(ACQF_PTRS) + 7 + 3 + 1
    assert len(_lib.SIGNATURES[BLOCK][1]) == len(BLOCK_PTRS) + 5 + 2 + 1


def test_grouped_value_pass_rejects_bad_arguments():
    for own in (False, True):
        for name in GROUPED_PTRS:
            want = 0 if name in OPTIONAL else _lib.E_BADARG      # (optional, as in (5e); Mq = 0 keeps the GPU out)
            assert _grouped(own=own, Mq=0, **{name: None}) == want, (own, name)
        for name in ("mu", "var", "cov"):
            assert _grouped(own=own, **{name: None}) == _lib.E_BADARG, (own, name)
        assert _grouped(own=own, kind=5) == _lib.E_BADARG
        for bad in (dict(T=-1), dict(Mq=-16), dict(G=-1), dict(N=0), dict(Ma_max=0), dict(D=0)):
            assert _grouped(own=own, **bad) == _lib.E_BADARG, (own, bad)
        for Mq in (1, 15, 17, 40):                               # whole strips of 16 only
            assert _grouped(own=own, Mq=Mq) == _lib.E_BADARG, (own, Mq)
    assert _grouped(own=True, task_base=None) == _lib.E_BADARG and _grouped(own=True, Tsrc=0) == _lib.E_BADARG


def test_grouped_value_pass_limits_and_no_ops():
    for own in (False, True):
        assert _grouped(own=own, D=16) == _lib.E_TOOLARGE and _grouped(own=own, Ma_max=97, N=128) == _lib.E_TOOLARGE
        assert _grouped(own=own, Ma_max=33, N=32) == _lib.E_TOOLARGE
        assert _grouped(own=own, N=L.scaml_posterior_max_n() + 1) == _lib.E_TOOLARGE
        # bad arguments answer before the size limits
        assert _grouped(own=own, D=16, kind=5) == _lib.E_BADARG and _grouped(own=own, D=16, Mq=17) == _lib.E_BADARG
        assert _grouped(own=own, Ma_max=97, N=128, group=None) == _lib.E_BADARG
        # at the limits, nothing to do
        assert _grouped(own=own, D=15, Ma_max=96, N=96, Mq=0) == 0
        assert _grouped(own=own, Mq=0) == 0 and _grouped(own=own, G=0) == 0 and _grouped(own=own, T=0) == 0


def test_strip_scoring_rejects_bad_arguments():
    for name in ACQF_PTRS:
        assert _score(**{name: None}) == _lib.E_BADARG, name
    assert _score(value=None) == _lib.E_BADARG
    assert _score(kind=5) == _lib.E_BADARG and _score(acqf=2) == _lib.E_BADARG and _score(acqf=-1) == _lib.E_BADARG
    for bad in (dict(Mq=-16), dict(G=-1), dict(n_max=0), dict(T=0), dict(D=0)):
        assert _score(**bad) == _lib.E_BADARG, bad
    for Mq in (1, 15, 17, 40):
        assert _score(Mq=Mq) == _lib.E_BADARG, Mq


def test_strip_scoring_limits_and_no_ops():
    assert _score(n_max=97) == _lib.E_TOOLARGE and _score(D=16) == _lib.E_TOOLARGE
    assert _score(n_max=97, kind=5) == _lib.E_BADARG and _score(D=16, Mq=17) == _lib.E_BADARG and _score(n_max=1000, mu=None) == _lib.E_BADARG
    assert _score(n_max=96, D=15, Mq=0) == 0                     # at the limits, nothing to do
    assert _score(Mq=0) == 0 and _score(G=0) == 0
    assert _score(Mq=0, mu_out=ONE, var_out=ONE) == 0            # the posterior outputs are optional


def test_train_block_checks():
    for name in BLOCK_PTRS:
        assert _block(**{name: None}) == _lib.E_BADARG, name
    assert _block(Knn=None) == _lib.E_BADARG and _block(resid=None) == _lib.E_BADARG
    assert _block(kind=5) == _lib.E_BADARG
    for bad in (dict(G=-1), dict(n_max=0), dict(T=0), dict(D=0)):
        assert _block(**bad) == _lib.E_BADARG, bad
    assert _block(n_max=L.scaml_fit_max_n() + 1) == _lib.E_TOOLARGE
    assert _block(n_max=L.scaml_fit_max_n() + 1, kind=5) == _lib.E_BADARG
    assert _block(n_max=L.scaml_fit_max_n(), G=0) == 0
