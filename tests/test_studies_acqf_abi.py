"""The lock-step acquisition entry points (include/scaml_gp.h (5e), (7g)): exported, declared and bound with the header's argument
lists; the argument checks and size limits answer before any HIP call (never-dereferenced pointers, no GPU)."""
import ctypes
import os
import re

from scamlgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first
NAMES = ("scaml_posterior_linv_grad_grouped_f64", "scaml_target_acqf_batched_f64")
GROUPED_PTRS = ("Xq", "group", "Xa", "n_points_a", "VA_tab", "X", "theta", "Linv", "alpha", "y_mean", "y_std", "n_points")
ACQF_PTRS = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha", "n_points", "m_all", "s_all", "info",
             "acqf_param")


def _grouped(T=3, N=32, Mq=5, G=2, Ma_max=8, D=2, kind=0, mu=ONE, var=ONE, cov=ONE, **ptrs):
    args = [ptrs.get(k, ONE) for k in GROUPED_PTRS]
    return L.scaml_posterior_linv_grad_grouped_f64(*args, T, N, Mq, G, Ma_max, D, kind, mu, var, cov, None)


def _acqf(Mq=5, G=2, n_max=8, T=3, D=2, kind=0, acqf=0, value=ONE, grad=ONE, mu_out=None, var_out=None, **ptrs):
    args = [ptrs.get(k, ONE) for k in ACQF_PTRS]
    return L.scaml_target_acqf_batched_f64(*args, Mq, G, n_max, T, D, kind, acqf, value, grad, mu_out, var_out, None)


def _header_argtypes(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    ret, args = re.search(r"(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    out = []
    for a in (x.strip() for x in args.split(",")):
        if "*" in a:
            out.append(ctypes.c_void_p)
        elif a.startswith("double"):
            out.append(ctypes.c_double)
        elif a.startswith("unsigned"):
            out.append(ctypes.c_uint)
        else:
            assert a.startswith("int "), a
            out.append(ctypes.c_int)
    return (ctypes.c_longlong if ret == "long long" else ctypes.c_int), out


def test_symbols_are_exported_declared_and_bound():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name


def test_ctypes_table_matches_the_header():
    for name in NAMES + ("scaml_posterior_linv_grad_f64",):   # (the ungrouped pass: the parser reads a known row right)
        restype, argtypes = _header_argtypes(name)
        assert _lib.SIGNATURES[name][0] is restype, name
        assert list(_lib.SIGNATURES[name][1]) == argtypes, name
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == len(GROUPED_PTRS) + 7 + 4
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == len(ACQF_PTRS) + 7 + 5


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    for name in GROUPED_PTRS:
        want = 0 if name in ("y_mean", "y_std", "n_points") else _lib.E_BADARG   # (optional, as in (5d); Mq = 0 below keeps the GPU out)
        assert _grouped(Mq=0, **{name: None}) == want, name
    for name in ("mu", "var", "cov"):
        assert _grouped(**{name: None}) == _lib.E_BADARG, name
    assert _grouped(kind=5) == _lib.E_BADARG
    assert _grouped(T=-1) == _lib.E_BADARG and _grouped(Mq=-1) == _lib.E_BADARG and _grouped(G=-1) == _lib.E_BADARG
    assert _grouped(N=0) == _lib.E_BADARG and _grouped(Ma_max=0) == _lib.E_BADARG and _grouped(D=0) == _lib.E_BADARG
    for name in ACQF_PTRS:
        assert _acqf(**{name: None}) == _lib.E_BADARG, name
    assert _acqf(value=None) == _lib.E_BADARG
    assert _acqf(kind=5) == _lib.E_BADARG and _acqf(acqf=2) == _lib.E_BADARG and _acqf(acqf=-1) == _lib.E_BADARG
    assert _acqf(Mq=-1) == _lib.E_BADARG and _acqf(G=-1) == _lib.E_BADARG
    assert _acqf(n_max=0) == _lib.E_BADARG and _acqf(T=0) == _lib.E_BADARG and _acqf(D=0) == _lib.E_BADARG


def test_sizes_beyond_the_kernels_are_too_large():
    assert _acqf(n_max=97) == _lib.E_TOOLARGE and _acqf(D=16) == _lib.E_TOOLARGE
    assert _acqf(n_max=96, D=15, Mq=0) == 0                    # at the limits, nothing to do
    assert _grouped(Ma_max=97, N=128) == _lib.E_TOOLARGE and _grouped(D=16) == _lib.E_TOOLARGE
    assert _grouped(Ma_max=33, N=32) == _lib.E_TOOLARGE        # more leading points than the LDS strip of the pass holds
    assert _grouped(N=L.scaml_posterior_max_n() + 1) == _lib.E_TOOLARGE
    # bad arguments answer before the size limits
    assert _acqf(n_max=97, kind=5) == _lib.E_BADARG and _acqf(D=16, acqf=3) == _lib.E_BADARG and _acqf(n_max=1000, mu=None) == _lib.E_BADARG
    assert _grouped(D=16, kind=5) == _lib.E_BADARG and _grouped(Ma_max=97, N=128, group=None) == _lib.E_BADARG


def test_nothing_to_do_is_a_no_op():
    assert _acqf(Mq=0) == 0 and _acqf(G=0) == 0
    assert _acqf(Mq=0, grad=None) == 0                         # the gradient and the posterior outputs are optional
    assert _grouped(Mq=0) == 0 and _grouped(G=0) == 0 and _grouped(T=0) == 0
