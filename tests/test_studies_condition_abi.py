"""The entry points of the studies' batched fantasy set-up (include/scaml_gp.h (7m), (7n)): exported, declared and bound with the
header's argument lists; the argument checks and size limits answer before any HIP call (never-dereferenced pointers, no GPU).  A shape
at all limits at once is taken through every check with nothing to enqueue (G = 0)."""
import ctypes
import os
import re

from scamlgp_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first
BLOCK, FANT = "scaml_studies_condition_block_f64", "scaml_studies_fantasy_condition_f64"
BLOCK_PTRS = ("mu", "cov", "strip_base", "w", "active", "Xt", "theta", "y", "n_points", "n_obs", "m_all", "s_all")
BLOCK_OUT = ("Knn", "resid", "mean_p")
FANT_PTRS = ("L", "resid", "mean_p", "n_points", "n_obs", "info", "eps", "n_fant", "m_all", "s_all")
FANT_OUT = ("alpha_f", "y_fant", "mu_p")


def _block(Mq=32, G=2, n_max=8, T=3, D=2, kind=0, **ptrs):
    args = [ptrs.get(k, ONE) for k in BLOCK_PTRS]
    return L.scaml_studies_condition_block_f64(*args, Mq, G, n_max, T, D, kind, *[ptrs.get(k, ONE) for k in BLOCK_OUT], None)


def _fant(G=2, n_max=8, p_max=2, F_max=4, **ptrs):
    args = [ptrs.get(k, ONE) for k in FANT_PTRS]
    return L.scaml_studies_fantasy_condition_f64(*args, G, n_max, p_max, F_max, *[ptrs.get(k, ONE) for k in FANT_OUT], None)


def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    ret, args = re.search(r"(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    return ret, [x.strip() for x in args.split(",")]


def _argtypes(args):
    out = []
    for a in args:
        if "*" in a:
            out.append(ctypes.c_void_p)
        else:
            assert a.startswith("int "), a
            out.append(ctypes.c_int)
    return out


def test_symbols_are_exported_declared_and_bound():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    for name in (BLOCK, FANT):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert callable(ops.studies_condition_block) and callable(ops.studies_fantasy_condition)


def test_ctypes_table_matches_the_header():
    last = lambda args: [a.split()[-1].lstrip("*") for a in args]   # noqa: E731
    for name, ptrs, dims, outs in ((BLOCK, BLOCK_PTRS, ("Mq", "G", "n_max", "T", "D", "kind"), BLOCK_OUT),
                                   (FANT, FANT_PTRS, ("G", "n_max", "p_max", "F_max"), FANT_OUT)):
        ret, args = _header_args(name)
        assert ret == "int" and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        assert list(_lib.SIGNATURES[name][1]) == _argtypes(args), name
        assert last(args) == list(ptrs) + list(dims) + list(outs) + ["stream"], name


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    for name in BLOCK_PTRS + BLOCK_OUT:
        assert _block(**{name: None}) == _lib.E_BADARG, name
    assert _block(kind=5) == _lib.E_BADARG and _block(kind=-1) == _lib.E_BADARG
    assert _block(Mq=-16) == _lib.E_BADARG and _block(Mq=24) == _lib.E_BADARG and _block(G=-1) == _lib.E_BADARG   # whole strips of 16
    assert _block(n_max=0) == _lib.E_BADARG and _block(T=0) == _lib.E_BADARG and _block(D=0) == _lib.E_BADARG
    for name in FANT_PTRS + FANT_OUT:
        assert _fant(**{name: None}) == _lib.E_BADARG, name
    assert _fant(G=-1) == _lib.E_BADARG and _fant(n_max=0) == _lib.E_BADARG and _fant(p_max=0) == _lib.E_BADARG
    assert _fant(F_max=0) == _lib.E_BADARG and _fant(F_max=-3) == _lib.E_BADARG


def test_sizes_beyond_the_kernels_are_too_large():
    assert _block(n_max=97) == _lib.E_TOOLARGE and _block(D=16) == _lib.E_TOOLARGE
    assert _fant(n_max=97) == _lib.E_TOOLARGE and _fant(F_max=65) == _lib.E_TOOLARGE and _fant(p_max=97) == _lib.E_TOOLARGE
    # all limits at once pass every check, the LDS footprint included (nothing to enqueue)
    assert _block(n_max=96, D=15, G=0) == 0 and _fant(n_max=96, p_max=95, F_max=64, G=0) == 0
    # bad arguments answer before the size limits
    assert _block(n_max=97, kind=5) == _lib.E_BADARG and _block(D=16, mu=None) == _lib.E_BADARG and _block(n_max=97, Mq=8) == _lib.E_BADARG
    assert _fant(n_max=97, eps=None) == _lib.E_BADARG and _fant(F_max=65, p_max=0) == _lib.E_BADARG and _fant(F_max=65, mu_p=None) == _lib.E_BADARG


def test_nothing_to_do_is_a_no_op():
    assert _block(G=0) == 0 and _block(G=0, Mq=0) == 0 and _fant(G=0) == 0
