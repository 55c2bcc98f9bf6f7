"""The batched target-fit entry points (include/scaml_gp.h (8b)): exported, declared and bound with the header's argument lists;
scaml_target_fit_batched_workspace_doubles grows with S and B; the argument checks and size limits answer before any HIP call
(never-dereferenced pointers, no GPU)."""
import ctypes
import os
import re

from scamlgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first
SPEC = (ctypes.c_double * 19)(1e-4, 1e2, 1e-4, 1e2, 1e-8, 1e-2, 2, 0.5, 1.5, 2, -2.0, 3.0, 2, -8.0, 2.0, 1, 1.0, 1.0, 1e-10)
NAMES = ("scaml_target_fit_batched_workspace_doubles", "scaml_target_mll_batched_f64", "scaml_target_fit_batched_f64")
BIG = 1 << 40


def _mll(means=ONE, covs=ONE, X=ONE, y=ONE, n_points=ONE, m_all=ONE, s_all=ONE, spec=SPEC, z=ONE, S=3, B=2, n_max=8, T=3, D=2, kind=0,
         value=ONE, grad=ONE, info=ONE):
    return L.scaml_target_mll_batched_f64(means, covs, X, y, n_points, m_all, s_all, spec, z, S, B, n_max, T, D, kind, value, grad, info,
                                          None, None)


def _fit(means=ONE, covs=ONE, X=ONE, y=ONE, n_points=ONE, m_all=ONE, s_all=ONE, spec=SPEC, z=ONE, S=3, B=2, n_max=8, T=3, D=2, kind=0,
         max_iter=50, history=10, value=ONE, info=ONE, ws=ONE, ws_doubles=BIG):
    return L.scaml_target_fit_batched_f64(means, covs, X, y, n_points, m_all, s_all, spec, z, S, B, n_max, T, D, kind, max_iter, history,
                                          1e-5, 2.2e-9, value, info, None, None, ws, ws_doubles, None)


def test_symbols_are_exported_declared_and_bound():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "scaml_gp.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name


def _header_argtypes(name):
    """The declaration in include/scaml_gp.h as ctypes classes: pointers (one host pointer: spec_host), int, long long, double."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    ret, args = re.search(r"(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    out = []
    for a in (x.strip() for x in args.split(",")):
        if a == "void":
            continue
        if "*" in a:
            pname = a.split("*")[-1].strip()
            out.append(_lib._host_spec if pname == "spec_host" else ctypes.c_void_p)
        elif a.startswith("long long"):
            out.append(ctypes.c_longlong)
        elif a.startswith("double"):
            out.append(ctypes.c_double)
        elif a.startswith("unsigned"):
            out.append(ctypes.c_uint)
        else:
            assert a.startswith("int "), a
            out.append(ctypes.c_int)
    return (ctypes.c_longlong if ret == "long long" else ctypes.c_int), out


def test_ctypes_table_matches_the_header():
    for name in NAMES + ("scaml_target_mll_f64", "scaml_target_fit_f64"):   # (the single-problem pair: the parser reads a known row right)
        restype, argtypes = _header_argtypes(name)
        assert _lib.SIGNATURES[name][0] is restype, name
        assert list(_lib.SIGNATURES[name][1]) == argtypes, name
    # the problem block of (8b) is that of (8) with the counts added and the standardisers by pointer
    single, batched = _lib.SIGNATURES["scaml_target_fit_f64"][1], _lib.SIGNATURES["scaml_target_fit_batched_f64"][1]
    assert len(batched) == len(single) + 2   # + n_points, + S
    assert single[4:6] == [ctypes.c_double] * 2 and batched[4:7] == [ctypes.c_void_p] * 3


def test_workspace_doubles_is_monotone_in_S_and_B():
    f = L.scaml_target_fit_batched_workspace_doubles
    assert f(3, 2, 32, 6, 10) == 3 * 2 * 26 * 40
    # one study is the single-problem workspace
    assert f(1, 5, 32, 6, 10) == L.scaml_target_fit_workspace_doubles(5, 32, 6, 10)
    for name, at in (("S", lambda v: f(v, 3, 32, 6, 10)), ("B", lambda v: f(7, v, 32, 6, 10))):
        sizes = [at(v) for v in range(0, 70)]
        assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:])), name
    assert f(-1, 3, 32, 6, 10) == 0 and f(3, -1, 32, 6, 10) == 0 and f(3, 3, 0, 6, 10) == 0 and f(3, 3, 32, 0, 10) == 0 and f(3, 3, 32, 6, 0) == 0


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    for call in (_mll, _fit):
        for name in ("means", "covs", "X", "y", "n_points", "m_all", "s_all", "spec", "z", "value", "info"):
            assert call(**{name: None}) == _lib.E_BADARG, (call.__name__, name)
        assert call(kind=5) == _lib.E_BADARG
        assert call(S=-1) == _lib.E_BADARG and call(B=-1) == _lib.E_BADARG
        assert call(n_max=0) == _lib.E_BADARG and call(T=0) == _lib.E_BADARG and call(D=0) == _lib.E_BADARG
        bad = (ctypes.c_double * 19)(*SPEC)
        bad[0], bad[1] = 1.0, 0.5                                # inverted lengthscale interval
        assert call(spec=bad) == _lib.E_BADARG
        bad = (ctypes.c_double * 19)(*SPEC)
        bad[6] = 7                                               # unknown prior kind
        assert call(spec=bad) == _lib.E_BADARG
    assert _mll(grad=None) == _lib.E_BADARG
    assert _fit(ws=None) == _lib.E_BADARG
    assert _fit(history=0) == _lib.E_BADARG and _fit(history=17) == _lib.E_BADARG and _fit(max_iter=-1) == _lib.E_BADARG
    need = L.scaml_target_fit_batched_workspace_doubles(3, 2, 3, 2, 10)
    assert _fit(ws_doubles=need - 1) == _lib.E_BADARG            # workspace too small
    assert _fit(ws_doubles=need, S=0) == 0


def test_sizes_beyond_the_kernel_are_too_large():
    n_lim = L.scaml_target_fit_max_n(3, 2)
    for call in (_mll, _fit):
        assert call(D=L.scaml_target_fit_max_d() + 1) == _lib.E_TOOLARGE
        assert call(n_max=n_lim + 1) == _lib.E_TOOLARGE
        assert call(n_max=100000) == _lib.E_TOOLARGE
        assert call(n_max=n_lim, S=0) == 0                       # at the limit, no problems: a no-op
        assert call(S=0) == 0 and call(B=0) == 0
        # bad arguments answer before size limits
        assert call(n_max=100000, kind=5) == _lib.E_BADARG
