"""The device-side acquisition optimiser's entry points (include/scaml_gp.h (7h)): exported, declared and bound with the header's
argument lists; the argument checks and size limits answer before any HIP call (never-dereferenced pointers, no GPU)."""
import ctypes
import os
import re

from scamlgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first (and 16-byte aligned, as the workspace has to be)
NAMES = ("scaml_studies_acqf_opt_max_d", "scaml_studies_acqf_opt_workspace_bytes", "scaml_studies_acqf_opt_f64")
ARRAYS = ("x0", "group", "VA_tab", "X", "theta_s", "Linv", "alpha_s", "y_mean", "y_std", "n_points_s", "w", "active", "Xt", "theta_t", "L",
          "Linv_diag", "alpha_t", "n_points_t", "m_all", "s_all", "info", "acqf_param")
OPTIONAL = ("y_mean", "y_std", "n_points_s")
OUTPUTS = ("lo", "hi", "workspace", "x", "f", "stats")


def _opt(B=5, G=2, n_max=8, T=3, N=32, D=2, kind_s=0, kind_t=0, acqf=0, max_iter=10, history=10, max_ls=20, gtol=1e-5, ftol=2.2e-9, c1=1e-4, n_evals=1,
         flags=0, **ptrs):
    a = [ptrs.get(k, ONE) for k in ARRAYS]
    o = {k: ptrs.get(k, ONE) for k in OUTPUTS}
    return L.scaml_studies_acqf_opt_f64(*a, B, G, n_max, T, N, D, kind_s, kind_t, acqf, o["lo"], o["hi"], max_iter, history, max_ls, gtol, ftol, c1,
                                        n_evals, flags, o["workspace"], o["x"], o["f"], o["stats"], None)


def _header_argtypes(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    ret, args = re.search(r"(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    out = []
    for a in (x.strip() for x in args.split(",")):
        if a == "void":
            continue
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
    assert re.search(r"#define\s+SCAML_ACQF_OPT_CONTINUE\s+1u", header) and _lib.ACQF_OPT_CONTINUE == 1


def test_ctypes_table_matches_the_header():
    for name in NAMES + ("scaml_stack_fit_workspace_bytes",):   # (a known row: the parser reads it right)
        restype, argtypes = _header_argtypes(name)
        assert _lib.SIGNATURES[name][0] is restype, name
        assert list(_lib.SIGNATURES[name][1]) == argtypes, name
    assert len(_lib.SIGNATURES[NAMES[2]][1]) == len(ARRAYS) + 9 + 2 + 3 + 3 + 2 + 4 + 1


def test_limits_and_the_python_mirror():
    from scamlgp_amd import ops

    assert L.scaml_studies_acqf_opt_max_d() == 15
    assert ops.ACQF_OPT_EVALS_PER_CALL >= 1
    # the state opens the workspace: B = 1 start and nothing else to hold gives the stride, rounded up to the 256-byte sections
    for D, history in ((1, 1), (2, 10), (15, 16)):
        stride = ops.studies_acqf_opt_state_doubles(D, history)
        assert stride == (4 + 2 * history) * D + history + 16
        assert L.scaml_studies_acqf_opt_workspace_bytes(1, 1, 1, 1, D, history) >= 8 * stride


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    for name in ARRAYS:
        want = 0 if name in OPTIONAL else _lib.E_BADARG   # (optional, as in (5e); B = 0 below keeps the GPU out)
        assert _opt(B=0, **{name: None}) == want, name
    for name in OUTPUTS:
        assert _opt(**{name: None}) == _lib.E_BADARG, name
    assert _opt(workspace=ctypes.c_void_p(24)) == _lib.E_BADARG   # not 16-byte aligned
    assert _opt(kind_s=5) == _lib.E_BADARG and _opt(kind_t=-1) == _lib.E_BADARG and _opt(acqf=2) == _lib.E_BADARG and _opt(acqf=-1) == _lib.E_BADARG
    assert _opt(flags=2) == _lib.E_BADARG and _opt(flags=3) == _lib.E_BADARG
    for k in ("B", "G", "n_evals", "max_iter"):
        assert _opt(**{k: -1}) == _lib.E_BADARG, k
    for k in ("n_max", "T", "N", "D", "max_ls", "history"):
        assert _opt(**{k: 0}) == _lib.E_BADARG, k
    assert _opt(history=17) == _lib.E_BADARG
    assert _opt(gtol=-1.0) == _lib.E_BADARG and _opt(gtol=float("nan")) == _lib.E_BADARG
    assert _opt(c1=0.0) == _lib.E_BADARG and _opt(ftol=float("nan")) == _lib.E_BADARG


def test_sizes_beyond_the_kernels_are_too_large():
    assert _opt(n_max=97, N=128) == _lib.E_TOOLARGE and _opt(D=16) == _lib.E_TOOLARGE
    assert _opt(n_max=33, N=32) == _lib.E_TOOLARGE                    # more training points than the source pass's LDS strip holds
    assert _opt(N=L.scaml_posterior_max_n() + 1) == _lib.E_TOOLARGE
    assert _opt(n_max=96, N=128, D=15, B=0) == 0                      # at the limits, nothing to do
    # bad arguments answer before the size limits
    assert _opt(n_max=97, N=128, kind_t=5) == _lib.E_BADARG and _opt(D=16, acqf=3) == _lib.E_BADARG
    assert _opt(n_max=1000, x0=None) == _lib.E_BADARG and _opt(D=16, history=0) == _lib.E_BADARG and _opt(D=16, flags=4) == _lib.E_BADARG


def test_nothing_to_do_is_a_no_op():
    assert _opt(B=0) == 0 and _opt(G=0) == 0
    assert _opt(B=0, n_evals=0) == 0 and _opt(B=0, flags=1) == 0


def test_workspace_bytes_is_monotone_and_zero_outside_the_limits():
    wb = L.scaml_studies_acqf_opt_workspace_bytes
    base = dict(B=10, G=3, n_max=16, T=4, D=3, history=5)
    order = ("B", "G", "n_max", "T", "D", "history")
    at = lambda **kw: wb(*[{**base, **kw}[k] for k in order])   # noqa: E731
    assert at() > 0 and at() % 256 == 0
    for k in ("B", "n_max", "T", "D", "history"):
        vals = [at(**{k: v}) for v in range(base[k], base[k] + 4)]
        assert all(b >= a for a, b in zip(vals, vals[1:])) and vals[-1] > vals[0], (k, vals)
    assert at(G=30) == at()                                          # nothing in the workspace is per study
    assert at(B=0) == 0 or at(B=0) < at(B=1)
    # the sections the header names: state, Xq, live groups, mu / var / cov, value / grad
    B, n_max, T, D, history = (base[k] for k in ("B", "n_max", "T", "D", "history"))
    need = 8 * (B * ((4 + 2 * history) * D + history + 16) + B * D + 2 * T * B * 16 + T * n_max * B * 16 + B + B * D) + 4 * B
    assert need <= at() <= need + 8 * 256
    for bad in (dict(B=-1), dict(G=-1), dict(n_max=0), dict(n_max=97), dict(T=0), dict(D=0), dict(D=16), dict(history=0), dict(history=17)):
        assert at(**bad) == 0, bad
