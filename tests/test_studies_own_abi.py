"""The entry points for studies that own their source tasks (include/scaml_gp.h (5e'), (7h')): exported, declared and bound with the
header's argument lists -- (5e)'s / (7h)'s plus ``task_base`` and ``Tsrc`` --; their own two checks and every bad-argument and
too-large case of (5e) / (7h) answer before any HIP call (never-dereferenced pointers, no GPU); empty shapes are no-ops."""
import ctypes
import os
import re

from scamlgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first (and 16-byte aligned, as the workspace has to be)
GROUPED, OPT = "scaml_posterior_linv_grad_grouped_own_f64", "scaml_studies_acqf_opt_own_f64"
GROUPED_PTRS = ("Xq", "group", "Xa", "n_points_a", "VA_tab", "X", "theta", "Linv", "alpha", "y_mean", "y_std", "n_points")
ARRAYS = ("x0", "group", "VA_tab", "X", "theta_s", "Linv", "alpha_s", "y_mean", "y_std", "n_points_s", "w", "active", "Xt", "theta_t", "L",
          "Linv_diag", "alpha_t", "n_points_t", "m_all", "s_all", "info", "acqf_param")
OPTIONAL = ("y_mean", "y_std", "n_points_s", "n_points")
OUTPUTS = ("lo", "hi", "workspace", "x", "f", "stats")


def _grouped(T=3, N=32, Mq=5, G=2, Ma_max=8, D=2, kind=0, mu=ONE, var=ONE, cov=ONE, task_base=ONE, Tsrc=6, **ptrs):
    args = [ptrs.get(k, ONE) for k in GROUPED_PTRS]
    return getattr(L, GROUPED)(*args, T, N, Mq, G, Ma_max, D, kind, mu, var, cov, task_base, Tsrc, None)


def _opt(B=5, G=2, n_max=8, T=3, N=32, D=2, kind_s=0, kind_t=0, acqf=0, max_iter=10, history=10, max_ls=20, gtol=1e-5, ftol=2.2e-9, c1=1e-4, n_evals=1,
         flags=0, task_base=ONE, Tsrc=6, **ptrs):
    a = [ptrs.get(k, ONE) for k in ARRAYS]
    o = {k: ptrs.get(k, ONE) for k in OUTPUTS}
    return getattr(L, OPT)(*a, B, G, n_max, T, N, D, kind_s, kind_t, acqf, o["lo"], o["hi"], max_iter, history, max_ls, gtol, ftol, c1,
                           n_evals, flags, o["workspace"], o["x"], o["f"], o["stats"], task_base, Tsrc, None)


def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    ret, args = re.search(r"(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    return ret, [re.sub(r"\s+", " ", a.strip()) for a in args.split(",")]


def _argtypes(args):
    out = []
    for a in args:
        if "*" in a:
            out.append(ctypes.c_void_p)
        elif a.startswith("double"):
            out.append(ctypes.c_double)
        elif a.startswith("unsigned"):
            out.append(ctypes.c_uint)
        else:
            assert a.startswith("int "), a
            out.append(ctypes.c_int)
    return out


def test_symbols_are_exported_declared_and_bound():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    for name in (GROUPED, OPT):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name


def test_ctypes_table_matches_the_header():
    for name in (GROUPED, OPT):
        ret, args = _header_args(name)
        assert ret == "int" and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        assert list(_lib.SIGNATURES[name][1]) == _argtypes(args), name


def test_argument_lists_are_those_of_5e_and_7h_plus_the_table():
    """The header's lists: the old entry point's arguments up to the stream, then ``task_base`` and ``Tsrc``, then the stream."""
    for own, old in ((GROUPED, "scaml_posterior_linv_grad_grouped_f64"), (OPT, "scaml_studies_acqf_opt_f64")):
        a_own, a_old = _header_args(own)[1], _header_args(old)[1]
        assert a_own == a_old[:-1] + ["const int32_t* task_base", "int Tsrc", "void* stream"], own
    assert len(_lib.SIGNATURES[GROUPED][1]) == len(GROUPED_PTRS) + 7 + 3 + 2 + 1
    assert len(_lib.SIGNATURES[OPT][1]) == len(ARRAYS) + 9 + 2 + 3 + 3 + 2 + 4 + 2 + 1


def test_the_table_is_required():
    assert _grouped(task_base=None) == _lib.E_BADARG and _opt(task_base=None) == _lib.E_BADARG
    for bad in (0, -1):
        assert _grouped(Tsrc=bad) == _lib.E_BADARG and _opt(Tsrc=bad) == _lib.E_BADARG
    # also where there is nothing to do, and before the size limits
    assert _grouped(Mq=0, task_base=None) == _lib.E_BADARG and _grouped(T=0, Tsrc=0) == _lib.E_BADARG
    assert _opt(B=0, task_base=None) == _lib.E_BADARG and _opt(G=0, Tsrc=0) == _lib.E_BADARG
    assert _grouped(D=16, task_base=None) == _lib.E_BADARG and _opt(D=16, Tsrc=0) == _lib.E_BADARG
    # Tsrc need not be a multiple of T, nor at least T: a slot past the arrays is a padding row
    assert _grouped(Mq=0, Tsrc=1) == 0 and _opt(B=0, Tsrc=1) == 0


def test_grouped_bad_arguments_are_rejected_without_touching_the_gpu():
    for name in GROUPED_PTRS:
        want = 0 if name in OPTIONAL else _lib.E_BADARG   # (optional, as in (5e); Mq = 0 keeps the GPU out)
        assert _grouped(Mq=0, **{name: None}) == want, name
    for name in ("mu", "var", "cov"):
        assert _grouped(**{name: None}) == _lib.E_BADARG, name
    assert _grouped(kind=5) == _lib.E_BADARG
    assert _grouped(T=-1) == _lib.E_BADARG and _grouped(Mq=-1) == _lib.E_BADARG and _grouped(G=-1) == _lib.E_BADARG
    assert _grouped(N=0) == _lib.E_BADARG and _grouped(Ma_max=0) == _lib.E_BADARG and _grouped(D=0) == _lib.E_BADARG


def test_grouped_sizes_beyond_the_kernel_are_too_large():
    assert _grouped(Ma_max=97, N=128) == _lib.E_TOOLARGE and _grouped(D=16) == _lib.E_TOOLARGE
    assert _grouped(Ma_max=33, N=32) == _lib.E_TOOLARGE        # more leading points than the LDS strip of the pass holds
    assert _grouped(N=L.scaml_posterior_max_n() + 1) == _lib.E_TOOLARGE
    assert _grouped(Mq=(1 << 26) + 1) == _lib.E_TOOLARGE
    assert _grouped(Ma_max=96, N=128, D=15, Mq=0) == 0         # at the limits, nothing to do
    # bad arguments answer before the size limits
    assert _grouped(D=16, kind=5) == _lib.E_BADARG and _grouped(Ma_max=97, N=128, group=None) == _lib.E_BADARG


def test_optimiser_bad_arguments_are_rejected_without_touching_the_gpu():
    for name in ARRAYS:
        want = 0 if name in OPTIONAL else _lib.E_BADARG   # (optional, as in (7h); B = 0 keeps the GPU out)
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


def test_optimiser_sizes_beyond_the_kernels_are_too_large():
    assert _opt(n_max=97, N=128) == _lib.E_TOOLARGE and _opt(D=16) == _lib.E_TOOLARGE
    assert _opt(n_max=33, N=32) == _lib.E_TOOLARGE                    # more training points than the source pass's LDS strip holds
    assert _opt(N=L.scaml_posterior_max_n() + 1) == _lib.E_TOOLARGE
    assert _opt(B=(1 << 26) + 1) == _lib.E_TOOLARGE
    assert _opt(n_max=96, N=128, D=15, B=0) == 0                      # at the limits, nothing to do
    # bad arguments answer before the size limits
    assert _opt(n_max=97, N=128, kind_t=5) == _lib.E_BADARG and _opt(D=16, acqf=3) == _lib.E_BADARG
    assert _opt(n_max=1000, x0=None) == _lib.E_BADARG and _opt(D=16, history=0) == _lib.E_BADARG and _opt(D=16, flags=4) == _lib.E_BADARG


def test_nothing_to_do_is_a_no_op():
    assert _grouped(Mq=0) == 0 and _grouped(G=0) == 0 and _grouped(T=0) == 0
    assert _opt(B=0) == 0 and _opt(G=0) == 0
    assert _opt(B=0, n_evals=0) == 0 and _opt(B=0, flags=1) == 0
