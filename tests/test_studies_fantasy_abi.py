"""The entry points for studies with pending evaluations (include/scaml_gp.h (7k), (7l)): exported, declared and bound with the
header's argument lists; the argument checks and size limits answer before any HIP call (never-dereferenced pointers, no GPU).  A shape
at all three limits at once is taken through every check in both layouts (with nothing to enqueue: Mq = 0 / B = 0)."""
import ctypes
import os
import re

from scamlgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first (and 16-byte aligned, as the workspace has to be)
ACQF, SCORE, OPT = "scaml_target_fantasy_acqf_batched_f64", "scaml_target_fantasy_score_batched_f64", "scaml_studies_fantasy_acqf_opt_f64"
ACQF_PTRS = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha_f", "n_fant", "n_points", "m_all", "s_all",
             "info", "acqf_param")
OPT_ARRAYS = ("x0", "group", "VA_tab", "X", "theta_s", "Linv", "alpha_s", "y_mean", "y_std", "n_points_s", "w", "active", "Xt", "theta_t", "L",
              "Linv_diag", "alpha_f", "n_fant", "n_points_t", "m_all", "s_all", "info", "acqf_param")
OPTIONAL = ("y_mean", "y_std", "n_points_s")
OUTPUTS = ("lo", "hi", "workspace", "x", "f", "stats")


def _acqf(Mq=5, G=2, n_max=8, F_max=4, T=3, D=2, kind=0, acqf=0, value=ONE, grad=ONE, **ptrs):
    args = [ptrs.get(k, ONE) for k in ACQF_PTRS]
    return L.scaml_target_fantasy_acqf_batched_f64(*args, Mq, G, n_max, F_max, T, D, kind, acqf, value, grad, None)


def _score(Mq=32, G=2, n_max=8, F_max=4, T=3, D=2, kind=0, acqf=0, value=ONE, **ptrs):
    args = [ptrs.get(k, ONE) for k in ACQF_PTRS]
    return L.scaml_target_fantasy_score_batched_f64(*args, Mq, G, n_max, F_max, T, D, kind, acqf, value, None)


def _opt(B=5, G=2, n_max=8, F_max=4, T=3, N=32, D=2, kind_s=0, kind_t=0, acqf=0, max_iter=10, history=10, max_ls=20, gtol=1e-5, ftol=2.2e-9, c1=1e-4,
         n_evals=1, flags=0, task_base=None, Tsrc=0, **ptrs):
    a = [ptrs.get(k, ONE) for k in OPT_ARRAYS]
    o = {k: ptrs.get(k, ONE) for k in OUTPUTS}
    return L.scaml_studies_fantasy_acqf_opt_f64(*a, B, G, n_max, F_max, T, N, D, kind_s, kind_t, acqf, o["lo"], o["hi"], max_iter, history, max_ls, gtol,
                                                ftol, c1, n_evals, flags, o["workspace"], o["x"], o["f"], o["stats"], task_base, Tsrc, None)


def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    ret, args = re.search(r"(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    return ret, [x.strip() for x in args.split(",")]


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
    for name in (ACQF, SCORE, OPT):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name


def test_ctypes_table_matches_the_header():
    for name in (ACQF, SCORE, OPT, "scaml_target_acqf_batched_f64"):   # (the last: a known row, the parser reads it right)
        ret, args = _header_args(name)
        assert ret == "int" and _lib.SIGNATURES[name][0] is ctypes.c_int, name
        assert list(_lib.SIGNATURES[name][1]) == _argtypes(args), name
    last = lambda args: [a.split()[-1].lstrip("*") for a in args]   # noqa: E731
    # (7g)'s / (7i)'s arguments with alpha_f, n_fant for alpha, F_max after n_max, no mu_out / var_out
    g7 = [a for a in last(_header_args("scaml_target_acqf_batched_f64")[1]) if a not in ("mu_out", "var_out")]
    want = g7[:g7.index("alpha")] + ["alpha_f", "n_fant"] + g7[g7.index("alpha") + 1:]
    want.insert(want.index("n_max") + 1, "F_max")
    assert last(_header_args(ACQF)[1]) == want
    assert last(_header_args(SCORE)[1]) == [a for a in want if a != "grad"]
    assert last(_header_args(ACQF)[1])[:len(ACQF_PTRS)] == list(ACQF_PTRS)
    # (7h')'s arguments likewise
    h7 = last(_header_args("scaml_studies_acqf_opt_own_f64")[1])
    want = h7[:h7.index("alpha_t")] + ["alpha_f", "n_fant"] + h7[h7.index("alpha_t") + 1:]
    want.insert(want.index("n_max") + 1, "F_max")
    assert last(_header_args(OPT)[1]) == want
    assert last(_header_args(OPT)[1])[:len(OPT_ARRAYS)] == list(OPT_ARRAYS)


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    for fn in (_acqf, _score):
        for name in ACQF_PTRS:
            assert fn(**{name: None}) == _lib.E_BADARG, name
        assert fn(value=None) == _lib.E_BADARG
        assert fn(kind=5) == _lib.E_BADARG and fn(acqf=2) == _lib.E_BADARG and fn(acqf=-1) == _lib.E_BADARG
        assert fn(Mq=-1) == _lib.E_BADARG and fn(G=-1) == _lib.E_BADARG
        assert fn(n_max=0) == _lib.E_BADARG and fn(T=0) == _lib.E_BADARG and fn(D=0) == _lib.E_BADARG
        assert fn(F_max=0) == _lib.E_BADARG and fn(F_max=-3) == _lib.E_BADARG
    assert _score(Mq=24) == _lib.E_BADARG                      # whole strips of 16
    assert _acqf(Mq=0, grad=None) == 0                         # the gradient is optional
    for name in OPT_ARRAYS:
        want = 0 if name in OPTIONAL else _lib.E_BADARG        # (optional, as in (5e); B = 0 keeps the GPU out)
        assert _opt(B=0, **{name: None}) == want, name
    for name in OUTPUTS:
        assert _opt(**{name: None}) == _lib.E_BADARG, name
    assert _opt(workspace=ctypes.c_void_p(24)) == _lib.E_BADARG   # not 16-byte aligned
    assert _opt(kind_s=5) == _lib.E_BADARG and _opt(kind_t=-1) == _lib.E_BADARG and _opt(acqf=2) == _lib.E_BADARG and _opt(acqf=-1) == _lib.E_BADARG
    assert _opt(flags=2) == _lib.E_BADARG and _opt(F_max=0) == _lib.E_BADARG
    for k in ("B", "G", "n_evals", "max_iter"):
        assert _opt(**{k: -1}) == _lib.E_BADARG, k
    for k in ("n_max", "T", "N", "D", "max_ls", "history"):
        assert _opt(**{k: 0}) == _lib.E_BADARG, k
    # task_base NULL: the shared stack, Tsrc is not looked at; with the table Tsrc >= 1
    assert _opt(B=0, task_base=None, Tsrc=-7) == 0
    assert _opt(B=0, task_base=ONE, Tsrc=0) == _lib.E_BADARG and _opt(B=0, task_base=ONE, Tsrc=6) == 0


def test_sizes_beyond_the_kernels_are_too_large():
    for fn in (_acqf, _score):
        assert fn(F_max=65) == _lib.E_TOOLARGE and fn(n_max=97) == _lib.E_TOOLARGE and fn(D=16) == _lib.E_TOOLARGE
        # all three limits at once pass every check, the LDS footprint included (nothing to enqueue)
        assert fn(n_max=96, F_max=64, D=15, Mq=0) == 0 and fn(n_max=96, F_max=64, D=15, G=0) == 0
        # bad arguments answer before the size limits
        assert fn(F_max=65, kind=5) == _lib.E_BADARG and fn(n_max=97, acqf=3) == _lib.E_BADARG and fn(D=16, alpha_f=None) == _lib.E_BADARG
        assert fn(n_max=97, F_max=0) == _lib.E_BADARG and fn(F_max=1000, n_fant=None) == _lib.E_BADARG and fn(F_max=65, Mq=-1) == _lib.E_BADARG
    assert _opt(F_max=65) == _lib.E_TOOLARGE and _opt(n_max=97, N=128) == _lib.E_TOOLARGE and _opt(D=16) == _lib.E_TOOLARGE
    assert _opt(n_max=33, N=32) == _lib.E_TOOLARGE                    # more training points than the source pass's LDS strip holds
    assert _opt(n_max=96, F_max=64, N=128, D=15, B=0) == 0            # at the limits, nothing to do
    # the source pass's own limit: the largest N passes with its ordered sums' static LDS counted, in both stack forms; one more does not
    n_top = L.scaml_posterior_max_n()
    assert _opt(n_max=96, F_max=64, N=n_top, D=15, B=0) == 0 and _opt(n_max=96, F_max=64, N=n_top, D=15, B=0, task_base=ONE, Tsrc=2) == 0
    assert _opt(N=n_top + 1, B=0) == _lib.E_TOOLARGE
    assert _opt(F_max=65, kind_t=5) == _lib.E_BADARG and _opt(F_max=65, x0=None) == _lib.E_BADARG and _opt(D=16, F_max=0) == _lib.E_BADARG
    assert _opt(F_max=65, flags=4) == _lib.E_BADARG


def test_nothing_to_do_is_a_no_op():
    assert _acqf(Mq=0) == 0 and _acqf(G=0) == 0 and _score(Mq=0) == 0 and _score(G=0) == 0
    assert _opt(B=0) == 0 and _opt(G=0) == 0 and _opt(B=0, n_evals=0) == 0 and _opt(B=0, flags=1) == 0
