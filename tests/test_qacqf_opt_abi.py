"""The entry points of the joint acquisition's device optimiser (include/scaml_gp.h (7s), (7t)): exported, declared and bound with the
header's argument lists; the argument checks and size limits answer before any HIP call (never-dereferenced pointers, no GPU)."""
import ctypes
import os
import re

from scamlgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first (and 16-byte aligned, as the workspace has to be)
NAMES = ("scaml_qacqf_opt_max_p", "scaml_qacqf_opt_step_workspace_bytes", "scaml_qacqf_opt_workspace_bytes", "scaml_qacqf_opt_step_f64",
         "scaml_qacqf_opt_f64")
HEAD = ("x0", "slots", "Xa", "X", "theta_s", "Linv", "alpha_s", "y_mean", "y_std", "n_points_s", "VA", "w", "active", "mu_t", "cov_tt", "var_t",
        "Xt", "theta_t", "targets", "L", "Linv_diag", "alpha_t")
TAIL = ("info", "base_samples", "Xp", "Zp", "mu_p", "Sigma_pp")
PENDING = ("Xp", "Zp", "mu_p", "Sigma_pp")
OPTIONAL = ("slots", "y_mean", "y_std", "n_points_s", "active", "info") + PENDING     # (the pending set: optional while p == 0)
OUTPUTS = ("lo", "hi", "workspace", "x", "f", "stats")
BIG = 1 << 40


def _opt(B=5, Bs=None, n=8, p=0, q=2, S=16, T=3, N=32, D=2, kind_s=0, kind_t=0, acqf=0, acqf_param=1.0, m_all=0.0, s_all=1.0, max_iter=10,
         history=10, max_ls=20, gtol=1e-5, ftol=2.2e-9, c1=1e-4, n_evals=1, flags=0, workspace_bytes=BIG, **ptrs):
    Bs = B if Bs is None else Bs
    h = [ptrs.get(k, ONE) for k in HEAD]
    t = [ptrs.get(k, ONE) for k in TAIL]
    o = {k: ptrs.get(k, ONE) for k in OUTPUTS}
    return L.scaml_qacqf_opt_f64(*h, m_all, s_all, *t, B, Bs, n, p, q, S, T, N, D, kind_s, kind_t, acqf, acqf_param, o["lo"], o["hi"], max_iter,
                                 history, max_ls, gtol, ftol, c1, n_evals, flags, o["workspace"], workspace_bytes, o["x"], o["f"], o["stats"], None)


def _header_argtypes(name):
    """(restype, argtypes) of a declaration of include/scaml_gp.h, as ctypes reads them."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    ret, args = re.search(r"(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    kinds = (("double", ctypes.c_double), ("unsigned", ctypes.c_uint), ("long long ", ctypes.c_longlong), ("int ", ctypes.c_int))
    out = []
    for a in (x.strip() for x in args.split(",")):
        if a == "void":
            continue
        out.append(ctypes.c_void_p if "*" in a else next(t for prefix, t in kinds if a.startswith(prefix)))
    return (ctypes.c_longlong if ret == "long long" else ctypes.c_int), out


STEP_ARRAYS = ("value", "grad", "slots", "x0", "lo", "hi")
STEP_OUTPUTS = ("state", "Xq", "x", "f", "stats")


def _step(B=5, Bs=None, P=24, mode=1, max_iter=10, history=10, max_ls=20, gtol=1e-5, ftol=2.2e-9, c1=1e-4, **ptrs):
    Bs = B if Bs is None else Bs
    a = [ptrs.get(k, ONE) for k in STEP_ARRAYS]
    o = [ptrs.get(k, ONE) for k in STEP_OUTPUTS]
    return L.scaml_qacqf_opt_step_f64(*a, B, Bs, P, mode, max_iter, history, max_ls, gtol, ftol, c1, *o, None)


def test_symbols_are_exported_declared_and_bound():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaml_gp.h")).read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name


def test_ctypes_table_matches_the_header():
    for name in NAMES:
        restype, argtypes = _header_argtypes(name)
        assert _lib.SIGNATURES[name][0] is restype, name
        assert list(_lib.SIGNATURES[name][1]) == argtypes, name
    assert len(_lib.SIGNATURES["scaml_qacqf_opt_f64"][1]) == len(HEAD) + 2 + len(TAIL) + 12 + 1 + 2 + 3 + 3 + 2 + 2 + 3 + 1
    assert len(_lib.SIGNATURES["scaml_qacqf_opt_step_f64"][1]) == len(STEP_ARRAYS) + 7 + 3 + len(STEP_OUTPUTS) + 1


def test_limits_and_the_python_mirror():
    from scamlgp_amd import ops

    assert L.scaml_qacqf_opt_max_p() == 128 == ops.qacqf_opt_max_p()
    assert ops.QACQF_OPT_EVALS_PER_CALL >= 1
    for P, history in ((1, 1), (24, 10), (120, 16), (128, 16)):
        stride = ops.studies_acqf_opt_state_doubles(P, history)
        assert stride == (4 + 2 * history) * P + history + 16
        assert L.scaml_qacqf_opt_step_workspace_bytes(3, P, history) == 3 * 8 * stride
    # the state opens (7s)'s workspace
    assert L.scaml_qacqf_opt_workspace_bytes(1, 1, 0, 8, 1, 16, 15, 16) >= 8 * ops.studies_acqf_opt_state_doubles(120, 16)


def test_step_refusals_answer_without_touching_the_gpu():
    for name in STEP_OUTPUTS + ("lo", "hi"):
        assert _step(**{name: None}) == _lib.E_BADARG, name
    assert _step(mode=0, x0=None) == _lib.E_BADARG and _step(mode=1, value=None) == _lib.E_BADARG and _step(mode=1, grad=None) == _lib.E_BADARG
    assert _step(Bs=0, mode=1, x0=None) == 0 and _step(Bs=0, mode=0, value=None, grad=None) == 0 and _step(Bs=0, mode=2, x0=None, value=None, grad=None) == 0
    assert _step(slots=None, Bs=3) == _lib.E_BADARG          # NULL is the identity: Bs = B
    assert _step(slots=None, B=0) == 0
    assert _step(Bs=6) == _lib.E_BADARG and _step(B=-1, Bs=-1) == _lib.E_BADARG and _step(Bs=-1) == _lib.E_BADARG
    assert _step(mode=3) == _lib.E_BADARG and _step(mode=-1) == _lib.E_BADARG
    assert _step(P=0) == _lib.E_BADARG and _step(max_iter=-1) == _lib.E_BADARG and _step(max_ls=0) == _lib.E_BADARG
    assert _step(history=0) == _lib.E_BADARG and _step(history=17) == _lib.E_BADARG
    assert _step(gtol=-1.0) == _lib.E_BADARG and _step(gtol=float("nan")) == _lib.E_BADARG
    assert _step(c1=0.0) == _lib.E_BADARG and _step(ftol=float("nan")) == _lib.E_BADARG
    # the size limits, behind the bad arguments
    assert _step(P=129) == _lib.E_TOOLARGE and _step(P=128, Bs=0) == 0
    assert _step(P=129, mode=5) == _lib.E_BADARG and _step(P=129, f=None) == _lib.E_BADARG and _step(P=1000, history=0) == _lib.E_BADARG
    wb = L.scaml_qacqf_opt_step_workspace_bytes
    assert wb(4, 128, 16) > 0 and wb(4, 129, 16) == 0 and wb(4, 0, 16) == 0 and wb(-1, 8, 4) == 0 and wb(4, 8, 0) == 0 and wb(4, 8, 17) == 0


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    for name in HEAD + TAIL:
        want = 0 if name in OPTIONAL else _lib.E_BADARG   # (B = 0 below keeps the GPU out)
        assert _opt(B=0, **{name: None}) == want, name
    for name in PENDING:                                   # read when p > 0
        assert _opt(B=0, p=2, **{name: None}) == _lib.E_BADARG, name
    for name in OUTPUTS:
        assert _opt(**{name: None}) == _lib.E_BADARG, name
    assert _opt(workspace=ctypes.c_void_p(24)) == _lib.E_BADARG   # not 16-byte aligned
    need = L.scaml_qacqf_opt_workspace_bytes(5, 8, 0, 2, 3, 32, 2, 10)
    assert need > 0 and _opt(workspace_bytes=need - 1) == _lib.E_BADARG and _opt(B=0, workspace_bytes=need) == 0
    assert _opt(kind_s=5) == _lib.E_BADARG and _opt(kind_t=-1) == _lib.E_BADARG
    assert _opt(acqf=2) == _lib.E_BADARG and _opt(acqf=17) == _lib.E_BADARG and _opt(acqf=-1) == _lib.E_BADARG   # (no joint LogEI)
    assert _opt(flags=2) == _lib.E_BADARG and _opt(flags=3) == _lib.E_BADARG
    assert _opt(s_all=0.0) == _lib.E_BADARG and _opt(s_all=float("nan")) == _lib.E_BADARG
    for k in ("B", "Bs", "n_evals", "max_iter", "p"):
        assert _opt(**{k: -1}) == _lib.E_BADARG, k
    for k in ("n", "q", "S", "T", "N", "D", "max_ls", "history"):
        assert _opt(**{k: 0}) == _lib.E_BADARG, k
    assert _opt(Bs=6) == _lib.E_BADARG and _opt(slots=None, Bs=3) == _lib.E_BADARG
    assert _opt(history=17) == _lib.E_BADARG
    assert _opt(gtol=-1.0) == _lib.E_BADARG and _opt(gtol=float("nan")) == _lib.E_BADARG
    assert _opt(c1=0.0) == _lib.E_BADARG and _opt(ftol=float("nan")) == _lib.E_BADARG


def test_sizes_beyond_the_kernels_are_too_large():
    big = dict(N=128)
    assert _opt(q=8, p=1, **big) == _lib.E_TOOLARGE and _opt(q=9, **big) == _lib.E_TOOLARGE and _opt(q=1, p=8, **big) == _lib.E_TOOLARGE
    assert _opt(n=90, q=4, p=3, **big) == _lib.E_TOOLARGE and _opt(n=95, q=2, **big) == _lib.E_TOOLARGE      # n + p + q = 97
    assert _opt(n=30, q=3, N=32) == _lib.E_TOOLARGE                                                        # n + p + q > N
    assert _opt(D=16) == _lib.E_TOOLARGE and _opt(S=513) == _lib.E_TOOLARGE
    assert _opt(N=L.scaml_posterior_max_n() + 1) == _lib.E_TOOLARGE
    # at the limits, nothing to do
    assert _opt(n=88, q=8, D=15, S=512, B=0, **big) == 0 and _opt(n=89, q=1, p=6, B=0, **big) == 0 and _opt(n=88, q=1, p=7, B=0, **big) == 0
    # bad arguments answer before the size limits
    assert _opt(q=9, kind_t=5, **big) == _lib.E_BADARG and _opt(D=16, acqf=3) == _lib.E_BADARG and _opt(n=97, x0=None, **big) == _lib.E_BADARG
    assert _opt(D=16, history=0) == _lib.E_BADARG and _opt(D=16, flags=4) == _lib.E_BADARG and _opt(S=513, base_samples=None) == _lib.E_BADARG
    assert _opt(q=8, p=1, Xp=None, **big) == _lib.E_BADARG and _opt(n=1000, Xt=None) == _lib.E_BADARG


def test_nothing_to_do_is_a_no_op():
    assert _opt(B=0) == 0 and _opt(Bs=0) == 0 and _opt(n_evals=0) == 0
    assert _opt(B=0, n_evals=0) == 0 and _opt(B=0, flags=1) == 0 and _opt(Bs=0, flags=1) == 0


def test_workspace_bytes_is_monotone_and_zero_exactly_for_the_refused_shapes():
    wb = L.scaml_qacqf_opt_workspace_bytes
    base = dict(B=10, n=16, p=1, q=3, T=4, N=64, D=3, history=5)
    order = ("B", "n", "p", "q", "T", "N", "D", "history")
    at = lambda **kw: wb(*[{**base, **kw}[k] for k in order])   # noqa: E731
    assert at() > 0 and at() % 256 == 0
    for k in order:
        vals = [at(**{k: v}) for v in range(base[k], base[k] + 4)]
        assert all(b >= a for a, b in zip(vals, vals[1:])) and vals[-1] > vals[0], (k, vals)
    assert at(B=0) < at(B=1)
    # the limits of (5g) / (7p) / (7q) and nothing narrower
    assert at(q=8, p=0) > 0 and at(q=1, p=7) > 0 and at(q=5, p=4) == 0 and at(q=9, p=0) == 0            # q + p = 9
    assert at(n=88, q=8, p=0, N=96) > 0 and at(n=89, q=8, p=0, N=128) == 0 and at(n=90, q=3, p=4, N=128) == 0   # n + p + q = 97
    assert at(n=60, q=3, p=1, N=64) > 0 and at(n=61, q=3, p=1, N=64) == 0                                # n + p + q <= N
    assert at(D=15) > 0 and at(D=16) == 0 and at(history=16) > 0 and at(history=17) == 0
    assert at(N=L.scaml_posterior_max_n()) > 0 and at(N=L.scaml_posterior_max_n() + 1) == 0
    for bad in (dict(B=-1), dict(n=0), dict(p=-1), dict(q=0), dict(T=0), dict(N=0), dict(D=0), dict(history=0)):
        assert at(**bad) == 0, bad
    # whatever the call takes has a workspace, and the other way round (shape limits; S is not the workspace's)
    for shape in (dict(q=8, p=0), dict(q=5, p=4), dict(n=60, q=3, p=1), dict(n=61, q=3, p=1), dict(D=16), dict(history=17)):
        s = {**base, **shape}
        rc = _opt(B=0, **{k: s[k] for k in ("n", "p", "q", "T", "N", "D", "history")})
        assert (rc == 0) == (at(**shape) > 0), (shape, rc)
