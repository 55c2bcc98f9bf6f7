"""The launcher's dispatch plans (csrc/gp_dispatch.h) for the tests: the header compiled as host code (tests/host_emul/dispatch_emul.cpp),
built once per process when this module is first imported.  A test helper that has to name the kernel instance a case exercises asks
here, so the answer is the launcher's own and moves with it; tests/test_dispatch.py pins every edge of the rules themselves."""
import ctypes
import tempfile
from collections import namedtuple

from tests._host_emul import build

_DIR = tempfile.TemporaryDirectory(prefix="scaml_dispatch_")      # (kept for the life of the process)
_lib = build(None, "dispatch_emul", _DIR.name)
_LL = ctypes.c_longlong
_lib.emul_lds_limit.restype = _LL
_lib.emul_blocked_plan.argtypes = [ctypes.c_int] * 5 + [_LL, ctypes.c_int, ctypes.POINTER(_LL)]

LDS_LIMIT = int(_lib.emul_lds_limit())
LINV_TARGET_WORKGROUPS = int(_lib.emul_linv_target_workgroups())
_limits = (_LL * 3)()
_lib.emul_studies_limits(_limits)
STUDIES_MAX_N, STUDIES_MAX_D, STUDIES_MAX_FANTASIES = (int(v) for v in _limits)   # csrc/gp_studies_acqf.h

FitPlan = namedtuple("FitPlan", "variant nb wu block lds_doubles")
BlockedPlan = namedtuple("BlockedPlan", "path t8 parts lds_coop flag_bytes need nt solve_small_d rounds lds_solve lds_syrk")
GradPlan = namedtuple("GradPlan", "single sc nbt dma split grid_x grid_y block lds_doubles")
TargetFitPlan = namedtuple("TargetFitPlan", "use_mfma lds_doubles")
PosteriorPlan = namedtuple("PosteriorPlan", "waves xl")


def _plan(cls, fn, *args):
    out = (_LL * len(cls._fields))()
    fn(*[int(a) for a in args], out)
    return cls(*[int(v) for v in out])


def fit_class(N):
    return int(_lib.emul_fit_class(N))


def fit_class_max_d(N):
    return int(_lib.emul_fit_class_max_d(N))


def fit_plan(T, N, D, cus):
    return _plan(FitPlan, _lib.emul_fit_plan, T, N, D, cus)


def narrow_fit_tasks(cus, N=128, D=1):
    """The smallest stack the launcher sends to the narrow (8, 3) instance of the 64 < N <= 128 class on a device of `cus` CUs."""
    T = next(T for T in range(1, 1 << 16) if fit_plan(T, N, D, cus).variant == 2)
    p = fit_plan(T, N, D, cus)
    assert (p.nb, p.wu) == (8, 3), p
    return T


def blocked_plan(T, N, D, cus, mode=0, workspace_bytes=2 ** 62, no_retry=False):
    """workspace_bytes: the default never binds."""
    return _plan(BlockedPlan, _lib.emul_blocked_plan, T, N, D, cus, mode, workspace_bytes, no_retry)


def grad_plan(T, N, D, cus, mode=0, no_split=False, ragged=False, aligned16=True):
    return _plan(GradPlan, _lib.emul_grad_plan, T, N, D, cus, mode, no_split, ragged, aligned16)


def target_fit_plan(n, T, D, mode=0, batched=False):
    return _plan(TargetFitPlan, _lib.emul_target_fit_plan, n, T, D, mode, batched)


def posterior_plan(N, D):
    return _plan(PosteriorPlan, _lib.emul_posterior_plan, N, D)


def strip_solve_waves(np_):
    return int(_lib.emul_strip_solve_waves(np_))


def linv_groups(T, nb, waves):
    return int(_lib.emul_linv_groups(T, nb, waves))
