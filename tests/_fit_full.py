"""The launcher's rule for the full-tile instance of the fused fit (fit_full_instance, csrc/gp_dispatch.h) for the tests: the header
compiled as host code (tests/host_emul/fit_full_emul.cpp), built once per process when this module is first imported.
tests/test_fit_full_dispatch.py pins the rule; tests/test_fit_full_instance_gpu.py names the instance a case takes with it."""
import ctypes
import tempfile

from tests._host_emul import build

_DIR = tempfile.TemporaryDirectory(prefix="scaml_fit_full_")      # (kept for the life of the process)
_lib = build(None, "fit_full_emul", _DIR.name)
_I, _ULL = ctypes.c_int, ctypes.c_ulonglong
_lib.emul_fit_full_instance.argtypes = [_I] * 7 + [_ULL, _I]
_lib.emul_fit_full_of_call.argtypes = [_I] * 8 + [_ULL, _I]


def fit_full_instance(nb, wu, N, ragged=False, from_matrix=False, blocked=False, stores_l=True, l_addr=0, mode=0):
    """The rule on the instance <nb, wu>.  The defaults satisfy the contract: a test switches one clause off at a time."""
    return bool(_lib.emul_fit_full_instance(nb, wu, N, int(ragged), int(from_matrix), int(blocked), int(stores_l), int(l_addr), mode))


def fit_full_of_call(T, N, D, cus, ragged=False, from_matrix=False, blocked=False, stores_l=True, l_addr=0, mode=0):
    """... on the instance the launcher's plan gives the call (fit_plan), as fit_common of csrc/scaml_host.cpp asks it."""
    return bool(_lib.emul_fit_full_of_call(T, N, D, cus, int(ragged), int(from_matrix), int(blocked), int(stores_l), int(l_addr), mode))
