"""Scaffolding of the host-emulation tests (tests/test_*_emul.py): a kernel source of csrc/ compiled as single-threaded host code
(tests/host_emul/<name>.cpp) and loaded through ctypes.  Test infrastructure, not a conftest: each test module keeps its own ``emul``
fixture, which calls ``build`` and declares the argtypes of the entry points it uses."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scalable-meta-learning-with-gaussian-processes_amd", "csrc")
DP, IP, BP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)


def build(tmp_path_factory, name: str, out_dir=None) -> ctypes.CDLL:
    """tests/host_emul/<name>.cpp -> a shared object in a temporary directory (or in out_dir, for a module that builds once outside
    a fixture), loaded."""
    so = os.path.join(out_dir, name + ".so") if out_dir else str(tmp_path_factory.mktemp("emul") / (name + ".so"))
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host_emul", name + ".cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def ptr(a: np.ndarray):
    """The array's data as the pointer type of its dtype: int32 -> IP, uint8 -> BP, anything else DP."""
    return a.ctypes.data_as({np.dtype(np.int32): IP, np.dtype(np.uint8): BP}.get(a.dtype, DP))
