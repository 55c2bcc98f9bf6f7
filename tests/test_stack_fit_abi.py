"""scaml_stack_fit_f64 answers bad arguments before any HIP call (never-dereferenced pointers, no GPU), and
scaml_stack_fit_workspace_bytes grows with every argument."""
import ctypes

from scamlgp_amd import _lib

L = _lib.lib
ONE = ctypes.c_void_p(16)   # never dereferenced: validation fails first
SPEC = (ctypes.c_double * 15)(1e-4, 1e2, 1e-4, 1e2, 1e-8, 1e-2, 1, 3.0, 6.0, 1, 2.0, 0.15, 2, -8.0, 2.0)
BIG = 1 << 40


def _call(X=ONE, y=ONE, spec=SPEC, z=ONE, B=2, N=64, D=3, kind=0, n_evals=1, flags=0, max_iter=50, history=10, value=ONE, stats=ONE,
          ws=ONE, ws_bytes=BIG):
    return L.scaml_stack_fit_f64(X, y, None, spec, z, B, N, D, kind, n_evals, flags, max_iter, history, 1e-5, 2.2e-9, value, stats, ws,
                                 ws_bytes, None)


def test_limits():
    assert 8 <= L.scaml_stack_fit_max_d() <= 62   # one lane per variable: D + 2 <= 64


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    for name in ("X", "y", "spec", "z", "value", "stats", "ws"):
        assert _call(**{name: None}) == _lib.E_BADARG, name
    assert _call(kind=5) == _lib.E_BADARG
    assert _call(flags=2) == _lib.E_BADARG                        # only SCAML_STACK_FIT_CONTINUE is defined
    assert _call(history=0) == _lib.E_BADARG
    assert _call(history=17) == _lib.E_BADARG
    assert _call(n_evals=-1) == _lib.E_BADARG
    assert _call(B=-1) == _lib.E_BADARG
    bad = (ctypes.c_double * 15)(*SPEC)
    bad[4], bad[5] = 1e-2, 1e-8                                   # inverted noise interval
    assert _call(spec=bad) == _lib.E_BADARG
    bad = (ctypes.c_double * 15)(*SPEC)
    bad[9] = 7                                                    # unknown prior kind
    assert _call(spec=bad) == _lib.E_BADARG
    bad = (ctypes.c_double * 15)(*SPEC)
    bad[8] = -1.0                                                 # Gamma rate must be positive
    assert _call(spec=bad) == _lib.E_BADARG
    need = L.scaml_stack_fit_workspace_bytes(2, 64, 3, 10)
    assert need > 0
    assert _call(ws_bytes=need - 1) == _lib.E_BADARG              # workspace too small
    assert _call(ws=ctypes.c_void_p(24)) == _lib.E_BADARG         # not 16-byte aligned


def test_sizes_beyond_the_kernels_are_too_large():
    assert _call(N=513) == _lib.E_TOOLARGE
    assert _call(N=264) == _lib.E_TOOLARGE                        # beyond 256 points: multiples of 16 only
    assert _call(N=100000) == _lib.E_TOOLARGE
    assert _call(D=L.scaml_stack_fit_max_d() + 1) == _lib.E_TOOLARGE
    assert _call(N=256, D=L.scaml_fit_max_d(256) + 1) == _lib.E_TOOLARGE
    assert _call(N=512, D=L.scaml_fit_blocked_max_d() + 1) == _lib.E_TOOLARGE


def test_nothing_to_do_is_a_no_op():
    assert _call(B=0) == 0
    assert _call(n_evals=0) == 0
    assert _call(n_evals=0, flags=_lib.STACK_FIT_CONTINUE) == 0


def test_workspace_bytes_is_monotone_in_each_argument():
    f = L.scaml_stack_fit_workspace_bytes
    base = dict(B=6, N=128, D=4, history=5)
    steps = dict(B=range(0, 70, 3), N=[1, 15, 16, 17, 100, 128, 255, 256, 272, 384, 512], D=range(1, 9), history=range(1, 17))
    for name, values in steps.items():
        sizes = [f(*{**base, name: v}.values()) for v in values]
        assert all(s > 0 for s in sizes[1:]), (name, sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (name, sizes)
        assert sizes[-1] > sizes[0], (name, sizes)
    # it holds what the fit and gradient paths need next to the optimiser state
    assert f(6, 128, 4, 5) >= 6 * 128 * 128 * 8 + L.scaml_mll_backward_workspace_doubles(6, 128, 4) * 8
    assert f(6, 384, 4, 5) >= f(6, 256, 4, 5) + L.scaml_gp_fit_blocked_workspace_bytes(6, 384)
    # out of range: no size
    assert f(-1, 128, 4, 5) == 0 and f(6, 513, 4, 5) == 0 and f(6, 128, 0, 5) == 0 and f(6, 128, 4, 17) == 0
