"""The fit family (scaml_gp_fit_fused_f64 in its five variants, scaml_gp_fit_blocked_f64 on both paths, scaml_potrf_batched_f64 at
T > 1, scaml_kernel_matrix_f64) and the MLL gradient (scaml_mll_backward_f64: every dispatchable instance) on the device against the
long-double references of tests/_fit_bounds.py, every output element held to its a-priori bound (capped as that module states), on
the input sets it lists.  The case ids name the kernel instance the dispatch of csrc/scaml_host.cpp sends the case to.  The fit's
output buffers carry one guard task more than the call may write and are handed over full of a sentinel (L of the fused fit and the
POTRF: rows and columns at or past n_t must keep it), zeros (alpha; L of the blocked fit, whose later launches read it) or NaN
(zero_upper = False).  The last test prints the table of the largest error / bound and bound / scale per instance, family and output
(profiles/fit_bounds_notes.md records it)."""
import numpy as np
import pytest
import torch

from scamlgp_amd import _lib, ops
from tests import _fit_bounds as B
from tests._posterior_bounds import SENTINEL

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else t.data_ptr()


class Device:
    """The backend interface of tests/_fit_bounds.py on the C ABI: numpy in, numpy out."""
    name = "device"

    def __init__(self, device):
        self.dev, self.lib = device, _lib.lib
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        assert cus == B.CUS, f"the cases of tests/_fit_bounds.py are chosen for {B.CUS} CUs, this device has {cus}"

    def up(self, a, dtype=torch.float64):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dtype)

    def buf(self, fill, *shape, dtype=torch.float64):
        """shape[0] + 1 slices: the live ones hold `fill`, the last one is the guard and holds the sentinel."""
        b = torch.full((shape[0] + 1, *shape[1:]), fill, dtype=dtype, device=self.dev)
        b[-1] = -7 if dtype == torch.int32 else SENTINEL
        return b

    @staticmethod
    def take(b):
        if b is None:
            return None
        assert bool((b[-1] == (-7 if b.dtype == torch.int32 else SENTINEL)).all()), "the call wrote past the end of an output"
        return b[:-1].cpu().numpy()

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _outputs(self, T, N, fill, store_L, want_alpha):
        NB = (N + 15) // 16
        o = dict(L=self.buf(fill, T, N, N) if store_L else None, alpha=self.buf(0.0, T, N) if want_alpha else None, info=self.buf(-7, T, dtype=torch.int32),
                 Linv_diag=self.buf(SENTINEL, T, NB, 16, 16))
        o.update({k: self.buf(SENTINEL, T) for k in ("quad", "logdet", "mll", "jitter")})
        return o

    def _result(self, o, fill):
        out = {k: self.take(v) for k, v in o.items()}
        out["fill"] = fill
        return out

    def fit(self, c, inp, store_L=True, want_alpha=True, zero_upper=True):
        T, N, D = c.T, c.N, c.D
        X, y, theta, jit = (self.up(inp[k]) for k in ("X", "y", "theta", "jitter_in"))
        npts = self.up(inp["n_points"], torch.int32)
        blocked = N > 256
        fill = (0.0 if blocked else SENTINEL) if zero_upper else float("nan")
        o = self._outputs(T, N, fill, store_L, want_alpha)
        flags = (_lib.FIT_STORE_L if store_L else 0) | (_lib.FIT_ZERO_UPPER if store_L and zero_upper else 0)
        args = (_p(X), _p(y), _p(theta), _p(npts), _p(jit), T, N, D, int(c.kind), _p(o["L"]), _p(o["alpha"]), _p(o["quad"]), _p(o["logdet"]), _p(o["mll"]),
                _p(o["info"]), _p(o["jitter"]), _p(o["Linv_diag"]), flags)
        if not blocked:
            _lib.check_rc(self.lib.scaml_gp_fit_fused_f64(*args, self.stream), "scaml_gp_fit_fused_f64")
            return self._result(o, fill)
        nbytes = int(self.lib.scaml_gp_fit_blocked_workspace_bytes(T, N))
        ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=self.dev)
        was = self.lib.scaml_debug_blocked_fit_path(c.path)
        try:
            _lib.check_rc(self.lib.scaml_gp_fit_blocked_f64(*args, _p(ws), nbytes, self.stream), "scaml_gp_fit_blocked_f64")
            torch.cuda.synchronize(self.dev)
            took = self.lib.scaml_debug_blocked_fit_path(-1)
        finally:
            self.lib.scaml_debug_blocked_fit_path(was)
        assert took == c.path, f"{B.fit_id(c)}: the blocked fit took path {took}"
        return self._result(o, fill)

    def potrf(self, c, inp):
        T, N = c.T, c.N
        A, y = self.up(inp["A"]), self.up(inp["y"])
        npts = self.up(inp["n_points"], torch.int32)
        o = self._outputs(T, N, SENTINEL, True, True)
        del o["mll"]
        _lib.check_rc(self.lib.scaml_potrf_batched_f64(_p(A), _p(y), _p(npts), None, T, N, _p(o["L"]), _p(o["alpha"]), _p(o["quad"]), _p(o["logdet"]), _p(o["info"]),
                                                       _p(o["jitter"]), _p(o["Linv_diag"]), _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER, self.stream),
                      "scaml_potrf_batched_f64")
        return self._result(o, SENTINEL)

    def kmat(self, X, X2, theta, kind, add_noise):
        T, N1, D = X.shape
        N2 = N1 if X2 is None else X2.shape[-2]
        Xd, X2d, th = self.up(X), self.up(X2), self.up(theta)
        K = self.buf(SENTINEL, T, N1, N2)
        _lib.check_rc(self.lib.scaml_kernel_matrix_f64(_p(Xd), _p(X2d), _p(th), T, N1, N2, D, int(kind), 1 if (X2 is not None and X2.ndim == 2) else 0,
                                                       1 if add_noise else 0, _p(K), self.stream), "scaml_kernel_matrix_f64")
        return self.take(K)

    def fit_for_grad(self, fc, inp):
        """The device's own fit of the set through the Python wrapper (the blocked fit past 256 points), kept on the device for `grad`."""
        X, y, theta = (self.up(inp[k]) for k in ("X", "y", "theta"))
        npts = self.up(inp["n_points"], torch.int32)
        fit = ops.gp_fit_fused(X, y, theta, fc.kind, n_points=npts, want_linv=True)
        live = torch.tensor([n > 0 for n in B.counts(fc, inp)], device=self.dev)
        assert not bool((fit["info"] != 0)[live].any())
        return dict(L=fit["L"].cpu().numpy(), alpha=fit["alpha"].cpu().numpy(), Linv_diag=fit["Linv_diag"].cpu().numpy(), dev=(X, theta, npts, fit))

    def grad(self, c, inp, fit, form):
        X, theta, npts, f = fit["dev"]
        was = self.lib.scaml_debug_force_two_launch_grad({"single": 2, "two": 1, "default": 0}[form])
        try:
            g = ops.mll_backward(X, theta, c.kind, f["L"], f["Linv_diag"], f["alpha"], n_points=npts).cpu().numpy()
        finally:
            self.lib.scaml_debug_force_two_launch_grad(was)
        return g


def test_the_limits_the_cases_are_chosen_for():
    """The largest D per class and of the blocked fit, as tests/_fit_bounds.py has them, against the library."""
    for np_, d in B.FIT_MAX_D.items():
        assert _lib.lib.scaml_fit_max_d(np_) == d and _lib.lib.scaml_fit_max_d(np_ // 2 + 1) == d
    assert _lib.lib.scaml_fit_blocked_max_d() == B.BLOCKED_MAX_D
    assert _lib.lib.scaml_fit_max_n() == 256 and _lib.lib.scaml_fit_blocked_max_n() == 512


@pytest.mark.parametrize("case", B.FIT_CASES, ids=B.fit_id)
def test_fit_within_its_bounds(case, device):
    """L L^T, the padding, Linv_diag, alpha, quad, logdet, mll of every referenced task; info and jitter_used exact; a task with a NaN
    coordinate reports info > 0 and leaves its neighbours within their bounds."""
    B.check_fit(Device(device), case)


@pytest.mark.parametrize("case", B.FLAG_CASES, ids=B.fit_id)
def test_fit_flags(case, device):
    """store_L = False with alpha = NULL: the same scalars bit for bit; zero_upper = False: a NaN-filled upper triangle stays NaN."""
    B.check_flags(Device(device), case)


@pytest.mark.parametrize("case", B.POTRF_CASES, ids=B.potrf_id)
def test_potrf_within_its_bounds(case, device):
    B.check_potrf(Device(device), case)


@pytest.mark.parametrize("case", B.KMAT_CASES, ids=B.kmat_id)
def test_kernel_matrix_within_its_bound(case, device):
    B.check_kmat(Device(device), case)


@pytest.mark.parametrize("case", B.GRAD_CASES, ids=B.grad_id)
def test_mll_gradient_within_its_bound(case, device):
    """The device's own fit of the set, then the gradient on the forced path the id names (`default->`: by shape, against both forced
    paths): every referenced task within its bound, an empty task exactly zero."""
    B.check_grad(Device(device), case)


def test_zz_ratio_table(device):
    """Module-level summary (runs last): the largest error / bound and bound / scale per kernel instance, family and output."""
    lines = B.report()
    assert lines, "no comparison was made"
    print("\n" + "\n".join(lines))
