"""The target GP's objective and gradient (scaml_target_mll_f64, scaml_target_fit_f64 and their batched forms: csrc/gp_target_fit.hip,
both factorisations) on the MI355X against the long-double reference of tests/_target_fit_bounds.py: the value and every gradient
entry of every start point held to the a-priori bound (capped as that module states) on the input sets it lists; info and
jitter_used exact; the rows past B of every output buffer, handed over full of a sentinel, untouched; non-finite inputs fail alone.
The case ids name the factorisation the dispatch sends the shape to (`forced`: through scaml_debug_target_fit_path(1)).  The last
test prints the table of the largest error / bound and bound / scale per path, family and output
(profiles/target_fit_bounds_notes.md records it)."""
import ctypes

import numpy as np
import pytest
import torch

from scamlgp_amd import _lib
from tests import _target_fit_bounds as TF
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF, SENTINEL

pytestmark = pytest.mark.gpu


def _p(t):
    return t.data_ptr()


class Device:
    """The backend interface of tests/_target_fit_bounds.py on the C ABI: numpy in, numpy out."""
    name, arith = "device", TF.DEVICE_ARITH

    def __init__(self, device):
        self.dev, self.lib = device, _lib.lib

    def up(self, a, dtype=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dtype)

    def max_n(self, T, D):
        return int(self.lib.scaml_target_fit_max_n(T, D))

    def path_of(self, n, T, D, forced):
        """(tests/test_target_fit_bounds.py checks target_fit_mfma_shape for every n <= 112 of the input sets)"""
        return TF.device_path(n, T, D, forced)

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _buffers(self, rows, P):
        r = rows + TF.GUARD
        return dict(value=torch.full((r,), SENTINEL, dtype=torch.float64, device=self.dev), grad=torch.full((r, P), SENTINEL, dtype=torch.float64, device=self.dev),
                    info=torch.full((r,), -7, dtype=torch.int32, device=self.dev), jitter=torch.full((r,), SENTINEL, dtype=torch.float64, device=self.dev))

    def _forced(self, forced, call):
        was = self.lib.scaml_debug_target_fit_path(1 if forced else 0)
        try:
            rc = call()
            torch.cuda.synchronize(self.dev)
        finally:
            self.lib.scaml_debug_target_fit_path(was)
        return rc

    @staticmethod
    def _spec(spec):
        return (ctypes.c_double * len(spec))(*[float(v) for v in spec])

    def _single_args(self, prob, z):
        t = [self.up(prob[k]) for k in ("means_t", "covs_p", "X", "y")]
        return t, (*[_p(x) for x in t], float(prob["m_all"]), float(prob["s_all"]), self._spec(prob["spec"]), _p(z), z.shape[0], prob["n"], prob["T"], prob["D"],
                   int(prob["kind"]))

    def _batch_args(self, b, z):
        t = [self.up(b[k]) for k in ("means_t", "covs_p", "X", "y")] + [self.up(b["n_points"], torch.int32), self.up(b["m_all"]), self.up(b["s_all"])]
        return t, (*[_p(x) for x in t], self._spec(b["spec"]), _p(z), z.shape[0], z.shape[1], b["n_max"], b["T"], b["D"], int(b["kind"]))

    def _mll(self, name, keep, head, rows, P, forced):
        o = self._buffers(rows, P)
        rc = self._forced(forced, lambda: getattr(self.lib, name)(*head, _p(o["value"]), _p(o["grad"]), _p(o["info"]), _p(o["jitter"]), self.stream))
        _lib.check_rc(rc, name)
        return {k: v.cpu().numpy() for k, v in o.items()}

    def mll(self, prob, z, forced):
        zd = self.up(z)
        keep, head = self._single_args(prob, zd)
        return self._mll("scaml_target_mll_f64", keep, head, z.shape[0], z.shape[1], forced)

    def mll_batched(self, b, z, forced):
        zd = self.up(z)
        keep, head = self._batch_args(b, zd)
        return self._mll("scaml_target_mll_batched_f64", keep, head, z.shape[0] * z.shape[1], z.shape[2], forced)

    def _fit(self, name, wsname, keep, head, lead, zd, forced, max_iter, T, D):
        rows, P = int(np.prod(lead)), zd.shape[-1]
        o = self._buffers(rows, P)
        stats = torch.zeros((*lead, 4), dtype=torch.int32, device=self.dev)
        nws = int(getattr(self.lib, wsname)(*lead, T, D, 10))
        ws = torch.empty(max(nws, 1), dtype=torch.float64, device=self.dev)
        rc = self._forced(forced, lambda: getattr(self.lib, name)(*head, int(max_iter), 10, 1e-5, 2.2e-9, _p(o["value"]), _p(o["info"]), _p(o["jitter"]), _p(stats), _p(ws),
                                                                 nws, self.stream))
        _lib.check_rc(rc, name)
        res = {k: o[k].cpu().numpy() for k in ("value", "info", "jitter")}
        for k in res:
            assert (res[k][rows:] == (-7 if k == "info" else SENTINEL)).all(), f"{name}: {k} was written past row {rows}"
        out = {k: v[:rows].reshape(lead) for k, v in res.items()}
        out.update(z=zd.cpu().numpy(), stats=stats.cpu().numpy())
        return out

    def fit(self, prob, z0, forced, max_iter):
        zd = self.up(z0.copy())
        keep, head = self._single_args(prob, zd)
        return self._fit("scaml_target_fit_f64", "scaml_target_fit_workspace_doubles", keep, head, (z0.shape[0],), zd, forced, max_iter, prob["T"], prob["D"])

    def fit_batched(self, b, z0, forced, max_iter):
        zd = self.up(z0.copy())
        keep, head = self._batch_args(b, zd)
        return self._fit("scaml_target_fit_batched_f64", "scaml_target_fit_batched_workspace_doubles", keep, head, z0.shape[:2], zd, forced, max_iter, b["T"], b["D"])


def test_the_limits_the_cases_are_chosen_for(device):
    be = Device(device)
    assert be.lib.scaml_target_fit_max_d() == 16
    for c in TF.CASES:
        c = TF.resolve(be, c)
        assert c.n <= be.max_n(c.T, c.D) and c.D <= 16, TF.case_id(c)
    assert 128 < be.max_n(4, 4) <= 144


@pytest.mark.parametrize("case", TF.CASES, ids=TF.case_id)
def test_objective_and_gradient_within_bounds(case, device):
    TF.check_mll(Device(device), case)


@pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])
def test_ragged_batch_within_bounds(kind, device):
    TF.check_ragged(Device(device), kind)


@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
@pytest.mark.parametrize("case", TF.REFIT_CASES, ids=TF.case_id)
def test_refit_value_within_bound_at_returned_point(case, batched, device):
    TF.check_refit(Device(device), case, batched)


@pytest.mark.parametrize("forced", [False, True], ids=["matrix-core", "column-by-column"])
def test_jitter_set(forced, device):
    TF.check_jitter(Device(device), forced)


@pytest.mark.parametrize("case", TF.NAN_CASES, ids=TF.case_id)
@pytest.mark.parametrize("what", ["weight", "ls", float("nan"), float("inf")], ids=["weight", "lengthscale", "x-nan", "x-inf"])
def test_non_finite_inputs_fail_alone(case, what, device):
    if isinstance(what, str):
        TF.check_nan_start(Device(device), case, what)
    else:
        TF.check_nan_point(Device(device), case, what)


def test_zz_ratio_table(device):
    """Module-level summary (runs last): the largest error / bound and bound / scale per path, family and output."""
    lines = TF.report()
    assert lines, "no comparison was made"
    print("\n" + "\n".join(lines))
