"""scaml_target_fantasy_acqf_f64 ((7f), csrc/gp_fantasy.hip) through the C ABI against the long-double reference of
tests/_fantasy_bounds.py, value and gradient held element by element to its a-priori bound (capped at 1e-8 of the output's scale), on
the input sets that module lists: the shape edges of the three phases, both families and acquisition functions, the clamps, EI's
tails, info, the refusals, the non-finite-query rule, the F = 1 cross-check against the finish and the target gradient, and the real
pipeline.  scaml_target_acqf_batched_f64's value is held to the transform bound alone, from its own mu_out / var_out.  Every output
buffer holds a sentinel and one guard row more than the call may write.  Each test prints the largest error / bound and bound /
scale seen so far (profiles/fantasy_bounds_notes.md records them).

The batched acquisition's check here sees only the transform from the kernel's own mu_out / var_out.  The full bound of that kernel
body -- the task sums, the solve, the posterior and the gradient of all four entry points of sa_block -- lives in
tests/_studies_bounds.py and is held by tests/test_studies_bounds.py / tests/test_studies_bounds_gpu.py."""
import numpy as np
import pytest
import torch

from scamlgp_amd import _lib
from tests import _fantasy_bounds as FB
from tests import _target_bounds as B
from tests import test_studies_acqf_emul as SE
from tests._fantasy_bounds import EI, UCB
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF
from tests.test_target_bounds_gpu import Device as TargetDevice, _p

pytestmark = pytest.mark.gpu
FAMILIES = pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])


class Device(TargetDevice):
    """tests/test_target_bounds_gpu.Device with the fantasy kernel: the buffers have the shapes of the ARRAYS, the scalars are passed as
    the set states them (a refused call brings the buffers of a legal one)."""

    def fantasy(self, a, info):
        want_grad = bool(a.get("grad"))
        ins = [self.up(a[k]) for k in ("Knq", "Z", "alpha", "mean_q", "var_q")]
        gin = [self.up(a[k]) if want_grad else None for k in ("cov_g", "mu_g", "var_g", "Xt", "Xq", "theta")]
        inf = None if info is None else torch.tensor([info], dtype=torch.int32, device=self.dev)
        value = self.out(a["mean_q"].shape[0])
        grad = self.out(a["mean_q"].shape[0], a["Xq"].shape[1]) if want_grad else None
        rc = self.lib.scaml_target_fantasy_acqf_f64(*[_p(x) for x in ins], float(a["m"]), float(a["s"]), float(a["noise_add"]), _p(inf), int(a["acqf"]),
                                                    float(a["param"]), *[_p(x) for x in gin], int(a["n"]), int(a["M"]), int(a["F"]), int(a["D"]),
                                                    int(a["kind"]), _p(value), _p(grad), self.stream)
        return rc, self.take(value), (self.take(grad) if want_grad else None)


def _show():
    for line in FB.report():
        print(line)


@pytest.mark.parametrize("case", FB.GRAD_CASES, ids=FB.grad_id)
def test_value_and_gradient_within_their_bounds(case, device):
    """UCB and EI, info NULL / 0 / 2 (NaN everywhere, nothing written past the outputs)."""
    FB.check_grad_case(Device(device), case)
    _show()


@pytest.mark.parametrize("shape", FB.VALUE_SHAPES, ids=lambda s: f"n{s[0]}-F{s[1]}-M{s[2]}")
def test_value_only_within_its_bound(shape, device):
    """Beyond the gradient's limits, up to n = 256; kind = 7 is accepted there and changes nothing."""
    FB.check_value_only(Device(device), shape)
    _show()


@FAMILIES
@pytest.mark.parametrize("mode,acqf", FB.CLAMP_MODES, ids=lambda x: FB.ACQ.get(x, x) if isinstance(x, int) else x)
def test_clamped_partial_is_exactly_absent(mode, acqf, kind, device):
    FB.check_clamp(Device(device), mode, acqf, kind)


@FAMILIES
@pytest.mark.parametrize("mode", ["span", "deep"])
def test_ei_tails(mode, kind, device):
    """u_f from -9 to +9 within one call; every u_f <= -40: value and gradient 0 within the absolute term."""
    FB.check_tails(Device(device), mode, kind)
    _show()


@FAMILIES
@pytest.mark.parametrize("what", [np.nan, np.inf, "col", "knq"], ids=["nan", "inf", "nan-column", "nan-knq"])
@pytest.mark.parametrize("shape", [FB.CLAMP_SHAPE, FB.EDGE_SHAPE], ids=["n9", "n65"])
def test_non_finite_query_gives_nan_in_every_gradient_entry(shape, what, kind, device):
    """The rule of (7f): a NaN / infinite coordinate (finite source columns), or a NaN column of Knq and Z (the value is NaN too); the
    other queries within their bounds."""
    for acqf in (UCB, EI):
        FB.check_nonfinite(Device(device), shape, kind, acqf, what)


def test_refusals_write_nothing(device):
    FB.check_refusals(Device(device))


@pytest.mark.parametrize("case", [c for c in FB.GRAD_CASES if c[1] == 1], ids=FB.grad_id)
def test_f1_ucb_agrees_with_finish_and_target_gradient(case, device):
    FB.check_against_finish_and_gradient(Device(device), case)
    _show()


@FAMILIES
def test_chain_within_its_bounds(kind, device):
    """The real pipeline: source passes, weighted sums, assemble, POTRF, the solves for alpha (n, F) and Z, then the fantasy kernel, its
    reference fed the device's own upstream outputs."""
    FB.check_chain(Device(device), kind)
    _show()


@FAMILIES
def test_batched_acquisition_value_within_the_transform_bound(kind, device):
    """scaml_target_acqf_batched_f64 on the synthetic studies of tests/test_studies_acqf_emul.py: value against the transform of ITS OWN
    mu_out / var_out (E_mu = E_v = 0; the formulas of csrc/gp_studies_formulas.h) -- the other place EI's erf runs on the device."""
    be = Device(device)
    prob = SE.Problem(6, kind, seed=11)
    order = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha", "n_points", "m_all", "s_all", "info", "acqf_param")
    dtypes = dict(group=torch.int32, n_points=torch.int32, info=torch.int32, active=torch.uint8)
    for acqf in (UCB, EI):
        a = prob.arrays(acqf)
        Mq, D = a["Xq"].shape
        ins = [be.up(a[k], dtypes.get(k, torch.float64)) for k in order]
        outs = [be.out(Mq), be.out(Mq, D), be.out(Mq), be.out(Mq)]
        _lib.check_rc(be.lib.scaml_target_acqf_batched_f64(*[_p(x) for x in ins], Mq, prob.G, prob.n_max, SE.T, D, kind, acqf, *[_p(x) for x in outs],
                                                           be.stream), "scaml_target_acqf_batched_f64")
        value, _, mu, var = (be.take(x) for x in outs)
        live = np.asarray(a["group"]) >= 0
        assert (value[~live] == 0).all()
        par = np.asarray(a["acqf_param"])[np.asarray(a["group"])[live]]
        q = FB.batched_value_reference(acqf, par, mu[live], var[live])
        assert var[live].min() < 0 < var[live].max(), "the studies hold a query on the clamp and queries off it"
        B.within(f"acqf-batched-{FB.ACQ[acqf]}", ("acqf_batched", B.FAMILY[kind], f"value/{FB.ACQ[acqf]}"), value[live], q)
    _show()
