"""scaml_target_qacqf_f64 (7p), scaml_target_qacqf_pending_f64 (7q) and scaml_target_qacqf_value_f64 (7r) through the C ABI against the
long-double reference of tests/_qacqf_bounds.py, value and gradient held element by element to its a-priori bound (capped at 1e-8 of
the output's scale; the ladder sets at 1e-4), jitter and info exactly, on the planted input sets that module lists: the shape edges
(q in 4 .. 7, S in {2, 3, 5, 257, 509, 511}, D = 1, the launches above 64 KB of dynamic LDS at (88, 8, 512) and the pending corner
n + p + q = 96), both families and codes, every q of the value packing, cond(Sigma) up to 1e4, the clamps, the whole jitter ladder and
info 1, info NULL / 0 / 2, the non-finite inputs, two calls bit for bit, and the real pipeline with the reference fed the device's own
upstream outputs.  Every output buffer holds a sentinel and one guard row more than the call may write; every entry must be
written.  Each test is a single launch shape of at most 17 workgroups.  tests/test_qacqf_bounds.py holds the host builds to the same
bounds and shows that the bounds reject planted errors.  Each test prints the largest error / bound and bound / scale seen so far
(profiles/qacqf_bounds_notes.md records them)."""
import numpy as np
import pytest
import torch

from tests import _qacqf_bounds as QB
from tests import _target_bounds as B
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF, SENTINEL
from tests._qacqf_bounds import EI, UCB
from tests.test_target_bounds_gpu import Device as TargetDevice, _p

pytestmark = pytest.mark.gpu
FAMILIES = pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])
CODES = pytest.mark.parametrize("acqf", [UCB, EI], ids=["qucb", "qei"])
ALL_SHAPES = [("7p", s) for s in QB.SETS_7P] + [("7q", s) for s in QB.SETS_7Q]


class Device(TargetDevice):
    """The backend of tests/_qacqf_bounds.py on the C ABI."""

    def run(self, a, info):
        n, q, p, S, D, Bn = a["n"], a["q"], a["p"], a["S"], a["D"], a["B"]
        t = {k: (None if a.get(k) is None or np.asarray(a[k]).size == 0 else self.up(a[k])) for k in
             ("Knq", "Z", "alpha", "mean_q", "var_q", "cov", "mu_g", "var_g", "Xt", "Xq", "theta", "eps", "Xp", "Zp", "mu_p", "Sigma_pp")}
        Mq = a["Knq"].shape[1]
        inf = None if info is None else torch.tensor([info], dtype=torch.int32, device=self.dev)
        value, jitter = self.out(Bn), self.out(Bn)
        info_out = torch.full((Bn + 1,), QB.ISENTINEL, dtype=torch.int32, device=self.dev)
        grad = None if a["layout"] == "value" else self.out(Bn * q, D)
        head = [_p(t[k]) for k in ("Knq", "Z", "alpha", "mean_q", "var_q")] + [float(a["m"]), float(a["s"]), _p(inf)]
        pend = [_p(t[k]) for k in ("Xp", "Zp", "mu_p", "Sigma_pp")]
        body = [_p(t[k]) for k in ("cov", "mu_g", "var_g", "Xt", "Xq", "theta", "eps")]
        if a["entry"] == "7p":
            rc = self.lib.scaml_target_qacqf_f64(*head, *body, int(a["acqf"]), float(a["param"]), n, Mq, q, S, D, int(a["kind"]), _p(value), _p(grad),
                                                 _p(jitter), _p(info_out), self.stream)
        elif a["entry"] == "7q":
            rc = self.lib.scaml_target_qacqf_pending_f64(*head, *body, *pend, int(a["acqf"]), float(a["param"]), n, Mq, q, p, S, D, int(a["kind"]),
                                                         _p(value), _p(grad), _p(jitter), _p(info_out), self.stream)
        else:
            rc = self.lib.scaml_target_qacqf_value_f64(*head, *[_p(t[k]) for k in ("cov", "Xq", "theta", "eps")], *pend, int(a["acqf"]),
                                                       float(a["param"]), n, Mq, Bn, q, p, S, D, int(a["kind"]), _p(value), _p(jitter), _p(info_out),
                                                       self.stream)
        io = info_out.cpu().numpy()
        assert io[-1] == QB.ISENTINEL, "the call wrote past the end of info_out"
        v, j, g = self.take(value), self.take(jitter), (None if grad is None else self.take(grad))
        if rc == 0:
            assert not (v == SENTINEL).any() and not (j == SENTINEL).any() and not (io[:-1] == QB.ISENTINEL).any() \
                and (g is None or not (g == SENTINEL).any()), "an output entry was not written"
        return rc, v, g, j, io[:-1]


def _show():
    for line in QB.report():
        print(line)


@FAMILIES
@pytest.mark.parametrize("entry,shape", ALL_SHAPES, ids=[f"{e}-{QB.set_id(s)}" for e, s in ALL_SHAPES])
def test_value_and_gradient_within_their_bounds(entry, shape, kind, device):
    """(7p) and (7q), both codes (qEI with best_f in the bulk), info NULL / 0 / 2.  (88, 8, 512) and (88, 3, 5, 512) launch above 64 KB
    of dynamic LDS."""
    QB.check_shape(Device(device), entry, shape, kind)
    _show()


@FAMILIES
@pytest.mark.parametrize("shape", QB.SETS_7R, ids=QB.set_id)
def test_value_layout_within_its_bound_and_bit_equal_to_the_grad_layout(shape, kind, device):
    QB.check_value_layout(Device(device), shape, kind)
    _show()


@FAMILIES
@pytest.mark.parametrize("cond", QB.CONDS, ids=lambda c: f"cond{c:.0e}")
def test_conditioning(cond, kind, device):
    QB.check_cond(Device(device), cond, kind)
    _show()


@FAMILIES
def test_best_f_below_every_sample_gives_exact_zeros(kind, device):
    QB.check_below(Device(device), kind)


@FAMILIES
def test_qucb_with_beta_zero(kind, device):
    QB.check_beta0(Device(device), kind)


@CODES
@FAMILIES
def test_ladder(kind, acqf, device):
    """jitter exactly 0, 1e-8, 1e-7, 1e-6, NaN; info (0, 0, 0, 0, 1); batch 4 NaN; batches 0 .. 3 within their bounds and bit-equal to a
    call without batch 4."""
    QB.check_ladder(Device(device), kind, acqf)
    _show()


@CODES
@pytest.mark.parametrize("what", sorted(QB.NONFINITE))
def test_non_finite_inputs(what, acqf, device):
    QB.check_nonfinite(Device(device), what, KIND_MATERN52 if acqf == EI else KIND_RBF, acqf)


@pytest.mark.parametrize("entry", ["7p", "7q", "7r"])
def test_two_calls_bit_for_bit(entry, device):
    QB.check_twice(Device(device), entry, KIND_RBF, EI)


@pytest.mark.parametrize("p", [0, 3], ids=["7p", "7q"])
def test_chain_within_its_bounds(p, device):
    """The real pipeline (T = 3, ragged N = 32, n = 17: the smallest JointProblem of tests/test_qacqf_gpu.py and
    tests/test_qacqf_pending_gpu.py): the kernel's reference is fed the device's own upstream outputs."""
    from scamlgp_amd import ops
    from tests._qacqf_problem import JointProblem

    q, S = 2, 64
    pr = JointProblem((32, 20, 17), 2, 17, 5, q, 0, 0, 1)
    _, model = pr.model(device)
    eps = torch.randn(S, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(101))
    Xp = torch.rand(p, pr.D, dtype=torch.float64, generator=torch.Generator().manual_seed(501)) if p else None
    kw = model.joint_acqf_inputs(pr.X, eps, X_pending=Xp)
    kw.pop("shape")
    host = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    assert int(host["info"].reshape(-1)[0]) == 0
    for acqf in (UCB, EI):
        par = 4.0 if acqf == UCB else pr.best_f()
        a = QB.chain_set(host, acqf, par, "7q" if p else "7p", f"chain-p{p}-{QB.ACQ[acqf]}")
        out = (ops.target_qacqf_pending if p else ops.target_qacqf)(**kw, acqf=acqf, acqf_param=par)
        got = (0, out["value"].cpu().numpy(), out["grad"].cpu().numpy(), out["jitter"].cpu().numpy(), out["info"].cpu().numpy())
        QB.hold(a["name"], a, QB.reference(a), got, k=lambda name: ("qacqf_chain", f"{a['entry']}/rbf/{QB.ACQ[acqf]}", name))
    for line in B.report("qacqf_chain"):
        print(line)
