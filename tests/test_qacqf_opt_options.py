"""``joint_opt_mode`` of the joint route of ``bo.optimize_acqf`` / ``ScaMLGPBOLoop.suggest_batch`` without a device: defaults, refused
strings, and the stages of ``"device"`` mode on a stub acquisition object whose ``optimize`` is the host twin of the device
optimiser (``hyper.batched_lbfgs`` with bounds on its ``value_and_grad``)."""
import inspect

import pytest
import torch

from scamlgp_amd import bo, hyper

F64 = torch.float64


class StubJoint:
    """-(sum over the batch of |x - c|^2) + bump: a joint 'acquisition' on the CPU that counts its calls."""

    def __init__(self, q, dim, with_optimize=True, scale=1.0):
        gen = torch.Generator().manual_seed(5)
        self.c = torch.rand(q, dim, dtype=F64, generator=gen) * 1.4 - 0.2      # partly outside the box
        self.calls, self.optimized, self.scale = 0, 0, scale
        if with_optimize:
            self.optimize = self._optimize

    def __call__(self, X):
        self.calls += 1
        return -self.scale * ((torch.as_tensor(X, dtype=F64) - self.c) ** 2).sum((-1, -2))

    def value_and_grad(self, X):
        X = torch.as_tensor(X, dtype=F64)
        return -self.scale * ((X - self.c) ** 2).sum((-1, -2)), -2.0 * self.scale * (X - self.c)

    def _optimize(self, x0, max_iter, evals_per_call=None, **options):
        self.optimized += 1
        R, q, dim = x0.shape

        def fun(z):
            v, g = self.value_and_grad(z.reshape(R, q, dim))
            return -v, -g.reshape(R, q * dim)

        res = hyper.batched_lbfgs(fun, x0.reshape(R, q * dim).clone(), max_iter=max_iter, bounds=(0.0, 1.0), **options)
        stats = torch.stack([torch.full((R,), res.n_iter), torch.full((R,), res.n_eval), torch.where(res.converged, 1, 5), torch.zeros(R, dtype=torch.long)], 1)
        return dict(x=res.x.reshape(R, q, dim), f=-res.f, stats=stats.to(torch.int32), n_eval=res.n_eval, n_calls=1)


def test_defaults_and_refused_strings():
    assert bo.JOINT_OPT_MODES == ("scipy", "device")
    assert inspect.signature(bo.optimize_acqf).parameters["joint_opt_mode"].default == "scipy"
    assert inspect.signature(bo._optimize_acqf_joint).parameters["joint_opt_mode"].default == "scipy"
    assert inspect.signature(bo.acqf_local_optimization).parameters["joint_opt_mode"].default == "scipy"
    assert inspect.signature(bo.ScaMLGPBOLoop.__init__).parameters["joint_opt_mode"].default == "scipy"
    af = StubJoint(2, 3)
    for bad in ("Device", "gpu", "", "host"):
        with pytest.raises(ValueError, match="joint_opt_mode"):
            bo.optimize_acqf(af, 3, 16, 2, q=2, joint_opt_mode=bad)
        with pytest.raises(ValueError, match="joint_opt_mode"):
            bo.acqf_local_optimization(af, torch.rand(2, 2, 3, dtype=F64), joint_opt_mode=bad)
        with pytest.raises(ValueError, match="joint_opt_mode"):
            bo.ScaMLGPBOLoop({}, 3, joint_opt_mode=bad)
    assert af.calls == 0


def test_the_loop_refuses_the_string_before_it_builds_anything():
    # (source_gps is never read: the constructor checks its mode strings first)
    with pytest.raises(ValueError, match="'scipy' or 'device'"):
        bo.ScaMLGPBOLoop(None, 2, joint_opt_mode="cuda")


def test_device_mode_scores_once_and_takes_f_for_the_end_batches():
    q, dim = 3, 2
    twins = {}
    for mode in bo.JOINT_OPT_MODES:
        af, gen = StubJoint(q, dim), torch.Generator().manual_seed(11)
        info = {}
        X, v = bo._optimize_acqf_joint(af, dim, q, 64, 4, 50, gen, 2.0, mode, info)
        twins[mode] = (af, gen, X, float(v), info)
    dev, sci = twins["device"], twins["scipy"]
    assert dev[0].calls == 1 and dev[0].optimized == 1          # stage 1 only; f stands for stage 3
    assert sci[0].calls == 2 and sci[0].optimized == 0
    assert torch.equal(dev[1].get_state(), sci[1].get_state())  # stage 2 draws nothing
    # both reach the clipped optimum of the concave stub
    want = dev[0].c.clamp(0.0, 1.0)
    torch.testing.assert_close(dev[2], want, rtol=0, atol=1e-5)
    assert abs(dev[3] - float(dev[0](want))) < 1e-9 and abs(dev[3] - sci[3]) < 1e-6
    assert set(dev[4]) == {"n_eval", "n_calls", "evals_per_start", "status"} and len(dev[4]["status"]) == 4 and sci[4] == {}
    # through the public entry too
    af, gen = StubJoint(q, dim), torch.Generator().manual_seed(11)
    X2, v2 = bo.optimize_acqf(af, dim, 64, 4, 50, gen, q=q, joint_opt_mode="device")
    assert torch.equal(X2, dev[2]) and float(v2) == dev[3] and af.calls == 1


def test_the_best_raw_batch_wins_when_it_beats_every_end_batch():
    q, dim = 2, 2

    class Worse(StubJoint):
        def _optimize(self, x0, max_iter, evals_per_call=None, **options):
            out = super()._optimize(x0, max_iter, evals_per_call, **options)
            out["f"] = out["f"] - 100.0          # every end batch reports a value below the raw candidates'
            return out

    af, gen = Worse(q, dim), torch.Generator().manual_seed(3)
    X, v = bo._optimize_acqf_joint(af, dim, q, 32, 3, 20, gen, 2.0, "device")
    cand = torch.rand(32, q, dim, dtype=F64, generator=torch.Generator().manual_seed(3))
    vals = StubJoint(q, dim)(cand)
    assert torch.equal(X, cand[int(vals.argmax())]) and float(v) == float(vals.max())
    # a start that failed (-inf, or NaN) never wins
    class Failed(StubJoint):
        def _optimize(self, x0, max_iter, evals_per_call=None, **options):
            out = super()._optimize(x0, max_iter, evals_per_call, **options)
            out["f"] = torch.full_like(out["f"], float("nan"))
            return out

    X, v = bo._optimize_acqf_joint(Failed(q, dim), dim, q, 32, 3, 20, torch.Generator().manual_seed(3), 2.0, "device")
    assert torch.equal(X, cand[int(vals.argmax())])


def test_an_acquisition_object_without_optimize_is_refused_by_name_of_the_mode():
    af = StubJoint(2, 2, with_optimize=False)
    with pytest.raises(TypeError, match="joint_opt_mode='device'"):
        bo._optimize_acqf_joint(af, 2, 2, 16, 2, 10, torch.Generator().manual_seed(0), 2.0, "device")
    with pytest.raises(TypeError, match="joint_opt_mode='device'"):
        bo.acqf_local_optimization(af, torch.rand(2, 2, 2, dtype=F64), joint_opt_mode="device")
    # the default mode does not ask for it
    X, _ = bo._optimize_acqf_joint(af, 2, 2, 16, 2, 10, torch.Generator().manual_seed(0), 2.0)
    assert X.shape == (2, 2)
