"""ScaMLGPBOLoop(joint_pending=...): the refusals of the Python layer that are decided before the model or the device is touched -- no
GPU needed.  (What needs a model -- q + p beyond the kernel's 8 points, n + p + q beyond the covariance block -- is in
tests/test_qacqf_pending_gpu.py.)"""
import pytest
import torch

from scamlgp_amd.bo import OptimizerNotReady, ScaMLGPBOLoop


def test_joint_pending_values():
    # (refused in front of the model's construction: the empty source dict is never read)
    for bad in ("fantasy", "Joint", "", None):
        with pytest.raises(ValueError, match="joint_pending"):
            ScaMLGPBOLoop({}, 2, joint_pending=bad)


def _loop(pending: int, k, joint_pending: str, acquisition: str = "ucb") -> ScaMLGPBOLoop:
    """A loop with ``pending`` points pending and WITHOUT a model: ``suggest_batch`` decides its refusals from these four attributes
    before it reads anything else, so a loop that gets past them fails on the missing model (AttributeError), not on a device."""
    lp = ScaMLGPBOLoop.__new__(ScaMLGPBOLoop)
    lp.acquisition, lp.max_pending_evaluations, lp.joint_pending = acquisition, k, joint_pending
    lp.pending = torch.rand(pending, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    return lp


def test_the_default_still_refuses_with_points_pending():
    with pytest.raises(NotImplementedError, match="pending"):
        _loop(2, 4, "refuse").suggest_batch(1)
    with pytest.raises(NotImplementedError, match="pending"):
        _loop(4, 4, "refuse").suggest_batch(1)          # (the refusal it always was, also where "joint" would say "not ready")


def test_limits_of_the_joint_mode():
    with pytest.raises(OptimizerNotReady):
        _loop(4, 4, "joint").suggest_batch(1)           # p >= k
    with pytest.raises(OptimizerNotReady):
        _loop(5, 4, "joint").suggest_batch(1)
    with pytest.raises(ValueError, match="max_pending_evaluations=4"):
        _loop(2, 4, "joint").suggest_batch(3)           # q + p > k
    with pytest.raises(ValueError, match="max_pending_evaluations=4"):
        _loop(0, 4, "joint").suggest_batch(5)           # q > k, as without pending points
    with pytest.raises(ValueError, match="max_pending_evaluations=4"):
        _loop(0, 4, "refuse").suggest_batch(5)
    with pytest.raises(ValueError, match="LogEI"):
        _loop(2, 4, "joint", acquisition="logei").suggest_batch(1)
    with pytest.raises(ValueError):
        _loop(2, 4, "joint").suggest_batch(0)
    # inside the limits the refusals are passed: the next thing the call reads is the model this loop does not have
    with pytest.raises(AttributeError, match="model"):
        _loop(2, 4, "joint").suggest_batch(2)
