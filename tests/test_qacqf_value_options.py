"""The opt-in switches of the value-only scoring route -- ``score_mode`` of utils.qExpectedImprovement / qUpperConfidenceBound and
``joint_score_mode`` of ScaMLGPBOLoop -- as far as they are decided before a model or the device is touched: no GPU needed."""
import inspect
from types import SimpleNamespace

import pytest

from scamlgp_amd import utils
from scamlgp_amd.bo import ScaMLGPBOLoop

CLASSES = (utils.qExpectedImprovement, utils.qUpperConfidenceBound)


def test_the_defaults_are_the_gradient_route():
    assert inspect.signature(ScaMLGPBOLoop.__init__).parameters["joint_score_mode"].default == "grad_pass"
    for cls in CLASSES + (utils._JointAcquisition,):
        assert inspect.signature(cls.__init__).parameters["score_mode"].default == "grad_pass"
    assert utils._JointAcquisition.SCORE_MODES == ("grad_pass", "value_pass")
    assert utils._JointAcquisition.SCORE_COV_CAP_BYTES == utils.StudiesAcquisition.SCORE_COV_CAP_BYTES == 256 << 20


def test_the_loop_refuses_other_modes_at_construction():
    # (refused in front of the model's construction: the empty source dict is never read)
    for bad in ("value", "Value_pass", "batched", "", None):
        with pytest.raises(ValueError, match="joint_score_mode"):
            ScaMLGPBOLoop({}, 2, joint_score_mode=bad)
    with pytest.raises(ValueError, match="joint_pending"):
        ScaMLGPBOLoop({}, 2, joint_score_mode="value_pass", joint_pending="fantasy")


def test_the_classes_refuse_other_modes_at_construction():
    # (in front of everything else: the model is never read)
    for cls, par in zip(CLASSES, (0.0, 4.0)):
        for bad in ("value", "grad", "", None):
            with pytest.raises(ValueError, match="score_mode"):
                cls(None, par, score_mode=bad)
    # a fantasy model is refused in both modes
    fantasy = SimpleNamespace(num_fantasies=4)
    for mode in utils._JointAcquisition.SCORE_MODES:
        with pytest.raises(NotImplementedError):
            utils.qExpectedImprovement(fantasy, 0.0, score_mode=mode)


def _af(q, p, n, T, cap=None):
    af = utils.qExpectedImprovement.__new__(utils.qExpectedImprovement)
    af.q, af.p, af.model = q, p, SimpleNamespace(n=n, _stack=SimpleNamespace(T=T))
    if cap is not None:
        af.SCORE_COV_CAP_BYTES = cap
    return af


def test_chunks_are_whole_strips_within_the_cap():
    # configs[4]: T = 32, n = 80, 1024 batches of 4 are 256 strips, 32 * 84 * 4096 * 8 bytes = 88 MB: one chunk
    step = _af(4, 0, 80, 32)._value_pass_step()
    assert step % 4 == 0 and step >= 1024
    assert 8 * 32 * 84 * 16 * (step // 4) <= 256 << 20 < 8 * 32 * 84 * 16 * (step // 4 + 1)
    # whole strips: a multiple of 16 // q batches, whatever q and the cap; one strip at the least
    for q in range(1, 9):
        for cap in (1, 10 ** 6, 256 << 20):
            s = _af(q, 8 - q, 17, 3, cap)._value_pass_step()
            assert s >= 16 // q and s % (16 // q) == 0, (q, cap)
        assert _af(q, 0, 17, 3, 1)._value_pass_step() == 16 // q
