"""Host logic of ``ScaMLGPBOStudies(..., fantasy_setup=...)``: the keyword's values, what it may be combined with, and the default.  The
checks answer before any study is built, so no source stack (and no GPU) is needed."""
import inspect

import pytest

from scamlgp_amd import bo, model


def _studies(**kw):
    return bo.ScaMLGPBOStudies({}, 2, 2, **kw)


def test_the_default_is_per_study():
    sig = inspect.signature(bo.ScaMLGPBOStudies.__init__)
    assert sig.parameters["fantasy_setup"].default == "per_study"
    assert sig.parameters["pending_mode"].default == "per_study" and sig.parameters["score_mode"].default == "per_study"
    assert sig.parameters["suggest_mode"].default == "sequential"


def test_an_unknown_value_is_refused():
    with pytest.raises(ValueError, match="fantasy_setup must be 'per_study' or 'batched'"):
        _studies(suggest_mode="device", pending_mode="batched", fantasy_setup="grouped")


@pytest.mark.parametrize("kw", [dict(), dict(suggest_mode="lockstep"), dict(suggest_mode="device"), dict(suggest_mode="device", score_mode="batched"),
                                dict(suggest_mode="device", pending_mode="per_study")])
def test_batched_needs_the_batched_pending_mode(kw):
    with pytest.raises(ValueError, match="fantasy_setup='batched' needs pending_mode='batched'"):
        _studies(fantasy_setup="batched", **kw)


def test_the_other_opt_ins_answer_first():
    with pytest.raises(ValueError, match="pending_mode='batched' needs suggest_mode"):
        _studies(pending_mode="batched", fantasy_setup="batched")


def test_fantasize_studies_checks_its_lists_before_any_launch():
    assert model.fantasize_studies([], [], 4, []) == []
    with pytest.raises(ValueError, match="pending sets"):
        model.fantasize_studies([object()], [], 4, [None])
    with pytest.raises(NotImplementedError, match="observation noise"):
        model.fantasize_studies([object()], [None], 4, [None], observation_noise=False)
