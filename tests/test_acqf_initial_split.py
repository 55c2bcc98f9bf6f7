"""``bo.acqf_initial_conditions`` split into its draw (``acqf_draw_candidates``) and its pick (``acqf_pick_initial_conditions``) is the
function it was: against a copy of the unsplit function kept here, the candidates, the values, the picks and the generator's end state
are equal -- for R = 1, R > raw_samples, a constant ``vals`` and an ordinary case.  No GPU."""
import pytest
import torch

from scamlgp_amd import bo


def _original(af, dim, raw_samples, num_restarts, generator, eta=2.0):
    """The function as it stood before the split, word for word (plus the picks among its results)."""
    cand = torch.rand(raw_samples, dim, dtype=torch.float64, generator=generator)
    vals = af(cand).detach().cpu()
    R = min(num_restarts, raw_samples)
    best0 = int(vals.argmax())
    picks = [best0]
    if R > 1:
        z = (vals - vals.mean()) / vals.std().clamp_min(1e-12)
        pr = torch.exp(eta * (z - z.max()))
        pr[best0] = 0.0
        if float(pr.sum()) > 0:
            k = min(R - 1, int((pr > 0).sum()))
            picks += torch.multinomial(pr, k, replacement=False, generator=generator).tolist()
    return cand, vals, best0, cand[picks], picks


def _smooth(x):
    return torch.sin(3.0 * x.sum(-1)) + (x ** 2).sum(-1)


def _constant(x):
    return torch.full((x.shape[0],), 1.25, dtype=torch.float64)


@pytest.mark.parametrize("af, raw_samples, num_restarts", [(_smooth, 64, 4), (_smooth, 64, 1), (_smooth, 5, 9), (_constant, 32, 4),
                                                           (_smooth, 1, 3)])
def test_split_equals_the_original(af, raw_samples, num_restarts):
    dim, seed = 3, 17
    g0, g1, g2 = (torch.Generator().manual_seed(seed) for _ in range(3))
    cand0, vals0, best0, x0, picks0 = _original(af, dim, raw_samples, num_restarts, g0)
    # the whole function, as optimize_acqf calls it
    cand1, vals1, best1, x1 = bo.acqf_initial_conditions(af, dim, raw_samples, num_restarts, g1)
    assert torch.equal(cand1, cand0) and torch.equal(vals1, vals0) and best1 == best0 and torch.equal(x1, x0)
    assert torch.equal(g1.get_state(), g0.get_state())
    # the two halves with the scoring in between, as ScaMLGPBOStudies calls them
    cand2 = bo.acqf_draw_candidates(dim, raw_samples, g2)
    vals2 = af(cand2).detach().cpu()
    best2, picks2 = bo.acqf_pick_initial_conditions(vals2, num_restarts, g2)
    assert torch.equal(cand2, cand0) and best2 == best0 and picks2 == picks0 and torch.equal(cand2[picks2], x0)
    assert torch.equal(g2.get_state(), g0.get_state())
    assert len(picks0) <= min(num_restarts, raw_samples) and picks0[0] == best0


def test_score_mode_is_an_explicit_constructor_parameter():
    """Checked before any study is built: no source stack, no GPU."""
    with pytest.raises(ValueError, match="score_mode"):
        bo.ScaMLGPBOStudies({}, 2, 1, suggest_mode="sequential", score_mode="batched")
    with pytest.raises(ValueError, match="score_mode"):
        bo.ScaMLGPBOStudies({}, 2, 1, suggest_mode="device", score_mode="everything")
