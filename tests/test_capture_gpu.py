"""utils.capture_graph on the MI355X: a function of a static buffer captured into a HIP graph after ``warmup`` eager calls; a replay
after new values were copied into the buffer gives exactly what the eager call gives -- for a tuple of outputs and for a single
tensor, with the warm-up counts the package uses (2: bo.GraphedAcquisition, 3: the two graphed objectives of utils)."""
import pytest
import torch

from scamlgp_amd.utils import capture_graph

pytestmark = pytest.mark.gpu


def _pair(x):
    return (x * 2).sum(1), x + 1


def _single(x):
    return (x * 2).sum(1) + 1


@pytest.mark.parametrize("warmup", [2, 3])
@pytest.mark.parametrize("fn", [_pair, _single], ids=["tuple", "tensor"])
def test_replay_equals_the_eager_call(device, fn, warmup):
    x = torch.zeros(4, 3, dtype=torch.float64, device=device)
    calls = [0]

    def body():
        calls[0] += 1
        return fn(x)

    graph, out = capture_graph(body, device, warmup)
    assert calls[0] == warmup + 1                # the warm-up calls and the captured one
    assert isinstance(out, tuple) == (fn is _pair)
    for seed in (1, 2):                          # two replays: the outputs follow the buffer, not the values at capture
        new = torch.rand(4, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(device)
        x.copy_(new)
        graph.replay()
        want = fn(new)
        if fn is _pair:
            assert len(out) == 2 and all(torch.equal(o, w) for o, w in zip(out, want))
        else:
            assert torch.equal(out, want)
