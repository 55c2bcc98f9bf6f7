"""model._StateCache on plain CPU tensors: a value is kept per name for exactly as long as the tensors it was computed from are the
same objects and have not been modified in place -- what ``ScaMLGP.theta``, the pruned weights, the training prior and the cached
factor of Knn rely on between a refit and the next."""
import torch

from scamlgp_amd.model import _StateCache


def _key():
    return (torch.arange(3, dtype=torch.float64), torch.ones(2, dtype=torch.float64))


def test_miss_before_any_put():
    assert _StateCache().get("theta", _key()) is None


def test_hit_returns_the_stored_object():
    c, key, value = _StateCache(), _key(), object()
    assert c.put("theta", key, value) is value
    assert c.get("theta", key) is value
    assert c.get("theta", tuple(key)) is value   # (the tensors are the key, not the tuple that lists them)


def test_in_place_modification_of_any_key_tensor_is_a_miss():
    for i in range(2):
        c, key = _StateCache(), _key()
        c.put("theta", key, "v")
        before = key[i]._version
        key[i].add_(0)
        assert key[i]._version > before
        assert c.get("theta", key) is None


def test_replacement_by_an_equal_tensor_is_a_miss():
    c, key = _StateCache(), _key()
    c.put("theta", key, "v")
    twin = (key[0], key[1].clone())
    assert torch.equal(twin[1], key[1])
    assert c.get("theta", twin) is None
    assert c.get("theta", key[:1]) is None       # (fewer tensors than the value was computed from)
    assert c.get("theta", key) == "v"


def test_names_are_independent():
    c, key, w = _StateCache(), _key(), (torch.ones(4, dtype=torch.float64),)
    c.put("theta", key, "t")
    assert c.get("factor", key) is None
    c.put("factor", w + key, "f")
    assert c.get("theta", key) == "t" and c.get("factor", w + key) == "f"
    w[0].mul_(1.0)                               # the weights change: the factor goes, theta (not computed from them) stays
    assert c.get("factor", w + key) is None and c.get("theta", key) == "t"
