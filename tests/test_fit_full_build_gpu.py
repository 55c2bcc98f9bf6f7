"""GPU: the kernel-matrix build of the full-tile instance of the fused fit (csrc/gp_fit_fused.hip, FULL: the lane parts of the
operand, image and zero-store addresses worked out once per attempt, the tile's part a wave-uniform offset) against the generic
instance of the same library, which works every address out per tile.  One process, one library: the launcher reads
SCAML_FIT_NO_FULL at every launch (the switch and the buffers: tests/_fit_full_run.py).

The full-tile build does the generic build's floating-point operations in the generic order, so every output is compared with
array_equal, alpha included (its terms meet in LDS atomics, but in an order the kernel fixes).  N = 256 is the only N the
instance exists for: every launch runs all eight waves and all 136 tiles, the six tile images of the panel wave among them.
D covers the edges of D4 = 4 ceil(D / 4), the length of the distance chain (1, 4 | 5, 8 | 20: the last D with the early chain,
21: the first without); flags: no L, L without the upper zeros, L with them."""
import functools

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import ops
from tests import _failpath_cases as C
from tests import _fit_full as F
from tests._fit_full_run import N, cus, filled, switch      # noqa: F401  (switch: the fixture)
from tests.test_fit_gpu import _stack

pytestmark = pytest.mark.gpu

T = 3
KINDS = [pytest.param(O.KIND_RBF, id="rbf"), pytest.param(O.KIND_MATERN52, id="matern")]
OUTPUTS = ("L", "alpha", "quad", "logdet", "mll", "jitter", "info", "Linv_diag")


@functools.lru_cache(maxsize=None)
def _inputs(D):
    """One stack per D, shared by the kinds and flags (never written to)."""
    return _stack(T, N, D, seed=1300 + D)


def _assert_equal(full, gen):
    for k in OUTPUTS:
        if full.get(k) is None:
            assert gen.get(k) is None, k
            continue
        assert np.array_equal(full[k].cpu().numpy(), gen[k].cpu().numpy(), equal_nan=True), k


def _run_both(switch, device, X, y, theta, kind, flags, fill=-3.5, **kw):
    res = {}
    for mode in (0, 1):
        switch(mode)
        res[mode] = ops.gp_fit_fused(X, y, theta, kind, store_L=bool(flags & 1), zero_upper=bool(flags & 2), want_linv=True,
                                     out=filled(X.shape[0], device, bool(flags & 1), True, fill), **kw)
        torch.cuda.synchronize()
        assert F.fit_full_of_call(X.shape[0], N, X.shape[2], cus(device), stores_l=bool(flags & 1), l_addr=0, mode=mode) == (mode == 0)
    return res[0], res[1]


@pytest.mark.parametrize("flags", [0, 1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [1, 4, 5, 8, 20, 21])
def test_full_build_equals_generic_build(D, kind, flags, device, switch):
    X, y, theta = (a.to(device) for a in _inputs(D))
    full, gen = _run_both(switch, device, X, y, theta, kind, flags)
    assert not full["info"].cpu().any() and float(full["jitter"].abs().max()) == 0.0
    _assert_equal(full, gen)
    if flags == 1:      # zero_upper off: nothing above the diagonal is written
        up = torch.triu(torch.ones(N, N, dtype=torch.bool, device=device), diagonal=1)
        assert bool((full["L"][:, up] == -3.5).all())
    if flags == 3:
        assert float(torch.triu(full["L"], diagonal=1).abs().max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_jitter_retry_rebuilds_the_same_matrix(kind, device, switch):
    """Task 1 has two coincident points and a slightly negative noise (tools/dev_failpath_check.py builds its rescued tasks so):
    the first attempt fails, the out-of-line retry copy builds the matrix again with the 1e-8 jitter and succeeds."""
    D = 8
    g = torch.Generator().manual_seed(77 + kind)
    X = torch.rand(T, N, D, dtype=torch.float64, generator=g)
    y = torch.randn(T, N, dtype=torch.float64, generator=g)
    theta = torch.cat([torch.full((T, D), 0.5, dtype=torch.float64), torch.ones(T, 1, dtype=torch.float64),
                       torch.full((T, 1), 1e-3, dtype=torch.float64)], 1)
    X[1, 200] = X[1, 17]
    theta[1, D + 1] = -2e-9
    full, gen = _run_both(switch, device, X.to(device), y.to(device), theta.to(device), kind, 3)
    assert full["info"].cpu().tolist() == [0, 0, 0]
    assert full["jitter"].cpu().tolist() == [0.0, C.RUNGS[0], 0.0] and C.RUNGS[0] == 1e-8
    _assert_equal(full, gen)
    assert float(torch.triu(full["L"], diagonal=1).abs().max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_upper_triangle_is_zero_over_a_nan_prefill(kind, device, switch):
    """flags 3 into an L full of NaN: every element is written -- the strict upper triangle exactly zero (the mirror tiles
    by the wave that builds the lower one, the diagonal tiles' upper halves with the diagonal block), nothing left NaN."""
    X, y, theta = (a.to(device) for a in _inputs(8))
    full, gen = _run_both(switch, device, X, y, theta, kind, 3, fill=float("nan"))
    assert not full["info"].cpu().any()
    L = full["L"]
    assert not bool(torch.isnan(L).any())
    up = torch.triu(torch.ones(N, N, dtype=torch.bool, device=device), diagonal=1)
    assert bool((L[:, up] == 0.0).all())
    assert bool((torch.diagonal(L, dim1=1, dim2=2) > 0).all())
    _assert_equal(full, gen)
