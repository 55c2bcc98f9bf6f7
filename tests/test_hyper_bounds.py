"""``hyper.batched_lbfgs(bounds=(lo, hi))``: the box-constrained batched L-BFGS the lock-step acquisition optimiser runs, on analytic
functions (no GPU).  B independent problems, each with its own history, step and stopping flag."""
import numpy as np
import scipy.optimize
import torch

from scamlgp_amd import hyper as H
from scamlgp_amd import synthetic as S

torch.set_num_threads(1)
F64 = torch.float64
H6_SEED = 3   # the 16 starts of the Hartmann-6 tests: torch.Generator().manual_seed(H6_SEED)


def neg_hartmann6(x: torch.Tensor):
    """-synthetic.hartmann6 (>= 0: minimising it drives the iterates towards the faces and corners of the unit cube) and its analytic
    gradient, row by row."""
    A, P = torch.from_numpy(S.HARTMANN6_A), torch.from_numpy(S.HARTMANN6_P)
    al = torch.as_tensor(np.asarray(S.HARTMANN_ALPHA_DEFAULT, dtype=np.float64))
    diff = x.unsqueeze(1) - P.unsqueeze(0)                       # (B, 4, 6)
    e = al * torch.exp(-(A * diff * diff).sum(-1))               # (B, 4)
    return e.sum(-1), (-2.0 * e.unsqueeze(-1) * A * diff).sum(1)


def h6_starts():
    return torch.rand(16, 6, dtype=F64, generator=torch.Generator().manual_seed(H6_SEED))


def test_the_restated_hartmann6_is_the_package_s():
    """A self-check of this file's helper (it holds without ``bounds=``): the objective the tests below minimise is the package's."""
    x = h6_starts()
    f, g = neg_hartmann6(x)
    np.testing.assert_allclose(f.numpy(), -S.hartmann6(x.numpy()), rtol=1e-13)
    xr = x.clone().requires_grad_(True)
    (ga,) = torch.autograd.grad(neg_hartmann6(xr)[0].sum(), xr)
    np.testing.assert_allclose(g.numpy(), ga.numpy(), rtol=1e-12, atol=1e-15)


def test_separable_quadratic_ends_at_the_clipped_optimum():
    # optima inside the box, on faces and at corners (per problem: coordinates of c below 0, inside, above 1)
    gen = torch.Generator().manual_seed(0)
    c = torch.rand(16, 6, dtype=F64, generator=gen) * 2.0 - 0.5
    c[0] = torch.tensor([0.2, 0.4, 0.5, 0.6, 0.7, 0.9], dtype=F64)           # interior
    c[1] = torch.tensor([-0.3, 1.4, -1.0, 2.0, 1.1, -0.1], dtype=F64)         # a corner
    c[2] = torch.tensor([0.5, 0.5, 1.5, 0.5, 0.5, 0.5], dtype=F64)            # a face
    a = 0.5 + 3.0 * torch.rand(16, 6, dtype=F64, generator=gen)

    def fun(x):
        return (a * (x - c) ** 2).sum(-1), 2.0 * a * (x - c)

    x0 = torch.rand(16, 6, dtype=F64, generator=gen)
    res = H.batched_lbfgs(fun, x0, max_iter=200, gtol=1e-10, ftol=0.0, bounds=(0.0, 1.0))
    assert not res.failed.any()   # (the flag `converged` needs max |P(x - g) - x| <= 1e-10 here, below what f ~ 1 resolves: not asked)
    torch.testing.assert_close(res.x, c.clamp(0.0, 1.0), rtol=0, atol=1e-8)
    # (P,) bounds and a start outside the box
    lo, hi = torch.full((6,), 0.25, dtype=F64), torch.tensor([0.75, 0.75, 0.75, 2.0, 2.0, 2.0], dtype=F64)
    res2 = H.batched_lbfgs(fun, x0 * 3.0 - 1.0, max_iter=200, gtol=1e-10, ftol=0.0, bounds=(lo, hi))
    torch.testing.assert_close(res2.x, torch.minimum(torch.maximum(c, lo), hi), rtol=0, atol=1e-8)


def _trace(x0, **kw):
    seen, path = [], []

    def fun(x):
        seen.append(x.clone())
        return neg_hartmann6(x)

    res = H.batched_lbfgs(fun, x0, bounds=(0.0, 1.0), callback=lambda it, x, f, done: path.append((it, x.clone(), f.clone(), done.clone())), **kw)
    return res, seen, path


def test_hartmann6_iterates_stay_in_the_box_and_descend():
    res, seen, path = _trace(h6_starts(), max_iter=100)
    for x in seen:                                  # every point the objective was asked for
        assert bool(((x >= 0.0) & (x <= 1.0)).all())
    for (_, _, f0, _), (_, _, f1, _) in zip(path, path[1:]):
        assert bool((f1 <= f0).all())               # f never increases between accepted steps
    assert bool(res.converged.any())
    _, g = neg_hartmann6(res.x)
    pg = H.projected_gradient(res.x, g, torch.zeros(6, dtype=F64), torch.ones(6, dtype=F64)).abs().amax(-1)
    assert bool((pg[res.converged] <= 1e-5).all())  # the projected-gradient rule, gtol = 1e-5 (the default)
    assert bool(((res.x >= 0.0) & (res.x <= 1.0)).all())


def test_best_of_starts_against_scipy_lbfgsb():
    x0 = h6_starts()
    res = H.batched_lbfgs(lambda x: neg_hartmann6(x), x0, max_iter=200, bounds=(0.0, 1.0))

    def f1(v):
        f, g = neg_hartmann6(torch.from_numpy(v).unsqueeze(0))
        return float(f[0]), g[0].numpy()

    sp = [scipy.optimize.minimize(f1, x.numpy(), jac=True, method="L-BFGS-B", bounds=[(0.0, 1.0)] * 6, options=dict(maxiter=200)).fun for x in x0]
    ours, theirs = float(res.f.min()), float(min(sp))
    print(f"best of 16 starts (seed {H6_SEED}): batched_lbfgs {ours:.12e}, scipy L-BFGS-B {theirs:.12e}")
    assert ours <= theirs + 1e-6


def test_a_start_s_trajectory_does_not_depend_on_its_companions():
    x0 = h6_starts()
    _, _, together = _trace(x0, max_iter=60)
    for b in (0, 7, 15):
        _, _, alone = _trace(x0[b:b + 1], max_iter=60)
        assert len(alone) <= len(together)
        for (it, x, f, _), (it2, x2, f2, _) in zip(alone, together):
            assert it == it2 and torch.equal(x[0], x2[b]) and torch.equal(f[0], f2[b]), (b, it)
        for _, x2, f2, _ in together[len(alone):]:   # stopped alone: it stays where it stopped in company
            assert torch.equal(alone[-1][1][0], x2[b]) and torch.equal(alone[-1][2][0], f2[b])


def test_bounds_none_is_the_function_as_it_was():
    # the Rosenbrock family of tests/test_hyper.py: the unconstrained path must give the same bits with the new arguments left alone
    B, P = 7, 4
    scale = torch.linspace(1.0, 20.0, B, dtype=F64)

    def fun(x):
        x = x.clone().requires_grad_(True)
        f = (scale.unsqueeze(-1) * (x[:, 1:] - x[:, :-1] ** 2) ** 2 + (1 - x[:, :-1]) ** 2).sum(-1)
        (g,) = torch.autograd.grad(f.sum(), x)
        return f.detach(), g

    x0 = torch.zeros(B, P, dtype=F64)
    a = H.batched_lbfgs(fun, x0, max_iter=500, gtol=1e-8, ftol=0.0)
    b = H.batched_lbfgs(fun, x0, max_iter=500, gtol=1e-8, ftol=0.0, bounds=None)
    assert torch.equal(a.x, b.x) and torch.equal(a.f, b.f) and a.n_iter == b.n_iter and a.n_eval == b.n_eval
    assert bool(a.converged.all())
    torch.testing.assert_close(a.x, torch.ones(B, P, dtype=F64), rtol=0, atol=1e-5)
    # and a box that never binds leads to the same optimum
    c = H.batched_lbfgs(fun, x0, max_iter=500, gtol=1e-8, ftol=0.0, bounds=(-10.0, 10.0))
    torch.testing.assert_close(c.x, torch.ones(B, P, dtype=F64), rtol=0, atol=1e-5)
