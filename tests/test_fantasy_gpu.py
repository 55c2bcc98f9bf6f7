"""Pending evaluations on the MI355X: ScaMLGP.condition_on_observations / fantasize against the oracle's target posterior on the
augmented training set, the fantasy acquisition kernel (scaml_target_fantasy_acqf_f64) against a torch composition of its inputs and
against autograd through the oracle path, HIP-graph replay, seeded reproducibility, and the BO loop with max_pending_evaluations."""
import math

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import model as M, ops, synthetic, utils
from scamlgp_amd.bo import GraphedAcquisition, OptimizerNotReady, ScaMLGPBOLoop

pytestmark = pytest.mark.gpu


def _close(got, ref, rtol):
    torch.testing.assert_close(got, ref, rtol=rtol, atol=rtol * float(ref.abs().max()) + 1e-300)


def _stack(device, kind, T, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(T, N, D, dtype=torch.float64, generator=g)
    Y = torch.sin(3.0 * X.sum(-1) + torch.arange(T, dtype=torch.float64).unsqueeze(-1)) + 0.1 * torch.randn(T, N, dtype=torch.float64, generator=g)
    stack = M.SourceGPStack([f"s{t}" for t in range(T)], list(X), [y.unsqueeze(-1) for y in Y], kind=kind, device=device)
    stack.set_theta(torch.cat([0.4 + 0.6 * torch.rand(T, D, dtype=torch.float64, generator=g), 0.5 + torch.rand(T, 1, dtype=torch.float64, generator=g),
                               1e-3 + 5e-3 * torch.rand(T, 1, dtype=torch.float64, generator=g)], 1))
    stack.refresh()
    return stack, {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}, g


def _parent(device, kind, T, N, D, n, seed=0):
    stack, gps, g = _stack(device, kind, T, N, D, seed)
    Xt = torch.rand(n, D, dtype=torch.float64, generator=g)
    yt = (torch.sin(3.0 * Xt.sum(-1)) + 0.3 * Xt[:, 0]).unsqueeze(-1)
    model = M.ScaMLGP(Xt, yt, gps).eval()
    model.weights = 0.05 + 0.3 * torch.rand(T, dtype=torch.float64, generator=g)
    return stack, model, g


# (the c5r-sized Matern stack of tests/test_fit_gpu.py, and a small RBF one)
STACKS = [(O.KIND_MATERN52, 8, 128, 6), (O.KIND_RBF, 4, 64, 3)]


def _oracle_posterior(stack, model, xq, Xt, yt, m_all, s_all):
    """O.target_posterior on the training set (Xt, yt) with the given transform, over the significant tasks of ``model``."""
    fits = [O.gp_fit(stack.X[t].cpu(), stack.y[t].cpu(), stack.theta[t].cpu(), stack.kind) for t in range(stack.T)]
    w = model.weights.cpu()
    mask = O.significant_weights_mask(w, stack.y_std.cpu(), 1e-3)
    xall = torch.cat([Xt, xq])
    mus, covs = [], []
    for t in range(stack.T):
        if bool(mask[t]):
            mu, cov = O.source_posterior(xall, stack.X[t].cpu(), stack.theta[t].cpu(), stack.kind, fits[t]["L"], fits[t]["alpha"],
                                         float(stack.y_mean[t]), float(stack.y_std[t]))
            mus.append(mu)
            covs.append(cov)
    mu_j, cov_j = O.target_prior(torch.stack(mus), torch.stack(covs), w[mask])
    mu, S = O.target_posterior(xq, Xt, yt, mu_j, cov_j, model.theta.cpu(), model.kind, m_all, s_all)
    return mu, S.diagonal()


@pytest.mark.parametrize("kind,T,N,D", STACKS)
def test_conditioning_matches_the_oracle_on_the_augmented_set(device, kind, T, N, D):
    stack, parent, g = _parent(device, kind, T, N, D, n=12)
    Xp = torch.rand(3, D, dtype=torch.float64, generator=g)
    Yp = torch.randn(3, 1, dtype=torch.float64, generator=g)
    child = parent.condition_on_observations(Xp, Yp)
    assert child.n == 15 and child.num_fantasies is None and child.batch_shape == torch.Size()
    # fixed transform, same parameters (copies), same weights, same stack
    assert float(child.m_all) == float(parent.m_all) and float(child.s_all) == float(parent.s_all)
    assert torch.equal(child.raw_theta, parent.raw_theta) and torch.equal(child.weights, parent.weights)
    assert child.likelihood is not parent.likelihood and child.covar_module is not parent.covar_module
    assert child._stack is parent._stack
    Xq = torch.rand(20, D, dtype=torch.float64, generator=g)
    post = child.posterior(Xq)
    mu_ref, var_ref = _oracle_posterior(stack, parent, Xq, torch.cat([parent.train_X.cpu(), Xp]), torch.cat([parent.train_Y.cpu(), Yp]).squeeze(-1),
                                        float(parent.m_all), float(parent.s_all))
    _close(post.mvn.mean.cpu(), mu_ref, 1e-4)
    _close(post.mvn.variance.cpu(), var_ref, 1e-4)
    # a copy, not a shared module: changing the child's parameters leaves the parent alone
    before = parent.raw_theta.clone()
    child.covar_module.base_kernel.raw_lengthscale.add_(0.1)
    child.likelihood.raw_noise.add_(0.1)
    assert torch.equal(parent.raw_theta, before)


@pytest.mark.parametrize("kind,T,N,D", STACKS)
def test_fantasy_batch(device, kind, T, N, D):
    stack, parent, g = _parent(device, kind, T, N, D, n=12, seed=1)
    F, Mq = 5, 17
    Xp = torch.rand(3, D, dtype=torch.float64, generator=g)
    Yf = torch.randn(F, 3, 1, dtype=torch.float64, generator=g)
    Xq = torch.rand(Mq, D, dtype=torch.float64, generator=g)
    fm = parent.condition_on_observations(Xp, Yf)
    assert fm.num_fantasies == F and fm.batch_shape == torch.Size([F]) and fm.n == 15
    post = fm.posterior(Xq)
    assert post.mean.shape == (F, Mq, 1) and post.variance.shape == (F, Mq, 1)
    var = post.variance.cpu()
    assert torch.equal(var, var[:1].expand_as(var))
    for f in range(F):
        single = parent.condition_on_observations(Xp, Yf[f]).posterior(Xq)
        _close(post.mean[f, :, 0].cpu(), single.mvn.mean.cpu(), 1e-10)
        _close(var[f, :, 0], single.mvn.variance.cpu(), 1e-10)
    # the joint covariance does not depend on the targets either
    assert post.mvn.covariance_matrix.shape == (F, Mq, Mq)
    # no refit of a fantasy model
    with pytest.raises(NotImplementedError):
        fm.mll()
    with pytest.raises(NotImplementedError):
        utils.optimize_marginal_likelihood(fm)
    # conditioning on the parent's own posterior mean leaves the mean alone and shrinks no variance
    pp = parent.posterior(Xq)
    same = parent.condition_on_observations(Xp, parent.posterior(Xp).mean).posterior(Xq)
    _close(same.mvn.mean.cpu(), pp.mvn.mean.cpu(), 1e-8)
    assert bool((same.mvn.variance <= pp.mvn.variance * (1 + 1e-9) + 1e-12).all())


def _torch_fantasy_acqf(Knq, Z, alpha, mean_q, var_q, m, s, acqf, param, gi=None, kind=O.KIND_RBF):
    """The kernel's formulas as a torch composition (CPU, fp64)."""
    mu = m + s * (mean_q.unsqueeze(1) + Knq.transpose(0, 1) @ alpha)             # (M, F)
    v = (s * s * (var_q - (Knq * Z).sum(0))).unsqueeze(1).expand_as(mu)         # (M, F)
    if acqf == ops.ACQF_UCB:
        sd = torch.sqrt(param * v.clamp_min(0.0))
        A, Amu = -mu + sd, -torch.ones_like(mu)
        Av = torch.where(v > 0, 0.5 * param / sd.clamp_min(1e-300), torch.zeros_like(sd))
    else:
        sig = v.clamp_min(1e-9).sqrt()
        u = -(mu - param) / sig
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
        cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2.0)))
        A, Amu, Av = sig * (pdf + u * cdf), -cdf, torch.where(v > 1e-9, 0.5 * pdf / sig, torch.zeros_like(sig))
    value = A.mean(1)
    if gi is None:
        return value, None
    n, Mq = Knq.shape
    D = gi["Xq"].shape[1]
    th = gi["theta"]
    diff = (gi["Xq"].unsqueeze(0) - gi["Xt"].unsqueeze(1)) / th[:D] ** 2                 # (n, M, D): (x_q - x_a) / l^2
    r2 = (((gi["Xq"].unsqueeze(0) - gi["Xt"].unsqueeze(1)) / th[:D]) ** 2).sum(-1)        # (n, M)
    if kind == O.KIND_RBF:
        dk = -th[D] * torch.exp(-0.5 * r2).unsqueeze(-1) * diff
    else:
        r = r2.sqrt()
        dk = -th[D] * (5.0 / 3.0) * ((1 + math.sqrt(5.0) * r) * torch.exp(-math.sqrt(5.0) * r)).unsqueeze(-1) * diff
    dkn = gi["cov_g"].reshape(n, Mq, 16)[:, :, 1:1 + D] / (s * s) + dk
    dmu = gi["mu_g"].reshape(Mq, 16)[:, 1:1 + D].unsqueeze(1) + s * torch.einsum("af,aqd->qfd", alpha, dkn)   # (M, F, D)
    dvar = gi["var_g"].reshape(Mq, 16)[:, 1:1 + D] - 2 * s * s * torch.einsum("aq,aqd->qd", Z, dkn)           # (M, D)
    grad = (Amu.unsqueeze(-1) * dmu + Av.unsqueeze(-1) * dvar.unsqueeze(1)).mean(1)
    return value, grad


# boundary shapes: F in {1, 2, 63, 64}, n' in {1, 16, 17, 96}, M in {1, 127, 1024}, D in {1, 6, 15}
SHAPES = [(1, 1, 1, 1), (2, 16, 127, 6), (63, 17, 1024, 15), (64, 96, 127, 6), (64, 96, 1024, 15), (16, 1, 1024, 1), (1, 17, 127, 15),
          (2, 96, 1, 6)]


@pytest.mark.parametrize("kind", [O.KIND_RBF, O.KIND_MATERN52])
@pytest.mark.parametrize("F,n,Mq,D", SHAPES)
def test_fantasy_kernel_matches_torch_composition(device, kind, F, n, Mq, D):
    g = torch.Generator().manual_seed(F * 1000 + n * 10 + D + kind)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    Knq, Z, alpha = 0.3 * r(n, Mq), 0.01 * r(n, Mq), r(n, F)
    mean_q, var_q = r(Mq), 0.5 + torch.rand(Mq, dtype=torch.float64, generator=g)
    gi = dict(cov_g=0.1 * r(n, Mq * 16), mu_g=r(Mq * 16), var_g=r(Mq * 16), Xt=torch.rand(n, D, dtype=torch.float64, generator=g),
              Xq=torch.rand(Mq, D, dtype=torch.float64, generator=g),
              theta=torch.cat([0.3 + torch.rand(D, dtype=torch.float64, generator=g), torch.tensor([1.3, 1e-3], dtype=torch.float64)]))
    m, s = 0.3, 1.7
    dev = lambda t: t.to(device)   # noqa: E731
    gid = {k: dev(v) for k, v in gi.items()}
    for acqf, param in ((ops.ACQF_UCB, 9.0), (ops.ACQF_EI, 0.1)):
        val, grad = ops.target_fantasy_acqf(dev(Knq), dev(Z), dev(alpha), dev(mean_q), dev(var_q), m, s, None, acqf, param, 0.0, gid, kind)
        vref, gref = _torch_fantasy_acqf(Knq, Z, alpha, mean_q, var_q, m, s, acqf, param, gi, kind)
        _close(val.cpu(), vref, 1e-10)
        _close(grad.cpu(), gref, 1e-10)
        v2, g2 = ops.target_fantasy_acqf(dev(Knq), dev(Z), dev(alpha), dev(mean_q), dev(var_q), m, s, None, acqf, param)
        assert g2 is None
        _close(v2.cpu(), vref, 1e-10)
    # a factorisation that failed even with jitter: NaN everywhere, value and gradient
    info = torch.tensor([2], dtype=torch.int32, device=device)
    val, grad = ops.target_fantasy_acqf(dev(Knq), dev(Z), dev(alpha), dev(mean_q), dev(var_q), m, s, info, ops.ACQF_EI, 0.1, 0.0, gid, kind)
    assert bool(torch.isnan(val).all()) and bool(torch.isnan(grad).all())
    val, _ = ops.target_fantasy_acqf(dev(Knq), dev(Z), dev(alpha), dev(mean_q), dev(var_q), m, s, info, ops.ACQF_UCB, 9.0)
    assert bool(torch.isnan(val).all())


def test_fantasy_kernel_value_path_beyond_the_gradient_block(device):
    """n' = 200 (value path only: up to scaml_fit_max_n()); the gradient path refuses n' > 96."""
    g = torch.Generator().manual_seed(5)
    n, Mq, F = 200, 300, 16
    Knq, Z, alpha = 0.1 * torch.randn(n, Mq, dtype=torch.float64, generator=g), 1e-3 * torch.randn(n, Mq, dtype=torch.float64, generator=g), \
        torch.randn(n, F, dtype=torch.float64, generator=g)
    mean_q, var_q = torch.randn(Mq, dtype=torch.float64, generator=g), 1.0 + torch.rand(Mq, dtype=torch.float64, generator=g)
    val, _ = ops.target_fantasy_acqf(Knq.to(device), Z.to(device), alpha.to(device), mean_q.to(device), var_q.to(device), 0.1, 2.0, None,
                                     ops.ACQF_EI, -0.5)
    ref, _ = _torch_fantasy_acqf(Knq, Z, alpha, mean_q, var_q, 0.1, 2.0, ops.ACQF_EI, -0.5)
    _close(val.cpu(), ref, 1e-10)


@pytest.mark.parametrize("kind,T,N,D", STACKS)
def test_fantasy_acquisition_matches_oracle_autograd(device, kind, T, N, D):
    stack, parent, g = _parent(device, kind, T, N, D, n=12, seed=2)
    Xp = torch.rand(3, D, dtype=torch.float64, generator=g)
    fm = parent.fantasize(Xp, 4, generator=torch.Generator().manual_seed(11))
    assert fm.supports_posterior_grad()
    Xq = torch.rand(5, D, dtype=torch.float64, generator=g)
    best_f = float(parent.train_Y.min())
    Xt = torch.cat([parent.train_X.cpu(), Xp])
    xq = Xq.clone().requires_grad_(True)
    refs = [_oracle_posterior(stack, parent, xq, Xt, fm.train_Y[f].cpu().squeeze(-1), float(parent.m_all), float(parent.s_all)) for f in range(4)]
    for af, fn in ((utils.UpperConfidenceBound(fm), lambda m, v: O.ucb_minimize(m, v)),
                   (utils.ExpectedImprovement(fm, best_f), lambda m, v: O.expected_improvement_minimize(m, v, best_f))):
        val, grad = af.value_and_grad(Xq)
        ref = torch.stack([fn(m, v) for m, v in refs]).mean(0)
        (gref,) = torch.autograd.grad(ref.sum(), xq, retain_graph=True)
        _close(val.cpu(), ref.detach(), 1e-6)
        _close(grad.cpu(), gref, 1e-6)
        # the value-only call (scoring pass: the plain source pass instead of the GRAD pass) gives the same numbers
        _close(af(Xq).cpu(), val.cpu(), 1e-9)
        assert af(Xq.unsqueeze(1)).shape == (5,)


def test_graph_replay_on_a_fantasy_model(device):
    stack, parent, g = _parent(device, O.KIND_MATERN52, 8, 128, 6, n=12, seed=3)
    fm = parent.fantasize(torch.rand(4, 6, dtype=torch.float64, generator=g), 16, generator=torch.Generator().manual_seed(0))
    for af in (utils.UpperConfidenceBound(fm), utils.ExpectedImprovement(fm, float(parent.train_Y.min()))):
        ga = GraphedAcquisition(af.value_and_grad, 10, 6, device)
        for _ in range(3):
            X = torch.rand(10, 6, dtype=torch.float64, generator=g).to(device)
            v, gr = ga(X)
            ve, ge = af.value_and_grad(X)
            # (the source pass sums in LDS with float atomics: two evaluations agree to rounding, not bit for bit)
            _close(v.cpu(), ve.cpu(), 1e-10)
            _close(gr.cpu(), ge.cpu(), 1e-10)


def _hartmann_gps(device, T=4, N=64, seed=3):
    d = synthetic.hartmann6_task_stack(T, N, seed=seed, noise_std=0.1)
    stack = M.SourceGPStack([f"h{t}" for t in range(T)], [torch.from_numpy(d["X"][t]) for t in range(T)],
                            [torch.from_numpy(d["Y"][t]).unsqueeze(-1) for t in range(T)], kind=O.KIND_MATERN52, device=device)
    rng = np.random.default_rng(seed)
    stack.set_theta(torch.from_numpy(np.concatenate([0.6 + 0.8 * rng.uniform(size=(T, 6)), 0.5 + rng.uniform(size=(T, 1)),
                                                     1e-3 + 5e-3 * rng.uniform(size=(T, 1))], 1)))
    stack.refresh()
    return {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}


def _obj(x):
    return float(synthetic.hartmann6(np.asarray(x, dtype=np.float64).reshape(1, -1))[0])


def _loop(gps, k, seed=0, acq="ucb"):
    return ScaMLGPBOLoop(gps, dim=6, acquisition=acq, num_restarts_log_likelihood=1, raw_samples=256, num_restarts=4, af_max_iter=20, seed=seed,
                         max_pending_evaluations=k, num_fantasies=8)


def test_reproducible_fantasies_and_suggestions(device):
    gps = _hartmann_gps(device)
    g = torch.Generator().manual_seed(4)
    X0 = torch.rand(6, 6, dtype=torch.float64, generator=g)
    model = M.ScaMLGP(X0, torch.tensor([[_obj(x)] for x in X0]), gps).eval()
    Xp = torch.rand(3, 6, dtype=torch.float64, generator=g)
    # the base samples come from the generator alone: on one posterior the samples are identical bit for bit
    post = model.posterior(Xp, observation_noise=True)
    s1 = post.rsample(torch.Size([8]), generator=torch.Generator().manual_seed(9))
    s2 = post.rsample(torch.Size([8]), generator=torch.Generator().manual_seed(9))
    assert s1.shape == (8, 3, 1) and torch.equal(s1, s2)
    # (two posterior evaluations agree to rounding -- the source pass sums in LDS with float atomics -- so two fantasize calls do too)
    a = model.fantasize(Xp, 8, generator=torch.Generator().manual_seed(9))
    b = model.fantasize(Xp, 8, generator=torch.Generator().manual_seed(9))
    c = model.fantasize(Xp, 8, generator=torch.Generator().manual_seed(10))
    _close(a.train_Y.cpu(), b.train_Y.cpu(), 1e-10)
    assert float((a.train_Y - c.train_Y).abs().max()) > 1e-3
    runs = []
    for _ in range(2):
        loop = _loop(gps, 3, seed=5, acq="ei")
        loop.report(X0, [_obj(x) for x in X0])
        runs.append(torch.stack([loop.suggest() for _ in range(3)]))
    torch.testing.assert_close(runs[0], runs[1], rtol=0, atol=1e-6)


def test_bo_loop_with_pending_evaluations(device):
    gps = _hartmann_gps(device)
    g = torch.Generator().manual_seed(6)
    loop = _loop(gps, 3)
    X0 = torch.rand(4, 6, dtype=torch.float64, generator=g)
    loop.report(X0, torch.tensor([_obj(x) for x in X0]))    # several points at once: one refit
    assert loop.model.n == 4 and loop.pending.shape == (0, 6)
    xs = [loop.suggest() for _ in range(3)]
    assert loop.pending.shape == (3, 6)
    for i in range(3):
        for j in range(i):
            assert float((xs[i] - xs[j]).norm()) > 1e-3
    with pytest.raises(OptimizerNotReady):
        loop.suggest()
    loop.report(xs[1], _obj(xs[1]))
    assert loop.pending.shape == (2, 6) and not bool((loop.pending == xs[1]).all(-1).any())
    x4 = loop.suggest()
    assert loop.pending.shape == (3, 6) and bool(((x4 >= 0) & (x4 <= 1)).all())
    # a point that was never suggested may still be reported; it leaves the pending set as it is
    loop.report(torch.full((6,), 0.5, dtype=torch.float64), 0.0)
    assert loop.pending.shape == (3, 6) and loop.model.n == 6


def test_missing_objective_is_kept_but_not_fitted(device):
    """optimizer_test.py:55-97: five specifications before any report, reported together, one without an objective value."""
    gps = _hartmann_gps(device)
    loop = _loop(gps, 5)
    xs = [loop.suggest() for _ in range(5)]
    assert loop.pending.shape == (5, 6)
    ys = [0.42 + 0.1 * i for i in range(5)]
    ys[-2] = None
    loop.report(torch.stack(xs), ys)
    assert loop.X.shape == (5, 6) and loop.Y.shape == (5, 1) and bool(torch.isnan(loop.Y[-2]).all())
    assert loop.model.n == 4 and loop.model.train_targets.numel() == 4
    assert loop.pending.shape == (0, 6)
    loop.suggest()
    assert loop.pending.shape == (1, 6)
    loop.report(loop.pending[0], float("nan"))   # NaN counts as missing too
    assert loop.X.shape == (6, 6) and loop.model.n == 4 and loop.pending.shape == (0, 6)
