"""The batched acquisition of many studies on the MI355X (scaml_posterior_linv_grad_grouped_f64 + scaml_target_acqf_batched_f64 through
``utils.StudiesAcquisition``) against each study's OWN path -- ``af.value_and_grad`` / ``ScaMLGP.posterior_with_grad``, which
tests/test_posterior_grad_gpu.py holds to the oracle -- and once against torch autograd through the oracle directly.

Bound against the studies' own path: 1e-10 of max |ref| per quantity (tests/test_studies_gpu.py::_close, tests/test_model_gpu.py).
The own path is first measured against itself (two calls at the same points: the source pass adds the waves' shares of a mean with
LDS float atomics), the figure printed and held under 1e-11, where the 1e-10 applies as it stands.  Measured on the MI355X: that
scatter is 4e-16 .. 4e-15 over all stacks of this file (the ungrouped source pass against itself 5e-16 .. 6e-16), the batched
evaluation differs from the own path by at most 1.2e-12, a graph replay from the eager evaluation by at most 3.3e-15, and the batch
from torch autograd through the oracle by at most 2.1e-14.

Stacks: the c5r-shaped one of tests/test_studies_gpu.py (Hartmann-6, T = 2, N = 64, Matern-5/2) with n = (1, 16, 17, 40); the
ragged golden stack (T = 4, N = 48, per-task counts 48 / 17 / 1 / 33) with an RBF target kernel, where a study's n is bounded by the
stack's N = 48 (the GRAD pass keeps the covariance tiles in the task's LDS strip: Ma <= N); and n = 96, the kernels' limit, on a
Hartmann-6 stack of N = 96 with an RBF target kernel.

The 1e-10 here is a max-norm tolerance between two sets of kernels.  The per-element fp64 bound of the kernel body itself
(sa_block of csrc/gp_studies_acqf.h: value, grad, mu_out, var_out against a long-double reference) lives in
tests/_studies_bounds.py and is held by tests/test_studies_bounds.py / tests/test_studies_bounds_gpu.py."""
import os

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import _lib, hyper, model as M, ops, studies, synthetic, utils
from scamlgp_amd.bo import GraphedAcquisition

pytestmark = pytest.mark.gpu
BOUND = 1e-10         # batched against own path, of max |ref| per quantity
SCATTER_MAX = 1e-11   # what the own path may differ from itself for that bound to be the right one
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


def _hartmann_gps(device, T=2, N=64, seed=3):
    d = synthetic.hartmann6_task_stack(T, N, seed=seed, noise_std=0.1)
    stack = M.SourceGPStack([f"h{t}" for t in range(T)], [torch.from_numpy(d["X"][t]) for t in range(T)],
                            [torch.from_numpy(d["Y"][t]).unsqueeze(-1) for t in range(T)], kind=O.KIND_MATERN52, device=device)
    rng = np.random.default_rng(seed)
    stack.set_theta(torch.from_numpy(np.concatenate([0.6 + 0.8 * rng.uniform(size=(T, 6)), 0.5 + rng.uniform(size=(T, 1)),
                                                     1e-3 + 5e-3 * rng.uniform(size=(T, 1))], 1)))
    stack.refresh()
    return {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}


def _ragged_gps(device):
    d = np.load(os.path.join(GOLDEN, "edge_ragged_T4_N48_matern.npz"))
    n = d["n_points"]
    X = [torch.from_numpy(d["X"][t, :n[t]]) for t in range(4)]
    Y = [torch.from_numpy(d["y"][t, :n[t]] * d["y_std"][t] + d["y_mean"][t]).unsqueeze(-1) for t in range(4)]
    stack = M.SourceGPStack([f"r{t}" for t in range(4)], X, Y, kind=int(d["kind"]), device=device)
    stack.set_theta(torch.from_numpy(d["theta"]))
    stack.refresh()
    assert stack.n_points is not None
    return {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}


def _models(gps, ns, kernel, seed, prune=(1, 0)):
    """One ScaMLGP per n: own training set, own weights (model ``prune[0]`` has task ``prune[1]`` below the pruning threshold), own theta."""
    g = torch.Generator().manual_seed(seed)
    stack = next(iter(gps.values()))._stack
    D, T = stack.D, stack.T
    models = []
    for i, n in enumerate(ns):
        X = torch.rand(n, D, dtype=torch.float64, generator=g)
        Y = torch.sin(3.0 * X.sum(-1, keepdim=True)) + 0.1 * torch.randn(n, 1, dtype=torch.float64, generator=g) + 0.5 * i
        cov = hyper.get_default_kernel(kernel, D)
        m = M.ScaMLGP(X, Y, gps, covar_module=cov)
        w = 0.2 + torch.rand(T, dtype=torch.float64, generator=g)
        if i == prune[0]:
            w[prune[1]] = 1e-9
        m.weights = w
        th = torch.cat([0.5 + torch.rand(D, dtype=torch.float64, generator=g), 0.3 + torch.rand(1, dtype=torch.float64, generator=g),
                        1e-3 + 1e-2 * torch.rand(1, dtype=torch.float64, generator=g)])
        m.raw_theta = m.spec.to_raw(th.to(m.device))
        models.append(m.eval())
    assert not bool(models[prune[0]]._active_tasks()[1].all()) and all(bool(mm._active_tasks()[1].all()) for j, mm in enumerate(models) if j != prune[0])
    return models


def _afs(models, which):
    if which == "ucb":
        return [utils.UpperConfidenceBound(m, 4.0 + i) for i, m in enumerate(models)]
    return [utils.ExpectedImprovement(m, float(m.train_Y.min()) - 0.05 * i) for i, m in enumerate(models)]


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _check_batch(models, counts, seed):
    D, dev = models[0]._stack.D, models[0].device
    g = torch.Generator().manual_seed(seed)
    Xs = [torch.rand(c, D, dtype=torch.float64, generator=g).to(dev) for c in counts]
    # the own path against itself: the scatter of the source pass's LDS atomics
    scatter = 0.0
    for m, x in zip(models, Xs):
        a, b = m.posterior_with_grad(x), m.posterior_with_grad(x)
        scatter = max(scatter, max(_rel(u, v) for u, v in zip(a, b)))
    print(f"own path against itself: {scatter:.3e}")
    assert scatter <= SCATTER_MAX
    bound = BOUND
    for which in ("ucb", "ei"):
        afs = _afs(models, which)
        sa = utils.StudiesAcquisition(afs)
        group = sa.group_of(counts)
        out = sa.evaluate(torch.cat(Xs), group, want_posterior=True)
        torch.cuda.synchronize()
        for k, chunks in ((k, out[k].split(list(counts))) for k in ("value", "grad", "mu", "var")):
            for s, (af, m, x) in enumerate(zip(afs, models, Xs)):
                v, gr = af.value_and_grad(x)
                mu, var, _, _ = m.posterior_with_grad(x)
                ref = dict(value=v, grad=gr, mu=mu, var=var)[k]
                err = _rel(chunks[s], ref)
                print(f"{which} study {s} (n = {m.n}) {k}: {err:.3e}")
                assert err <= bound, (which, s, k, err)
    return sa, group, torch.cat(Xs)


def test_batched_evaluation_matches_each_study(device):
    """S = 4 models, n = (1, 16, 17, 40), one task pruned in model 1, R_s = (4, 4, 3, 1) starts, UCB then EI with per-study best_f.  The
    scatter of the own path and every difference are printed before they are asserted."""
    models = _models(_hartmann_gps(device), (1, 16, 17, 40), hyper.MaternKernel, seed=1)
    _check_batch(models, (4, 4, 3, 1), seed=2)


def test_batched_evaluation_ragged_stack_rbf_and_the_size_limit(device):
    models = _models(_ragged_gps(device), (3, 48, 16), hyper.RBFKernel, seed=3, prune=(2, 1))
    _check_batch(models, (2, 3, 2), seed=4)
    models = _models(_hartmann_gps(device, T=2, N=96), (96, 5), hyper.RBFKernel, seed=5)
    _check_batch(models, (3, 2), seed=6)


def test_against_oracle(device):
    """UCB of the first batch against torch autograd through the oracle's source and target posterior, rel. 1e-4
    (tests/test_posterior_grad_gpu.py's bound)."""
    gps = _hartmann_gps(device)
    models = _models(gps, (1, 16, 17, 40), hyper.MaternKernel, seed=1)
    stack = models[0]._stack
    counts = (4, 4, 3, 1)
    afs = _afs(models, "ucb")
    sa = utils.StudiesAcquisition(afs)
    g = torch.Generator().manual_seed(2)
    Xs = [torch.rand(c, stack.D, dtype=torch.float64, generator=g) for c in counts]
    out = sa.evaluate(torch.cat(Xs).to(device), sa.group_of(counts), want_posterior=True)
    fits = [O.gp_fit(stack.X[t].cpu(), stack.y[t].cpu(), stack.theta[t].cpu(), stack.kind) for t in range(stack.T)]
    for s, (af, m, x) in enumerate(zip(afs, models, Xs)):
        xq = x.clone().requires_grad_(True)
        w = m.weights.cpu()
        mask = O.significant_weights_mask(w, stack.y_std.cpu(), 1e-3)
        xall = torch.cat([m.train_X.cpu(), xq])
        post = [O.source_posterior(xall, stack.X[t].cpu(), stack.theta[t].cpu(), stack.kind, fits[t]["L"], fits[t]["alpha"], float(stack.y_mean[t]),
                                   float(stack.y_std[t])) for t in range(stack.T) if bool(mask[t])]
        mu_j, cov_j = O.target_prior(torch.stack([p[0] for p in post]), torch.stack([p[1] for p in post]), w[mask])
        mu, Sg = O.target_posterior(xq, m.train_X.cpu(), m.train_Y.cpu().squeeze(-1), mu_j, cov_j, m.theta.cpu(), m.kind, float(m.m_all), float(m.s_all))
        var = Sg.diagonal()
        val = -mu + torch.sqrt(af.beta * var.clamp_min(0.0))
        (gr,) = torch.autograd.grad(val.sum(), xq)
        for k, ref in (("value", val), ("grad", gr), ("mu", mu), ("var", var)):
            err = _rel(out[k].split(list(counts))[s], ref)
            print(f"oracle, study {s} {k}: {err:.3e}")
            assert err <= 1e-4, (s, k, err)


def test_grouped_pass_equals_ungrouped(device):
    models = _models(_hartmann_gps(device), (1, 17, 40), hyper.MaternKernel, seed=7)
    sa = utils.StudiesAcquisition(_afs(models, "ucb"))
    st, f = models[0]._stack, models[0]._stack.fit
    g = torch.Generator().manual_seed(8)
    counts = (2, 3, 2)
    Xq = torch.rand(sum(counts) + 1, st.D, dtype=torch.float64, generator=g).to(device)
    group = torch.cat([sa.group_of(counts)[:5], torch.tensor([-1], dtype=torch.int32, device=device), sa.group_of(counts)[5:]])   # a padding row inside
    out = ops.source_posteriors_grad_grouped(Xq, group, sa.Xt, sa.n_points, sa.VA_tab, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean,
                                             st.y_std, st.n_points)
    cov = out["cov"].reshape(st.T, sa.n_max, Xq.shape[0], 16)
    for s, m in enumerate(models):
        rows = torch.nonzero(group == s).flatten()
        call = lambda: ops.source_posteriors_grad(Xq[rows], m.train_X, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean, st.y_std,   # noqa: E731
                                                  st.n_points, m._train_VA())
        ref, again = call(), call()
        scatter = max(_rel(ref["mu"], again["mu"]), _rel(ref["var"], again["var"]))
        print(f"group {s}: ungrouped pass against itself {scatter:.3e}")
        assert scatter <= SCATTER_MAX
        bound = BOUND
        assert _rel(out["mu"][:, rows], ref["mu"]) <= bound and _rel(out["var"][:, rows], ref["var"]) <= bound
        # the covariance block is summed in a fixed order on both sides
        assert torch.equal(cov[:, :m.n][:, :, rows], ref["cov"].reshape(st.T, m.n, rows.numel(), 16))
    assert not bool(out["mu"][:, 5].any()) and not bool(out["var"][:, 5].any())
    assert studies.MAX_STACK_N == _lib.lib.scaml_posterior_max_n()   # the pass's limit on the stack's N, as the Python layer states it


def test_graph_replay_equals_eager(device):
    models = _models(_hartmann_gps(device), (1, 16, 17, 40), hyper.MaternKernel, seed=1)
    sa, group, X = _check_batch(models[:2], (4, 4), seed=9)
    graphed = GraphedAcquisition(lambda x: sa.value_and_grad(x, group), X.shape[0], X.shape[1], device)
    g = torch.Generator().manual_seed(10)
    for x in (X, torch.rand(X.shape, dtype=torch.float64, generator=g).to(device)):
        (v1, g1), (v0, g0), (v2, g2) = graphed(x), sa.value_and_grad(x, group), sa.value_and_grad(x, group)
        scatter = max(_rel(v0, v2), _rel(g0, g2))
        assert scatter <= SCATTER_MAX
        bound = BOUND
        print(f"eager against itself {scatter:.3e}; replay against eager {_rel(v1, v0):.3e} / {_rel(g1, g0):.3e}")
        assert _rel(v1, v0) <= bound and _rel(g1, g0) <= bound
