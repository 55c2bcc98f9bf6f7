"""Lock-step studies with one source stack PER study on the MI355X: slices of one parent stack (``SourceGPStack.slice``), the grouped
GRAD source pass with per-group source tasks (``scaml_posterior_linv_grad_grouped_own_f64``), the device optimiser on top of it
(``scaml_studies_acqf_opt_own_f64``) and ``bo.ScaMLGPBOStudies`` on a list of per-study dicts.

Helpers and bounds are those of tests/test_studies_acqf_gpu.py: ``BOUND`` = 1e-10 of max |ref| per quantity, the own path first
measured against itself and held under ``SCATTER_MAX`` = 1e-11 (the source pass adds the waves' shares of a mean with LDS float
atomics).  Every figure is printed before it is asserted (``pytest -s`` shows them).

Parents.  ``hartmann``: S * T = 3 * 2 Hartmann-6 tasks, N = 64, Matern-5/2, fixed thetas as ``_hartmann_gps`` draws them; the studies
are the slices [0, 2), [2, 4), [4, 6).  ``ragged``: the ragged golden stack twice (2 * 4 tasks, N = 48, per-task counts 48 / 17 / 1 /
33); its studies are the slices [0, 4), [1, 5) and [4, 8) -- two copies in the same order have equal counts at a slot and at its
source task, so the slice [1, 5) (counts 17 / 1 / 33 / 48 at slots 0 .. 3) is what tells ``n_points[src]`` from ``n_points[slot]``.
Study sizes n = (1, 17, 40), one task pruned in one study only, one query a padding row."""
import os

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import hyper, model as M, ops, synthetic, utils
from scamlgp_amd.bo import ScaMLGPBOLoop, ScaMLGPBOStudies, acqf_local_optimization
from tests.test_studies_acqf_gpu import BOUND, GOLDEN, SCATTER_MAX, _afs, _rel

pytestmark = pytest.mark.gpu
NS = (1, 17, 40)
RUNNING = 0


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


def _dicts(stacks):
    return [{tid: M.SourceGP(st, i) for i, tid in enumerate(st.task_ids)} for st in stacks]


def _build(ids, X, Y, theta, kind, device):
    st = M.SourceGPStack(ids, X, Y, kind=kind, device=device)
    st.set_theta(theta)
    st.refresh()
    return st


def _hartmann_data(S=3, T=2, N=64, seed=3):
    d = synthetic.hartmann6_task_stack(S * T, N, seed=seed, noise_std=0.1)
    rng = np.random.default_rng(seed)
    theta = torch.from_numpy(np.concatenate([0.6 + 0.8 * rng.uniform(size=(S * T, 6)), 0.5 + rng.uniform(size=(S * T, 1)),
                                             1e-3 + 5e-3 * rng.uniform(size=(S * T, 1))], 1))
    X = [torch.from_numpy(d["X"][t]) for t in range(S * T)]
    Y = [torch.from_numpy(d["Y"][t]).unsqueeze(-1) for t in range(S * T)]
    return X, Y, theta, O.KIND_MATERN52, [(2 * s, 2 * s + 2) for s in range(S)]


def _ragged_data():
    d = np.load(os.path.join(GOLDEN, "edge_ragged_T4_N48_matern.npz"))
    n = d["n_points"]
    assert n.tolist() == [48, 17, 1, 33]
    X = [torch.from_numpy(d["X"][t, :n[t]]) for t in range(4)] * 2
    Y = [torch.from_numpy(d["y"][t, :n[t]] * d["y_std"][t] + d["y_mean"][t]).unsqueeze(-1) for t in range(4)] * 2
    return X, Y, torch.from_numpy(np.concatenate([d["theta"], d["theta"]])), int(d["kind"]), [(0, 4), (1, 5), (4, 8)]


class _Case:
    """A parent stack, its slices, and per slice a standalone stack built from the same tasks' data and thetas."""

    def __init__(self, data, device):
        X, Y, theta, kind, ranges = data
        self.parent = _build([f"p{t}" for t in range(len(X))], X, Y, theta, kind, device)
        self.ranges = ranges
        self.slices = [self.parent.slice(lo, hi) for lo, hi in ranges]
        self.alone = [_build([f"p{t}" for t in range(lo, hi)], X[lo:hi], Y[lo:hi], theta[lo:hi], kind, device) for lo, hi in ranges]
        self.T, self.D = ranges[0][1] - ranges[0][0], self.parent.D


@pytest.fixture(scope="module")
def hartmann(device):
    return _Case(_hartmann_data(), device)


@pytest.fixture(scope="module")
def ragged(device):
    c = _Case(_ragged_data(), device)
    assert c.parent.n_points is not None and c.slices[1].n_points.tolist() == [17, 1, 33, 48]
    return c


def _study_models(dicts, ns, kernel, seed, prune=(1, 0)):
    """tests/test_studies_acqf_gpu.py::_models with one source dict per study: own training set, own weights (model ``prune[0]`` has
    task ``prune[1]`` below the pruning threshold), own theta -- the same for the same seed, whatever the dicts.  (The noise is drawn
    from [1e-3, 9e-3]: that file's 1e-3 + 1e-2 u can leave the likelihood's interval, and the raw value is then NaN.)"""
    g = torch.Generator().manual_seed(seed)
    models = []
    for i, (n, gps) in enumerate(zip(ns, dicts)):
        stack = next(iter(gps.values()))._stack
        D, T = stack.D, stack.T
        X = torch.rand(n, D, dtype=torch.float64, generator=g)
        Y = torch.sin(3.0 * X.sum(-1, keepdim=True)) + 0.1 * torch.randn(n, 1, dtype=torch.float64, generator=g) + 0.5 * i
        m = M.ScaMLGP(X, Y, gps, covar_module=hyper.get_default_kernel(kernel, D))
        w = 0.2 + torch.rand(T, dtype=torch.float64, generator=g)
        if i == prune[0]:
            w[prune[1]] = 1e-9
        m.weights = w
        th = torch.cat([0.5 + torch.rand(D, dtype=torch.float64, generator=g), 0.3 + torch.rand(1, dtype=torch.float64, generator=g),
                        1e-3 + 8e-3 * torch.rand(1, dtype=torch.float64, generator=g)])   # (inside the noise constraint's (1e-8, 1e-2))
        m.raw_theta = m.spec.to_raw(th.to(m.device))
        assert bool(torch.isfinite(m.raw_theta).all())
        models.append(m.eval())
    assert [bool(mm._active_tasks()[1].all()) for mm in models] == [j != prune[0] for j in range(len(models))]
    return models


def _slice_models(case, seed=1, kernel=hyper.MaternKernel):
    return _study_models(_dicts(case.slices), NS, kernel, seed)


def _queries(case, counts, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(c, case.D, dtype=torch.float64, generator=g).to(case.parent.device) for c in counts]


def _own_scatter(models, Xs):
    scatter = 0.0
    for m, x in zip(models, Xs):
        a, b = m.posterior_with_grad(x), m.posterior_with_grad(x)
        assert all(bool(torch.isfinite(u).all()) for u in a)
        scatter = max(scatter, max(_rel(u, v) for u, v in zip(a, b)))
    print(f"own path against itself: {scatter:.3e}")
    assert scatter <= SCATTER_MAX
    return scatter


# ---- 1. a model on a slice is the model on a standalone stack of the same tasks ---------------------------------------------------------
@pytest.mark.parametrize("name", ["hartmann", "ragged"])
def test_slice_model_equals_standalone_model(name, request):
    """The standardiser (m_all, s_all over the study's OWN tasks' observations and its targets), the cached source terms and the posterior
    with its input gradient, per study, within BOUND."""
    case = request.getfixturevalue(name)
    on_slice = _slice_models(case)
    alone = _study_models(_dicts(case.alone), NS, hyper.MaternKernel, 1)
    Xs = _queries(case, (3, 3, 3), seed=2)
    _own_scatter(on_slice, Xs)
    for s, (a, b, x) in enumerate(zip(on_slice, alone, Xs)):
        assert a.T == b.T == case.T and a._stack.T == case.T and a._stack is case.slices[s]
        for what, u, v in (("m_all", a.m_all, b.m_all), ("s_all", a.s_all, b.s_all)):
            err = _rel(u.reshape(1), v.reshape(1))
            print(f"{name} study {s} {what}: {err:.3e}")
            assert err <= BOUND, (s, what, err)
        # the parent's other tasks are not in the standardiser: over all of them it is another number
        every = M.standardize_fit(torch.cat([case.parent.raw_targets(), a.train_Y], dim=-2))
        assert abs(float(every[0]) - float(a.m_all)) > 1e-6 * abs(float(a.m_all)) or abs(float(every[1]) - float(a.s_all)) > 1e-6 * float(a.s_all)
        for what, u, v in zip(("mu", "var", "dmu", "dvar"), a.posterior_with_grad(x), b.posterior_with_grad(x)):
            err = _rel(u, v)
            print(f"{name} study {s} (n = {a.n}) {what}: {err:.3e}")
            assert err <= BOUND, (s, what, err)


# ---- 2. the batched evaluation against each study's own path -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hartmann", "ragged"])
def test_batched_evaluation_matches_each_study(name, request):
    case = request.getfixturevalue(name)
    models = _slice_models(case)
    counts = (4, 3, 2)
    Xs = _queries(case, counts, seed=3)
    _own_scatter(models, Xs)
    pad = torch.rand(1, case.D, dtype=torch.float64).to(case.parent.device)
    for which in ("ucb", "ei"):
        afs = _afs(models, which)
        sa = utils.StudiesAcquisition(afs)
        assert sa.task_base.tolist() == [lo for lo, _ in case.ranges] and sa.source is case.parent and tuple(sa.w.shape) == (3, case.T)
        grp = sa.group_of(counts)
        # one padding row, inside study 1's points
        X = torch.cat([Xs[0], Xs[1][:1], pad, Xs[1][1:], Xs[2]])
        group = torch.cat([grp[:5], torch.tensor([-1], dtype=torch.int32, device=grp.device), grp[5:]])
        out = sa.evaluate(X, group, want_posterior=True)
        torch.cuda.synchronize()
        real = torch.nonzero(group >= 0).flatten()
        for k in ("value", "grad", "mu", "var"):
            assert not bool(out[k][5].any()), k     # the padding row: zeros
            chunks = out[k][real].split(list(counts))
            for s, (af, m, x) in enumerate(zip(afs, models, Xs)):
                v, gr = af.value_and_grad(x)
                mu, var, _, _ = m.posterior_with_grad(x)
                err = _rel(chunks[s], dict(value=v, grad=gr, mu=mu, var=var)[k])
                print(f"{name} {which} study {s} (n = {m.n}) {k}: {err:.3e}")
                assert err <= BOUND, (which, s, k, err)


# ---- 3. / 4. the raw pass: no cross-talk between studies, a task base that leaves the arrays ------------------------------------------
def _raw_pass(sa, X, group, task_base=None, cov_out=None):
    st, f = sa.source, sa.source.fit
    args = (X, group, sa.Xt, sa.n_points, sa.VA_tab, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean, st.y_std, st.n_points)
    tb = sa.task_base if task_base is None else task_base
    return ops.source_posteriors_grad_grouped(*args, task_base=tb, tasks_per_group=sa.w.shape[1], cov_out=cov_out)   # (cov_out: a prefilled cov)


def _strips(out, sa, group, g):
    """Group g's strips of mu, var and the written rows of cov."""
    rows = torch.nonzero(group == g).flatten()
    T, Mq = out["mu"].shape[0], out["mu"].shape[1]
    cov = out["cov"].reshape(T, sa.n_max, Mq, 16)
    return out["mu"][:, rows], out["var"][:, rows], cov[:, :int(sa.n_points[g])][:, :, rows]


@pytest.mark.parametrize("name,scaled", [("hartmann", (2, 3)), ("ragged", (0,))])
def test_no_cross_talk_between_studies(name, scaled, request):
    """The source ``alpha`` of some parent tasks times 3 -- hartmann: study 1's two tasks; ragged (overlapping slices): task 0, which only
    study 0 reads.  The raw strips of the studies that do not read those tasks stay within SCATTER_MAX of the run before, the others'
    means change (variances and covariances do not depend on alpha)."""
    case = request.getfixturevalue(name)
    sa = utils.StudiesAcquisition(_afs(_slice_models(case), "ucb"))
    counts = (3, 3, 3)
    X, group = torch.cat(_queries(case, counts, seed=4)), sa.group_of(counts)
    before, again = _raw_pass(sa, X, group), _raw_pass(sa, X, group)
    alpha = case.parent.fit["alpha"]
    keep = alpha.clone()
    try:
        alpha[list(scaled)] *= 3.0
        after = _raw_pass(sa, X, group)
        torch.cuda.synchronize()
    finally:
        alpha.copy_(keep)
    touched = {g for g, (lo, hi) in enumerate(case.ranges) if any(lo <= t < hi for t in scaled)}
    assert touched == ({1} if name == "hartmann" else {0})
    for g in range(3):
        for what, u, v, w in zip(("mu", "var", "cov"), _strips(before, sa, group, g), _strips(after, sa, group, g), _strips(again, sa, group, g)):
            err, scatter = _rel(v, u), _rel(w, u)
            print(f"{name} study {g} {what}: after against before {err:.3e} (a repeat against before {scatter:.3e})")
            assert scatter <= SCATTER_MAX
            if g not in touched or what != "mu":
                assert err <= SCATTER_MAX, (g, what, err)
            else:
                assert err > 1e-3, (g, what, err)


def test_task_base_outside_the_source_arrays_is_a_padding_row(hartmann):
    case = hartmann
    sa = utils.StudiesAcquisition(_afs(_slice_models(case), "ucb"))
    dev = case.parent.device
    counts = (3, 3, 3)
    X, group = torch.cat(_queries(case, counts, seed=5)), sa.group_of(counts)
    good = _raw_pass(sa, X, group)
    st, f = case.parent, case.parent.fit
    rows = torch.nonzero(group == 1).flatten()
    plain = ops.source_posteriors_grad(X[rows], None, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean, st.y_std, st.n_points, None)
    SENT = -777.25
    # (base, the slot that leaves the arrays, the slot that stays and the source task it reads): Tsrc = 6, T = 2
    for base, out_slot, in_slot, src in ((5, 1, 0, 5), (-1, 0, 1, 0), (2 ** 31 - 1, None, None, None), (-(2 ** 31), None, None, None)):
        tb = torch.tensor([0, base, 4], dtype=torch.int32, device=dev)
        cov = torch.full((case.T, sa.n_max, X.shape[0] * 16), SENT, dtype=torch.float64, device=dev)
        out = _raw_pass(sa, X, group, task_base=tb, cov_out=cov)
        torch.cuda.synchronize()
        cov4 = out["cov"].reshape(case.T, sa.n_max, X.shape[0], 16)
        for slot in ((0, 1) if out_slot is None else (out_slot,)):
            assert not bool(out["mu"][slot, rows].any()) and not bool(out["var"][slot, rows].any()), (base, slot)
            assert bool((cov4[slot][:, rows] == SENT).all()), (base, slot)     # no cov row written
        if in_slot is not None:       # the slot inside the arrays reads task `src`: its mean and variance at these points
            for what in ("mu", "var"):
                err = _rel(out[what][in_slot, rows], plain[what][src])
                print(f"base {base}: slot {in_slot} = task {src}, {what} against the ungrouped pass {err:.3e}")
                assert err <= BOUND
            assert bool((cov4[in_slot, :int(sa.n_points[1])][:, rows] != SENT).all())
        for g in (0, 2):
            for what, u, v in zip(("mu", "var", "cov"), _strips(good, sa, group, g), _strips(out, sa, group, g)):
                assert _rel(v, u) <= SCATTER_MAX, (base, g, what)


# ---- 5. the device optimiser -----------------------------------------------------------------------------------------------
def test_device_optimiser_on_per_study_stacks(hartmann, device):
    """4 starts per study, max_iter = 20, UCB: every start stops, ``f`` is the value at ``x``, and per study the best end value is no
    worse than the best end point of that study's own ``bo.acqf_local_optimization`` (stage 2 of ``optimize_acqf``: scipy L-BFGS-B around
    the model's own ``af.value_and_grad``) from the same starts by more than 1e-6 of |f| -- tests/test_acqf_opt_gpu.py's tolerance
    between two drivers (RTOL_DRIVERS), which it applies to ``hyper.batched_lbfgs`` around the batched evaluation; that comparison is
    made here as well, around each model's own evaluation."""
    case = hartmann
    models = _slice_models(case)
    afs = _afs(models, "ucb")
    sa = utils.StudiesAcquisition(afs)
    counts = (4, 4, 4)
    g = torch.Generator().manual_seed(6)
    X0 = torch.rand(sum(counts), case.D, dtype=torch.float64, generator=g)
    group = sa.group_of(counts)
    run = sa.optimizer(X0, group, 20)
    assert run._own is not None and run._own[1] == case.parent.T
    res = sa.optimize(X0, group, 20)
    x, f, stats = res["x"], res["f"].cpu(), res["stats"]
    print(f"rounds {res['n_eval']} in {res['n_calls']} calls; per start (it, evals, status, pairs) {stats.tolist()}")
    assert not bool((stats[:, 2] == RUNNING).any())
    assert bool(((x >= 0.0) & (x <= 1.0)).all())
    v = sa.value(x, group).cpu()
    err = float((f - v).abs().max()) / float(v.abs().max())
    print(f"f against sa.value at x: {err:.3e}")
    assert err <= BOUND
    for s, (af, x0, fs) in enumerate(zip(afs, X0.split(list(counts)), f.split(list(counts)))):
        xs = acqf_local_optimization(af, x0, max_iter=20)
        ref = float(af(xs.to(device)).max())

        def fun(xh, af=af):
            vv, gg = af.value_and_grad(xh.to(device))
            return -vv.cpu(), -gg.cpu()

        host = float((-hyper.batched_lbfgs(fun, x0, max_iter=20, bounds=(0.0, 1.0)).f).max())
        best = float(fs.max())
        print(f"study {s}: best end value, device {best:.12f}, own optimize_acqf stage {ref:.12f}, own batched_lbfgs {host:.12f}")
        assert best >= ref - 1e-6 * abs(ref), (s, best, ref)
        assert abs(best - host) <= 1e-6 * max(abs(best), abs(host)), (s, best, host)


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
KW = dict(acquisition="ucb", raw_samples=64, num_restarts=4, num_restarts_log_likelihood=1, af_max_iter=20)
SEEDS = [41, 42, 43]


def _obj(x):
    return float(synthetic.hartmann6(np.asarray(x, dtype=np.float64).reshape(1, -1))[0])


class _Twin:
    """A ScaMLGPBOLoop whose restart samples follow a generator's stream, as a study's ``fit_gens`` entry does
    (tests/test_studies_gpu.py)."""

    def __init__(self, gps, seed):
        self.loop = ScaMLGPBOLoop(gps, 6, seed=seed, **KW)
        self.gen = torch.Generator().manual_seed(seed)

    def report(self, x, y):
        with utils._rng_of(self.gen):
            self.loop.report(x, y)


@pytest.mark.parametrize("mode", ["sequential", "lockstep", "device"])
def test_studies_on_a_list_of_dicts(hartmann, device, mode):
    """Two steps of ``ScaMLGPBOStudies`` on three per-study dicts in every mode.  ``"sequential"`` runs next to three ScaMLGPBOLoops on
    STANDALONE stacks of the same tasks, with the same seeds and told the same evaluations.

    Comparison used: the ACQUISITION VALUES at the two sides' suggested points (both scored by the loop's acquisition function), within
    1e-8 of |value| -- not the points themselves within 1e-8.  Measured on the MI355X over 20 runs of this case: the points differ by
    1e-15 .. 1.2e-5 (max over coordinates); of 12 runs that asserted 1e-8 on the points 4 failed (1.6e-8, 2.0e-8, 3.8e-8, 7.7e-8, always
    study 1 at step 1).
    The cause is the one tests/test_studies_gpu.py documents: the source pass's LDS atomics scatter the source means of a training
    set by ~1e-15 between the slice and the standalone stack (check 1: 3e-16 .. 3e-15), the refit on ONE point is flat along the raw
    outputscale and turns that into 0 .. 9e-5 (relative) in the fitted raw hyper-parameters, and the next acquisition optimum moves with
    them.  The acquisition values at the two points agreed to 1.7e-11 relative or better in all 20 runs (4.4e-13 in the first 12).  The
    bound: L-BFGS-B stops on a relative decrease of 2.2e-9, which is how well an end value is determined; 1e-8 is 4.5 of those.  The
    point differences are printed."""
    case = hartmann
    dicts = _dicts(case.slices)
    studies = ScaMLGPBOStudies(dicts, dim=6, num_studies=3, seeds=SEEDS, suggest_mode=mode, **KW)
    twins = [_Twin(d, s) for d, s in zip(_dicts(case.alone), SEEDS)] if mode == "sequential" else None
    for step in range(2):
        X = studies.suggest()
        assert X.shape == (3, 6) and bool(((X >= 0.0) & (X <= 1.0)).all())
        if mode != "sequential":
            assert studies.last_suggest_info["batched"] == ([] if step == 0 else [0, 1, 2])
        if twins:
            for s, tw in enumerate(twins):
                xl = tw.loop.suggest()
                af = tw.loop.acquisition_function()
                v = af(torch.stack([X[s], xl]).to(device)).cpu()
                print(f"step {step} study {s}: suggested points max |diff| {float((X[s] - xl).abs().max()):.3e}; acquisition value there, "
                      f"study {float(v[0]):.12f}, loop {float(v[1]):.12f}")
                assert abs(float(v[0]) - float(v[1])) <= 1e-8 * max(abs(float(v[0])), abs(float(v[1]))), (step, s, v.tolist())
        ys = [_obj(x) for x in X]
        studies.report(X, ys)
        if twins:
            for s, tw in enumerate(twins):
                tw.report(X[s], ys[s])
                a, b = studies[s].model, tw.loop.model
                print(f"step {step} study {s}: fitted raw hyper-parameters {_rel(a.raw_theta, b.raw_theta):.3e}, weights {_rel(a.weights, b.weights):.3e}")
        assert all(st.model.T == 2 and st.model._stack.T == 2 and st.model.n == step + 1 for st in studies.studies)
    with pytest.raises(ValueError):
        ScaMLGPBOStudies(dicts[:2], dim=6, num_studies=3, suggest_mode=mode, **KW)


# ---- 7. the shared-stack path is the one it was ---------------------------------------------------------------------------------
def test_shared_stack_takes_the_old_entry_points(hartmann, monkeypatch):
    case = hartmann
    shared = _dicts([case.alone[0]])[0]
    models = _study_models([shared] * 3, NS, hyper.MaternKernel, 1)
    sa = utils.StudiesAcquisition(_afs(models, "ucb"))
    assert sa.task_base is None and sa.source is case.alone[0]
    seen = []
    plain = ops.source_posteriors_grad_grouped
    monkeypatch.setattr(utils.ops, "source_posteriors_grad_grouped", lambda *a, **kw: (seen.append(kw), plain(*a, **kw))[1])
    counts = (2, 2, 2)
    X = torch.cat(_queries(case, counts, seed=7))
    out = sa.evaluate(X, sa.group_of(counts))
    assert seen == [{}] and bool(torch.isfinite(out["value"]).all())
    assert sa.optimizer(X, sa.group_of(counts), 5)._own is None
    # models of one and the same slice share a stack too; slices of different parents, or a slice next to a whole stack, do not
    same = _study_models(_dicts([case.slices[1]]) * 3, NS, hyper.MaternKernel, 1)
    assert utils.StudiesAcquisition(_afs(same, "ucb")).task_base is None
    mixed = _study_models([_dicts([case.slices[0]])[0], shared, _dicts([case.slices[2]])[0]], NS, hyper.MaternKernel, 1)
    with pytest.raises(ValueError, match="must share one source stack"):
        utils.StudiesAcquisition(_afs(mixed, "ucb"))
