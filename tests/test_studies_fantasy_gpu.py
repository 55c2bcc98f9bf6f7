"""Studies with pending evaluations in the batched acquisition on the MI355X: ``utils.StudiesAcquisition`` on a mix of ordinary and
fantasy models (scaml_target_fantasy_acqf_batched_f64 / scaml_target_fantasy_score_batched_f64 behind the grouped source passes), the
device optimiser on it (scaml_studies_fantasy_acqf_opt_f64) and ``bo.ScaMLGPBOStudies(pending_mode="batched")`` next to a
``"per_study"`` twin.

Evaluation.  The mix is (n, p, F) = (1, 1, 2), (14, 3, 8), (16, 1, 63), (40, 0, -) on the stacks of tests/test_studies_acqf_gpu.py --
Hartmann-6 (T = 2, N = 64, Matern-5/2) and the ragged golden stack with an RBF target kernel -- and (92, 4, 64) with an ordinary n = 5
on its N = 96 stack.  The reference is each study's own ``af.value_and_grad``: (7f) for a fantasy model.  That file's construction: the
own path is measured against itself first (the source pass adds the waves' shares of a mean with LDS float atomics), printed and held
under SCATTER_MAX = 1e-11; then the batch is held within BOUND = 1e-10 of max |ref| per quantity, UCB and EI, eager and through
``GraphedAcquisition``.

Bit for bit.  The F = 1 rule -- an ordinary study in a mixed launch gets the bits of (7g) -- and score == value are properties of the
target kernels: they hold for the same per-task numbers, and two source-pass launches do not deliver the same numbers (the scatter
above; tests/test_studies_score_gpu.py compares the two layouts on the same device inputs for that reason).  So ONE grouped source pass
feeds both sides here: its outputs go to the new kernel with the mixed set's arrays and, sliced to the ordinary studies' rows, to
``ops.target_acqf_batched`` with the arrays of an all-ordinary ``StudiesAcquisition``; column 0 of the same pass, re-laid as strips,
goes to the strip kernel.  ``torch.equal`` on value and gradient.  The same comparisons through two ``StudiesAcquisition`` calls (each
with its own source pass) are printed and held within SCATTER_MAX, resp. BOUND for ``score`` (another instance of the pass).

Every figure is printed before it is asserted (``pytest -s``); profiles/studies_pending_notes.md records them."""
import pytest
import torch

from scamlgp_amd import bo, hyper, ops, utils
from scamlgp_amd.bo import GraphedAcquisition, OptimizerNotReady, ScaMLGPBOLoop, ScaMLGPBOStudies
from tests.test_acqf_opt_gpu import MAX_ITER, MAX_LS, PADDING, RTOL_DRIVERS, RUNNING
from tests.test_studies_acqf_gpu import BOUND, SCATTER_MAX, _afs, _hartmann_gps, _models, _ragged_gps, _rel
from tests.test_studies_lockstep_gpu import KW, _gps, _obj

pytestmark = pytest.mark.gpu

MIX = ((1, 1, 2), (14, 3, 8), (16, 1, 63), (40, 0, None))
CASES = {
    "hartmann_matern": (_hartmann_gps, MIX, hyper.MaternKernel, (1, 0)),
    "ragged_rbf": (_ragged_gps, MIX, hyper.RBFKernel, (2, 1)),
    "hartmann_n96": (lambda dev: _hartmann_gps(dev, T=2, N=96), ((92, 4, 64), (5, 0, None)), hyper.RBFKernel, (1, 0)),
}


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, device):
    """The models of one stack -- ordinary ones, of which those with p > 0 are then conditioned on F fantasies of p pending points --,
    shared and unchanged."""
    make, mix, kernel, prune = CASES[request.param]
    # (seed: one under which every noise ``_models`` draws, 1e-3 + 1e-2 u, lies inside the likelihood's interval (.., 1e-2) on all three
    # stacks -- beyond it the raw value, and with it the study, is NaN on every path)
    base = _models(make(device), [n for n, _, _ in mix], kernel, seed=42, prune=prune)
    assert all(bool(torch.isfinite(m.theta).all()) for m in base)
    g = torch.Generator().manual_seed(42)
    D = base[0]._stack.D
    models = []
    for m, (n, p, F) in zip(base, mix):
        if p:
            m = m.fantasize(torch.rand(p, D, dtype=torch.float64, generator=g), F, generator=g).eval()
            assert m.num_fantasies == F and m.n == n + p
        models.append(m)
    return dict(models=models, mix=mix, D=D, name=request.param)


@pytest.mark.parametrize("which", ["ucb", "ei"])
def test_batched_evaluation_matches_each_study(case, device, which):
    models, D = case["models"], case["D"]
    counts = [3 + (s % 2) for s in range(len(models))]
    g = torch.Generator().manual_seed(43)
    Xs = [torch.rand(c, D, dtype=torch.float64, generator=g).to(device) for c in counts]
    afs = _afs(models, which)
    refs, scatter = [], 0.0
    for af, x in zip(afs, Xs):
        a, b = af.value_and_grad(x), af.value_and_grad(x)
        scatter = max(scatter, _rel(a[0], b[0]), _rel(a[1], b[1]))
        refs.append(a)
    print(f"{case['name']} {which}: own path against itself {scatter:.3e}")
    assert scatter <= SCATTER_MAX
    sa = utils.StudiesAcquisition(afs)
    assert sa.fantasy and sa.n_fant.tolist() == [F or 1 for _, _, F in case["mix"]] and sa.n_points.tolist() == [n + p for n, p, _ in case["mix"]]
    group = sa.group_of(counts)
    X = torch.cat(Xs)
    v, gr = sa.value_and_grad(X, group)
    graphed = GraphedAcquisition(lambda x: sa.value_and_grad(x, group), X.shape[0], D, device)
    vg, gg = graphed(X)
    torch.cuda.synchronize()
    for s, (ref, m) in enumerate(zip(refs, models)):
        for k, got, rep, want in (("value", v, vg, ref[0]), ("grad", gr, gg, ref[1])):
            err, err_g = _rel(got.split(counts)[s], want), _rel(rep.split(counts)[s], want)
            print(f"{case['name']} {which} study {s} (n' = {m.n}, F = {m.num_fantasies}) {k}: eager {err:.3e}, graph replay {err_g:.3e}")
            assert err <= BOUND and err_g <= BOUND, (which, s, k, err, err_g)
    assert _rel(sa.value(X, group), v) <= SCATTER_MAX   # value only: the same numbers
    with pytest.raises(ValueError):
        sa.evaluate(X, group, want_posterior=True)


@pytest.mark.parametrize("which", ["ucb", "ei"])
def test_ordinary_studies_and_strips_bit_for_bit_on_one_source_pass(case, device, which):
    models, D = case["models"], case["D"]
    G = len(models)
    afs = _afs(models, which)
    sa = utils.StudiesAcquisition(afs)
    ordinary = [s for s, m in enumerate(models) if m.num_fantasies is None]
    sa_ord = utils.StudiesAcquisition([afs[s] for s in ordinary])
    assert not sa_ord.fantasy and sa_ord.alpha_f is None
    g = torch.Generator().manual_seed(44)
    X = torch.rand(16 * G, D, dtype=torch.float64, generator=g).to(device)   # a strip of 16 per study
    group = sa.group_of([16] * G)
    st, f = sa.source, sa.source.fit
    src = ops.source_posteriors_grad_grouped(X, group, sa.Xt, sa.n_points, sa.VA_tab, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean,
                                             st.y_std, st.n_points)
    tail = (sa.n_points, sa.m_all, sa.s_all, sa.info, sa.acqf_param, sa.acqf, sa.kind)
    mixed = ops.target_fantasy_acqf_batched(src["mu"], src["var"], src["cov"], group, X, sa.w, sa.active, sa.Xt, sa.theta, sa.L, sa.Linv_diag,
                                            sa.alpha_f, sa.n_fant, *tail)
    # the ordinary studies' rows of the SAME pass under (7g), with the arrays of the all-ordinary set
    rows = torch.cat([torch.arange(16 * s, 16 * s + 16) for s in ordinary]).to(device)
    T, nm = sa.w.shape[1], sa_ord.n_max
    cov = src["cov"].reshape(T, sa.n_max, 16 * G, 16)[:, :nm][:, :, rows].reshape(T, nm, -1).contiguous()
    plain = ops.target_acqf_batched(src["mu"][:, rows].contiguous(), src["var"][:, rows].contiguous(), cov, sa_ord.group_of([16] * len(ordinary)),
                                    X[rows].contiguous(), sa_ord.w, sa_ord.active, sa_ord.Xt, sa_ord.theta, sa_ord.L, sa_ord.Linv_diag, sa_ord.alpha,
                                    sa_ord.n_points, sa_ord.m_all, sa_ord.s_all, sa_ord.info, sa_ord.acqf_param, sa_ord.acqf, sa_ord.kind)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain["value"]).all()) and bool(torch.isfinite(plain["grad"]).all())
    assert torch.equal(mixed["value"][rows], plain["value"]) and torch.equal(mixed["grad"][rows], plain["grad"])
    # column 0 of the same pass as strips: the strip kernel's values are the query kernel's
    cov0 = src["cov"].reshape(T, sa.n_max, 16 * G, 16)[..., 0].contiguous()
    strips = ops.target_fantasy_score_batched(src["mu"][..., 0].contiguous(), src["var"][..., 0].contiguous(), cov0,
                                              torch.arange(G, dtype=torch.int32, device=device), X, sa.w, sa.active, sa.Xt, sa.theta, sa.L,
                                              sa.Linv_diag, sa.alpha_f, sa.n_fant, *tail)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mixed["value"]).all()) and torch.equal(strips["value"], mixed["value"])
    # through the public calls, each with a source pass of its own: within the pass's scatter, resp. the bound between two instances of it
    pub = sa.evaluate(X, group)
    pub_ord = sa_ord.evaluate(X[rows], sa_ord.group_of([16] * len(ordinary)))
    e1 = max(_rel(pub["value"][rows], pub_ord["value"]), _rel(pub["grad"][rows], pub_ord["grad"]))
    e2 = _rel(sa.score(X, torch.arange(G, dtype=torch.int32, device=device))["value"], sa.value(X, group))
    print(f"{case['name']} {which}: ordinary studies, mixed against all-ordinary call {e1:.3e}; score against value {e2:.3e}")
    assert e1 <= SCATTER_MAX and e2 <= BOUND


def _starts(case, device):
    G, D = len(case["models"]), case["D"]
    sa = utils.StudiesAcquisition(_afs(case["models"], "ucb"))
    g = torch.Generator().manual_seed(45)
    X0 = torch.rand(3 * G + 1, D, dtype=torch.float64, generator=g) * 1.4 - 0.2
    per = [s for s in range(G) for _ in range(3)]
    gh = torch.tensor(per[:4] + [-1] + per[4:], dtype=torch.int32)   # a padding row inside
    return sa, X0, gh, gh.to(device)


def test_device_optimiser_on_the_mixed_set(case, device):
    """From identical starts: the end values of scaml_studies_fantasy_acqf_opt_f64 against ``hyper.batched_lbfgs(bounds=...)`` driven by
    the new evaluation (RTOL_DRIVERS of tests/test_acqf_opt_gpu.py, best end value per study)."""
    sa, X0, gh, group = _starts(case, device)
    G = sa.G
    full = sa.optimize(X0, group, MAX_ITER)
    x, f, stats = full["x"].cpu(), full["f"].cpu(), full["stats"]
    real = gh >= 0
    print(f"{case['name']}: rounds {full['n_eval']} in {full['n_calls']} calls; statuses {stats[:, 2].tolist()}")
    assert not bool((stats[:, 2] == RUNNING).any()) and stats[~real].tolist() == [[0, 0, PADDING, 0]]
    assert bool(((x >= 0.0) & (x <= 1.0)).all()) and bool(torch.isfinite(f[real]).all())
    err = _rel(f[real], sa.value(x.to(device), group).cpu()[real])
    print(f"{case['name']}: f against the value at x {err:.3e}")
    assert err <= SCATTER_MAX


    def fun(xh):
        vv, gg = sa.value_and_grad(xh.to(device), group)
        return -vv.cpu(), -gg.cpu()

    ref = hyper.batched_lbfgs(fun, X0, max_iter=MAX_ITER, bounds=(0.0, 1.0))
    for s in range(G):
        a, b = float(f[gh == s].max()), float((-ref.f)[gh == s].max())
        print(f"{case['name']} study {s}: best end value, device {a:.12f}, host driver {b:.12f}")
        assert abs(a - b) <= RTOL_DRIVERS * max(abs(a), abs(b)), (s, a, b)


def test_chunking_one_and_all_evaluations_per_call_agree_bit_for_bit(case, device):
    """One evaluation per call against all of them in one call: x, f and stats bit for bit.  The rounds of
    scaml_studies_fantasy_acqf_opt_f64 run the grouped GRAD pass in its instantiation with ordered sums (DET of csrc/gp_posterior.hip:
    the waves' shares of a mean and of a variance are added in wave order, not with LDS float atomics), the acquisition launch and the
    step kernel are pure functions of their inputs, so a round is one of the state and the chunking cannot show.  (With the pass of
    (7h), whose atomics arrive in another order from run to run, the two chunkings differed by 6e-15 in x and 2e-14 in f, and so did
    two runs of ONE chunking of (7h) itself: profiles/studies_pending_notes.md.)"""
    sa, X0, gh, group = _starts(case, device)
    one = sa.optimize(X0, group, MAX_ITER, evals_per_call=1)
    full = sa.optimize(X0, group, MAX_ITER, evals_per_call=1 + MAX_ITER * MAX_LS)
    real = gh >= 0
    dx = float((one["x"].cpu() - full["x"].cpu()).abs().max())
    df = float((one["f"].cpu()[real] - full["f"].cpu()[real]).abs().max())
    print(f"{case['name']}: chunking 1 ({one['n_calls']} calls) against all in one call: max |dx| {dx:.3e}, max |df| {df:.3e}, "
          f"stats equal {torch.equal(one['stats'], full['stats'])}")
    assert one["n_calls"] == one["n_eval"] and full["n_calls"] == 1
    assert torch.equal(one["stats"], full["stats"])
    assert torch.equal(one["x"], full["x"]) and torch.equal(one["f"], full["f"])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
S, DIM, SEEDS = 3, 6, [51, 52, 53]


def _spies(monkeypatch):
    """What a suggest() did: the studies that took ScaMLGPBOLoop.suggest, every acquisition function built (per study), and the best raw
    candidate of every final choice (in the order of the batch)."""
    calls, afs, raws = [], {}, []
    plain, build, final = ScaMLGPBOLoop.suggest, ScaMLGPBOLoop.acquisition_function, bo.acqf_final_choice
    monkeypatch.setattr(ScaMLGPBOLoop, "suggest", lambda self: (calls.append(self), plain(self))[1])
    monkeypatch.setattr(ScaMLGPBOLoop, "acquisition_function", lambda self: afs.setdefault(id(self), build(self)))
    monkeypatch.setattr(bo, "acqf_final_choice", lambda cand, vals, best0, xs, fin: (raws.append(cand[best0]), final(cand, vals, best0, xs, fin))[1])
    return calls, afs, raws


@pytest.mark.parametrize("suggest_mode, score_mode", [("lockstep", "per_study"), ("device", "batched")])
def test_pending_studies_stay_in_the_batch_next_to_a_per_study_twin(device, monkeypatch, suggest_mode, score_mode):
    gps = _gps(device)
    assert KW["max_pending_evaluations"] == 2 and KW["num_fantasies"] == 8
    mk = lambda mode: ScaMLGPBOStudies(gps, DIM, S, seeds=SEEDS, suggest_mode=suggest_mode, score_mode=score_mode, pending_mode=mode, **KW)   # noqa: E731
    bat, twin = mk("batched"), mk("per_study")
    assert ScaMLGPBOStudies(gps, DIM, S, seeds=SEEDS, suggest_mode=suggest_mode, **KW).pending_mode == "per_study"
    with pytest.raises(ValueError):
        ScaMLGPBOStudies(gps, DIM, S, seeds=SEEDS, pending_mode="batched", **KW)          # the sequential mode runs every study on its own
    with pytest.raises(ValueError):
        ScaMLGPBOStudies(gps, DIM, S, seeds=SEEDS, suggest_mode=suggest_mode, pending_mode="all", **KW)
    g = torch.Generator().manual_seed(0)
    init = {s: torch.rand(3 + s, DIM, dtype=torch.float64, generator=g) for s in range(S)}
    for side in (bat, twin):
        side.report_some({s: (x, [_obj(r) for r in x]) for s, x in init.items()})
    calls, afs, raws = _spies(monkeypatch)
    held = {}
    for step in range(3):
        pend = [s for s in range(S) if bat[s].pending.shape[0] > 0]
        assert pend == ([] if step == 0 else [1]) and [twin[s].pending.shape[0] for s in range(S)] == [bat[s].pending.shape[0] for s in range(S)]
        before = [st.pending.shape[0] for st in bat.studies]
        calls.clear(), afs.clear(), raws.clear()
        Xb = bat.suggest()
        info = bat.last_suggest_info
        assert calls == [] and info["batched"] == list(range(S)), (step, info["batched"])   # study 1 with its pending point included
        assert [st.pending.shape[0] for st in bat.studies] == [b + 1 for b in before]
        assert bool(((Xb >= 0.0) & (Xb <= 1.0)).all())
        for i, s in enumerate(info["batched"]):
            af = afs[id(bat[s])]
            assert (af.model.num_fantasies == 8) == (s in pend)
            v = af(torch.stack([Xb[s], raws[i]]).to(device)).cpu()
            print(f"{suggest_mode} step {step} study {s} (pending {before[s]}): af(suggestion) = {float(v[0]):.12f}, af(best raw candidate) = {float(v[1]):.12f}")
            assert float(v[0]) >= float(v[1]) - 1e-9 * max(1.0, abs(float(v[1])))
        calls.clear(), afs.clear(), raws.clear()
        Xt = twin.suggest()
        assert [twin.studies.index(st) for st in calls] == pend and twin.last_suggest_info["batched"] == [s for s in range(S) if s not in pend]
        assert set(info) == set(twin.last_suggest_info)
        for s in range(S):
            assert torch.equal(bat[s].gen.get_state(), twin[s].gen.get_state()), (step, s)
        # both sides are told the twin's points; study 1's evaluation of step 0 stays pending to the end
        for s in range(S):
            bat[s].pending = twin[s].pending.clone()
        evals = {s: (Xt[s], _obj(Xt[s])) for s in range(S)}
        if step == 0:
            held[1] = evals.pop(1)
        for side in (bat, twin):
            side.report_some(evals)
    # OptimizerNotReady as in the default mode: study 1 holds two pending points now
    monkeypatch.undo()
    for side in (bat, twin):
        side[1].pending = torch.cat([side[1].pending, torch.rand(1, DIM, dtype=torch.float64)])
        before = [st.pending.shape[0] for st in side.studies]
        with pytest.raises(OptimizerNotReady):
            side.suggest()
        assert [st.pending.shape[0] for st in side.studies] == [before[0] + 1, before[1], before[2]]


def test_a_study_beyond_96_points_falls_back(device, monkeypatch):
    """n + p = 97: the decision is made before the fantasies are drawn, the study takes its own ScaMLGPBOLoop.suggest() once and its
    generator ends where the twin's does."""
    gps = _hartmann_gps(device, T=2, N=96)
    kw = dict(KW, raw_samples=32, num_restarts=2, af_max_iter=3, num_restarts_log_likelihood=0)
    bat = ScaMLGPBOStudies(gps, DIM, 2, seeds=[61, 62], suggest_mode="device", pending_mode="batched", **kw)
    twin = ScaMLGPBOStudies(gps, DIM, 2, seeds=[61, 62], suggest_mode="device", **kw)
    g = torch.Generator().manual_seed(1)
    init = {0: torch.rand(96, DIM, dtype=torch.float64, generator=g), 1: torch.rand(4, DIM, dtype=torch.float64, generator=g)}
    pend = torch.rand(1, DIM, dtype=torch.float64, generator=g)
    for side in (bat, twin):
        side.report_some({s: (x, [_obj(r) for r in x]) for s, x in init.items()})
        side[0].pending = pend.clone()   # 96 + 1
        side[1].pending = pend.clone()   # 4 + 1
    assert not bat._takes_study(bat[0]) and bat._takes_study(bat[1]) and not twin._takes_study(twin[1])
    calls, _, _ = _spies(monkeypatch)
    bat.suggest()
    assert [bat.studies.index(st) for st in calls] == [0] and bat.last_suggest_info["batched"] == [1]
    calls.clear()
    twin.suggest()
    assert [twin.studies.index(st) for st in calls] == [0, 1] and twin.last_suggest_info["batched"] == []
    for s in range(2):
        assert torch.equal(bat[s].gen.get_state(), twin[s].gen.get_state()), s
