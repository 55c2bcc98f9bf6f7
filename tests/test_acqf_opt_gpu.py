"""The device-side acquisition optimiser on the MI355X (``scaml_studies_acqf_opt_f64`` through ``utils.StudiesAcquisition.optimize`` and
``bo.ScaMLGPBOStudies(suggest_mode="device")``): rounds of grouped source pass + batched acquisition + optimiser step kernel, against
the existing evaluation (``StudiesAcquisition.value_and_grad``), the host driver (``hyper.batched_lbfgs(bounds=(0, 1))`` around that
evaluation, which is what ``suggest_mode="lockstep"`` runs) and a lock-step twin.  The step kernel's arithmetic is held to the host
optimiser bit for bit on the CPU (tests/test_acqf_opt_emul.py); here the evaluations come from the source pass, whose LDS float atomics
scatter by about 1e-15 from run to run, so nothing is asserted bit for bit between runs or chunkings.

Bounds.  1e-11 of max |ref| between two evaluations of the same points (tests/test_studies_acqf_gpu.py: SCATTER_MAX, derived there from
the atomics); rtol = 1e-6 between the best end values of two drivers of the same optimiser (tests/test_stack_fit_emul.py's between the two
stack-fit drivers); 2 gtol on the projected gradient of a converged start (gtol on the state's own gradient, the re-evaluated one
differs by the scatter).

Stacks: the golden rbf stack c1_branin_T4_N32_rbf and the ragged Matern stack edge_ragged_T4_N48_matern (both D = 2), G = 3 studies of
ragged sizes, 4 starts per study plus one padding row, max_iter <= 20, UCB and EI.  A study's n is bounded by the stack's N (the source
pass keeps the covariance tiles in the task's LDS strip), so the study sizes are (1, 17, N) on the golden stacks -- (1, 17, 32) and
(1, 17, 48) -- and the sizes (1, 17, 96), with n = 96 the kernels' limit, run on the N = 96 Hartmann-6 stack of
tests/test_studies_acqf_gpu.py (D = 6).

Measured on the MI355X (every figure is printed before it is asserted; ``pytest -s tests/test_acqf_opt_gpu.py`` shows them): the state after one round against ``value_and_grad`` 0 ..
9.2e-16 of max |ref|, ``f`` against the value at ``x`` 0 .. 2.3e-15, the projected gradient of converged starts at most 7.5e-6, the best
end value per study against the host driver's equal to 1e-13 relative or better, the chosen acquisition values of the device mode and
its lock-step twin equal to the 12 digits printed."""
import os

import numpy as np
import pytest
import torch

from scamlgp_amd import hyper, model as M, ops, utils
from scamlgp_amd.bo import ScaMLGPBOLoop, ScaMLGPBOStudies
from tests.test_studies_acqf_gpu import _afs, _hartmann_gps, _models, _ragged_gps

pytestmark = pytest.mark.gpu
SCATTER = 1e-11
RTOL_DRIVERS = 1e-6
GTOL, MAX_ITER, MAX_LS = 1e-5, 20, 20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNNING, CONVERGED, FTOL, STALLED, FAILED, MAXITER, PADDING = range(7)
COUNTS = (4, 4, 4)


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


def _branin_gps(device):
    d = np.load(os.path.join(GOLDEN, "c1_branin_T4_N32_rbf.npz"))
    T = d["X"].shape[0]
    X = [torch.from_numpy(d["X"][t]) for t in range(T)]
    Y = [torch.from_numpy(d["y"][t] * d["y_std"][t] + d["y_mean"][t]).unsqueeze(-1) for t in range(T)]
    stack = M.SourceGPStack([f"b{t}" for t in range(T)], X, Y, kind=int(d["kind"]), device=device)
    stack.set_theta(torch.from_numpy(d["theta"]))
    stack.refresh()
    return {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}


CASES = {
    "branin_rbf": (_branin_gps, (1, 17, 32), hyper.RBFKernel, (1, 0)),
    "ragged_matern": (_ragged_gps, (1, 17, 48), hyper.MaternKernel, (2, 1)),
    "hartmann_n96": (lambda dev: _hartmann_gps(dev, T=2, N=96), (1, 17, 96), hyper.RBFKernel, (1, 0)),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, device):
    """The models of one stack, the starts (some outside the box) and the group table with one padding row inside; shared, unchanged."""
    make, ns, kernel, prune = CASES[request.param]
    models = _models(make(device), ns, kernel, seed=21, prune=prune)
    D = models[0]._stack.D
    g = torch.Generator().manual_seed(22)
    X0 = torch.rand(sum(COUNTS) + 1, D, dtype=torch.float64, generator=g) * 1.4 - 0.2
    group = torch.tensor([0] * 4 + [1] * 2 + [-1] + [1] * 2 + [2] * 4, dtype=torch.int32)
    return dict(models=models, X0=X0, group=group, D=D)


def _sa(case, which):
    return utils.StudiesAcquisition(_afs(case["models"], which))


def _best_per_study(values, group, G):
    return [float(values[group == g].max()) for g in range(G)]


@pytest.mark.parametrize("which", ["ucb", "ei"])
def test_one_round_after_reset_holds_the_evaluation_at_the_projected_starts(case, device, which):
    sa, X0, group, D = _sa(case, which), case["X0"], case["group"].to(device), case["D"]
    run = sa.optimizer(X0, group, MAX_ITER)
    run.enqueue(1)
    st = run.state().cpu()
    stats = run.stats.cpu()
    proj = X0.clamp(0.0, 1.0)
    v, gr = sa.value_and_grad(proj.to(device), group)
    v, gr = v.cpu(), gr.cpu()
    real = (group >= 0).cpu()
    f_state, g_state = st[:, (4 + 20) * D + 10 + 0], st[:, D:2 * D]   # scalars open after x, g, d, xt, S, Y (history 10) and rho
    assert ops.studies_acqf_opt_state_doubles(D, 10) == st.shape[1]
    ef = float((f_state[real] + v[real]).abs().max()) / float(v[real].abs().max())
    eg = float((g_state[real] + gr[real]).abs().max()) / float(gr[real].abs().max())
    print(f"{which}: state f against -value {ef:.3e}, state g against -grad {eg:.3e}")
    assert ef <= SCATTER and eg <= SCATTER
    assert torch.equal(st[:, :D], proj)                      # the accepted point is the projected start
    assert stats[real, 1].tolist() == [1] * int(real.sum())    # one evaluation each
    assert stats[~real].tolist() == [[0, 0, PADDING, 0]]
    assert torch.equal(run.x.cpu()[~real], proj[~real])


@pytest.mark.parametrize("which", ["ucb", "ei"])
def test_a_whole_optimisation(case, device, which):
    sa, X0, group, D = _sa(case, which), case["X0"], case["group"].to(device), case["D"]
    gh = group.cpu()
    real = gh >= 0
    res = sa.optimize(X0, group, MAX_ITER)
    x, f, stats = res["x"].cpu(), res["f"].cpu(), res["stats"]
    print(f"{which}: rounds {res['n_eval']} in {res['n_calls']} calls; per start (it, evals, status, pairs) {stats.tolist()}")
    assert not bool((stats[:, 2] == RUNNING).any())
    assert bool(((x >= 0.0) & (x <= 1.0)).all())
    assert int(stats[:, 1].max()) <= 1 + MAX_ITER * MAX_LS and res["n_eval"] <= 1 + MAX_ITER * MAX_LS
    assert stats[~real].tolist() == [[0, 0, PADDING, 0]] and torch.equal(x[~real], X0.clamp(0.0, 1.0)[~real])
    assert bool((stats[real, 2] != FAILED).all()) and bool((stats[real, 2] != PADDING).all())
    # f is the acquisition value AT x (the evaluation made when x was accepted), and no worse than the projected start's
    v, gr = sa.value_and_grad(x.to(device), group)
    v, gr = v.cpu(), gr.cpu()
    scale = float(v[real].abs().max())
    err = float((f[real] - v[real]).abs().max()) / scale
    print(f"{which}: f against the value at x {err:.3e}")
    assert err <= SCATTER
    v0 = sa.value(X0.clamp(0.0, 1.0).to(device), group).cpu()
    assert bool((f[real] >= v0[real] - SCATTER * float(v0[real].abs().max())).all())
    # a converged start: the projected gradient of the MINIMISED function, g = -grad
    pg = hyper.projected_gradient(x, -gr, torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)).abs().amax(-1)
    conv = stats[:, 2] == CONVERGED
    print(f"{which}: converged {int(conv.sum())} of {int(real.sum())}, largest projected gradient among them {float(pg[conv].max()) if bool(conv.any()) else 0.0:.3e}")
    assert bool((pg[conv] <= 2.0 * GTOL).all())
    # the host driver from the same starts: what suggest_mode="lockstep" runs
    def fun(xh):
        vv, gg = sa.value_and_grad(xh.to(device), group)
        return -vv.cpu(), -gg.cpu()

    ref = hyper.batched_lbfgs(fun, X0, max_iter=MAX_ITER, bounds=(0.0, 1.0))
    best_dev, best_host = _best_per_study(f, gh, sa.G), _best_per_study(-ref.f, gh, sa.G)
    print(f"{which}: best per study, device {best_dev}, host {best_host}; host evaluations {ref.n_eval}")
    for a, b in zip(best_dev, best_host):
        assert abs(a - b) <= RTOL_DRIVERS * max(abs(a), abs(b)), (a, b)


def test_chunking_reaches_the_same_optimum(case, device):
    """1, 3 and all rounds per call: the same statuses' worth of work, end values within the drivers' tolerance (not bit for bit)."""
    sa, X0, group = _sa(case, "ucb"), case["X0"], case["group"].to(device)
    gh = group.cpu()
    base = None
    for per_call in (1, 3, 1 + MAX_ITER * MAX_LS):
        res = sa.optimize(X0, group, MAX_ITER, evals_per_call=per_call)
        assert not bool((res["stats"][:, 2] == RUNNING).any())
        assert res["n_calls"] == (1 if per_call > 3 else -(-res["n_eval"] // per_call))
        best = _best_per_study(res["f"].cpu(), gh, sa.G)
        base = base or best
        for a, b in zip(best, base):
            assert abs(a - b) <= RTOL_DRIVERS * max(abs(a), abs(b)), (per_call, a, b)


def test_a_failed_study_fails_its_starts_and_leaves_the_others_alone(case, device):
    sa, X0, group = _sa(case, "ucb"), case["X0"], case["group"].to(device)
    gh = group.cpu()
    good = sa.optimize(X0, group, MAX_ITER)
    sa.info[1] = 3
    bad = sa.optimize(X0, group, MAX_ITER)
    st = bad["stats"]
    assert st[gh == 1, 2].tolist() == [FAILED] * 4 and st[gh == 1, 1].tolist() == [1] * 4
    assert torch.equal(bad["x"].cpu()[gh == 1], X0.clamp(0.0, 1.0)[gh == 1])
    assert bool(torch.isinf(bad["f"].cpu()[gh == 1]).all())
    assert st[gh == -1].tolist() == [[0, 0, PADDING, 0]]
    for g in (0, 2):
        assert bool((st[gh == g, 2] != FAILED).all()) and bool((st[gh == g, 2] != RUNNING).all())
        a, b = float(bad["f"].cpu()[gh == g].max()), float(good["f"].cpu()[gh == g].max())
        assert abs(a - b) <= RTOL_DRIVERS * max(abs(a), abs(b)), (g, a, b)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
KW = dict(acquisition="ucb", num_restarts_log_likelihood=2, raw_samples=64, num_restarts=4, af_max_iter=20)


def _obj(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return float(np.sin(3.0 * x.sum()) + ((x - 0.3) ** 2).sum())


def test_device_suggest_next_to_a_lockstep_twin(device):
    gps = _branin_gps(device)
    S, DIM, seeds = 3, 2, [31, 32, 33]
    dev_side = ScaMLGPBOStudies(gps, DIM, S, seeds=seeds, suggest_mode="device", **KW)
    twin = ScaMLGPBOStudies(gps, DIM, S, seeds=seeds, suggest_mode="lockstep", **KW)
    g = torch.Generator().manual_seed(0)
    init = {s: torch.rand(2 + 3 * s, DIM, dtype=torch.float64, generator=g) for s in (1, 2)}   # study 0 starts without data: its own path
    for side in (dev_side, twin):
        side.report_some({s: (x, [_obj(r) for r in x]) for s, x in init.items()})
    for step in range(3):
        Xd, Xt = dev_side.suggest(), twin.suggest()
        info = dev_side.last_suggest_info
        assert info["batched"] == twin.last_suggest_info["batched"] == ([1, 2] if step == 0 else [0, 1, 2])
        assert bool(((Xd >= 0.0) & (Xd <= 1.0)).all())
        nb = 4 * len(info["batched"])
        assert len(info["evals_per_start"]) == nb and max(info["evals_per_start"]) <= info["n_eval"] <= 1 + 20 * 20
        assert all(s not in (RUNNING, PADDING) for s in info["status"]) and info["n_calls"] >= 1
        print(f"step {step}: device rounds {info['n_eval']} ({info['n_calls']} calls), evaluations per start {info['evals_per_start']}; "
              f"lock-step evaluations {twin.last_suggest_info['n_eval']}")
        for s in range(S):
            assert torch.equal(dev_side[s].gen.get_state(), twin[s].gen.get_state()), (step, s)
            if s not in info["batched"]:
                continue
            af = twin[s].acquisition_function()      # (the two sides' models are the same: both are told the twin's points below)
            v = af(torch.stack([Xd[s], Xt[s]]).to(device)).cpu()
            print(f"step {step} study {s}: chosen value, device {float(v[0]):.12f}, lock-step {float(v[1]):.12f}")
            assert abs(float(v[0]) - float(v[1])) <= RTOL_DRIVERS * max(abs(float(v[0])), abs(float(v[1])))
        ys = [_obj(x) for x in Xt]
        dev_side.report(Xt, ys)
        twin.report(Xt, ys)


def test_one_study_and_a_pending_evaluation(device, monkeypatch):
    gps = _branin_gps(device)
    one = ScaMLGPBOStudies(gps, 2, 1, seeds=[5], suggest_mode="device", **KW)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(5, 2, dtype=torch.float64, generator=g)
    one.report_some({0: (x, [_obj(r) for r in x])})
    X = one.suggest()
    assert X.shape == (1, 2) and bool(((X >= 0.0) & (X <= 1.0)).all())
    assert one.last_suggest_info["batched"] == [0] and len(one.last_suggest_info["evals_per_start"]) == 4
    # a study with a pending evaluation is a fantasy model: its own suggest(), in the same call
    par = ScaMLGPBOStudies(gps, 2, 3, seeds=[6, 7, 8], suggest_mode="device", max_pending_evaluations=2, num_fantasies=8, **KW)
    par.report_some({s: (x, [_obj(r) for r in x]) for s in range(3)})
    X = par.suggest()
    assert par.last_suggest_info["batched"] == [0, 1, 2]
    par.report_some({s: (X[s], _obj(X[s])) for s in (0, 2)})     # study 1's evaluation stays pending
    calls = []
    plain = ScaMLGPBOLoop.suggest
    monkeypatch.setattr(ScaMLGPBOLoop, "suggest", lambda self: (calls.append(self), plain(self))[1])
    X = par.suggest()
    assert [par.studies.index(st) for st in calls] == [1] and par.last_suggest_info["batched"] == [0, 2]
    assert bool(((X >= 0.0) & (X <= 1.0)).all())
