"""scaml_qacqf_opt_f64 (include/scaml_gp.h (7s)) on the MI355X: the device optimiser of the joint q-point acquisition behind
``utils._JointAcquisition.optimize`` / ``ops.QAcqfOpt`` and ``ScaMLGPBOLoop(joint_opt_mode="device")``, on tests/_qacqf_problem's small
problems.  A round's launches are ``value_and_grad``'s, so its values agree with that route to rounding (1e-9 of max |ref| is the
project's bound for two device routes to one joint quantity, tests/test_qacqf_gpu.py); the evaluations scatter by the source pass's
float atomics, so nothing is asserted bit for bit between runs or chunkings; the drivers' optima agree within RTOL_DRIVERS of
tests/test_acqf_opt_gpu.py.  The shapes are the smallest at which something here can go wrong (see CASES)."""
import pytest
import torch

from scamlgp_amd import hyper, ops, utils as U
from scamlgp_amd.bo import ScaMLGPBOLoop
from tests._qacqf_problem import JointProblem

pytestmark = pytest.mark.gpu
ROUTES = 1e-9            # two device routes to one joint quantity, relative to max |ref|
RTOL_DRIVERS = 1e-6      # two drivers of one optimisation (tests/test_acqf_opt_gpu.py)
GTOL, MAX_ITER, MAX_LS, S = 1e-5, 15, 20, 64
RUNNING, CONVERGED, FTOL, STALLED, FAILED, MAXITER = range(6)
RBF, MATERN = 0, 1
#        name              ns            D   n   R  q  p  kinds            what it covers
CASES = [("ragged",        (32, 20, 17), 2,  12, 5, 2, 0, (RBF, RBF)),        # ragged stack, P = 4
         ("both_slots",    (32, 32, 32), 15, 1,  3, 5, 0, (MATERN, MATERN)),  # P = 75: both variables of a lane, n = 1
         ("limits",        (96, 96),     15, 88, 2, 8, 0, (MATERN, RBF)),     # P = 120, n + q = 96: both limits
         ("slot_full",     (32, 32, 32), 8,  8,  3, 8, 0, (RBF, MATERN)),     # P = 64: a lane's first variable exactly
         ("pending",       (32, 20, 17), 2,  10, 5, 2, 3, (RBF, RBF)),        # (7q) in the round
         ("pending_q1",    (32, 32, 32), 15, 1,  3, 1, 7, (MATERN, MATERN))]  # q = 1, q + p = 8
ACQFS = ("qei", "qucb")


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


_BUILT = {}


def _case(name, device):
    """The model of a case (built once per module), its start batches (the last one partly outside the box) and pending points."""
    if name not in _BUILT:
        _, ns, D, n, R, q, p, kinds = next(c for c in CASES if c[0] == name)
        prob = JointProblem(ns, D, n, R, q, kinds[0], kinds[1], seed=40 + len(name))
        stack, model = prob.model(device)
        gen = torch.Generator().manual_seed(7)
        Xp = torch.rand(p, D, dtype=torch.float64, generator=gen) if p else None
        x0 = prob.X.clone()
        x0[-1] = x0[-1] * 1.4 - 0.2
        _BUILT[name] = dict(prob=prob, stack=stack, model=model, Xp=Xp, x0=x0, q=q, p=p, D=D, R=R, afs={}, runs={})
    return _BUILT[name]


def _af(c, which):
    if which not in c["afs"]:
        gen = torch.Generator().manual_seed(3)
        if which == "qei":
            c["afs"][which] = U.qExpectedImprovement(c["model"], c["prob"].best_f(), S, gen, q=c["q"], X_pending=c["Xp"])
        else:
            c["afs"][which] = U.qUpperConfidenceBound(c["model"], 4.0, S, gen, q=c["q"], X_pending=c["Xp"])
    return c["afs"][which]


def _run(c, which, per_call=None):
    key = (which, per_call)
    if key not in c["runs"]:
        c["runs"][key] = _af(c, which).optimize(c["x0"], MAX_ITER, evals_per_call=per_call, gtol=GTOL, max_ls=MAX_LS)
    return c["runs"][key]


@pytest.fixture(scope="module", params=[c[0] for c in CASES])
def case(request, device):
    return _case(request.param, device)


@pytest.mark.parametrize("which", ACQFS)
def test_after_one_round_the_state_holds_the_evaluation_at_the_projected_starts(case, which, device):
    af = _af(case, which)
    R, q, D = case["R"], case["q"], case["D"]
    P = q * D
    kw = case["model"].joint_acqf_opt_inputs(af.base_samples, af._pending)
    lo, hi = torch.zeros(P, dtype=torch.float64, device=device), torch.ones(P, dtype=torch.float64, device=device)
    opt = ops.QAcqfOpt(kw, case["x0"].to(device), af.code, af.param, lo, hi, MAX_ITER, gtol=GTOL)
    opt.enqueue(1)
    state, stats = opt.state().cpu(), opt.stats.cpu()
    xs = case["x0"].clamp(0.0, 1.0)
    v, g = af.value_and_grad(xs.to(device))
    v, g = v.cpu(), g.cpu().reshape(R, P)
    H = 10
    f_state, g_state = state[:, (4 + 2 * H) * P + H], state[:, P:2 * P]
    ef, eg = float((f_state + v).abs().max() / v.abs().max()), float((g_state + g).abs().max() / g.abs().max())
    print(f"{which}: one round: |f + value| / max |value| = {ef:.3e}, |g + grad| / max |grad| = {eg:.3e}")
    assert ef <= ROUTES and eg <= ROUTES
    assert torch.equal(state[:, :P], xs.reshape(R, P)) and torch.equal(opt.x.cpu(), xs.reshape(R, P))     # the clamped start, bit for bit
    assert stats[:, 1].tolist() == [1] * R
    assert state.shape[1] == ops.studies_acqf_opt_state_doubles(P, H)


@pytest.mark.parametrize("which", ACQFS)
def test_a_whole_run_ends_every_start_at_a_point_no_worse_than_its_start(case, which, device):
    af, res = _af(case, which), _run(case, which)
    R, q, D = case["R"], case["q"], case["D"]
    stats, x, f = res["stats"], res["x"].cpu(), res["f"].cpu()
    print(f"{which}: status {stats[:, 2].tolist()}, evaluations {stats[:, 1].tolist()}, rounds {res['n_eval']} in {res['n_calls']} calls, live {res['live']}")
    assert bool((stats[:, 2] != RUNNING).all())
    assert bool((x >= 0.0).all()) and bool((x <= 1.0).all())
    assert res["n_eval"] <= 1 + MAX_ITER * MAX_LS and int(stats[:, 1].max()) <= res["n_eval"]
    v, g = af.value_and_grad(x.to(device))
    v, g = v.cpu(), g.cpu()
    ev = float((f - v).abs().max() / v.abs().max())
    print(f"{which}: |f - value(x)| / max |value| = {ev:.3e}")
    assert ev <= ROUTES
    v0 = af.value_and_grad(case["x0"].clamp(0.0, 1.0).to(device))[0].cpu()
    print(f"{which}: gain over the projected start {(f - v0).tolist()}")
    assert bool((f >= v0 - ROUTES * float(v0.abs().max())).all())
    # a converged start: the projected gradient of the MINIMISED function, g = -grad (tests/test_acqf_opt_gpu.py's rule: the state's
    # gradient met gtol; this one is a second evaluation of it)
    P = q * D
    pg = hyper.projected_gradient(x.reshape(R, P), -g.reshape(R, P), torch.zeros(P, dtype=torch.float64), torch.ones(P, dtype=torch.float64)).abs().amax(-1)
    conv = stats[:, 2] == CONVERGED
    print(f"{which}: converged {int(conv.sum())} of {R}, largest projected gradient among them {float(pg[conv].max()) if bool(conv.any()) else 0.0:.3e}")
    assert bool((pg[conv] <= 2.0 * GTOL).all())


@pytest.mark.parametrize("which", ACQFS)
def test_the_best_value_is_the_host_twins(case, which, device):
    af, res = _af(case, which), _run(case, which)
    R, q, D = case["R"], case["q"], case["D"]

    def fun(z):
        v, g = af.value_and_grad(z.reshape(R, q, D).to(device))
        return -v.cpu(), -g.cpu().reshape(R, q * D)

    ref = hyper.batched_lbfgs(fun, case["x0"].reshape(R, q * D).clone(), max_iter=MAX_ITER, gtol=GTOL, max_ls=MAX_LS, bounds=(0.0, 1.0))
    a, b = float(res["f"].max()), float((-ref.f).max())
    print(f"{which}: best value, device {a:.12f}, host twin {b:.12f}; device status {res['stats'][:, 2].tolist()} evaluations "
          f"{res['stats'][:, 1].tolist()}; host iterations {ref.n_iter} evaluations {ref.n_eval} converged {ref.converged.tolist()}")
    assert abs(a - b) <= RTOL_DRIVERS * max(abs(a), abs(b)), (a, b)


@pytest.mark.parametrize("which", ACQFS)
def test_chunkings_with_compaction_reach_the_same_optimum(case, which, device):
    base = _run(case, which)
    for per_call in (1, 3, 1 + MAX_ITER * MAX_LS):
        res = _run(case, which, per_call)
        a, b = float(res["f"].max()), float(base["f"].max())
        print(f"{which}: evals_per_call {per_call}: best {a:.12f} ({res['n_calls']} calls, live {res['live']}), status {res['stats'][:, 2].tolist()}")
        assert abs(a - b) <= RTOL_DRIVERS * max(abs(a), abs(b)), (per_call, a, b)
        # per start: what converged in the base run converges under every chunking, at the same value (the per-start check of the
        # compaction through the launcher: the relaunch for a changed table, the arrays repacked at the new Bs, the training block)
        conv = base["stats"][:, 2] == CONVERGED
        assert res["stats"][conv, 2].tolist() == [CONVERGED] * int(conv.sum()), (per_call, res["stats"][:, 2].tolist(), base["stats"][:, 2].tolist())
        fr, fb = res["f"].cpu()[conv], base["f"].cpu()[conv]
        assert bool(((fr - fb).abs() <= RTOL_DRIVERS * torch.maximum(fr.abs(), fb.abs())).all()), (per_call, fr.tolist(), fb.tolist())
        assert bool((res["stats"][:, 2] != RUNNING).all())
        assert res["live"] == sorted(res["live"], reverse=True) and res["live"][0] == case["R"]     # the table only shrinks


@pytest.mark.parametrize("which", ACQFS)
def test_a_nonfinite_start_fails_alone_and_a_failed_target_factor_fails_every_start(case, which, device):
    af, good = _af(case, which), _run(case, which)
    R = case["R"]
    x0 = case["x0"].clone()
    x0[0, 0, 0] = float("nan")
    res = af.optimize(x0, MAX_ITER, gtol=GTOL, max_ls=MAX_LS)
    assert res["stats"][0, :3].tolist() == [0, 1, FAILED] and float(res["f"][0]) == -float("inf")
    rest = slice(1, R)
    assert bool((res["stats"][rest, 2] != FAILED).all()) and bool((res["stats"][rest, 2] != RUNNING).all())
    x = torch.where(torch.isnan(res["x"].cpu()), torch.full_like(res["x"].cpu(), 0.5), res["x"].cpu())
    v = af.value_and_grad(x.to(device))[0].cpu()
    ev = float((res["f"].cpu()[rest] - v[rest]).abs().max() / v[rest].abs().max())
    a, b = float(res["f"][rest].max()), float(good["f"][rest].max())
    print(f"{which}: NaN start: the others' |f - value(x)| / max |value| = {ev:.3e}, best {a:.12f} against {b:.12f} without it")
    assert ev <= ROUTES and abs(a - b) <= RTOL_DRIVERS * max(abs(a), abs(b))
    # info[0] != 0: the factor of the target's training block failed
    kw = case["model"].joint_acqf_opt_inputs(af.base_samples, af._pending)
    kw["info"] = torch.ones(1, dtype=torch.int32, device=device)
    P = case["q"] * case["D"]
    lo, hi = torch.zeros(P, dtype=torch.float64, device=device), torch.ones(P, dtype=torch.float64, device=device)
    bad = ops.QAcqfOpt(kw, case["x0"].to(device), af.code, af.param, lo, hi, MAX_ITER, gtol=GTOL).run()
    assert bad["stats"][:, 2].tolist() == [FAILED] * R and bad["n_calls"] == 1


def test_refusals_are_joint_acqfs(device):
    c = _case("ragged", device)
    af = _af(c, "qei")
    with pytest.raises(ValueError):
        c["model"].joint_acqf_opt_inputs(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        c["model"].joint_acqf_opt_inputs(torch.zeros(4, 9, dtype=torch.float64))
    res = af.optimize(torch.empty(0, c["q"], c["D"], dtype=torch.float64), MAX_ITER)
    assert res["x"].shape == (0, c["q"], c["D"]) and res["n_calls"] == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_the_bo_loop_suggests_batches_on_the_device(device):
    prob = JointProblem((32, 32, 32), 2, 12, 1, 3, RBF, RBF, seed=9)
    stack, _ = prob.model(device)
    from scamlgp_amd import model as M
    gps = {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}
    obj = lambda x: float(torch.sin(3.0 * x.sum() / 2 ** 0.5 + 0.5))   # noqa: E731
    for acquisition, score_mode in (("ei", "grad_pass"), ("ucb", "value_pass")):
        loops = {}
        for mode in ("device", "scipy"):
            loop = ScaMLGPBOLoop(gps, 2, acquisition=acquisition, beta=4.0, raw_samples=64, num_restarts=4, af_max_iter=MAX_ITER, seed=5,
                                 num_restarts_log_likelihood=1, max_pending_evaluations=4, joint_pending="joint", joint_score_mode=score_mode,
                                 num_mc_samples=S, joint_opt_mode=mode)
            assert loop.last_suggest_info is None
            loop.record(prob.Xt, [obj(x) for x in prob.Xt])
            loops[mode] = loop
        dev, sci = loops["device"], loops["scipy"]
        for q, pending in ((3, 0), (2, 2)):
            for loop in (dev, sci):
                loop.pending = torch.rand(pending, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
            before = dev.gen.get_state()
            Xd, Xs = dev.suggest_batch(q), sci.suggest_batch(q)
            assert Xd.shape == (q, 2) and bool((Xd >= 0.0).all()) and bool((Xd <= 1.0).all())
            assert torch.equal(dev.gen.get_state(), sci.gen.get_state())
            info = dev.last_suggest_info
            assert set(info) >= {"n_eval", "n_calls", "evals_per_start", "status"} and len(info["status"]) == 4 and 0 not in info["status"]
            assert sci.last_suggest_info == {}
            # the call's own acquisition function and raw batches again (the same draws from the same generator state): the chosen
            # value against the best raw batch, and the scipy twin's next to it
            after = dev.gen.get_state()
            dev.gen.set_state(before)
            af = dev.joint_acquisition_function(q, dev.pending[:pending] if pending else None)
            cand = torch.rand(64, q, 2, dtype=torch.float64, generator=dev.gen)
            dev.gen.set_state(after)   # (the pick's draws followed the raw batches)
            raw = float(af(cand).max())
            vd, vs = (float(v) for v in af(torch.stack([Xd, Xs])).cpu())
            print(f"{acquisition} / {score_mode}: suggest_batch({q}) with {pending} pending: chosen value, device {vd:.12f}, scipy twin {vs:.12f}, "
                  f"best raw batch {raw:.12f}; {info}")
            assert vd >= raw - ROUTES * abs(raw)
