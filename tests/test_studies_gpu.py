"""ScaMLGPBOStudies on the MI355X: S = 4 studies on a c5r-shaped stack (Hartmann-6, T = 2, N = 64, Matern-5/2) stepped in lock-step,
against four ScaMLGPBOLoops fed the same initial designs, the same evaluations and the same random draws -- study 1 gets a report
without an objective value, study 2 leaves an evaluation pending for two steps (its next suggestions come from a fantasy model).

Both sides see the same data at every step (the single loops are handed the studies' points, which theirs must match to the 1e-6
that tests/test_fantasy_gpu.py allows two runs of one loop), and the same samples: a single loop draws its restart samples from the
global RNG, which is set to the stream of the study's ``fit_gens`` entry around its report.  The refit itself is bit-identical per
problem (tests/test_target_fit_batched_gpu.py), so the fitted state is held to the 1e-10 that tests/test_model_gpu.py and
tests/test_fantasy_gpu.py allow a model rebuilt from the same data.

"The same data" has to hold bit for bit for that.  The source pass adds the waves' shares of a posterior mean with LDS float atomics,
so two evaluations at the same points differ in the last bits (measured on this stack: 1e-15 in the source means of a training set,
covariances equal), and on three to nine points the objective is flat along the raw outputscale (fitted values of -26 .. -36, i.e. an
outputscale of 0), where 40 - 100 L-BFGS iterations blow a last-bit difference up without bound.  Measured at the initial design
between TWO PLAIN ScaMLGPBOLoops with the same seed and data, no batched code involved: the end points of one start 3.97 apart in the
raw outputscale and 14 iterations apart in ``stats`` (objective equal to 5e-7) for study 2, 1.13 and 6 iterations for study 3; the
lock-step study against a loop: 0.15 / 6 iterations and 1.07 / 1 iteration -- the same scatter, and nothing a refit could be held to
1e-10 against.  So ``_one_prior_per_training_set`` makes the shared stack answer a repeated training-set query with the tensors it
answered first: the study and its twin loop then fit the same numbers, and everything downstream is compared as the issue asks."""
import numpy as np
import pytest
import torch

import scamlgp_amd
from oracle import gp_oracle as O
from scamlgp_amd import model as M, results, synthetic
from scamlgp_amd.bo import OptimizerNotReady, ScaMLGPBOLoop, ScaMLGPBOStudies

pytestmark = pytest.mark.gpu

S, DIM = 4, 6
SEEDS = [11, 12, 13, 14]
KW = dict(acquisition="ucb", num_restarts_log_likelihood=2, raw_samples=256, num_restarts=4, af_max_iter=20, max_pending_evaluations=2,
          num_fantasies=8)


def _gps(device, T=2, N=64, seed=3):
    d = synthetic.hartmann6_task_stack(T, N, seed=seed, noise_std=0.1)
    stack = M.SourceGPStack([f"h{t}" for t in range(T)], [torch.from_numpy(d["X"][t]) for t in range(T)],
                            [torch.from_numpy(d["Y"][t]).unsqueeze(-1) for t in range(T)], kind=O.KIND_MATERN52, device=device)
    rng = np.random.default_rng(seed)
    stack.set_theta(torch.from_numpy(np.concatenate([0.6 + 0.8 * rng.uniform(size=(T, 6)), 0.5 + rng.uniform(size=(T, 1)),
                                                     1e-3 + 5e-3 * rng.uniform(size=(T, 1))], 1)))
    stack.refresh()
    return {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}


def _one_prior_per_training_set(gps):
    """The shared stack returns, for a training-set query (every point a leading point) it has answered before, that first answer:
    two models built on the same points get the same source means bit for bit (see the module docstring)."""
    stack = next(iter(gps.values()))._stack
    plain, memo = stack.posterior, {"hits": 0}

    def posterior(xq, cov_first=0, want_var=True, VA=None):
        if cov_first != xq.shape[0]:
            return plain(xq, cov_first=cov_first, want_var=want_var, VA=VA)
        key = (xq.detach().cpu().numpy().tobytes(), bool(want_var), VA is None)
        if key not in memo:
            memo[key] = plain(xq, cov_first=cov_first, want_var=want_var, VA=VA)
        else:
            memo["hits"] += 1
        return dict(memo[key])

    stack.posterior = posterior
    return memo


def _obj(x):
    return float(synthetic.hartmann6(np.asarray(x, dtype=np.float64).reshape(1, -1))[0])


def _close(got, ref, rtol, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
    print(f"{what}: max |diff| / max |ref| = {err:.3e}")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=rtol * float(ref.abs().max()) + 1e-300, msg=lambda m: f"{what}: {m}")


class _Twin:
    """A ScaMLGPBOLoop whose restart samples follow a generator's stream (the global RNG is switched to it around report)."""

    def __init__(self, gps, seed):
        self.loop = ScaMLGPBOLoop(gps, DIM, seed=seed, **KW)
        self.state = torch.Generator().manual_seed(seed).get_state()

    def report(self, x, y):
        saved = torch.get_rng_state()
        torch.set_rng_state(self.state)
        self.loop.report(x, y)
        self.state = torch.get_rng_state()
        torch.set_rng_state(saved)


def _compare_models(studies, twins, which, tag):
    for s in which:
        a, b = studies[s].model, twins[s].loop.model
        assert a.n == b.n and torch.equal(a.train_X, b.train_X) and torch.equal(a.train_Y, b.train_Y), (tag, s)
        _close(a.raw_theta, b.raw_theta, 1e-10, f"{tag} study {s} raw hyper-parameters")
        _close(a.weights, b.weights, 1e-10, f"{tag} study {s} weights")
        ia, ib = a.last_fit_info, b.last_fit_info
        assert torch.equal(ia["stats"], ib["stats"]), (tag, s, ia["stats"], ib["stats"])
        _close(ia["objective"], ib["objective"], 1e-10, f"{tag} study {s} objective of every start")


def test_public_class_is_exported():
    assert scamlgp_amd.ScaMLGPBOStudies is ScaMLGPBOStudies


def test_lockstep_studies_match_single_loops(device):
    gps = _gps(device)
    memo = _one_prior_per_training_set(gps)
    studies = ScaMLGPBOStudies(gps, DIM, num_studies=S, seeds=SEEDS, **KW)
    twins = [_Twin(gps, SEEDS[s]) for s in range(S)]
    assert len(studies) == S and studies[2] is studies.studies[2]
    g = torch.Generator().manual_seed(99)
    X0 = torch.rand(S, 3, DIM, dtype=torch.float64, generator=g)
    y0 = [[_obj(x) for x in X0[s]] for s in range(S)]
    studies.report_some({s: (X0[s], y0[s]) for s in range(S)})
    for s in range(S):
        twins[s].report(X0[s], y0[s])
    _compare_models(studies, twins, range(S), "initial design")
    held = None   # study 2's evaluation that stays pending
    for step in range(6):
        Xs = studies.suggest()
        assert Xs.shape == (S, DIM) and bool(((Xs >= 0) & (Xs <= 1)).all())
        for s in range(S):
            xl = twins[s].loop.suggest()
            print(f"step {step} study {s} suggestion: max |diff| = {float((Xs[s] - xl).abs().max()):.3e}")
            torch.testing.assert_close(Xs[s], xl, rtol=0, atol=1e-6)
            twins[s].loop.pending[-1] = Xs[s]   # the same point on both sides from here on
        ev = {}
        for s in range(S):
            y = _obj(Xs[s])
            if s == 1 and step == 2:
                y = None                                       # no objective value: kept in X / Y, out of the fit
            if s == 2 and step == 1:
                held = (Xs[s].clone(), y)                      # not reported now: pending
                continue
            if s == 2 and step == 3:
                ev[s] = (torch.stack([held[0], Xs[s]]), [held[1], y])   # the late evaluation and this step's, one refit
                continue
            ev[s] = (Xs[s], y)
        studies.report_some(ev)
        for s, (x, y) in ev.items():
            twins[s].report(x, y)
        if step in (1, 2):
            assert studies[2].pending.shape[0] == 1 and twins[2].loop.pending.shape[0] == 1   # the held evaluation
        _compare_models(studies, twins, range(S), f"step {step}")
    assert memo["hits"] >= S * 6   # (the twins' training sets were the studies')
    for s in range(S):
        st = studies[s]
        assert st.X.shape == (9, DIM) and st.pending.shape[0] == 0 and torch.equal(st.X, twins[s].loop.X)
        assert st.model.n == (8 if s == 1 else 9)
    assert bool(torch.isnan(studies[1].Y[5]).all())
    # a study's record goes through `results` as a single loop's does
    for s in (0, 3):
        recs = [results.study_record(l.X.tolist(), l.Y.squeeze(-1).tolist(), seed=SEEDS[s], optimum=-3.32237) for l in (studies[s], twins[s].loop)]
        assert len(recs[0]["evaluations"]) == 9 and results.regrets_of_study(recs[0], noise_free=False) == results.regrets_of_study(recs[1], noise_free=False)


def test_report_and_run_take_one_value_per_study(device):
    gps = _gps(device)
    kw = dict(KW, max_pending_evaluations=None, num_restarts_log_likelihood=1)
    studies = ScaMLGPBOStudies(gps, DIM, num_studies=3, seeds=[1, 2, 3], **kw)
    g = torch.Generator().manual_seed(5)
    X = torch.rand(3, DIM, dtype=torch.float64, generator=g)
    studies.report(X, [_obj(X[0]), None, float("nan")])
    assert [st.model.n for st in studies.studies] == [1, 0, 0] and all(st.X.shape == (1, DIM) for st in studies.studies)
    studies.report(X.flip(0), torch.tensor([_obj(x) for x in X.flip(0)]))
    assert [st.model.n for st in studies.studies] == [2, 1, 1]
    Xs, Ys = studies.run(lambda P: [_obj(x) for x in P], 1)
    assert all(x.shape == (3, DIM) for x in Xs) and all(y.shape == (3, 1) for y in Ys)
    Xs, Ys = studies.run([_obj, _obj, lambda x: 2.0 * _obj(x)], 1)
    assert all(x.shape == (4, DIM) for x in Xs)
    assert float(Ys[2][-1]) == 2.0 * _obj(Xs[2][-1])
    with pytest.raises(ValueError):
        studies.report(X[:2], [0.0, 0.0])
    with pytest.raises(ValueError):
        ScaMLGPBOStudies(gps, DIM, num_studies=2, seeds=[1])
    with pytest.raises(TypeError):
        ScaMLGPBOStudies(gps, DIM, num_studies=2, seed=1)


def test_pending_limit_is_per_study(device):
    gps = _gps(device)
    studies = ScaMLGPBOStudies(gps, DIM, num_studies=2, seeds=[7, 8], **dict(KW, max_pending_evaluations=1, num_restarts_log_likelihood=1))
    studies.suggest()
    with pytest.raises(OptimizerNotReady):
        studies.suggest()


def test_fantasy_models_are_not_refitted(device):
    from scamlgp_amd.utils import fit_targets_batched

    gps = _gps(device)
    g = torch.Generator().manual_seed(2)
    Xt = torch.rand(4, DIM, dtype=torch.float64, generator=g)
    model = M.ScaMLGP(Xt, torch.tensor([[_obj(x)] for x in Xt]), gps).eval()
    fm = model.fantasize(torch.rand(2, DIM, dtype=torch.float64, generator=g), 4, generator=g)
    with pytest.raises(NotImplementedError):
        fit_targets_batched([model, fm], 1)
