"""``ScaMLGPBOStudies(suggest_mode="lockstep")`` on the MI355X next to a default (sequential) instance fed the same data: S = 4 studies
on the c5r-shaped stack of tests/test_studies_gpu.py, its ``KW`` (``max_pending_evaluations=2``), 4 steps.  The sequential side's points
are what both sides report, so both stay on the same data.  After every ``suggest()``: each study's generator is where its sequential
twin's is (stage 1 of ``optimize_acqf`` consumed the same draws), the suggestions lie in the box, and each study's acquisition value at
its lock-step suggestion -- through the study's OWN acquisition function -- is at least its value at the best raw candidate (less
1e-9 of the value: the final choice compares the BATCHED evaluation of the end points with the raw candidates' scores, and the batched
evaluation agrees with the study's own to 1e-10 of the value, tests/test_studies_acqf_gpu.py -- a tie could fall either way; measured,
the suggestion beats the best raw candidate by 0.2 .. 0.8 at every step).  Study 0 has
no training data at the first step and study 2 holds an evaluation pending for a step: both take ``ScaMLGPBOLoop.suggest`` (counted)
while the others stay batched."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O
from scamlgp_amd import bo, model as M, synthetic
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


def _obj(x):
    return float(synthetic.hartmann6(np.asarray(x, dtype=np.float64).reshape(1, -1))[0])


def test_lockstep_suggest_next_to_the_sequential_one(monkeypatch):
    device = torch.device("cuda:0")
    gps = _gps(device)
    lock = ScaMLGPBOStudies(gps, DIM, S, seeds=SEEDS, suggest_mode="lockstep", **KW)
    seq = ScaMLGPBOStudies(gps, DIM, S, seeds=SEEDS, **KW)
    assert seq.suggest_mode == "sequential"
    with pytest.raises(ValueError):
        ScaMLGPBOStudies(gps, DIM, S, seeds=SEEDS, suggest_mode="both", **KW)
    # initial designs: studies 1 .. 3 start with data, study 0 with none (its first step is the prior-only model's)
    g = torch.Generator().manual_seed(0)
    init = {s: torch.rand(3 + s, DIM, dtype=torch.float64, generator=g) for s in (1, 2, 3)}
    for side in (lock, seq):
        side.report_some({s: (x, [_obj(r) for r in x]) for s, x in init.items()})

    calls = []
    plain = ScaMLGPBOLoop.suggest

    def counted(self):
        calls.append(self)
        return plain(self)

    monkeypatch.setattr(ScaMLGPBOLoop, "suggest", counted)
    held = None   # study 2's evaluation of step 1 is reported a step late
    for step in range(4):
        calls.clear()
        # the candidates of stage 1, per study, as the lock-step side scores them (for the value check below)
        seen = {}
        stage1 = bo.acqf_initial_conditions

        def spy(af, *a, **k):
            out = stage1(af, *a, **k)
            seen[id(af.model)] = (af, out[0][out[2]])
            return out

        monkeypatch.setattr(bo, "acqf_initial_conditions", spy)
        Xl = lock.suggest()
        monkeypatch.setattr(bo, "acqf_initial_conditions", stage1)
        own_path = [lock.studies.index(st) for st in calls]
        expected = ([0] if step == 0 else []) + ([2] if step == 2 else [])
        assert own_path == expected, (step, own_path)
        assert lock.last_suggest_info["batched"] == [s for s in range(S) if s not in expected]
        calls.clear()
        Xs = seq.suggest()
        assert len(calls) == S
        assert bool(((Xl >= 0.0) & (Xl <= 1.0)).all())
        for s in range(S):
            assert torch.equal(lock[s].gen.get_state(), seq[s].gen.get_state()), (step, s)
            if s in expected:
                continue
            af, best_raw = seen[id(lock[s].model)]
            v = af(torch.stack([Xl[s], best_raw]).to(device)).cpu()
            print(f"step {step} study {s}: af(suggestion) = {float(v[0]):.12f}, af(best raw candidate) = {float(v[1]):.12f}")
            # (the batched evaluation and the study's own agree to 1e-10 of the value: tests/test_studies_acqf_gpu.py)
            assert float(v[0]) >= float(v[1]) - 1e-9 * max(1.0, abs(float(v[1])))
        # both sides are told the sequential side's points; the lock-step side's own suggestions leave its pending lists
        for s in range(S):
            lock[s].pending = seq[s].pending.clone()
        evals = {s: (Xs[s], _obj(Xs[s])) for s in range(S)}
        if step == 1:
            held = evals.pop(2)
        if step == 2:
            evals[2] = (torch.stack([held[0], evals[2][0]]), [held[1], evals[2][1]])
        for side in (lock, seq):
            side.report_some(evals)
    # OptimizerNotReady as in the default mode: studies in front of the blocked one have suggested, it raises, the rest have not
    for side in (lock, seq):
        side.suggest()
        before = [st.pending.shape[0] for st in side.studies]
        side[1].pending = torch.cat([side[1].pending, torch.rand(1, DIM, dtype=torch.float64)])
        with pytest.raises(OptimizerNotReady):
            side.suggest()
        after = [st.pending.shape[0] for st in side.studies]
        assert after == [before[0] + 1, before[1] + 1, before[2], before[3]]
