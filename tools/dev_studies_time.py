"""One BO step of S studies against one source stack at configs[4] shapes (T = 32 Hartmann-6 sources of N = 512 points, D = 6, the
target set growing to n = 80, 2 restarts of the refit): ``ScaMLGPBOStudies`` (all refits in one launch of
scaml_target_fit_batched_f64) against S ``ScaMLGPBOLoop``s stepped one after the other -- what a caller had before --, in ONE process,
the two sides alternating step by step, for S in {1, 8, 32, 64}.

Per side and step the time is split into suggest (the acquisition optimisation of every study), model construction (ScaMLGP rebuilt on
the new point: the source posteriors at the training inputs) and refit.  Host clock around work that ends in a device synchronise;
medians over the timed steps (the first step of a size is a warm-up and is not counted).

  python tools/dev_studies_time.py [--sizes 1,8,32,64] [--steps K] [--out profiles/studies_timings.txt]
  python tools/dev_studies_time.py --suggest [--sweep 1,2,4,8,16] [--evals-per-call K]    suggest() alone, in its three modes
  python tools/dev_studies_time.py --score [--sizes 1,8,32,64] [--out profiles/studies_score_timings.txt]
      the device mode's suggest() by score_mode, the split of a suggest into its parts, and StudiesAcquisition.score alone
  python tools/dev_studies_time.py --own-stacks [--sizes 8,32,128] [--out profiles/studies_own_stacks_timings.txt]
      one source stack PER study at hartmann6.py's shape (see own_stacks_table)
  python tools/dev_studies_time.py --pending [--sizes 8,32] [--steps K] [--out profiles/studies_pending_timings.txt]
      every study holds pending evaluations: fantasy_setup='batched' and pending_mode='batched' against 'per_study' (see pending_table)
  python tools/dev_studies_time.py --acqf ucb,ei,logei [--against LIB] [--out profiles/logei_timings.txt]
      the evaluation launches per acquisition code (and against a second build of the library), EI against LogEI in suggest() (see acqf_table)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-meta-learning-with-gaussian-processes_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from scamlgp_amd import hyper, model as M, ops, synthetic, utils  # noqa: E402
from scamlgp_amd.bo import ScaMLGPBOLoop, ScaMLGPBOStudies  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1,8,32,64")
ap.add_argument("--steps", type=int, default=3, help="timed steps per size (n ends at 80)")
ap.add_argument("--out", default=None)
ap.add_argument("--suggest", action="store_true", help="time suggest(): suggest_mode='device', 'lockstep' and the default, interleaved in one process")
ap.add_argument("--sweep", default=None, help="with a list such as 1,2,4,8,16: the device mode's suggest() against ops.ACQF_OPT_EVALS_PER_CALL")
ap.add_argument("--evals-per-call", type=int, default=None, help="ops.ACQF_OPT_EVALS_PER_CALL for --suggest")
ap.add_argument("--score", action="store_true", help="device suggest(): score_mode='batched' against 'per_study', its split into parts, and score alone")
ap.add_argument("--own-stacks", action="store_true", help="per-study source stacks: meta-fit, BO step and the grouped pass against what a caller had before")
ap.add_argument("--pending", action="store_true", help="studies with pending evaluations: fantasy_setup='batched' against pending_mode='batched' against 'per_study', and the evaluation launch alone")
ap.add_argument("--acqf", default=None, help="with a list such as ucb,ei,logei: the evaluation launches (7g) / (7k) per acquisition code, and the device suggest() of EI against LogEI")
ap.add_argument("--against", default=None, help="with --acqf: a second build of the library (the parent commit's), timed in turn with this one")
args = ap.parse_args()

T, N, D, N_END, RESTARTS = 32, 512, 6, 80, 2
KW = dict(acquisition="ucb", num_restarts_log_likelihood=RESTARTS)
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def obj(x):
    return float(synthetic.hartmann6(np.asarray(x, dtype=np.float64).reshape(1, -1))[0])


def own_stacks_table():
    """Studies that each own their source stack, at the shape of the reference's configurations/hartmann6.py: T = 8 Hartmann-6 tasks of
    N = 128 points per study, D = 6, Matern-5/2, n = 40 target points, 10 starts per study, S in --sizes.  All sides alternate in one
    process; the first round of a size is a warm-up and is not counted; medians, spread = min .. max of the slower side.
      (a) meta-fit: ``meta_fit_scamlgp_studies`` (ONE stack of S T tasks) against S calls of ``meta_fit_scamlgp``; device driver,
          max_iter = 30, RESTARTS restarts each.
      (b) one BO step (suggest + report): ``ScaMLGPBOStudies`` on the per-study dicts, suggest_mode="device", against S
          ``ScaMLGPBOLoop``s on the S separately fitted stacks, stepped in turn; n = 40 at the last timed step.
      (c) one grouped source pass over S * 10 points: per-study tasks (task_base) against the same points through the shared-stack pass
          on study 0's stack alone -- the same T x Mq grid, so the ratio is what the lost sharing of L^-1 between studies costs."""
    To, No, n_end, starts = 8, 128, 40, 10
    kspec = M.KernelSpec(1)
    fit_kw = dict(covar_module=kspec, num_restarts_log_likelihood=RESTARTS, device=dev, fit_options=dict(driver="device", max_iter=30))
    # (the target GPs are Matern-5/2 as well: ScaMLGPBOStudies copies the module per study, every loop gets its own)
    tkern = lambda: hyper.get_default_kernel(hyper.MaternKernel, D)   # noqa: E731
    kw = dict(acquisition="ucb", num_restarts_log_likelihood=RESTARTS, num_restarts=starts)
    say(f"# one source stack per study: T = {To} tasks x N = {No}, D = {D}, Matern-5/2 (source and target kernels), n -> {n_end}, {starts} starts per study, {RESTARTS} restarts of "
        f"every fit; median of {args.steps} rounds, spread = min .. max of the slower side")
    for S in [int(v) for v in args.sizes.split(",")]:
        data = synthetic.hartmann6_task_stack(S * To, No, seed=S)
        metas = [{t: M.SupervisedDataset(torch.from_numpy(data["X"][s * To + t]), torch.from_numpy(data["Y"][s * To + t]).unsqueeze(-1))
                  for t in range(To)} for s in range(S)]
        # (a) ------------------------------------------------------------------------------------------------------------
        ta, tb = [], []
        for _ in range(args.steps + 1):
            dt, own = timed(lambda: M.meta_fit_scamlgp_studies(metas, seed=0, **fit_kw))
            ta.append(dt)
            dt, sep = timed(lambda: [M.meta_fit_scamlgp(md, seed=0, **fit_kw) for md in metas])
            tb.append(dt)
        ma, mb = statistics.median(ta[1:]), statistics.median(tb[1:])
        say(f"  (a) S = {S:>3}  meta-fit: one stack of {S * To} tasks {1e3 * ma:10.1f} ms   S calls {1e3 * mb:10.1f} ms ({1e3 * min(tb[1:]):.1f} .. "
            f"{1e3 * max(tb[1:]):.1f})   {mb / ma:6.2f}x")
        # (b) ------------------------------------------------------------------------------------------------------------
        steps = args.steps + 1
        seeds = list(range(100, 100 + S))
        studies = ScaMLGPBOStudies(own, D, num_studies=S, seeds=seeds, suggest_mode="device", gp_kernel=tkern(), **kw)
        loops = [ScaMLGPBOLoop(sep[s], D, seed=seeds[s], gp_kernel=tkern(), **kw) for s in range(S)]
        for s in range(S):
            g = torch.Generator().manual_seed(seeds[s])
            X0 = torch.rand(n_end - steps, D, dtype=torch.float64, generator=g)
            y0 = [obj(x) for x in X0]
            studies[s].record(X0, y0)
            loops[s].record(X0, y0)
        utils.fit_targets_batched([st.model for st in studies.studies], RESTARTS, rng=studies.fit_gens)
        for lp in loops:
            utils.optimize_marginal_likelihood(lp.model, RESTARTS)
        rows = {"studies": [], "loops": []}
        for _ in range(steps):
            t_s, X = timed(studies.suggest)
            ys = [obj(x) for x in X]
            t_r, _ = timed(lambda: studies.report(X, ys))
            rows["studies"].append((t_s, t_r))
            t_s = t_r = 0.0
            for lp in loops:
                dt, x = timed(lp.suggest)
                t_s += dt
                y = obj(x)
                dt, _ = timed(lambda: lp.report(x, y))
                t_r += dt
            rows["loops"].append((t_s, t_r))
        med = {k: [1e3 * statistics.median(r[i] for r in v[1:]) for i in range(2)] for k, v in rows.items()}
        tot = {k: [1e3 * sum(r) for r in v[1:]] for k, v in rows.items()}
        info = studies.last_suggest_info
        say(f"  (b) S = {S:>3}  BO step at n = {studies[0].model.n}: studies (device) suggest {med['studies'][0]:9.1f} + report {med['studies'][1]:9.1f} = "
            f"{statistics.median(tot['studies']):9.1f} ms   S loops suggest {med['loops'][0]:9.1f} + report {med['loops'][1]:9.1f} = "
            f"{statistics.median(tot['loops']):9.1f} ms ({min(tot['loops']):.1f} .. {max(tot['loops']):.1f})   "
            f"{statistics.median(tot['loops']) / statistics.median(tot['studies']):6.2f}x   [batched {len(info['batched'])} studies, {info['n_eval']} rounds]")
        # (c) ------------------------------------------------------------------------------------------------------------
        models = [st.model.eval() for st in studies.studies]
        sa_own = utils.StudiesAcquisition([utils.UpperConfidenceBound(m, 9.0) for m in models])
        twins = []
        for m in models:   # the same training sets, all on study 0's stack: the shared-stack pass
            tw = M.ScaMLGP(m.train_X, m.train_Y, own[0], covar_module=tkern()).eval()   # (the studies' target kernel family)
            tw.raw_theta, tw.weights = m.raw_theta.clone(), m.weights.clone()
            twins.append(tw)
        sa_sh = utils.StudiesAcquisition([utils.UpperConfidenceBound(m, 9.0) for m in twins])
        assert sa_own.task_base is not None and sa_sh.task_base is None
        g = torch.Generator().manual_seed(S)
        Xq = torch.rand(S * starts, D, dtype=torch.float64, generator=g).to(dev)
        group = sa_own.group_of([starts] * S)

        def source_pass(sa):
            st, f = sa.source, sa.source.fit
            theta = st.theta
            kwo = dict(task_base=sa.task_base, tasks_per_group=To) if sa.task_base is not None else {}
            return lambda: ops.source_posteriors_grad_grouped(Xq, group, sa.Xt, sa.n_points, sa.VA_tab, st.X, theta, st.kind, f["Linv"], f["alpha"],
                                                              st.y_mean, st.y_std, st.n_points, **kwo)

        calls = {"own": source_pass(sa_own), "shared": source_pass(sa_sh)}
        reps, inner = 10, 20
        got = {k: [] for k in calls}
        for r in range(reps + 1):
            for k, fn in calls.items():
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(inner):
                    fn()
                ev1.record()
                torch.cuda.synchronize()
                if r:
                    got[k].append(1e3 * ev0.elapsed_time(ev1) / inner)
        mo, msh = statistics.median(got["own"]), statistics.median(got["shared"])
        slow = "own" if mo >= msh else "shared"
        say(f"  (c) S = {S:>3}  grouped source pass, {S * starts} points x {To} task slots (n = {sa_own.n_max}): per-study tasks {mo:9.1f} us   shared stack "
            f"{msh:9.1f} us ({slow}: {min(got[slow]):.1f} .. {max(got[slow]):.1f})   own / shared = {mo / msh:5.2f}   [device events over {inner} calls, "
            f"allocation of the outputs included]")
        del studies, loops, own, sep, sa_own, sa_sh, twins, models
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if args.own_stacks:
    if args.sizes == ap.get_default("sizes"):
        args.sizes = "8,32,128"
    own_stacks_table()
    sys.exit(0)

d = synthetic.hartmann6_task_stack(T, N, seed=0)
stack = M.SourceGPStack(list(range(T)), [torch.from_numpy(d["X"][t]) for t in range(T)],
                        [torch.from_numpy(d["Y"][t]).unsqueeze(-1) for t in range(T)], kind=1, device=dev)
rng = np.random.default_rng(0)
stack.set_theta(torch.from_numpy(np.concatenate([0.6 + 0.8 * rng.uniform(size=(T, D)), 0.5 + rng.uniform(size=(T, 1)),
                                                 1e-3 + 5e-3 * rng.uniform(size=(T, 1))], 1)))
stack.refresh()
gps = {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}


def suggest_table():
    """suggest() in the three modes: three ScaMLGPBOStudies on the same data (all are told the sequential side's points), timed
    alternately step by step; n = 78 .. 80 over the three timed steps.  "rounds": batched evaluations (lock-step) or
    rounds enqueued (device); "ev/start": the evaluations a start consumed, mean over the starts; "ms/eval": lock-step only, the
    objective calls alone per evaluation (copy in, graph replay, copy out: the figure of DESIGN 4j); "sug/round": device only, the WHOLE
    suggest (stage 1 and packing included) divided by the rounds enqueued."""
    say(f"# suggest() of S studies, T = {T}, N = {N}, D = {D}, UCB, 10 starts per study, af_max_iter 50; ms, median of {args.steps} steps (n = "
        f"{N_END - args.steps + 1} .. {N_END}); spread = min .. max of that side's suggest over those steps; device: "
        f"{ops.ACQF_OPT_EVALS_PER_CALL} rounds per call")
    say(f"# {'S':>3} {'side':>10} {'suggest':>9} {'rounds':>6} {'ev/start':>8} {'ms/eval':>8} {'sug/round':>9} {'step':>9}   {'spread':>16}   lock-step / device   sequential / device")
    for S in [int(v) for v in args.sizes.split(",")]:
        steps = args.steps + 1
        n0 = N_END - steps
        seeds = list(range(100, 100 + S))
        modes = ("device", "lockstep", "sequential")
        sides = {k: ScaMLGPBOStudies(gps, D, num_studies=S, seeds=seeds, suggest_mode=k, **KW) for k in modes}
        for side in sides.values():
            for s in range(S):
                g = torch.Generator().manual_seed(seeds[s])
                X0 = torch.rand(n0, D, dtype=torch.float64, generator=g)
                side[s].record(X0, [obj(x) for x in X0])
            utils.fit_targets_batched([st.model for st in side.studies], RESTARTS, rng=side.fit_gens)
        rows = {k: [] for k in sides}
        for step in range(steps):
            t, info, X = {}, {}, None
            for k in modes:
                t[k], X = timed(sides[k].suggest)
                info[k] = dict(sides[k].last_suggest_info)
            ys = [obj(x) for x in X]   # (the sequential side's points)
            t_rep = {}
            for k, side in sides.items():
                t_rep[k], _ = timed(lambda: side.report(X, ys))
            ev = info["device"]["evals_per_start"]
            rows["device"].append((t["device"], t_rep["device"], info["device"]["n_eval"], sum(ev) / max(len(ev), 1), 0.0))
            rows["lockstep"].append((t["lockstep"], t_rep["lockstep"], info["lockstep"]["n_eval"], float(info["lockstep"]["n_eval"]),
                                     info["lockstep"]["eval_seconds"]))
            rows["sequential"].append((t["sequential"], t_rep["sequential"], 0, 0.0, 0.0))
        med = {k: [1e3 * statistics.median(r[i] for r in v[1:]) for i in range(2)] for k, v in rows.items()}
        ms = {k: [1e3 * r[0] for r in v[1:]] for k, v in rows.items()}
        for k in modes:
            ne = statistics.median(r[2] for r in rows[k][1:])
            per = statistics.median(r[3] for r in rows[k][1:])
            per_eval = statistics.median(1e3 * r[4] / max(r[2], 1) for r in rows[k][1:])   # the objective calls alone
            per_round = statistics.median(1e3 * r[0] / max(r[2], 1) for r in rows[k][1:])  # the whole suggest per round enqueued
            cols = {"device": f"{ne:6.0f} {per:8.1f} {'-':>8} {per_round:9.2f}", "lockstep": f"{ne:6.0f} {per:8.1f} {per_eval:8.2f} {'-':>9}",
                    "sequential": f"{'-':>6} {'-':>8} {'-':>8} {'-':>9}"}[k]
            tail = f"   {med['lockstep'][0] / med[k][0]:8.2f}x            {med['sequential'][0] / med[k][0]:8.2f}x" if k == "device" else ""
            say(f"  {S:>3} {k:>10} {med[k][0]:9.1f} {cols} {sum(med[k]):9.1f}   {min(ms[k]):7.1f} .. {max(ms[k]):5.1f}{tail}")
        lk = ms["lockstep"]
        say(f"#     n = {sides['device'][0].model.n}; lock-step - device = {med['lockstep'][0] - med['device'][0]:.1f} ms against a lock-step spread of "
            f"{max(lk) - min(lk):.1f} ms; sequential - device = {med['sequential'][0] - med['device'][0]:.1f} ms")


def sweep_table():
    """ops.ACQF_OPT_EVALS_PER_CALL: the device mode's suggest() at 1 / 2 / 4 / 8 / 16 rounds per call, the values alternating call by
    call on one set of studies (n = 80; each call draws new starts from the studies' generators), median of --steps calls."""
    chunks = [int(v) for v in args.sweep.split(",")]
    default_chunk = ops.ACQF_OPT_EVALS_PER_CALL
    say(f"# device suggest() against rounds per call, T = {T}, N = {N}, D = {D}, n = {N_END}; ms (rounds enqueued), median of {args.steps} calls")
    say(f"# {'S':>3} " + " ".join(f"{'k = ' + str(k):>16}" for k in chunks))
    for S in [int(v) for v in args.sizes.split(",")]:
        seeds = list(range(100, 100 + S))
        side = ScaMLGPBOStudies(gps, D, num_studies=S, seeds=seeds, suggest_mode="device", **KW)
        for s in range(S):
            g = torch.Generator().manual_seed(seeds[s])
            X0 = torch.rand(N_END, D, dtype=torch.float64, generator=g)
            side[s].record(X0, [obj(x) for x in X0])
        utils.fit_targets_batched([st.model for st in side.studies], RESTARTS, rng=side.fit_gens)
        side.suggest()   # warm-up
        got = {k: [] for k in chunks}
        for _ in range(args.steps):
            for k in chunks:
                ops.ACQF_OPT_EVALS_PER_CALL = k
                t, _ = timed(side.suggest)
                got[k].append((1e3 * t, side.last_suggest_info["n_eval"]))
        say(f"  {S:>3} " + " ".join(f"{statistics.median(v[0] for v in got[k]):9.1f} ({statistics.median(v[1] for v in got[k]):4.0f})" for k in chunks))
    ops.ACQF_OPT_EVALS_PER_CALL = default_chunk


def score_table():
    """score_mode="batched" against score_mode="per_study" (the path as it was), both with suggest_mode="device": two ScaMLGPBOStudies
    on the same data (both are told the per-study side's points), timed alternately step by step, n = 78 .. 80 over the three timed
    steps; median and min .. max of each side's suggest.  Then, at n = 80 and without reports in between, three more suggests per side
    with ``profile_parts`` (a device synchronisation at every boundary): the split into stage 1 (draw, scoring, picks), the
    StudiesAcquisition packing with the factors, the optimiser rounds and stage 3, medians.  Last, ``StudiesAcquisition.score`` alone
    for S x 1,024 candidates against S per-study scoring passes ``af(cand)`` (median of five, synchronised at the end of each side)."""
    say(f"# device suggest() of S studies by score_mode, T = {T}, N = {N}, D = {D}, UCB, 1,024 raw candidates and 10 starts per study; ms, median of "
        f"{args.steps} steps (n = {N_END - args.steps + 1} .. {N_END}), spread = min .. max of that side's suggest over those steps")
    for S in [int(v) for v in args.sizes.split(",")]:
        steps = args.steps + 1
        n0 = N_END - steps
        seeds = list(range(100, 100 + S))
        modes = ("per_study", "batched")
        sides = {k: ScaMLGPBOStudies(gps, D, num_studies=S, seeds=seeds, suggest_mode="device", score_mode=k, **KW) for k in modes}
        for side in sides.values():
            for s in range(S):
                g = torch.Generator().manual_seed(seeds[s])
                X0 = torch.rand(n0, D, dtype=torch.float64, generator=g)
                side[s].record(X0, [obj(x) for x in X0])
            utils.fit_targets_batched([st.model for st in side.studies], RESTARTS, rng=side.fit_gens)
        ms = {k: [] for k in modes}
        for step in range(steps):
            X = {}
            for k in modes:
                t, X[k] = timed(sides[k].suggest)
                if step:
                    ms[k].append(1e3 * t)
            ys = [obj(x) for x in X["per_study"]]
            for side in sides.values():
                side.report(X["per_study"], ys)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(ms["per_study"]) - min(ms["per_study"])
        gain = med["per_study"] - med["batched"]
        for k in modes:
            say(f"  S = {S:>3} {k:>10} suggest {med[k]:9.1f} ms   ({min(ms[k]):.1f} .. {max(ms[k]):.1f})   rounds {sides[k].last_suggest_info['n_eval']}")
        say(f"#     n = {sides['batched'][0].model.n}; per_study - batched = {gain:.1f} ms against a per_study spread of {spread:.1f} ms: "
            f"{'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}; per_study / batched = {med['per_study'] / med['batched']:.2f}x")
        for k in modes:
            sides[k].profile_parts = True
            got = []
            for _ in range(3):
                sides[k].suggest()
                got.append(dict(sides[k].last_suggest_info["parts"]))
            sides[k].profile_parts = False
            p = {name: 1e3 * statistics.median(g_.get(name, 0.0) for g_ in got) for name in ("stage1", "packing", "rounds", "stage3")}
            say(f"#     split, {k:>9}: stage 1 {p['stage1']:8.2f}   packing + factors {p['packing']:8.2f}   rounds {p['rounds']:8.2f}   stage 3 {p['stage3']:8.2f}   "
                f"(stage 1 + packing = {p['stage1'] + p['packing']:.2f} of {sum(p.values()):.2f} ms)")
        # score alone
        models = [st.model.eval() for st in sides["per_study"].studies]
        afs = [utils.UpperConfidenceBound(m, 9.0) for m in models]
        g = torch.Generator().manual_seed(S)
        cands = [torch.rand(1024, D, dtype=torch.float64, generator=g) for _ in range(S)]
        sa = utils.StudiesAcquisition(afs, batched_factors=True)
        table, group = torch.cat(cands).to(dev), sa.group_of([64] * S)
        tb, tp = [], []
        for r in range(6):
            dt, _ = timed(lambda: sa.score(table, group)["value"].cpu())
            tb.append(1e3 * dt)
            dt, _ = timed(lambda: [af(c).detach().cpu() for af, c in zip(afs, cands)])
            tp.append(1e3 * dt)
        say(f"#     score alone, {S} x 1,024 candidates: StudiesAcquisition.score {statistics.median(tb[1:]):8.2f} ms ({min(tb[1:]):.2f} .. {max(tb[1:]):.2f})   "
            f"{S} per-study passes {statistics.median(tp[1:]):8.2f} ms ({min(tp[1:]):.2f} .. {max(tp[1:]):.2f})")
        del sides, sa, afs, models
        torch.cuda.empty_cache()


def pending_table():
    """Every study holds p pending evaluations (p = 1, then 4; F = 16 fantasies, n = 80 observed points, 10 starts per study), three
    sides: ``pending_mode="batched"`` with ``fantasy_setup="batched"`` (all fantasy models from one ``model.fantasize_studies`` call),
    ``pending_mode="batched"`` alone (the fantasy model of every study from its own ``fantasize`` call: the yardstick of the first side)
    and ``"per_study"`` (every study its own ``ScaMLGPBOLoop.suggest()``), with both ``score_mode``s, in suggest_mode "device" and
    "lockstep".  Three ScaMLGPBOStudies on the same data, timed alternately call by call in one process; after every suggest the pending
    lists are put back to the p points, so every call sees the same shapes (each draws new fantasies and starts from the studies'
    generators).  The first call of a row is a warm-up and is not counted; median and min .. max per side.  A side counts as faster than
    its yardstick only if the gain exceeds the yardstick's own min .. max spread.
    Then the split of the two batched sides' suggest (``profile_parts``: "setup" is the ``fantasize_studies`` call; without it "stage1"
    holds the per-study set-up -- fantasize with the conditioned model's source pass, factor and alpha, through the study's own scoring
    pass), and the split of one ``fantasize_studies`` call: the S V' launches, the module copies, the rest.  Last, the evaluation launch
    alone on one grouped source pass's outputs: scaml_target_fantasy_acqf_batched_f64 against scaml_target_acqf_batched_f64 at F = 1
    (the same ordinary studies) and at F = 16 (the fantasy models; (7g) on their arrays with column 0 of alpha_f, for the time only)."""
    import copy

    F, starts = 16, 10
    kw = dict(KW, max_pending_evaluations=8, num_fantasies=F)
    say(f"# suggest() of S studies that all hold p pending evaluations, T = {T}, N = {N}, D = {D}, n = {N_END}, F = {F}, UCB, 1,024 raw candidates and "
        f"{starts} starts per study; ms, median of {args.steps} calls, (min .. max) per side")
    say("# sides: setup = pending_mode='batched' with fantasy_setup='batched'; batched = pending_mode='batched' (its yardstick); per_study")
    for S in [int(v) for v in args.sizes.split(",")]:
        seeds = list(range(100, 100 + S))
        make = {"setup": dict(pending_mode="batched", fantasy_setup="batched"), "batched": dict(pending_mode="batched"), "per_study": dict()}
        sides = {k: ScaMLGPBOStudies(gps, D, num_studies=S, seeds=seeds, suggest_mode="device", **o, **kw) for k, o in make.items()}
        for side in sides.values():
            for s in range(S):
                g = torch.Generator().manual_seed(seeds[s])
                X0 = torch.rand(N_END, D, dtype=torch.float64, generator=g)
                side[s].record(X0, [obj(x) for x in X0])
            utils.fit_targets_batched([st.model for st in side.studies], RESTARTS, rng=side.fit_gens)
        for p in (1, 4):
            g = torch.Generator().manual_seed(1000 + S + p)
            pend = [torch.rand(p, D, dtype=torch.float64, generator=g) for _ in range(S)]

            def reset():
                for side in sides.values():
                    for s in range(S):
                        side[s].pending = pend[s].clone()

            for score_mode, mode in (("per_study", "device"), ("batched", "device"), ("per_study", "lockstep"), ("batched", "lockstep")):
                ms = {k: [] for k in sides}
                for r in range(args.steps + 1):
                    for k, side in sides.items():
                        side.suggest_mode, side.score_mode = mode, score_mode
                        reset()
                        t, _ = timed(side.suggest)
                        if r:
                            ms[k].append(1e3 * t)
                        assert len(side.last_suggest_info["batched"]) == (0 if k == "per_study" else S)
                med = {k: statistics.median(v) for k, v in ms.items()}
                cell = lambda k: f"{k} {med[k]:9.1f} ({min(ms[k]):.1f} .. {max(ms[k]):.1f})"   # noqa: E731
                gain, spread = med["batched"] - med["setup"], max(ms["batched"]) - min(ms["batched"])
                say(f"  S = {S:>3} p = {p} score {score_mode:>9} {mode:>8}: {cell('setup')}   {cell('batched')}   {cell('per_study')}   "
                    f"batched / setup = {med['batched'] / med['setup']:5.2f}x   gain {gain:.1f} ms against a batched spread of {spread:.1f} ms: "
                    f"{'faster by more than the spread' if gain > spread else ('a LOSS' if gain < 0 else 'INSIDE the spread')}")
                for k in ("setup", "batched"):
                    side = sides[k]
                    side.profile_parts = True
                    got = []
                    for _ in range(3):
                        reset()
                        side.suggest()
                        got.append(dict(side.last_suggest_info["parts"]))
                    side.profile_parts = False
                    q = {name: 1e3 * statistics.median(g_.get(name, 0.0) for g_ in got) for name in ("setup", "stage1", "packing", "rounds", "stage3")}
                    say(f"#       split, {k:>7} {mode:>8}: set-up {q['setup']:8.2f}   stage 1 {q['stage1']:8.2f}   packing {q['packing']:8.2f}   "
                        f"rounds {q['rounds']:8.2f}   stage 3 {q['stage3']:8.2f}   ({(q['setup'] + q['stage1']) / S:.2f} ms of set-up + stage 1 per study)")
            # one fantasize_studies call, and what of it stays per study
            reset()
            studies = sides["setup"].studies
            models = [st.model.eval() for st in studies]
            gens = [torch.Generator().manual_seed(7 + s) for s in range(S)]
            whole, va, cp = [], [], []
            for r in range(args.steps + 1):
                t0, _ = timed(lambda: M.fantasize_studies(models, [st.pending for st in studies], F, gens))
                Xp = [torch.cat([m.train_X, st.pending.to(dev)], 0) for m, st in zip(models, studies)]

                def v_launches():
                    for m, x in zip(models, Xp):
                        stk, f = m._stack, m._stack.fit
                        ops.source_posteriors(x, stk.X, stk.theta, stk.kind, f["L"], f["Linv_diag"], f["alpha"], stk.y_mean, stk.y_std,
                                              n_points=stk.n_points, want_var=False, keep_V=True, Linv=f["Linv"])

                t1, _ = timed(v_launches)
                t2, _ = timed(lambda: [(copy.deepcopy(m.likelihood), copy.deepcopy(m.covar_module)) for m in models])
                if r:
                    whole.append(1e3 * t0), va.append(1e3 * t1), cp.append(1e3 * t2)
            w_, v_, c_ = statistics.median(whole), statistics.median(va), statistics.median(cp)
            say(f"#     fantasize_studies alone, S = {S}, p = {p}: {w_:8.2f} ms ({min(whole):.2f} .. {max(whole):.2f}), {w_ / S:.3f} ms per study; of it the S V' "
                f"launches {v_:.2f} ms ({100 * v_ / w_:.0f} %), the module copies {c_:.2f} ms ({100 * c_ / w_:.0f} %)")
        # the evaluation launch alone, on one source pass's outputs
        reset()
        studies = sides["batched"].studies
        models = gens = Xp = None
        ordinary = [utils.UpperConfidenceBound(st.model.eval(), 9.0) for st in studies]
        fantasy = [st.acquisition_function() for st in studies]
        Xq = torch.rand(S * starts, D, dtype=torch.float64, generator=torch.Generator().manual_seed(S)).to(dev)
        for name, afs in (("F = 1", ordinary), (f"F = {F}, p = 4", fantasy)):
            sa = utils.StudiesAcquisition(afs)
            group = sa.group_of([starts] * S)
            st, f = sa.source, sa.source.fit
            src = ops.source_posteriors_grad_grouped(Xq, group, sa.Xt, sa.n_points, sa.VA_tab, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean,
                                                     st.y_std, st.n_points)
            alpha_f = sa.alpha_f if sa.fantasy else sa.alpha.unsqueeze(-1).contiguous()
            n_fant = sa.n_fant if sa.fantasy else torch.ones(S, dtype=torch.int32, device=dev)
            head = (src["mu"], src["var"], src["cov"], group, Xq, sa.w, sa.active, sa.Xt, sa.theta, sa.L, sa.Linv_diag)
            tail = (sa.n_points, sa.m_all, sa.s_all, sa.info, sa.acqf_param, sa.acqf, sa.kind)
            a7 = alpha_f[:, :, 0].contiguous()
            calls = {"(7g)": lambda: ops.target_acqf_batched(*head, a7, *tail),
                     "(7k)": lambda: ops.target_fantasy_acqf_batched(*head, alpha_f, n_fant, *tail)}
            reps, inner = 8, 20
            got = {k: [] for k in calls}
            for r in range(reps + 1):
                for k, fn in calls.items():
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    ev0.record()
                    for _ in range(inner):
                        fn()
                    ev1.record()
                    torch.cuda.synchronize()
                    if r:
                        got[k].append(1e3 * ev0.elapsed_time(ev1) / inner)
            say(f"#     evaluation launch alone, {S * starts} query points, n' = {sa.n_max}, {name}: (7k) {statistics.median(got['(7k)']):8.1f} us "
                f"({min(got['(7k)']):.1f} .. {max(got['(7k)']):.1f})   (7g) {statistics.median(got['(7g)']):8.1f} us ({min(got['(7g)']):.1f} .. {max(got['(7g)']):.1f})   "
                f"[device events over {inner} calls, allocation of the outputs included]")
        del sides, studies, ordinary, fantasy, sa
        torch.cuda.empty_cache()


def acqf_table():
    """The acquisition codes against each other (``--acqf ucb,ei,logei``) and, with ``--against LIB``, this build against a second one
    (the parent commit's, which refuses LogEI), everything alternating in one process.
      (1) the evaluation launch alone on one grouped source pass's outputs, 32 studies x 10 starts = 320 query points, n = 80:
          scaml_target_acqf_batched_f64 (7g) and scaml_target_fantasy_acqf_batched_f64 (7k) at F = 1 (ordinary studies) and at F = 16
          (fantasy models of p = 4 pending points; (7g) on their arrays with column 0 of alpha_f, for the time only).  Device events
          over 20 calls, median of 5 rounds with min .. max, the first round a warm-up; the order of the calls turns round by round.
      (2) suggest() with suggest_mode="device" of S = 8 and 32 studies, acquisition "ei" against "logei" on the same data, median of
          5 calls with min .. max and the rounds enqueued (EI stops the starts whose gradient is exactly 0; LogEI moves them)."""
    import ctypes

    from scamlgp_amd import _lib

    names = args.acqf.split(",")
    libs = {"this": _lib.lib}
    if args.against:
        other = ctypes.CDLL(os.path.abspath(args.against))
        for name, (restype, argtypes) in _lib.SIGNATURES.items():
            if hasattr(other, name):
                fn = getattr(other, name)
                fn.restype, fn.argtypes = restype, argtypes
        libs["parent"] = other
    S, F, starts, p = 32, 16, 10, 4
    say(f"# acquisition codes {names}, builds {list(libs)}; T = {T}, N = {N}, D = {D}, n = {N_END}")
    seeds = list(range(100, 100 + S))
    side = ScaMLGPBOStudies(gps, D, num_studies=S, seeds=seeds, suggest_mode="device", **dict(KW, max_pending_evaluations=8, num_fantasies=F))
    for s in range(S):
        g = torch.Generator().manual_seed(seeds[s])
        X0 = torch.rand(N_END, D, dtype=torch.float64, generator=g)
        side[s].record(X0, [obj(x) for x in X0])
    utils.fit_targets_batched([st.model for st in side.studies], RESTARTS, rng=side.fit_gens)
    g = torch.Generator().manual_seed(1000 + S + p)
    pend = [torch.rand(p, D, dtype=torch.float64, generator=g) for _ in range(S)]
    Xq = torch.rand(S * starts, D, dtype=torch.float64, generator=torch.Generator().manual_seed(S)).to(dev)
    for label, pending in (("F = 1", False), (f"F = {F}, p = {p}", True)):
        calls = {}
        for name in names:
            for s, st in enumerate(side.studies):
                st.acquisition = name
                st.pending = pend[s].clone() if pending else pend[s][:0].clone()
                st.gen.manual_seed(seeds[s])    # the same fantasies for every code
            sa = utils.StudiesAcquisition([st.acquisition_function() for st in side.studies])
            group = sa.group_of([starts] * S)
            stk, f = sa.source, sa.source.fit
            src = ops.source_posteriors_grad_grouped(Xq, group, sa.Xt, sa.n_points, sa.VA_tab, stk.X, stk.theta, stk.kind, f["Linv"], f["alpha"],
                                                     stk.y_mean, stk.y_std, stk.n_points)
            alpha_f = sa.alpha_f if sa.fantasy else sa.alpha.unsqueeze(-1).contiguous()
            n_fant = sa.n_fant if sa.fantasy else torch.ones(S, dtype=torch.int32, device=dev)
            head = (src["mu"], src["var"], src["cov"], group, Xq, sa.w, sa.active, sa.Xt, sa.theta, sa.L, sa.Linv_diag)
            tail = (sa.n_points, sa.m_all, sa.s_all, sa.info, sa.acqf_param, sa.acqf, sa.kind)
            a7 = alpha_f[:, :, 0].contiguous()
            for build in libs:
                if build == "parent" and name == "logei":
                    continue
                calls[("(7g)", name, build)] = lambda head=head, a7=a7, tail=tail: ops.target_acqf_batched(*head, a7, *tail)
                calls[("(7k)", name, build)] = lambda head=head, alpha_f=alpha_f, n_fant=n_fant, tail=tail: ops.target_fantasy_acqf_batched(
                    *head, alpha_f, n_fant, *tail)
        reps, inner = 5, 20
        got = {k: [] for k in calls}
        for r in range(reps + 1):
            for k, fn in (list(calls.items()) if r % 2 else reversed(list(calls.items()))):   # the order turns round by round
                _lib.lib = libs[k[2]]
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(inner):
                    fn()
                ev1.record()
                torch.cuda.synchronize()
                if r:
                    got[k].append(1e3 * ev0.elapsed_time(ev1) / inner)
        _lib.lib = libs["this"]
        say(f"# (1) evaluation launch alone, {S * starts} query points, {label}; us, median of {reps} rounds (min .. max) [device events over {inner} calls, "
            f"allocation of the outputs included]")
        for k, v in got.items():
            note = ""
            base = got.get((k[0], k[1], "parent"))
            if k[2] == "this" and base:
                inside = min(base) <= statistics.median(v) <= max(base)
                note = f"   this / parent = {statistics.median(v) / statistics.median(base):5.3f}: {'INSIDE' if inside else 'OUTSIDE'} the parent's min .. max"
            elif k[2] == "this" and k[1] == "logei" and (k[0], "ei", "this") in got:
                note = f"   logei / ei = {statistics.median(v) / statistics.median(got[(k[0], 'ei', 'this')]):5.3f}"
            say(f"  {k[0]} {k[1]:>5} {k[2]:>6} {statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f}){note}")
    del side
    torch.cuda.empty_cache()
    pair = [n_ for n_ in ("ei", "logei") if n_ in names]
    if len(pair) < 2:
        return
    say("# (2) suggest(), suggest_mode='device', no pending evaluations; ms, median of 5 calls (min .. max), rounds enqueued in the last call")
    for S in (8, 32):
        seeds = list(range(100, 100 + S))
        sides = {k: ScaMLGPBOStudies(gps, D, num_studies=S, seeds=seeds, suggest_mode="device", **dict(KW, acquisition=k)) for k in pair}
        for sd in sides.values():
            for s in range(S):
                g = torch.Generator().manual_seed(seeds[s])
                X0 = torch.rand(N_END, D, dtype=torch.float64, generator=g)
                sd[s].record(X0, [obj(x) for x in X0])
            utils.fit_targets_batched([st.model for st in sd.studies], RESTARTS, rng=sd.fit_gens)
        ms = {k: [] for k in pair}
        for r in range(6):
            for k, sd in sides.items():
                t, _ = timed(sd.suggest)
                if r:
                    ms[k].append(1e3 * t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in pair:
            say(f"  S = {S:>3} {k:>5} suggest {med[k]:9.1f} ms ({min(ms[k]):.1f} .. {max(ms[k]):.1f})   rounds {sides[k].last_suggest_info['n_eval']}")
        say(f"#     logei / ei = {med['logei'] / med['ei']:5.2f}x")
        del sides
        torch.cuda.empty_cache()


if args.acqf:
    acqf_table()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
if args.pending:
    if args.sizes == ap.get_default("sizes"):
        args.sizes = "8,32"
    pending_table()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
if args.score:
    score_table()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
if args.sweep:
    sweep_table()
    if args.out:
        with open(args.out, "a" if args.suggest else "w") as f:
            f.write("\n".join(lines) + "\n")
    lines.clear()
    if not args.suggest:
        sys.exit(0)
if args.suggest:
    default_chunk = ops.ACQF_OPT_EVALS_PER_CALL
    ops.ACQF_OPT_EVALS_PER_CALL = args.evals_per_call or default_chunk
    suggest_table()
    if args.out:
        with open(args.out, "a" if args.sweep else "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
say(f"# BO step of S studies, T = {T}, N = {N}, D = {D}, n -> {N_END}, {RESTARTS} restarts (B = {1 + RESTARTS} starts per study), UCB; ms per step, median of "
    f"{args.steps} steps")
say("# batched = ScaMLGPBOStudies (one refit launch for all studies); sequential = S ScaMLGPBOLoops one after the other")
say(f"# {'S':>3} {'side':>10} {'suggest':>9} {'construct':>9} {'refit':>9} {'step':>9}   speed-up (step)   speed-up (refit)")
for S in [int(v) for v in args.sizes.split(",")]:
    steps = args.steps + 1
    n0 = N_END - steps          # history before the first step: the last timed refit is at n = 80
    seeds = list(range(100, 100 + S))
    studies = ScaMLGPBOStudies(gps, D, num_studies=S, seeds=seeds, **KW)
    loops = [ScaMLGPBOLoop(gps, D, seed=seeds[s], **KW) for s in range(S)]
    for s in range(S):
        g = torch.Generator().manual_seed(seeds[s])
        X0 = torch.rand(n0, D, dtype=torch.float64, generator=g)
        y0 = [obj(x) for x in X0]
        studies[s].record(X0, y0)
        loops[s].record(X0, y0)
    utils.fit_targets_batched([st.model for st in studies.studies], RESTARTS, rng=studies.fit_gens)
    for lp in loops:
        utils.optimize_marginal_likelihood(lp.model, RESTARTS)
    rows = {"batched": [], "sequential": []}
    for step in range(steps):
        # -- batched side --
        t_s, X = timed(studies.suggest)
        ys = [obj(x) for x in X]
        t_c, _ = timed(lambda: [studies[s].record(X[s], ys[s]) for s in range(S)])
        t_r, _ = timed(lambda: utils.fit_targets_batched([st.model for st in studies.studies], RESTARTS, rng=studies.fit_gens))
        rows["batched"].append((t_s, t_c, t_r))
        # -- sequential side: the same work, study after study --
        t_s, Xl = timed(lambda: [lp.suggest() for lp in loops])
        yl = [obj(x) for x in Xl]
        t_c = t_r = 0.0
        for s, lp in enumerate(loops):
            dt, _ = timed(lambda: lp.record(Xl[s], yl[s]))
            t_c += dt
            dt, _ = timed(lambda: utils.optimize_marginal_likelihood(lp.model, RESTARTS))
            t_r += dt
        rows["sequential"].append((t_s, t_c, t_r))
    med = {k: [1e3 * statistics.median(r[i] for r in v[1:]) for i in range(3)] for k, v in rows.items()}
    tot = {k: sum(v) for k, v in med.items()}
    n_now = studies[0].model.n
    ev = torch.stack([st.model.last_fit_info["stats"][:, 1] for st in studies.studies]).cpu()
    for k in ("batched", "sequential"):
        tail = f"   {tot['sequential'] / tot['batched']:6.2f}x            {med['sequential'][2] / med['batched'][2]:6.2f}x" if k == "batched" else ""
        say(f"  {S:>3} {k:>10} {med[k][0]:9.1f} {med[k][1]:9.1f} {med[k][2]:9.1f} {tot[k]:9.1f}{tail}")
    say(f"#     n = {n_now}; evaluations per start in the last batched refit: min {int(ev.min())}, median {int(ev.median())}, max {int(ev.max())}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
