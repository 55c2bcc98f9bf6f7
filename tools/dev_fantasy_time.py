"""Cost of pending evaluations at configs[4] shapes (T = 32 Hartmann-6 sources of N = 512 points, D = 6, n = 80 target points) with
p = 4 pending points and F = 16 fantasies, EI.

Times, in one process and alternating the variants, the 1024-candidate scoring pass and the R = 10 value + gradient evaluation (eager
and replayed from a HIP graph) on
  parent  -- the model without pending points,
  fantasy -- parent.fantasize(pending, 16): ONE source pass + one fantasy-acquisition launch per evaluation,
  naive   -- the F models parent.condition_on_observations(pending, y_f), one evaluation each (F source passes);
the once-per-suggest set-up (sampling + conditioning, the factor + F columns of alpha); and one suggest() with 0 and with 4 pending.
Host clock around work that ends in a device synchronise; medians over the repetitions.

  python tools/dev_fantasy_time.py [--reps K] [--quick] [--out FILE]
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

from scamlgp_amd import model as M, synthetic, utils  # noqa: E402
from scamlgp_amd.bo import GraphedAcquisition, ScaMLGPBOLoop  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--quick", action="store_true", help="few repetitions, no suggest() timing (profiler runs)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
reps = 5 if args.quick else args.reps

T, N, D, n, p, F, R, C = 32, 512, 6, 80, 4, 16, 10, 1024
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


d = synthetic.hartmann6_task_stack(T, N, seed=0)
stack = M.SourceGPStack(list(range(T)), [torch.from_numpy(d["X"][t]) for t in range(T)],
                        [torch.from_numpy(d["Y"][t]).unsqueeze(-1) for t in range(T)], kind=1, device=dev)
rng = np.random.default_rng(0)
stack.set_theta(torch.from_numpy(np.concatenate([0.6 + 0.8 * rng.uniform(size=(T, D)), 0.5 + rng.uniform(size=(T, 1)),
                                                 1e-3 + 5e-3 * rng.uniform(size=(T, 1))], 1)))
stack.refresh()
gps = {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}
g = torch.Generator().manual_seed(1)
obj = lambda x: synthetic.hartmann6(np.asarray(x, dtype=np.float64).reshape(-1, D))   # noqa: E731
Xt = torch.rand(n, D, dtype=torch.float64, generator=g)
yt = torch.from_numpy(obj(Xt.numpy())).unsqueeze(-1)
parent = M.ScaMLGP(Xt, yt, gps).eval()
parent.weights = torch.from_numpy(0.01 + 0.1 * rng.uniform(size=T))
Xp = torch.rand(p, D, dtype=torch.float64, generator=g)
best_f = float(yt.min())
say(f"configs[4] shapes: T={T} N={N} D={D} n={n} pending p={p} fantasies F={F}; EI; scoring pass {C} candidates, value+grad at R={R}")

# --- once-per-suggest set-up ---------------------------------------------------------------------------------------------
t_fz, t_fac = [], []
held = {}
for i in range(reps):
    t_fz.append(sync_time(lambda: held.update(fm=parent.fantasize(Xp, F, generator=torch.Generator().manual_seed(i)))))
    cand0 = torch.rand(1, D, dtype=torch.float64, generator=g)
    t_cold = sync_time(lambda: utils.ExpectedImprovement(held["fm"], best_f)(cand0))     # factor + F columns of alpha + one evaluation
    t_warm = sync_time(lambda: utils.ExpectedImprovement(held["fm"], best_f)(cand0))     # the evaluation alone
    t_fac.append(t_cold - t_warm)
say(f"set-up per suggest: fantasize (posterior at the pending points, {F} joint samples, conditioned model incl. its source pass at "
    f"n'={n + p}) {1e3 * statistics.median(t_fz):.3f} ms; target factor (T = 1, n' = {n + p}) + alpha for {F} right-hand sides "
    f"{1e6 * statistics.median(t_fac):.1f} us")

fm = parent.fantasize(Xp, F, generator=torch.Generator().manual_seed(0))
naive = [parent.condition_on_observations(Xp, fm.train_Y[f, n:]).eval() for f in range(F)]
af = {"parent": utils.ExpectedImprovement(parent, best_f), "fantasy": utils.ExpectedImprovement(fm, best_f)}
af_naive = [utils.ExpectedImprovement(m, best_f) for m in naive]
cand = torch.rand(C, D, dtype=torch.float64, generator=g).to(dev)
xr = torch.rand(R, D, dtype=torch.float64, generator=g).to(dev)

variants = {
    "parent score": lambda: af["parent"](cand),
    "fantasy score": lambda: af["fantasy"](cand),
    "naive score": lambda: [a(cand) for a in af_naive],
    "parent value+grad": lambda: af["parent"].value_and_grad(xr),
    "fantasy value+grad": lambda: af["fantasy"].value_and_grad(xr),
    "naive value+grad": lambda: [a.value_and_grad(xr) for a in af_naive],
}
graphs = {"parent value+grad (graph)": GraphedAcquisition(af["parent"].value_and_grad, R, D, dev),
          "fantasy value+grad (graph)": GraphedAcquisition(af["fantasy"].value_and_grad, R, D, dev)}
for k, ga in graphs.items():
    variants[k] = (lambda ga: lambda: ga(xr))(ga)
for fn in variants.values():   # warm-up: code objects, factor caches, allocator
    for _ in range(3):
        fn()
times = {k: [] for k in variants}
for _ in range(reps):
    for k, fn in variants.items():
        times[k].append(sync_time(fn))
med = {k: statistics.median(v) for k, v in times.items()}
for k in variants:
    say(f"{k:30s} median {1e6 * med[k]:9.1f} us  (min {1e6 * min(times[k]):9.1f}, {reps} reps)")
for what in ("score", "value+grad"):
    say(f"{what}: fantasy / parent = {med['fantasy ' + what] / med['parent ' + what]:.2f}x, naive / parent = "
        f"{med['naive ' + what] / med['parent ' + what]:.2f}x")
say(f"value+grad (graph): fantasy / parent = {med['fantasy value+grad (graph)'] / med['parent value+grad (graph)']:.2f}x")

# the fantasy average equals the naive one (same samples)
v_f, g_f = af["fantasy"].value_and_grad(xr)
vg = [a.value_and_grad(xr) for a in af_naive]
v_n, g_n = torch.stack([v for v, _ in vg]).mean(0), torch.stack([gr for _, gr in vg]).mean(0)
rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)   # noqa: E731
say(f"fantasy vs naive average (same samples): max |diff| / max |naive| value {rel(v_f, v_n):.2e} (max |naive| "
    f"{float(v_n.abs().max()):.2e}), gradient {rel(g_f, g_n):.2e}")

# --- one suggest() with 0 and with 4 pending ------------------------------------------------------------------------------
if not args.quick:
    loop = ScaMLGPBOLoop(gps, dim=D, acquisition="ei", num_restarts_log_likelihood=1, seed=0, max_pending_evaluations=p + 1,
                         num_fantasies=F)
    loop.report(Xt, yt.squeeze(-1))
    ts = {0: [], p: []}
    for i in range(4):
        for k in (0, p):
            loop.pending = Xp[:k].clone()
            ts[k].append(sync_time(loop.suggest))
    for k in (0, p):
        say(f"suggest() with {k} pending: median {1e3 * statistics.median(ts[k][1:]):.1f} ms over {len(ts[k]) - 1} calls "
            f"(first {1e3 * ts[k][0]:.1f} ms)")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
