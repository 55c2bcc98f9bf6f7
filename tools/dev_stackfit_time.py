"""Source-stack meta-fit: the host driver (hyper.batched_lbfgs around a replayed HIP graph of the objective) against the device
driver (scaml_stack_fit_f64: fit + gradient + optimiser step enqueued per evaluation, status read once per chunk), at

  configs[4]'s stack   T = 32,  N = 512, D = 6 Matern (Hartmann-6), 1 restart   -> B = 64 problems
  the C3 stack         T = 256, N = 256, D = 8 Matern (smooth fields), 5 restarts -> B = 1536 problems

Both drivers run in ONE process, after a warm-up of each, interleaved repetition by repetition, from identical start points (same
seed); host clock around a fit that ends in a device synchronise; medians.  "evaluations" are objective evaluations of the whole
batch (host driver: calls of the objective; device driver: rounds enqueued).  The device driver is timed for several values of
``evals_per_call`` -- the number of rounds between two reads of the status -- to find the knee.

  python tools/dev_stackfit_time.py [--reps K] [--max-iter I] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-meta-learning-with-gaussian-processes_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from scamlgp_amd import model as M, ops, synthetic, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-iter", type=int, default=30)
ap.add_argument("--chunks", default="1,2,4,8,16,32")
ap.add_argument("--out", default=None)
args = ap.parse_args()
chunks = [int(c) for c in args.chunks.split(",")]
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def run(stack, raw0, restarts, **opts):
    stack.raw = raw0.clone()
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    utils._fit_stack(stack, restarts, max_iter=args.max_iter, **opts)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, int(stack.last_fit_info["n_eval"]), float(stack.last_fit_info["objective"].sum())


say(f"source-stack meta-fit, host driver vs device driver; max_iter = {args.max_iter}, {args.reps} interleaved repetitions, medians")
for name, T, N, D, restarts, make in [("configs[4]", 32, 512, 6, 1, lambda: synthetic.hartmann6_task_stack(32, 512, seed=0)),
                                      ("C3", 256, 256, 8, 5, lambda: synthetic.smooth_field_task_stack(256, 256, 8, seed=0))]:
    d = make()
    stack = M.SourceGPStack(list(range(T)), [torch.from_numpy(d["X"][t]) for t in range(T)],
                            [torch.from_numpy(d["Y"][t]).unsqueeze(-1) for t in range(T)], kind=1, device=dev)
    raw0 = stack.raw.clone()
    variants = [("host", dict(driver="host"))] + [(f"device/{k}", dict(driver="device", evals_per_call=k)) for k in chunks]
    for _, opts in variants[:2]:   # warm-up: code object, allocator, graph capture path
        run(stack, raw0, restarts, **opts)
    times = {v: [] for v, _ in variants}
    evals, objs = {}, {}
    for _ in range(args.reps):
        for v, opts in variants:
            dt, ne, obj = run(stack, raw0, restarts, **opts)
            times[v].append(dt)
            evals[v], objs[v] = ne, obj
    say(f"{name}: T = {T}, N = {N}, D = {D}, {restarts} restart(s), B = {T * (1 + restarts)} problems")
    say(f"  {'driver':12s} {'wall [ms]':>10s} {'evaluations':>12s} {'wall / evaluation [us]':>24s} {'sum of objectives':>20s}")
    for v, _ in variants:
        t = statistics.median(times[v])
        say(f"  {v:12s} {t * 1e3:10.1f} {evals[v]:12d} {t / evals[v] * 1e6:24.1f} {objs[v]:20.6f}")

say(f"default evals_per_call of ops.stack_fit (the device/K row the 'device' driver runs as): {ops.STACK_FIT_EVALS_PER_CALL} -- wall time per "
    "evaluation is flat from there on; larger chunks only add evaluations after the last problem has stopped")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
