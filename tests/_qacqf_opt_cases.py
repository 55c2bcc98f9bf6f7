"""What tests/test_qacqf_opt_emul.py (CPU) and tests/test_qacqf_opt_step_gpu.py (MI355X) share: the test functions of the P-variable
box instance (csrc/gp_qacqf_opt.h) and the driver of its single-threaded host build (tests/host_emul/qacqf_opt_emul.cpp) with a slot
table.  Test infrastructure, not a conftest."""
import ctypes

import numpy as np
import torch

from scamlgp_amd import hyper as H
from scamlgp_amd import synthetic as S
from tests._host_emul import DP as dp, IP as ip, build, ptr

F64 = torch.float64
RUNNING, CONVERGED, FTOL, STALLED, FAILED, MAXITER = range(6)
CONTINUE = 1
EVAL_FN = ctypes.CFUNCTYPE(None)


def neg_hartmann6(x: torch.Tensor):
    """-synthetic.hartmann6 (>= 0: minimising it drives the iterates towards the faces and corners of the unit cube) and its analytic
    gradient, row by row: tests/test_hyper_bounds.py's function, restated here so that no test module is imported for it."""
    A, Pm = torch.from_numpy(S.HARTMANN6_A), torch.from_numpy(S.HARTMANN6_P)
    al = torch.as_tensor(np.asarray(S.HARTMANN_ALPHA_DEFAULT, dtype=np.float64))
    diff = x.unsqueeze(1) - Pm.unsqueeze(0)                      # (B, 4, 6)
    e = al * torch.exp(-(A * diff * diff).sum(-1))               # (B, 4)
    return e.sum(-1), (-2.0 * e.unsqueeze(-1) * A * diff).sum(1)


def host_alone(fun, x0, bounds, **kw):
    """``hyper.batched_lbfgs(bounds=...)`` on ONE start, with the accepted point after every iteration and why it stopped."""
    path = []
    res = H.batched_lbfgs(fun, x0, bounds=bounds, callback=lambda it, x, f, done: path.append((it, x[0].clone(), float(f[0]), bool(done[0]))), **kw)
    if bool(res.failed[0]):
        reason = FAILED
    elif bool(res.converged[0]):
        reason = CONVERGED
    elif not path[-1][3]:
        reason = MAXITER
    elif len(path) > 1 and torch.equal(path[-1][1], path[-2][1]):
        reason = STALLED     # (an accepted step has slope < 0: it moves the point)
    else:
        reason = FTOL
    return res, path, reason


def accepted_points(res):
    """The accepted point of start 0 whenever an iteration ended (the iteration counter moved on, or the start stopped): what the
    host optimiser's ``callback`` sees.  ``res``: ``drive``'s result with one round per call."""
    out, it_prev = [], 0
    for x, _, stats in res["path"]:
        it, status = int(stats[0, 0]), int(stats[0, 2])
        if it != it_prev or status != RUNNING:
            out.append(x[0].copy())
        it_prev = it
        if status != RUNNING:
            break
    return out


def rowsum(t):
    """Row sums in ascending column order (hyper._rowdot's order)."""
    acc = t[:, 0]
    for j in range(1, t.shape[1]):
        acc = acc + t[:, j]
    return acc


def quadratic(P: int, B: int, seed: int = 0):
    """A separable quadratic per start whose optimum lies partly outside [0, 1]^P; the last start lies outside the box.
    Returns (fun(x (k, P), idx) -> (f (k,), g (k, P)) of the MINIMISED function for the starts ``idx``, x0 (B, P))."""
    gen = torch.Generator().manual_seed(1000 * P + seed)
    c = torch.rand(B, P, dtype=F64, generator=gen) * 2.0 - 0.5
    a = 0.5 + 3.0 * torch.rand(B, P, dtype=F64, generator=gen)
    x0 = torch.rand(B, P, dtype=F64, generator=gen)
    x0[-1] = x0[-1] * 3.0 - 1.0

    def fun(x, idx):
        ai, ci = a[idx], c[idx]
        return rowsum(ai * (x - ci) ** 2), 2.0 * ai * (x - ci)

    return fun, x0


def coupled_hartmann(B: int, seed: int = 0, q: int = 4, coupling: float = 0.05):
    """tests/test_hyper_bounds.py's neg_hartmann6 summed over q blocks of 6 variables plus a small coupling between neighbouring
    blocks (P = 6 q): fun as ``quadratic``'s (the same function for every start), x0 (B, 6 q) with the last start outside the box."""
    P = 6 * q
    x0 = torch.rand(B, P, dtype=F64, generator=torch.Generator().manual_seed(77 + seed))
    x0[-1] = x0[-1] * 1.6 - 0.3

    def fun(x, idx):
        k = x.shape[0]
        xb = x.reshape(k, q, 6)
        parts = [neg_hartmann6(xb[:, j]) for j in range(q)]
        f = rowsum(torch.stack([p[0] for p in parts], 1))
        g = torch.stack([p[1] for p in parts], 1)
        d = xb[:, 1:] - xb[:, :-1]                                   # (k, q - 1, 6)
        f = f + coupling * rowsum((d * d).reshape(k, -1))
        g = g.clone()
        g[:, 1:] = g[:, 1:] + 2.0 * coupling * d
        g[:, :-1] = g[:, :-1] - 2.0 * coupling * d
        return f, g.reshape(k, P)

    return fun, x0


def load_emul(tmp_path_factory):
    lib = build(tmp_path_factory, "qacqf_opt_emul")
    i, d = ctypes.c_int, ctypes.c_double
    lib.emul_qacqf_opt_state_doubles.restype, lib.emul_qacqf_opt_state_doubles.argtypes = ctypes.c_longlong, [i] * 2
    lib.emul_qacqf_opt_max_p.restype, lib.emul_qacqf_opt_max_p.argtypes = i, []
    lib.emul_qacqf_opt_step.restype = None
    lib.emul_qacqf_opt_step.argtypes = [dp, dp, ip, dp, dp, dp, dp, dp, dp, dp, ip] + [i] * 7 + [d] * 3
    lib.emul_qacqf_opt_call.restype = None
    lib.emul_qacqf_opt_call.argtypes = [dp, dp, ip, dp, dp, dp, dp, dp, dp, dp, ip] + [i] * 6 + [d] * 3 + [i, ctypes.c_uint, EVAL_FN]
    lib.emul_qacqf_opt_gather.restype = None
    lib.emul_qacqf_opt_gather.argtypes = [dp] * 12 + [i] * 4
    return lib


def box(bounds, P):
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds[0], dtype=np.float64), (P,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds[1], dtype=np.float64), (P,)))
    return lo, hi


def drive(emul, fun, x0, bounds=(0.0, 1.0), max_iter=200, history=10, gtol=1e-5, ftol=2.2e-9, max_ls=20, c1=1e-4, per_call=1,
          compact=False, reverse=False, subset=None, state_fill=0.0, out_fill=0.0):
    """The chunk loop of ``ops.QAcqfOpt.run`` on the CPU.  ``fun(points (k, P), idx) -> (f, g)`` is the MINIMISED function of the
    starts ``idx``; the step is handed the maximised one.  ``subset``: the starts of the first table (default: all); ``reverse``:
    the table in descending order; ``compact``: the stopped starts leave the table after every call (else it never changes).
    Returns the outputs, the state, the accepted points after every call (``path``), the tables (``tables``) and every batch of
    points the function was asked for (``asked``: (slots, Xq rows) copies)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, P = x0.shape
    lo, hi = box(bounds, P)
    state = np.full((B, emul.emul_qacqf_opt_state_doubles(P, history)), state_fill)
    value, grad, Xq = np.zeros(B), np.zeros((B, P)), np.zeros((B, P))
    x, f = np.full((B, P), out_fill), np.full(B, out_fill)
    stats = np.full((B, 4), int(out_fill), dtype=np.int32)
    order = list(range(B)) if subset is None else list(subset)
    if reverse:
        order = order[::-1]
    slots = np.asarray(order, dtype=np.int32)
    asked, path, tables = [], [], []

    def evaluate():
        k = slots.shape[0]
        pts = Xq[:k].copy()
        asked.append((slots.copy(), pts))
        fv, gv = fun(torch.from_numpy(pts), slots.tolist())
        value[:k] = -fv.numpy()
        grad[:k] = -gv.numpy()

    cb = EVAL_FN(evaluate)
    budget = 1 + max_iter * max_ls
    rounds = calls = 0
    while True:
        k = min(per_call, budget - rounds)
        tables.append(slots.copy())
        emul.emul_qacqf_opt_call(ptr(value), ptr(grad), ptr(slots), ptr(x0), ptr(lo), ptr(hi), ptr(state), ptr(Xq), ptr(x), ptr(f), ptr(stats),
                                 B, int(slots.shape[0]), P, max_iter, history, max_ls, gtol, ftol, c1, k, CONTINUE if calls else 0, cb)
        rounds += k
        calls += 1
        path.append((x.copy(), f.copy(), stats.copy()))
        running = [b for b in slots.tolist() if stats[b, 2] == RUNNING]
        if not running or rounds >= budget:
            break
        if compact:
            slots = np.asarray(running, dtype=np.int32)
    return dict(x=x, f=f, stats=stats, state=state, rounds=rounds, calls=calls, path=path, asked=asked, tables=tables)
