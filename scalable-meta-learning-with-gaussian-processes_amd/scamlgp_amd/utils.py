"""Host-side mirror of ``scamlgp/utils.py``: marginal-likelihood fitting with restarts and the
acquisition functions, on top of the batched GPU path.

  optimize_marginal_likelihood   scamlgp/utils.py:139-212  (warm start + ``num_restarts`` prior
                                 samples, keep the best state, ModelFittingError if all failed)
  UpperConfidenceBound           scamlgp/utils.py:215-224  (beta = 9, maximize=False)
  ExpectedImprovement            scamlgp/optimizer.py:96-98 (botorch analytic EI, minimisation)
"""
from __future__ import annotations

import logging
import math
from typing import Dict, Optional, Sequence, Union

import numpy as np
import scipy.optimize
import torch

from . import dist as sdist
from . import hyper
from . import ops, studies
from .model import ScaMLGP, SourceGP, SourceGPStack

logger = logging.getLogger("scamlgp_amd")


class ModelFittingError(RuntimeError):
    """All optimisation attempts failed (mirrors botorch.exceptions.ModelFittingError)."""


def capture_graph(fn, device, warmup: int):
    """Capture one call of ``fn()`` into a HIP graph: ``warmup`` eager calls on a side stream first (allocator state, lazy module
    load, workspaces: all outside the graph's pool), then the captured call.  Returns (graph, outputs); ``graph.replay()`` recomputes
    ``outputs`` -- a tensor or a tuple of tensors -- in place from the static buffers ``fn`` reads."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outputs = fn()
    return graph, outputs


class _GraphedBatchObjective:
    """``fun(x) -> (f (B,), g (B, P))`` of the batched L-BFGS (one fused fit + one gradient launch + constraint transform, priors
    and their autograd backward: ~40 launches around ~0.1 ms of GPU work for a small stack) captured once into a HIP graph on a
    static input buffer and replayed per evaluation.  ``ok`` is False if capture is not possible; the caller keeps the eager one."""

    def __init__(self, fun, x0: torch.Tensor):
        self.ok = False
        dev = x0.device
        try:
            self.x = x0.detach().clone()
            # (the warm-up also allocates the factor buffers and the gradient workspace outside the graph's pool)
            self.graph, (self.f, self.g) = capture_graph(lambda: fun(self.x), dev, warmup=3)
            self.ok = True
        except Exception as e:
            logger.warning("stack objective: HIP graph capture failed (%s); evaluating eagerly", e)
            torch.cuda.synchronize(dev)

    def __call__(self, x: torch.Tensor):
        self.x.copy_(x)
        self.graph.replay()
        return self.f.clone(), self.g.clone()


def _stack_starts(stack: SourceGPStack, num_restarts: int) -> torch.Tensor:
    """Warm start + ``num_restarts`` prior samples per task, problem b = rep * T + task."""
    starts = [stack.raw.clone()]
    for _ in range(num_restarts):
        starts.append(stack.spec.to_raw(stack.spec.sample_prior((stack.T,), stack.D, device=stack.device)))
    return torch.cat(starts, 0)


def _keep_best(stack: SourceGPStack, x: torch.Tensor, f: torch.Tensor, reps: int, info: dict) -> None:
    """Best-of-starts per task (f (reps * T,), inf = failed attempt), then the stack's factors at the chosen parameters."""
    T, D = stack.T, stack.D
    f = f.reshape(reps, T)
    best = f.argmin(0)
    if bool(torch.isinf(f.min(0).values).any()):
        bad = torch.nonzero(torch.isinf(f.min(0).values)).flatten().tolist()
        raise ModelFittingError(
            "Hyperparameter optimization failed for all attempts. Usually this indicates a problem with model's "
            f"input data or hyperparameter priors definitions. (tasks {[stack.task_ids[i] for i in bad][:8]})")
    n_failed = int(torch.isinf(f).sum())
    if n_failed:
        logger.warning("%d of %d hyper-parameter optimisation attempts failed and were skipped.", n_failed, f.numel())
    stack.raw = x.reshape(reps, T, D + 2)[best, torch.arange(T, device=stack.device)].contiguous()
    stack.refresh()
    obj = -f.min(0).values
    # (a sharded stack also reports the objective summed over every rank's tasks: the fit's one collective)
    total = sdist.fused_allreduce([obj.sum().reshape(1)], stack.shard)[0]
    stack.last_fit_info = dict(objective=obj, objective_sum=total.squeeze(0), **info)


def _fit_stack_device(stack: SourceGPStack, num_restarts: int, max_iter: int, evals_per_call=None) -> None:
    """``_fit_stack`` with the optimiser on the device: ``ops.stack_fit`` enqueues fit + gradient + L-BFGS step for all problems and
    reads only the status column back, once per chunk of evaluations."""
    reps = 1 + num_restarts
    x0 = _stack_starts(stack, num_restarts)
    c = stack._replicated(reps)
    res = ops.stack_fit(c["X"], c["y"], c["npts"], stack.spec, x0, stack.kind, max_iter=max_iter, evals_per_call=evals_per_call)
    status = res["stats"][:, 2].to(stack.device)
    f = -res["value"]
    f = torch.where((status == 4) | ~torch.isfinite(f), torch.full_like(f, float("inf")), f)
    _keep_best(stack, res["z"], f, reps, dict(n_iter=int(res["stats"][:, 0].max()), n_eval=res["n_eval"], stats=res["stats"]))


def _fit_stack(stack: SourceGPStack, num_restarts: int, max_iter: int = 200, use_graph: bool = True, driver: str = "host",
               evals_per_call=None) -> None:
    """All T tasks x (1 + num_restarts) starts as ONE batch: every L-BFGS iteration is one fused-fit
    launch + one gradient launch over (1 + R) * T problems.  ``driver="device"`` keeps the optimiser itself on the device as well
    (``scaml_stack_fit_f64``: same starts, same algorithm per problem, no host round trip per evaluation)."""
    if getattr(stack, "parent", None) is not None:
        raise RuntimeError("a slice's hyper-parameters belong to its parent stack: fit the parent")
    if driver == "device":
        return _fit_stack_device(stack, num_restarts, max_iter, evals_per_call)
    if driver != "host":
        raise ValueError(f"driver must be 'host' or 'device', got {driver!r}")
    reps = 1 + num_restarts
    x0 = _stack_starts(stack, num_restarts)
    fun = lambda r: stack.objective(r, reps)   # noqa: E731
    if use_graph and stack.device.type == "cuda":
        gfun = _GraphedBatchObjective(fun, x0)
        if gfun.ok:
            fun = gfun
    res = hyper.batched_lbfgs(fun, x0, max_iter=max_iter)
    f = torch.where(res.failed | ~torch.isfinite(res.f), torch.full_like(res.f, float("inf")), res.f)
    _keep_best(stack, res.x, f, reps, dict(n_iter=res.n_iter, n_eval=res.n_eval))


class _GraphedObjective:
    """-mll(z) and its gradient for z = [raw_theta || raw_weights] of a ScaMLGP, captured once (torch.cuda.graph: autograd's
    backward included) and replayed.  ``ok`` is False if capture is not possible on this build; the caller then evaluates eagerly."""

    def __init__(self, model: ScaMLGP, D2: int):
        self.ok = False
        dev = model.device
        try:
            self.z = torch.zeros(D2 + model.T, dtype=torch.float64, device=dev, requires_grad=True)
            self.z.data.copy_(torch.cat([model.raw_theta, model.raw_weights]))
            self.host = torch.empty(1 + D2 + model.T, dtype=torch.float64).pin_memory()

            def body():
                val = -model.mll(self.z[:D2], self.z[D2:])
                (g,) = torch.autograd.grad(val, self.z)
                return torch.cat([val.detach().reshape(1), g])

            self.graph, self.out = capture_graph(body, dev, warmup=3)
            self.ok = True
        except Exception as e:  # capture unsupported for some op on this build: eager evaluation is always available
            logger.warning("target objective: HIP graph capture failed (%s); evaluating eagerly", e)
            torch.cuda.synchronize(dev)

    def __call__(self, z: np.ndarray) -> np.ndarray:
        self.z.data.copy_(torch.from_numpy(z), non_blocking=False)
        self.graph.replay()
        self.host.copy_(self.out, non_blocking=False)
        return self.host.numpy()


def _fit_target_scipy(model: ScaMLGP, starts: torch.Tensor, maxiter: int, use_graph: bool):
    """The refit where the library's target-fit kernel does not take the shape (n beyond its LDS, D > 16): scipy L-BFGS-B per
    start point, objective and gradient from torch autograd on the device (``ScaMLGP.mll``), replayed from a HIP graph.
    Returns (z (B, P), f (B,)) with f = -mll at the end points (inf for a failed run)."""
    D2, T = model.raw_theta.numel(), model.T
    bounds = [(None, None)] * D2 + [(model.weights_lower_bound, None)] * T

    def fun_eager(z: np.ndarray):
        zt = torch.tensor(z, dtype=torch.float64, device=model.device, requires_grad=True)
        try:
            val = -model.mll(zt[:D2], zt[D2:])
            (g,) = torch.autograd.grad(val, zt)
        except RuntimeError:  # Cholesky failure somewhere in the line search
            return float("inf"), np.zeros_like(z)
        v = float(val.detach())
        if not math.isfinite(v):
            return float("inf"), np.zeros_like(z)
        return v, g.cpu().numpy()

    # ~100 small launches per evaluation: forward AND backward are captured once into a HIP graph on static buffers and replayed per
    # evaluation; one device -> host copy of [value || gradient] per evaluation is the only synchronisation.
    graphed = _GraphedObjective(model, D2) if use_graph and model.device.type == "cuda" else None

    def fun(z: np.ndarray):
        if graphed is None or not graphed.ok:
            return fun_eager(z)
        out = graphed(z)
        v = float(out[0])
        if not math.isfinite(v):
            return float("inf"), np.zeros_like(z)
        return v, out[1:].copy()

    zs, fs = [], []
    for z0 in starts.cpu().numpy():
        r = scipy.optimize.minimize(fun, z0, jac=True, method="L-BFGS-B", bounds=bounds, options=dict(maxiter=maxiter))
        zs.append(torch.from_numpy(np.asarray(r.x, dtype=np.float64)))
        fs.append(float(r.fun))
    return torch.stack(zs), torch.tensor(fs, dtype=torch.float64)


def _target_starts(model: ScaMLGP, num_restarts: int) -> torch.Tensor:
    """(1 + num_restarts, P): the warm start, then prior samples of the hyper-parameters and weights (global torch RNG, one restart
    after the other: scamlgp/utils.py:184-199)."""
    D2, T = model.raw_theta.numel(), model.T
    starts = [torch.cat([model.raw_theta, model.raw_weights])]
    for _ in range(num_restarts):
        th = model.spec.sample_prior((), D2 - 2, device=model.device)
        w = model.weights_prior.sample((T,), device=model.device).clamp_min(model.weights_lower_bound)
        starts.append(torch.cat([model.spec.to_raw(th), w]))
    return torch.stack(starts)


def _kernel_fit_objective(model: ScaMLGP, res: dict) -> torch.Tensor:
    """f (B,) = -mll at the end points of a device refit (``ops.target_fit``, or one problem's rows of ``ops.target_fit_batched``), inf
    for a run that failed; records the run in ``model.last_fit_info``."""
    f = -res["value"]
    f = torch.where(torch.isfinite(f) & (res["stats"][:, 2] != 4), f, torch.full_like(f, float("inf")))
    model.last_fit_info = dict(stats=res["stats"], objective=res["value"])
    return f


def _best_start(z: torch.Tensor, f, best: torch.Tensor) -> None:
    """The best end point into ``best`` = [state || ok] (ok stays 0 if every start failed); f (B,) on the device or already on the host."""
    n_failed = int(torch.isinf(f).sum())     # (the one host synchronisation of the refit, unless f is a host tensor)
    if n_failed and n_failed < f.numel():
        logger.warning("Error occurred while optimizing the model hyperparameters; %d restart(s) will be skipped.", n_failed)
    if n_failed < f.numel():
        best[:-1] = z[int(f.argmin())]
        best[-1] = 1.0


def _load_best(model: ScaMLGP, best: torch.Tensor, ok: bool) -> None:
    """The end of a refit: ``best`` = [state || ok] becomes the model's state, or ModelFittingError if no start succeeded."""
    if not ok:
        raise ModelFittingError("Hyperparameter optimization failed for all attempts. Usually this indicates a problem with "
                                "model's input data or hyperparameter priors definitions.")
    D2 = model.raw_theta.numel()
    model.load_state_dict({"raw_theta": best[:D2].clone(), "raw_weights": best[D2:-1].clone()})


def _fit_target(model: ScaMLGP, num_restarts: int, maxiter: int = 200, use_graph: bool = True, use_kernel: bool = True) -> None:
    """Target GP: weights + kernel hyper-parameters (scamlgp/optimizer.py:176-185 -> scamlgp/utils.py:139-212).  The warm start
    and the ``num_restarts`` prior-sampled starts are ONE batch; ``scaml_target_fit_f64`` runs all their L-BFGS optimisations
    (box bound w >= 1e-10, scamlgp/model.py:334) to convergence in one launch on the device; the best end point is kept.
    On a sharded model rank 0 fits and broadcasts the result: every rank must hold the same weights and hyper-parameters (the
    weighted sums the ranks all-reduce in ``_source_prior`` are built from them)."""
    if model.n == 0:
        return
    shard = model._shard
    D2, T = model.raw_theta.numel(), model.T
    best = torch.zeros(D2 + T + 1, dtype=torch.float64, device=model.device)   # [state || ok]
    if shard is None or shard.rank == 0:
        z0 = _target_starts(model, num_restarts)
        prob = model.target_problem() if (use_kernel and model.device.type == "cuda") else None
        if prob is not None:
            res = ops.target_fit(prob, z0, max_iter=maxiter)
            z, f = res["z"], _kernel_fit_objective(model, res)
        else:
            z, f = _fit_target_scipy(model, z0, maxiter, use_graph)
            z, f = z.to(model.device), f.to(model.device)
        _best_start(z, f, best)
    if shard is not None and shard.world > 1:
        import torch.distributed as dist

        dist.broadcast(best, src=dist.get_global_rank(shard.group, 0) if shard.group is not None else 0, group=shard.group)
    _load_best(model, best, float(best[-1]) == 1.0)


def fit_targets_batched(models: Sequence[ScaMLGP], num_restarts: int, maxiter: int = 200, rng: Optional[Sequence[torch.Generator]] = None,
                        **fit_options) -> None:
    """``optimize_marginal_likelihood(model, num_restarts)`` for several ScaMLGP models -- on one source stack, or each on its own
    (slices of one parent, ``model.meta_fit_scamlgp_studies``: the kernel takes means and covariances per problem; the models need only
    agree in T, D and the kernel family) --, with every model the
    library's target-fit kernel takes refitted in ONE launch (``scaml_target_fit_batched_f64``: models x (1 + num_restarts) workgroups
    instead of 1 + num_restarts per launch, one launch after the other).  Per model the starts, the device optimisation and the
    best-of-restarts choice are those of the single call, so the fitted state is the same.  ``rng[i]``: the generator model i's
    restart samples are drawn from (its state stands in for the global RNG's while they are drawn, and moves on); None: the global RNG,
    model after model.  A model the kernel does not take (n beyond its LDS, D > 16) is refitted by the single call, on its own."""
    models = list(models)
    for m in models:
        if not isinstance(m, ScaMLGP):
            raise TypeError(f"cannot fit a {type(m).__name__}")
        if m.num_fantasies is not None:
            raise NotImplementedError("a fantasy model is not refitted: it keeps its parent's hyper-parameters")
        if m._shard is not None:
            raise NotImplementedError("the batched refit is not implemented for a task-sharded source stack (shard=True)")
    batch, starts = [], []
    for i, m in enumerate(models):
        if m.n == 0:
            continue
        with _rng_of(rng[i] if rng is not None else None):
            prob = m.target_problem() if m.device.type == "cuda" else None
            if prob is None:
                optimize_marginal_likelihood(m, num_restarts, maxiter=maxiter, **fit_options)
                continue
            starts.append(_target_starts(m, num_restarts))
        batch.append((m, prob))
    if not batch:
        return
    res = ops.target_fit_batched(ops.TargetFitBatch([p for _, p in batch]), torch.stack(starts), max_iter=maxiter)
    fs = [_kernel_fit_objective(m, {k: v[s] for k, v in res.items()}) for s, (m, _) in enumerate(batch)]
    f_host = torch.stack(fs).cpu()   # (the one host synchronisation of all the refits)
    for s, (m, _) in enumerate(batch):
        best = torch.zeros(m.raw_theta.numel() + m.T + 1, dtype=torch.float64, device=m.device)
        _best_start(res["z"][s], f_host[s], best)
        _load_best(m, best, float(f_host[s].min()) != float("inf"))   # (decided on the host copy: no further synchronisation)


class _rng_of:
    """While active, the global CPU RNG continues ``gen``'s stream (torch.distributions draws from the global RNG only); on exit
    ``gen`` holds the advanced state and the global RNG is back where it was.  ``gen`` None: nothing happens."""

    def __init__(self, gen: Optional[torch.Generator]):
        self.gen = gen

    def __enter__(self):
        if self.gen is not None:
            self.saved = torch.get_rng_state()
            torch.set_rng_state(self.gen.get_state())

    def __exit__(self, *exc):
        if self.gen is not None:
            self.gen.set_state(torch.get_rng_state())
            torch.set_rng_state(self.saved)
        return False


def optimize_marginal_likelihood(model: Union[SourceGPStack, ScaMLGP, Dict, SourceGP], num_restarts: int = 0, **fit_options):
    """Refit the model's hyper-parameters by maximising the marginal log likelihood (+ priors) on its
    training data: once warm-started from the current parameters, ``num_restarts`` times from prior
    samples; the best state is kept (scamlgp/utils.py:139-212)."""
    if isinstance(model, dict):
        model = list(model.values())[0]
    if isinstance(model, SourceGP):
        model = model._stack
    if isinstance(model, SourceGPStack):
        return _fit_stack(model, num_restarts, **fit_options)
    if isinstance(model, ScaMLGP):
        if model.num_fantasies is not None:
            raise NotImplementedError("a fantasy model is not refitted: it keeps its parent's hyper-parameters")
        return _fit_target(model, num_restarts, **fit_options)
    raise TypeError(f"cannot fit a {type(model).__name__}")


# --- acquisition functions (to be MAXIMISED, for minimising the objective) -------------------------
def _single_q(X: torch.Tensor) -> torch.Tensor:
    """botorch's analytic acquisition functions take ``batch_shape x 1 x d`` (t_batch_mode_transform(expected_q=1)) and return
    ``batch_shape`` values; a q > 1 batch is an error there and here.  X (M, D) -- this package's flat list of M points -- passes."""
    if X.dim() > 2 and X.shape[-2] != 1:
        raise ValueError(f"analytic acquisition functions take q = 1 (X of shape batch_shape x 1 x d), got q = {X.shape[-2]}")
    return X


def _drop_q(X: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    return v.squeeze(-1) if X.dim() > 2 else v


def _fantasy_value(model: ScaMLGP, X: torch.Tensor, acqf: int, param: float) -> torch.Tensor:
    """A fantasy model's acquisition value at X (M, D) or (*batch, 1, D), averaged over its fantasies."""
    v, _ = model.fantasy_acqf(X.reshape(-1, X.shape[-1]), acqf, param)
    return _drop_q(X, v.reshape(X.shape[:-1]))


class _AnalyticAcquisition:
    """What the three acquisition classes share: ``code`` (the library's ops.ACQF_*) and ``param`` (UCB's beta, best_f of EI and LogEI)
    for the library's kernels, and the fantasy-model branch of ``__call__`` / ``value_and_grad``.  A class states its formulas on an
    ordinary model in ``_value`` / ``_value_and_grad``."""

    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        X = _single_q(X)
        if self.model.num_fantasies is not None:
            return _fantasy_value(self.model, X, self.code, self.param)
        return _drop_q(X, self._value(X))

    def value_and_grad(self, X: torch.Tensor):
        """(value (M,), d value / d X (M, D)) from the model's analytic posterior gradients (ScaMLGP.posterior_with_grad); on a fantasy
        model the value over the fantasies (``ScaMLGP.fantasy_acqf``) and its exact gradient."""
        if self.model.num_fantasies is not None:
            return self.model.fantasy_acqf(X, self.code, self.param, want_grad=True)
        return self._value_and_grad(X)


class UpperConfidenceBound(_AnalyticAcquisition):
    """botorch UpperConfidenceBound(model, beta=9.0, maximize=False) (scamlgp/utils.py:215-224):
    value = -mu + sqrt(beta * var) per query point; X (M, D) -> (M,).  On a fantasy model (ScaMLGP.fantasize) the value is the
    mean over the fantasies of the per-fantasy value (``ScaMLGP.fantasy_acqf``)."""

    code = ops.ACQF_UCB
    param = property(lambda self: self.beta)

    def __init__(self, model: ScaMLGP, beta: float = 9.0):
        self.model, self.beta = model, beta

    def _value(self, X: torch.Tensor) -> torch.Tensor:
        mvn = self.model.posterior(X).mvn
        return -mvn.mean + torch.sqrt(self.beta * mvn.variance.clamp_min(0.0))

    def _value_and_grad(self, X: torch.Tensor):
        mu, var, dmu, dvar = self.model.posterior_with_grad(X)
        sd = torch.sqrt(self.beta * var.clamp_min(0.0))
        # d sqrt(beta var) = beta dvar / (2 sqrt(beta var)); zero where the variance is clamped
        coef = torch.where(var > 0, 0.5 * self.beta / sd.clamp_min(1e-300), torch.zeros_like(sd))
        return -mu + sd, -dmu + coef.unsqueeze(-1) * dvar


class ExpectedImprovement(_AnalyticAcquisition):
    """botorch analytic ExpectedImprovement(model, best_f, maximize=False) (scamlgp/optimizer.py:96-98):
    sigma = sqrt(max(var, 1e-9)), u = -(mu - best_f) / sigma, EI = sigma (phi(u) + u Phi(u)).  On a fantasy model: the mean over the
    fantasies of the per-fantasy EI, best_f still the caller's incumbent over observed data."""

    code = ops.ACQF_EI
    param = property(lambda self: self.best_f)

    def __init__(self, model: ScaMLGP, best_f: float):
        self.model, self.best_f = model, best_f

    def _value(self, X: torch.Tensor) -> torch.Tensor:
        mvn = self.model.posterior(X).mvn
        sigma = mvn.variance.clamp_min(1e-9).sqrt()
        u = -(mvn.mean - self.best_f) / sigma
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
        return sigma * (pdf + u * cdf)

    def _value_and_grad(self, X: torch.Tensor):
        """d EI = -Phi(u) d mu + phi(u) d sigma, d sigma = d var / (2 sigma) (zero where the variance sits on the 1e-9 floor)."""
        mu, var, dmu, dvar = self.model.posterior_with_grad(X)
        sigma = var.clamp_min(1e-9).sqrt()
        u = -(mu - self.best_f) / sigma
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
        dsig = torch.where(var > 1e-9, 0.5 / sigma, torch.zeros_like(sigma)).unsqueeze(-1) * dvar
        return sigma * (pdf + u * cdf), -cdf.unsqueeze(-1) * dmu + pdf.unsqueeze(-1) * dsig


class LogExpectedImprovement(_AnalyticAcquisition):
    """botorch LogExpectedImprovement(model, best_f, maximize=False): the logarithm of ``ExpectedImprovement``, with its clamp,
    log sigma + g(u), g(u) = log(phi(u) + u Phi(u)), evaluated without cancellation so that value and gradient stay finite and
    accurate where EI underflows to an exact 0 (u below about -38).  The transform of the posterior is the library's
    (``ops.acqf_transform``, include/scaml_gp.h (7o)) for every n, the prior-only model included.  On a fantasy model: the log of the
    MEAN EI over the fantasies (a log-sum-exp of the per-fantasy values), ``ScaMLGP.fantasy_acqf`` with ``ops.ACQF_LOGEI``."""

    code = ops.ACQF_LOGEI
    param = property(lambda self: self.best_f)

    def __init__(self, model: ScaMLGP, best_f: float):
        self.model, self.best_f = model, best_f

    def _value(self, X: torch.Tensor) -> torch.Tensor:
        mvn = self.model.posterior(X).mvn
        mu = mvn.mean
        A, _, _ = ops.acqf_transform(mu.detach(), mvn.variance.detach(), ops.ACQF_LOGEI, self.best_f, want_factors=False)
        return A.reshape(mu.shape)

    def _value_and_grad(self, X: torch.Tensor):
        """d LogEI = dA/dmu d mu + dA/dvar d var."""
        mu, var, dmu, dvar = self.model.posterior_with_grad(X)
        A, Amu, Av = ops.acqf_transform(mu, var, ops.ACQF_LOGEI, self.best_f)
        return A, Amu.unsqueeze(-1) * dmu + Av.unsqueeze(-1) * dvar


class _JointAcquisition:
    """What qEI and qUCB share: a Monte-Carlo acquisition function over the JOINT posterior of the q points of a batch (botorch's
    qExpectedImprovement / qUpperConfidenceBound under optimize_acqf(q = ...)), evaluated by ``ScaMLGP.joint_acqf``.  The base samples
    are drawn ONCE at construction with ``torch.randn`` from ``generator`` -- (num_samples, 8), of which a batch of q points reads the
    leading q columns -- and stay fixed: the function is deterministic, as L-BFGS-B needs it.  ``q`` is fixed by the ``q`` argument
    or by the first batch.

    ``X_pending`` (p, D): evaluations that are running (botorch's X_pending).  They are appended to every batch and held fixed: the
    utility's maximum runs over the q + p joint samples, a batch reads the leading q + p columns of the draws, and the gradient is the
    q moving points'.  What depends on the pending set alone (``ScaMLGP.joint_pending``) is computed here, once, for the model's
    parameters as they are now.

    ``score_mode``: how ``__call__`` (values only: an optimiser's scoring of raw candidates and of its end points) is evaluated.
    ``"grad_pass"`` (default): through ``ScaMLGP.joint_acqf``, the route of ``value_and_grad``, a strip of the source pass per point.
    ``"value_pass"``: through ``ScaMLGP.joint_acqf_value``, 16 points per strip and no derivative columns; the values agree with the
    default's to the rounding of the two source passes.  ``value_and_grad`` is the same in both modes."""

    SCORE_MODES = ("grad_pass", "value_pass")
    # __call__ in "value_pass" mode chunks in whole strips so that the source pass's covariance block, T (n + p + q) Mp doubles, stays
    # within this (StudiesAcquisition.SCORE_COV_CAP_BYTES' figure)
    SCORE_COV_CAP_BYTES = 256 << 20

    def __init__(self, model: ScaMLGP, num_samples: int = 128, generator: Optional[torch.Generator] = None, q: Optional[int] = None,
                 X_pending: Optional[torch.Tensor] = None, score_mode: str = "grad_pass"):
        if score_mode not in self.SCORE_MODES:
            raise ValueError(f"score_mode must be one of {self.SCORE_MODES}, got {score_mode!r}")
        self.score_mode = score_mode
        if model.num_fantasies is not None:
            raise NotImplementedError("the joint acquisition functions are not defined on a fantasy model")
        if not 1 <= num_samples <= ops.qacqf_max_samples():
            raise ValueError(f"num_samples must be within 1 .. {ops.qacqf_max_samples()}")
        self.model, self.num_samples = model, int(num_samples)
        self.p, self._pending = 0, None
        if X_pending is not None and torch.as_tensor(X_pending).numel() > 0:
            self._pending = model.joint_pending(X_pending)
            self.p = int(self._pending["Xp"].shape[0])
        # (num_samples, max q) draws, once; a batch of q points reads the leading q (+ p) columns
        self._eps = torch.randn(self.num_samples, ops.qacqf_max_q(), dtype=torch.float64, generator=generator).to(model.device)
        self.q, self.base_samples = None, None
        if q is not None:
            self._draw(int(q))

    def _draw(self, q: int) -> None:
        if not 1 <= q <= ops.qacqf_max_q():
            raise ValueError(f"q must be within 1 .. {ops.qacqf_max_q()}")
        if q + self.p > ops.qacqf_max_q():
            raise NotImplementedError(f"the joint acquisition kernel takes q + p <= {ops.qacqf_max_q()} points, got q = {q} and {self.p} pending")
        self.q, self.base_samples = q, self._eps[:, :q + self.p].contiguous()

    def _batches(self, X: torch.Tensor) -> torch.Tensor:
        X = torch.as_tensor(X, dtype=torch.float64)
        if X.dim() == 2:   # one batch (q, D); with q = 1, M single points (M, D), as the analytic functions read a flat list
            X = X.unsqueeze(1) if self.q == 1 else X.unsqueeze(0)
        if X.dim() != 3:
            raise ValueError("a joint acquisition function takes X (B, q, D)")
        if self.q is None:
            self._draw(int(X.shape[1]))
        if X.shape[1] != self.q:
            raise ValueError(f"this acquisition function was drawn for q = {self.q}, got q = {X.shape[1]}")
        return X

    def _value_pass_step(self) -> int:
        """Batches per call of the value route: whole strips, the covariance block within SCORE_COV_CAP_BYTES (one strip at the least)."""
        bps = 16 // self.q
        rows = self.model.n + self.p + self.q
        strips = int(self.SCORE_COV_CAP_BYTES) // (8 * self.model._stack.T * rows * 16)
        return max(1, strips) * bps

    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        X = self._batches(X)
        if self.score_mode == "value_pass":
            step = self._value_pass_step()
            vals = [self.model.joint_acqf_value(X[i:i + step], self.code, self.param, self.base_samples, X_pending=self._pending)
                    for i in range(0, X.shape[0], step)]
            return torch.cat(vals) if vals else X.new_empty((0,))
        # (in chunks of at most 256 points: the pass keeps 16 columns per point and covariance row, for every task)
        step = max(1, 256 // self.q)
        vals = [self.model.joint_acqf(X[i:i + step], self.code, self.param, self.base_samples, X_pending=self._pending)[0]
                for i in range(0, X.shape[0], step)]
        return torch.cat(vals) if vals else X.new_empty((0,))

    def value_and_grad(self, X: torch.Tensor):
        """(value (B,), d value / d X (B, q, D)), the exact gradient of the Monte-Carlo estimate at the fixed base samples."""
        return self.model.joint_acqf(self._batches(X), self.code, self.param, self.base_samples, want_grad=True, X_pending=self._pending)

    def optimize(self, x0: torch.Tensor, max_iter: int, evals_per_call: Optional[int] = None, **options) -> dict:
        """Maximise the function over [0, 1]^D from every batch of x0 (R, q, D) ON THE DEVICE (``ops.QAcqfOpt``, scaml_qacqf_opt_f64):
        R independent box L-BFGS runs whose rounds -- the launches of ``value_and_grad`` and the optimiser step -- are enqueued
        ``evals_per_call`` at a time without the host; between calls the status is read and the stopped starts leave the evaluation.
        The host twin is ``hyper.batched_lbfgs(fun, x0.reshape(R, q D), bounds=(0, 1))`` on ``value_and_grad``.  ``options``: history,
        max_ls, gtol, ftol, c1.  Returns dict(x (R, q, D), f (R,) the value AT x (-inf for a start whose first evaluation is not
        finite), stats (R, 4) int32 on the host [iterations, evaluations, status, pairs], n_eval rounds enqueued, n_calls, live: the
        starts evaluated by each call)."""
        X = self._batches(x0)
        R, q, D = X.shape
        dev = self.model.device
        kw = self.model.joint_acqf_opt_inputs(self.base_samples, self._pending)
        lo, hi = torch.zeros(q * D, dtype=torch.float64, device=dev), torch.ones(q * D, dtype=torch.float64, device=dev)
        opt = ops.QAcqfOpt(kw, X.to(dev).contiguous(), self.code, self.param, lo, hi, int(max_iter), **options)
        return opt.run(evals_per_call)


class qExpectedImprovement(_JointAcquisition):
    """botorch qExpectedImprovement (minimisation): (1/S) sum_s max_j max(best_f - f_sj, 0) over S joint posterior samples of the batch."""

    code = ops.ACQF_EI
    param = property(lambda self: self.best_f)

    def __init__(self, model: ScaMLGP, best_f: float, num_samples: int = 128, generator: Optional[torch.Generator] = None, q: Optional[int] = None,
                 X_pending: Optional[torch.Tensor] = None, score_mode: str = "grad_pass"):
        super().__init__(model, num_samples, generator, q, X_pending, score_mode)
        self.best_f = float(best_f)


class qUpperConfidenceBound(_JointAcquisition):
    """botorch qUpperConfidenceBound (minimisation): (1/S) sum_s max_j (-mu_j + sqrt(beta pi / 2) |f_sj - mu_j|)."""

    code = ops.ACQF_UCB
    param = property(lambda self: self.beta)

    def __init__(self, model: ScaMLGP, beta: float = 9.0, num_samples: int = 128, generator: Optional[torch.Generator] = None, q: Optional[int] = None,
                 X_pending: Optional[torch.Tensor] = None, score_mode: str = "grad_pass"):
        super().__init__(model, num_samples, generator, q, X_pending, score_mode)
        self.beta = float(beta)


class StudiesAcquisition:
    """The acquisition functions of S ScaMLGP models on ONE source stack (or on slices of one: see below), evaluated together: ``value_and_grad(X, group)`` is two
    library launches whatever S is -- the grouped GRAD source pass (``ops.source_posteriors_grad_grouped``: a query point's covariance
    block is taken against ITS study's training inputs) and the batched target acquisition (``ops.target_acqf_batched``: weighted
    task sums, Knq, the solve against the study's cached factor of Knn, posterior, gradient, UCB / EI) -- where each model's own
    ``af.value_and_grad`` is about fifteen.  Nothing is read back and every status stays on the device, so an evaluation can be
    captured into a HIP graph (``bo.GraphedAcquisition``).

    ``afs``: one ``UpperConfidenceBound``, ``ExpectedImprovement`` or ``LogExpectedImprovement`` per study, all of the same class, on models that share the source
    stack and the kernel family and ``supports_posterior_grad()``.  Built once per parameter state: the per-study
    arrays (pruned weights and mask, theta, training inputs, standardiser, the factor ``_target_factor()`` -- computed through the
    model's own posterior path where it is absent --, alpha, beta or best_f) are packed from the models' caches here, padded to the
    largest n.  The models' ``_train_VA()`` tensors are passed by address (10 MB each at configs[4]: no padded copy); this object
    keeps them alive.

    Per-study source stacks: the models' stacks may instead be slices of one parent with an equal number of tasks T
    (``model.meta_fit_scamlgp_studies``).  The source pass then reads the PARENT's arrays with ``task_base[g]`` = the first task of
    study g (``scaml_posterior_linv_grad_grouped_own_f64``: a study's query points meet only its own T tasks, the grid stays T x Mq);
    ``w`` / ``active`` stay (G, T) per slice.  ``task_base`` is None on the shared-stack path.

    Studies with pending evaluations: a model may be a fantasy model (``ScaMLGP.fantasize``, at most 64 fantasies, n + p <= 96 training
    and pending points).  It is packed with its n + p inputs, the factor of that block, its ``_train_VA()`` of the n + p points and the
    F columns of alpha (``alpha_f`` (G, n_max, F_max), ``n_fant``; an ordinary model is F = 1 with its alpha in column 0), which it gets
    through its own ``fantasy_acqf``.  A set with a fantasy model (``self.fantasy``) goes through the ``ops.target_fantasy_*`` entry
    points and ``scaml_studies_fantasy_acqf_opt_f64`` -- UCB / EI averaged over a study's fantasies, the ordinary studies' results bit for
    bit what they are without the fantasy models --; a set without one makes the calls it always made."""

    SCORE_COV_CAP_BYTES = 256 << 20   # `score`: the most the covariance workspace of one chunk of strips may take

    def __init__(self, afs: Sequence[Union[UpperConfidenceBound, ExpectedImprovement, LogExpectedImprovement]], batched_factors: bool = False):
        """``batched_factors``: the models that hold no ``_target_factor()`` for their parameter state get it from ONE batched assemble
        and ONE batched Cholesky for all of them (``ops.target_factors_batched``) instead of a posterior call each; every model keeps its
        slice (``_keep_target_factor``), so its own later calls reuse it.  False (default): the model's own posterior path, as before."""
        afs = list(afs)
        if not afs:
            raise ValueError("StudiesAcquisition needs at least one acquisition function")
        kinds = {type(a) for a in afs}
        if len(kinds) != 1 or not kinds <= {UpperConfidenceBound, ExpectedImprovement, LogExpectedImprovement}:
            raise TypeError("the acquisition functions must all be UpperConfidenceBound, all ExpectedImprovement or all "
                            "LogExpectedImprovement")
        self.acqf = afs[0].code
        models = [a.model for a in afs]
        m0 = models[0]
        # the source stacks: one object shared by all studies, or slices of one parent with an equal number of tasks (per-study stacks,
        # model.meta_fit_scamlgp_studies) -- then the pass reads the parent's arrays, study g's tasks from task_base[g]
        self.source, self._own = studies.source_stack(models, "the batched acquisition is")
        self.task_base = self._own.get("task_base")
        for m in models:
            if not m.supports_posterior_grad():
                raise NotImplementedError(f"the batched acquisition takes models with 1 <= n <= {studies.MAX_N} training (and pending) points, "
                                          f"D <= {studies.MAX_D} and at most {studies.MAX_FANTASIES} fantasies")
        self.models, self.kind, self.device = models, m0.kind, m0.device
        G, D, dev = len(models), m0._stack.D, m0.device
        n_max = max(m.n for m in models)
        self.G, self.D, self.n_max = G, D, n_max
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)   # noqa: E731
        self.L, self.Linv_diag, self.alpha = z(G, n_max, n_max), z(G, (n_max + 15) // 16, 16, 16), z(G, n_max)
        self.info = torch.zeros(G, dtype=torch.int32, device=dev)
        self._VA = []
        fant = [m.num_fantasies or 1 for m in models]
        self.fantasy = any(m.num_fantasies is not None for m in models)
        self.alpha_f = z(G, n_max, max(fant)) if self.fantasy else None
        if batched_factors:
            self._factors_batched([m for m in models if m.num_fantasies is None and m._target_factor() is None])
        for g, (af, m) in enumerate(zip(afs, models)):
            n = m.n
            f = m._target_factor()
            if f is None:   # (present after the study's scoring pass; otherwise the model's own path computes and caches it)
                if m.num_fantasies is not None:
                    m.fantasy_acqf(m.train_X[:1], self.acqf, float(af.param))
                else:
                    m.posterior_with_grad(m.train_X[:1])
                f = m._target_factor()
            self.L[g, :n, :n], self.Linv_diag[g, :(n + 15) // 16] = f["L"][0], f["Linv_diag"][0]
            if m.num_fantasies is not None:
                self.alpha_f[g, :n, :fant[g]] = f["alpha_f"]
            else:
                self.alpha[g, :n] = f["alpha"][0]
                if self.fantasy:
                    self.alpha_f[g, :n, 0] = f["alpha"][0]
            self.info[g] = f["info"][0]
            self._VA.append(m._train_VA().contiguous())
        for name, arr in studies.pack(models, self._VA).items():   # w, active, theta, Xt, n_points, m_all, s_all, VA_tab
            setattr(self, name, arr)
        self.acqf_param = torch.tensor([float(a.param) for a in afs], dtype=torch.float64).to(dev)
        self.n_fant = torch.tensor(fant, dtype=torch.int32).to(dev) if self.fantasy else None

    @staticmethod
    def _factors_batched(models: Sequence[ScaMLGP]):
        """The training-block factors of ``models`` in two launches (``ops.target_factors_batched``), each model keeping its slice in the
        layout its own ``ops.potrf_batched(Knn, resid, want_linv=True)`` returns.  A model the batch does not take -- no refit problem
        (``target_problem()`` is None), or source tasks listed in another order than its stack's -- is left without one: the caller's
        per-model path computes it.  Returns (the models taken, ``ops.target_factors_batched``'s dict for them), or ([], None)."""
        take = []
        for m in models:
            prob = m.target_problem()
            if prob is not None and [int(i) for i in m._idx] == list(range(m._stack.T)):
                take.append((m, prob))
        if not take:
            return [], None
        f = ops.target_factors_batched(ops.TargetFitBatch([p for _, p in take]), *studies.pack_parameters([m for m, _ in take]))
        for g, (m, _) in enumerate(take):
            m._keep_target_factor(studies.factor_slice(f, g, m.n))
        return [m for m, _ in take], f

    def score(self, X: torch.Tensor, group_per_strip: torch.Tensor, want_posterior: bool = False) -> Dict[str, torch.Tensor]:
        """The acquisition value of a TABLE of candidates: X (Mq, D) with Mq a multiple of 16, every 16 consecutive candidates one
        strip of ONE study, ``group_per_strip`` (Mq / 16,) int32 on the device naming it (negative: a padding strip, zeros).  Two
        launches for any number of studies -- the value-only grouped source pass (``ops.source_posteriors_grouped``; its OWN form when
        the models sit on slices of one parent stack) and the strip scoring kernel (``ops.target_score_batched``) --, no gradient.
        The strips are taken in chunks so that the source pass's covariance workspace, T x n_max x 16 doubles per strip, stays within
        ``SCORE_COV_CAP_BYTES`` (256 MiB: configs[4] with 32 studies x 1,024 candidates would need 0.67 GB in one piece and runs as three
        chunks; a chunk still holds ~800 strips, several per CU); two launches per chunk.
        Returns dict(value (Mq,), mu, var (Mq,) or None)."""
        Xq = torch.as_tensor(X, dtype=torch.float64).reshape(-1, self.D).to(self.device).contiguous()
        Mq = Xq.shape[0]
        if Mq % 16 or tuple(group_per_strip.shape) != (Mq // 16,) or group_per_strip.dtype != torch.int32:
            raise ValueError("score takes whole strips of 16 candidates and one int32 group per strip")
        if self.fantasy and want_posterior:
            raise ValueError("a set with fantasy models has no single posterior per candidate")
        group = group_per_strip.to(self.device)
        st, f = self.source, self.source.fit
        T = self.w.shape[1]
        per_chunk = max(1, self.SCORE_COV_CAP_BYTES // (T * self.n_max * 16 * 8))
        parts = []
        for s0 in range(0, Mq // 16, per_chunk):
            s1 = min(Mq // 16, s0 + per_chunk)
            xq, gr = Xq[16 * s0:16 * s1], group[s0:s1]
            g = ops.source_posteriors_grouped(xq, gr, self.Xt, self.n_points, self.VA_tab, st.X, st.theta, st.kind, f["Linv"], f["alpha"],
                                              st.y_mean, st.y_std, st.n_points, **self._own)
            if self.fantasy:
                v = ops.target_fantasy_score_batched(g["mu"], g["var"], g["cov"], gr, xq, self.w, self.active, self.Xt, self.theta, self.L,
                                                     self.Linv_diag, self.alpha_f, self.n_fant, self.n_points, self.m_all, self.s_all,
                                                     self.info, self.acqf_param, self.acqf, self.kind)
                parts.append(dict(value=v["value"], mu=None, var=None))
                continue
            parts.append(ops.target_score_batched(g["mu"], g["var"], g["cov"], gr, xq, self.w, self.active, self.Xt, self.theta, self.L,
                                                  self.Linv_diag, self.alpha, self.n_points, self.m_all, self.s_all, self.info, self.acqf_param,
                                                  self.acqf, self.kind, want_posterior=want_posterior))
        if len(parts) == 1:
            return parts[0]
        return {k: (torch.cat([p[k] for p in parts]) if parts[0][k] is not None else None) for k in parts[0]}

    def group_of(self, counts: Sequence[int]) -> torch.Tensor:
        """(sum counts,) int32 on the device: study s's index ``counts[s]`` times -- the ``group`` of a batch that lists the studies'
        points one study after the other."""
        return torch.repeat_interleave(torch.arange(self.G, dtype=torch.int32), torch.as_tensor(list(counts))).to(self.device)

    def strip_table(self, tables: Sequence[torch.Tensor]):
        """``score``'s X for the studies' candidate tables ``tables[s]`` (M_s, D) on the host: each padded to whole strips of 16 with a point
        of the box, whose values are dropped.  Returns (X (16 sum strips, D) on the host, strips per study -- ``group_of(strips)`` is
        ``score``'s ``group_per_strip`` --, the first row of every study's table in X)."""
        strips = [(t.shape[0] + 15) // 16 for t in tables]
        first = [16 * sum(strips[:s]) for s in range(len(tables))]
        X = torch.full((16 * sum(strips), self.D), 0.5, dtype=torch.float64)
        for t, o in zip(tables, first):
            X[o:o + t.shape[0]] = t
        return X, strips, first

    def evaluate(self, X: torch.Tensor, group: torch.Tensor, want_grad: bool = True, want_posterior: bool = False) -> Dict[str, torch.Tensor]:
        """dict(value (Mq,), grad (Mq, D) or None, mu, var (Mq,) or None) at X (Mq, D), point q scored by study ``group[q]`` (int32, on the
        device; a negative entry is a padding row and gives zeros)."""
        Xq = torch.as_tensor(X, dtype=torch.float64).reshape(-1, self.D).to(self.device).contiguous()
        st, f = self.source, self.source.fit
        g = ops.source_posteriors_grad_grouped(Xq, group, self.Xt, self.n_points, self.VA_tab, st.X, st.theta, st.kind, f["Linv"], f["alpha"],
                                               st.y_mean, st.y_std, st.n_points, **self._own)
        if self.fantasy:
            if want_posterior:
                raise ValueError("a set with fantasy models has no single posterior per query point")
            out = ops.target_fantasy_acqf_batched(g["mu"], g["var"], g["cov"], group, Xq, self.w, self.active, self.Xt, self.theta, self.L,
                                                  self.Linv_diag, self.alpha_f, self.n_fant, self.n_points, self.m_all, self.s_all, self.info,
                                                  self.acqf_param, self.acqf, self.kind, want_grad=want_grad)
            return dict(value=out["value"], grad=out["grad"], mu=None, var=None)
        return ops.target_acqf_batched(g["mu"], g["var"], g["cov"], group, Xq, self.w, self.active, self.Xt, self.theta, self.L, self.Linv_diag,
                                       self.alpha, self.n_points, self.m_all, self.s_all, self.info, self.acqf_param, self.acqf, self.kind,
                                       want_grad=want_grad, want_posterior=want_posterior)

    def value_and_grad(self, X: torch.Tensor, group: torch.Tensor):
        out = self.evaluate(X, group)
        return out["value"], out["grad"]

    def value(self, X: torch.Tensor, group: torch.Tensor) -> torch.Tensor:
        return self.evaluate(X, group, want_grad=False)["value"]

    def optimizer(self, X0: torch.Tensor, group: torch.Tensor, max_iter: int, bounds=(0.0, 1.0), **options) -> "ops.StudiesAcqfOpt":
        """The device-side optimisation of ``optimize`` before its first round: an ``ops.StudiesAcqfOpt`` on this object's arrays (packed
        once, at construction) whose rounds the caller enqueues itself (``enqueue`` / ``run``).  ``options``: history, max_ls, gtol, ftol,
        c1 of ``hyper.batched_lbfgs``."""
        D, dev = self.D, self.device
        X0 = torch.as_tensor(X0, dtype=torch.float64).reshape(-1, D).to(dev).contiguous()
        B = X0.shape[0]
        if tuple(group.shape) != (B,) or group.dtype != torch.int32:
            raise ValueError("group must be (B,) int32")
        lo = torch.as_tensor(bounds[0], dtype=torch.float64).expand(D).contiguous()
        hi = torch.as_tensor(bounds[1], dtype=torch.float64).expand(D).contiguous()
        if bool((lo > hi).any()):
            raise ValueError("bounds: lo > hi")
        st, f = self.source, self.source.fit
        arrays = [X0, group.to(dev), self.VA_tab, st.X, st.theta, f["Linv"], f["alpha"], st.y_mean, st.y_std, st.n_points, self.w, self.active,
                  self.Xt, self.theta, self.L, self.Linv_diag, self.alpha, self.n_points, self.m_all, self.s_all, self.info, self.acqf_param]
        T, N = self.w.shape[1], st.X.shape[1]
        if self.task_base is not None:   # per-study source tasks: T slots per study of the Tsrc tasks in the parent's arrays
            options = dict(options, task_base=self.task_base, Tsrc=st.X.shape[0])
        if self.fantasy:
            arrays[16] = None   # (alpha_t: not read; alpha_f and n_fant stand in its place)
            options = dict(options, fantasy=(self.alpha_f, self.n_fant))
        return ops.StudiesAcqfOpt(arrays, B, self.G, self.n_max, T, N, D, st.kind, self.kind, self.acqf, lo.to(dev), hi.to(dev), max_iter, **options)

    def optimize(self, X0: torch.Tensor, group: torch.Tensor, max_iter: int, bounds=(0.0, 1.0), evals_per_call: Optional[int] = None,
                 **options) -> Dict[str, torch.Tensor]:
        """Maximise every study's acquisition function from its starts ON THE DEVICE (``scaml_studies_acqf_opt_f64``):
        ``hyper.batched_lbfgs(bounds=...)`` per start, the optimiser step a kernel between the two evaluation launches.  X0 (B, D) start
        points, ``group`` (B,) int32 on the device (negative: a padding row), ``bounds`` scalars or (D,).  The loop enqueues
        ``evals_per_call`` (default ``ops.ACQF_OPT_EVALS_PER_CALL``) rounds per call while any start is running (at most
        1 + max_iter * max_ls evaluations) and reads ``stats`` once per call -- the only synchronisation.
        Returns dict(x (B, D), f (B,) the acquisition value at x -- the evaluation made there, no re-scoring --, stats (B, 4) int32 on
        the host [iterations, evaluations, status, pairs], n_eval rounds enqueued, n_calls, state)."""
        return self.optimizer(X0, group, max_iter, bounds, **options).run(evals_per_call)
