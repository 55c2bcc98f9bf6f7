"""A thin Bayesian-optimisation driver around the GPU path -- the caller of the hot path in the
reference is blackboxopt's ``SingleObjectiveBOTorchOptimizer`` (absent here); this module restates the
two things ``scamlgp/optimizer.py`` does with the model:

  report():  rebuild ScaMLGP on all target evaluations, handing the previous model's likelihood and kernel
             modules back in (warm start), and refit weights + hyper-parameters (optimizer.py:156-185)
  generate_evaluation_specification():  maximise the acquisition function (UCB with beta = 9 by
             default, utils.py:215-224) over the unit-cube search space.

The acquisition optimiser follows botorch's ``optimize_acqf`` recipe -- ``raw_samples`` random candidates, ``num_restarts``
initial conditions drawn from them (the best one plus a Boltzmann sample of the rest), box-constrained L-BFGS-B over all
starts jointly, best end point wins -- with exact gradients from the posterior's input-gradient kernels (round 3;
central differences where they do not apply).

Parallel evaluations (``max_pending_evaluations``, scamlgp/optimizer.py:41, 106, 149): points handed out by ``suggest()`` and not yet
reported are pending; the acquisition function is then built on ``model.fantasize(pending, num_fantasies)`` and averages over the
fantasised outcomes.  A ``report()`` without an objective value (None / NaN) keeps the point in ``X`` / ``Y`` and out of the fit
(scamlgp/optimizer.py:169-173)."""
from __future__ import annotations

from typing import Callable, Dict, Hashable, Optional, Sequence, Tuple, Union

import copy
import math
import time

import numpy as np
import scipy.optimize
import torch

from . import hyper
from . import studies as _studies
from .model import ScaMLGP, SourceGP, fantasize_studies
from .utils import ExpectedImprovement, LogExpectedImprovement, StudiesAcquisition, UpperConfidenceBound, capture_graph, fit_targets_batched, optimize_marginal_likelihood
from .utils import qExpectedImprovement, qUpperConfidenceBound


class OptimizerNotReady(RuntimeError):
    """``suggest()`` while ``max_pending_evaluations`` points are pending (blackboxopt's exception of the same name): report one
    first."""


class GraphedAcquisition:
    """An acquisition function for ONE batch shape, captured once into a HIP graph and replayed per evaluation.

    An evaluation of ``UpperConfidenceBound(model)(X)`` is ~15 launches of libscaml_hip.so (source posteriors with the
    fused covariance block, the weighted task sums, the target GP's assemble / Cholesky / solve / finish) plus a few torch
    element-wise kernels; at the batch sizes of the quasi-Newton phase (num_restarts x (2 dim + 1) points) the GPU work is
    shorter than the Python time to enqueue it.  The library never synchronises and keeps every status on the device, so
    the whole evaluation can be stream-captured: a replay is one host call.  The graph holds the ADDRESSES of the model's
    parameter tensors: build a new one after the model is refitted (ScaMLGPBOLoop.suggest does, per BO step)."""

    def __init__(self, af: Callable[[torch.Tensor], torch.Tensor], batch: int, dim: int, device: torch.device):
        self.af, self.batch = af, batch
        self.x = torch.zeros(batch, dim, dtype=torch.float64, device=device)
        # a tensor, or a tuple of tensors (value, gradient); a capture that fails raises (the callers have no eager twin to fall back on)
        self.graph, self.out = capture_graph(lambda: af(self.x), device, warmup=2)

    def __call__(self, X: torch.Tensor):
        if X.shape[0] != self.batch:
            return self.af(X)
        self.x.copy_(X, non_blocking=True)
        self.graph.replay()
        return tuple(o.clone() for o in self.out) if isinstance(self.out, tuple) else self.out.clone()


def acqf_initial_conditions(af: Callable[[torch.Tensor], torch.Tensor], dim: int, raw_samples: int, num_restarts: int,
                            generator: Optional[torch.Generator], eta: float = 2.0):
    """Stage 1 of ``optimize_acqf``: ``raw_samples`` uniform candidates scored in one pass, then ``num_restarts`` initial conditions (the
    best candidate plus a Boltzmann sample of the rest, botorch's ``initialize_q_batch``).  Everything drawn comes from ``generator``.
    Returns (cand (raw_samples, dim), vals (raw_samples,), best0, x0 (R, dim))."""
    cand = acqf_draw_candidates(dim, raw_samples, generator)
    vals = af(cand).detach().cpu()
    best0, picks = acqf_pick_initial_conditions(vals, num_restarts, generator, eta)
    return cand, vals, best0, cand[picks]


def acqf_draw_candidates(dim: int, raw_samples: int, generator: Optional[torch.Generator]) -> torch.Tensor:
    """The draw of ``acqf_initial_conditions``: ``raw_samples`` uniform candidates in [0, 1]^dim from ``generator`` (host, float64)."""
    return torch.rand(raw_samples, dim, dtype=torch.float64, generator=generator)


def acqf_pick_initial_conditions(vals: torch.Tensor, num_restarts: int, generator: Optional[torch.Generator], eta: float = 2.0):
    """The pick of ``acqf_initial_conditions`` from the candidates' values ``vals`` (raw_samples,) on the host: the best candidate plus
    a Boltzmann sample of the rest (botorch's ``initialize_q_batch``), drawn from ``generator``.  Returns (best0, picks): the index of
    the best candidate and the indices of the min(num_restarts, raw_samples) initial conditions, best first."""
    R = min(num_restarts, vals.shape[0])
    best0 = int(vals.argmax())
    picks = [best0]
    if R > 1:
        z = (vals - vals.mean()) / vals.std().clamp_min(1e-12)
        pr = torch.exp(eta * (z - z.max()))
        pr[best0] = 0.0
        if float(pr.sum()) > 0:
            k = min(R - 1, int((pr > 0).sum()))
            picks += torch.multinomial(pr, k, replacement=False, generator=generator).tolist()
    return best0, picks


JOINT_OPT_MODES = ("scipy", "device")


def _check_joint_opt_mode(mode: str) -> str:
    if mode not in JOINT_OPT_MODES:
        raise ValueError(f"joint_opt_mode must be 'scipy' or 'device', got {mode!r}")
    return mode


def acqf_local_optimization(af: Callable[[torch.Tensor], torch.Tensor], x0: torch.Tensor, max_iter: int = 50, fd_step: float = 1e-4,
                            graph_device: Optional[torch.device] = None, analytic_grad: bool = True, joint_opt_mode: str = "scipy") -> torch.Tensor:
    """Stage 2 of ``optimize_acqf``: ONE box-constrained scipy L-BFGS-B run over the R starts jointly (the summed acquisition value);
    returns the end points (R, dim) inside [0, 1]^dim.  x0 (R, q, dim): R q-batches of a joint acquisition function, one run over the
    R q dim variables on its ``value_and_grad``; the end points are (R, q, dim).  ``joint_opt_mode="device"`` (q-batches only): R
    independent box L-BFGS runs enqueued on the device instead (``_joint_device_optimization``)."""
    _check_joint_opt_mode(joint_opt_mode)
    if x0.dim() == 3:
        if joint_opt_mode == "device":
            return _joint_device_optimization(af, x0, max_iter)["x"]
        return _joint_local_optimization(af, x0, max_iter)
    R, dim = x0.shape
    eye = torch.eye(dim, dtype=torch.float64)
    analytic = analytic_grad and hasattr(af, "value_and_grad") and getattr(getattr(af, "model", None), "supports_posterior_grad", lambda: False)()
    if analytic:
        # exact gradients from the posterior's input-gradient kernels: an evaluation scores the R starts, nothing else
        vg = GraphedAcquisition(af.value_and_grad, R, dim, graph_device) if graph_device is not None else af.value_and_grad

        def fun(zv: np.ndarray):
            v, g = vg(torch.from_numpy(zv).reshape(R, dim))
            out = torch.cat([v.reshape(-1), g.reshape(-1)]).detach().cpu()   # one device -> host copy per evaluation
            f = float(out[:R].sum())
            if not math.isfinite(f):
                return float("inf"), np.zeros_like(zv)
            return -f, -torch.nan_to_num(out[R:]).numpy()
    else:
        af_step = GraphedAcquisition(af, R * (2 * dim + 1), dim, graph_device) if graph_device is not None else af

    def fun_fd(zv: np.ndarray):
        x = torch.from_numpy(zv).reshape(R, dim)
        xp = (x.unsqueeze(1) + fd_step * eye).clamp(0.0, 1.0)      # (R, dim, dim): start r shifted along dimension d
        xm = (x.unsqueeze(1) - fd_step * eye).clamp(0.0, 1.0)
        v = af_step(torch.cat([x, xp.reshape(-1, dim), xm.reshape(-1, dim)])).detach().cpu()
        dx = (xp - xm).diagonal(dim1=1, dim2=2)
        g = (v[R:R + R * dim].reshape(R, dim) - v[R + R * dim:].reshape(R, dim)) / dx
        f = float(v[:R].sum())
        if not math.isfinite(f):
            return float("inf"), np.zeros_like(zv)
        return -f, -torch.nan_to_num(g).reshape(-1).numpy()

    res = scipy.optimize.minimize(fun if analytic else fun_fd, x0.reshape(-1).numpy(), jac=True, method="L-BFGS-B", bounds=[(0.0, 1.0)] * (R * dim),
                                  options=dict(maxiter=max_iter))
    return torch.from_numpy(np.clip(res.x, 0.0, 1.0)).reshape(R, dim)


def _joint_local_optimization(af, x0: torch.Tensor, max_iter: int) -> torch.Tensor:
    """``acqf_local_optimization`` for R q-batches x0 (R, q, dim): exact gradients of the joint Monte-Carlo value (fixed base samples)."""
    R, q, dim = x0.shape

    def fun(zv: np.ndarray):
        v, g = af.value_and_grad(torch.from_numpy(zv).reshape(R, q, dim))
        out = torch.cat([v.reshape(-1), g.reshape(-1)]).detach().cpu()   # one device -> host copy per evaluation
        f = float(out[:R].sum())
        if not math.isfinite(f):
            return float("inf"), np.zeros_like(zv)
        return -f, -torch.nan_to_num(out[R:]).numpy()

    res = scipy.optimize.minimize(fun, x0.reshape(-1).numpy(), jac=True, method="L-BFGS-B", bounds=[(0.0, 1.0)] * (R * q * dim),
                                  options=dict(maxiter=max_iter))
    return torch.from_numpy(np.clip(res.x, 0.0, 1.0)).reshape(R, q, dim)


def _joint_device_optimization(af, x0: torch.Tensor, max_iter: int, evals_per_call: Optional[int] = None) -> dict:
    """Stage 2 for R q-batches x0 (R, q, dim) on the device: ``af.optimize`` (``utils._JointAcquisition.optimize``, scaml_qacqf_opt_f64)
    -- R independent box L-BFGS runs, not scipy's one run over the sum; the host twin is ``hyper.batched_lbfgs`` on
    ``af.value_and_grad``.  Returns its dict with x (R, q, dim) and f (R,) on the host: f is the value AT x, so no re-scoring follows."""
    if not callable(getattr(af, "optimize", None)):
        raise TypeError(f"joint_opt_mode='device' needs an acquisition function with an optimize method "
                        f"(utils.qExpectedImprovement, utils.qUpperConfidenceBound), got {type(af).__name__}")
    res = dict(af.optimize(x0, max_iter, evals_per_call=evals_per_call))
    res["x"] = res["x"].detach().cpu().clamp(0.0, 1.0).reshape(x0.shape)
    res["f"] = res["f"].detach().cpu()
    return res


def _optimize_acqf_joint(af, dim: int, q: int, raw_samples: int, num_restarts: int, max_iter: int, generator: Optional[torch.Generator], eta: float,
                         joint_opt_mode: str = "scipy", info: Optional[dict] = None):
    """``optimize_acqf`` for q > 1: ``raw_samples`` random q-batches, the Boltzmann pick over batches, one L-BFGS-B run over the
    R q dim variables, the best end batch.  Returns (X (q, dim), value).  ``joint_opt_mode="device"``: stage 2 runs on the device and
    its values at the end batches stand for stage 3's re-scoring call; stage 2 draws nothing from ``generator`` in either mode.
    ``info`` (a dict): receives n_eval, n_calls, evals_per_start and status of the device run."""
    _check_joint_opt_mode(joint_opt_mode)
    cand = torch.rand(raw_samples, q, dim, dtype=torch.float64, generator=generator)
    vals = af(cand).detach().cpu()
    best0, picks = acqf_pick_initial_conditions(vals, num_restarts, generator, eta)
    if joint_opt_mode == "device":
        res = _joint_device_optimization(af, cand[picks], max_iter)
        if info is not None:
            stats = torch.as_tensor(res["stats"])
            info.update(n_eval=int(res["n_eval"]), n_calls=int(res["n_calls"]), evals_per_start=stats[:, 1].tolist(), status=stats[:, 2].tolist())
        return acqf_final_choice(cand, vals, best0, res["x"], res["f"])
    xs = acqf_local_optimization(af, cand[picks], max_iter)
    return acqf_final_choice(cand, vals, best0, xs, af(xs))


def acqf_final_choice(cand: torch.Tensor, vals: torch.Tensor, best0: int, xs: torch.Tensor, fin: torch.Tensor):
    """Stage 3 of ``optimize_acqf``: the best end point (``fin`` = the acquisition values at ``xs``, re-scored), unless the best raw
    candidate is better.  Returns (x (dim,), value)."""
    fin = torch.nan_to_num(fin.detach().cpu(), nan=-float("inf"))
    j = int(fin.argmax())
    if float(fin[j]) >= float(vals[best0]):
        return xs[j], fin[j]
    return cand[best0], vals[best0]


def optimize_acqf(af: Callable[[torch.Tensor], torch.Tensor], dim: int, raw_samples: int = 1024, num_restarts: int = 10,
                  max_iter: int = 50, generator: Optional[torch.Generator] = None, fd_step: float = 1e-4,
                  eta: float = 2.0, graph_device: Optional[torch.device] = None, analytic_grad: bool = True, q: int = 1,
                  joint_opt_mode: str = "scipy") -> Tuple[torch.Tensor, torch.Tensor]:
    """Maximise ``af`` over [0, 1]^dim; returns (x_best (dim,), af(x_best)).  ``joint_opt_mode`` (read with q > 1 only): ``"scipy"``
    (default) or ``"device"`` -- stage 2 of the joint route enqueued on the device (``af.optimize``).  ``q`` > 1: ``af`` is a joint acquisition function
    (``utils.qExpectedImprovement`` / ``qUpperConfidenceBound``) over batches of q points, ``raw_samples`` counts q-batches, the Boltzmann
    pick is over batches, the L-BFGS-B run is over R q dim variables and the result is (X_best (q, dim), af(X_best)).  The joint route
    always runs on the exact gradients of ``af.value_and_grad``, evaluated eagerly: ``fd_step``, ``graph_device`` and ``analytic_grad``
    belong to the single-point route and are not read with q > 1.  botorch's ``optimize_acqf`` recipe:
    ``raw_samples`` random candidates -> ``num_restarts`` initial conditions (the best candidate plus a Boltzmann sample
    of the rest, ``initialize_q_batch``) -> ONE box-constrained L-BFGS-B run over all starts jointly (the summed
    acquisition value, which is separable over the starts: botorch's ``gen_candidates_scipy`` does the same) -> the
    best end point.  Gradients: analytic when the acquisition function offers ``value_and_grad`` and its model the posterior
    input-gradient kernels (``ScaMLGP.posterior_with_grad``: an evaluation then scores just the R starts); otherwise every
    objective evaluation is one batched posterior call over the starts and their central-difference stencils (one-sided at the
    box faces, 2 dim + 1 points per start).  With ``graph_device`` (the model's GPU) the evaluation is captured into a HIP graph
    once and replayed per L-BFGS-B step (``GraphedAcquisition``).  The three stages are functions of their own
    (``acqf_initial_conditions``, ``acqf_local_optimization``, ``acqf_final_choice``): ``ScaMLGPBOStudies`` runs the middle one for
    all its studies at once."""
    _check_joint_opt_mode(joint_opt_mode)
    if q != 1:
        if int(q) < 1:
            raise ValueError("q must be a positive integer")
        return _optimize_acqf_joint(af, dim, int(q), raw_samples, num_restarts, max_iter, generator, eta, joint_opt_mode)
    cand, vals, best0, x0 = acqf_initial_conditions(af, dim, raw_samples, num_restarts, generator, eta)
    xs = acqf_local_optimization(af, x0, max_iter, fd_step, graph_device, analytic_grad)
    return acqf_final_choice(cand, vals, best0, xs, af(xs))


class ScaMLGPBOLoop:
    def __init__(self, source_gps: Dict[Hashable, SourceGP], dim: int, acquisition: str = "ucb", beta: float = 9.0,
                 num_restarts_log_likelihood: int = 5, raw_samples: int = 1024, num_restarts: int = 10, af_max_iter: int = 50,
                 gp_likelihood: Optional[hyper.GaussianLikelihood] = None, gp_kernel: Optional[hyper.ScaleKernel] = None,
                 seed: Optional[int] = None, use_graph: bool = True, max_pending_evaluations: Optional[int] = None,
                 num_fantasies: int = 16, num_mc_samples: int = 128, joint_pending: str = "refuse", joint_score_mode: str = "grad_pass",
                 joint_opt_mode: str = "scipy"):
        """``num_mc_samples``: base samples of the joint acquisition function of ``suggest_batch``.
        ``joint_opt_mode``: where ``suggest_batch`` optimises its picked batches (stage 2) -- ``"scipy"`` (default): one scipy L-BFGS-B
        run over all of them on the host; ``"device"``: an independent box L-BFGS per batch enqueued on the device
        (scaml_qacqf_opt_f64), whose values at the end batches stand for the re-scoring call of stage 3.  ``last_suggest_info`` (None
        before the first ``suggest_batch``) then reports n_eval, n_calls, evals_per_start and status; with ``"scipy"`` it is ``{}``.
        ``joint_score_mode``: how ``suggest_batch`` scores its raw batches (stage 1) and its end batches (stage 3) -- ``"grad_pass"``
        (default): through the route of the gradient evaluations; ``"value_pass"``: through the value-only route
        (``ScaMLGP.joint_acqf_value``, 16 points per strip of the source pass).  Stage 2 runs on the exact gradients either way.
        ``joint_pending``: what ``suggest_batch`` does while evaluations are pending -- ``"refuse"`` (default): NotImplementedError;
        ``"joint"``: the pending points join every batch and are held fixed (botorch's X_pending, ``ScaMLGP.joint_acqf(X_pending=...)``).
        ``max_pending_evaluations``: None (default) -- strictly suggest -> report, no bookkeeping; an integer k -- ``suggest()``
        records its point in ``pending`` until it is reported, raises OptimizerNotReady while k points are pending, and builds the
        acquisition function on ``num_fantasies`` fantasies of the pending outcomes (ScaMLGP.fantasize, base samples from ``gen``)."""
        if max_pending_evaluations is not None and int(max_pending_evaluations) < 1:
            raise ValueError("max_pending_evaluations must be None or a positive integer")
        if joint_pending not in ("refuse", "joint"):
            raise ValueError(f"joint_pending must be 'refuse' or 'joint', got {joint_pending!r}")
        if joint_score_mode not in ("grad_pass", "value_pass"):
            raise ValueError(f"joint_score_mode must be 'grad_pass' or 'value_pass', got {joint_score_mode!r}")
        self.joint_pending, self.joint_score_mode = joint_pending, joint_score_mode
        self.joint_opt_mode = _check_joint_opt_mode(joint_opt_mode)
        self.last_suggest_info: Optional[dict] = None
        self.max_pending_evaluations = None if max_pending_evaluations is None else int(max_pending_evaluations)
        self.num_fantasies = int(num_fantasies)
        self.num_mc_samples = int(num_mc_samples)
        self.pending = torch.empty(0, dim, dtype=torch.float64)
        self.source_gps, self.dim = source_gps, dim
        self.acquisition, self.beta = acquisition, beta
        self.num_restarts_log_likelihood = num_restarts_log_likelihood
        self.raw_samples, self.num_restarts, self.af_max_iter = raw_samples, num_restarts, af_max_iter
        self.use_graph = use_graph
        self.gen = torch.Generator().manual_seed(0 if seed is None else seed)
        self.X = torch.empty(0, dim, dtype=torch.float64)
        self.Y = torch.empty(0, 1, dtype=torch.float64)
        # scamlgp/optimizer.py:142-148: the model before any evaluation (prior only)
        self.model = ScaMLGP(self.X, self.Y, source_gps, likelihood=gp_likelihood, covar_module=gp_kernel)

    def report(self, x: torch.Tensor, y: Union[float, None, Sequence[Optional[float]], torch.Tensor]) -> None:
        """Record evaluations and refit once: x (D,) with y a float, or x (q, D) with y (q,).  A y of None or NaN keeps the point in
        ``X`` / ``Y`` (as NaN) and out of the model's training set.  A reported point leaves ``pending`` (its first equal row, if any);
        reporting a point that was never suggested is allowed."""
        self.record(x, y)
        optimize_marginal_likelihood(self.model, self.num_restarts_log_likelihood)

    def record(self, x: torch.Tensor, y: Union[float, None, Sequence[Optional[float]], torch.Tensor]) -> None:
        """``report`` without the refit: the evaluations go into ``X`` / ``Y`` / ``pending`` and the model is rebuilt on them with the
        previous model's modules (the warm start); its weights and hyper-parameters are still to be fitted (``ScaMLGPBOStudies`` fits
        the models of all its studies together)."""
        xs = torch.as_tensor(x, dtype=torch.float64).reshape(-1, self.dim)
        if y is None or np.ndim(y) == 0:
            ys = [y]
        elif isinstance(y, torch.Tensor):
            ys = y.detach().cpu().reshape(-1).tolist()
        else:
            ys = list(np.asarray(y, dtype=object).reshape(-1))
        if len(ys) != xs.shape[0]:
            raise ValueError(f"report() got {xs.shape[0]} points and {len(ys)} objective values")
        yv = torch.tensor([[float("nan") if v is None else float(v)] for v in ys], dtype=torch.float64)
        for row in xs:
            hit = torch.nonzero((self.pending == row).all(-1)).flatten()
            if hit.numel():
                keep = torch.ones(self.pending.shape[0], dtype=torch.bool)
                keep[int(hit[0])] = False
                self.pending = self.pending[keep]
        self.X = torch.cat([self.X, xs], 0)
        self.Y = torch.cat([self.Y, yv], 0)
        ok = torch.isfinite(self.Y).squeeze(-1)
        # scamlgp/optimizer.py:176-185, same call sequence: the fitted modules go back in, the weights restart at 1/T
        # (evaluations without an objective value stay out of the fit, scamlgp/optimizer.py:169-173)
        self.model = ScaMLGP(
            self.X if bool(ok.all()) else self.X[ok],
            self.Y if bool(ok.all()) else self.Y[ok],
            self.source_gps,
            likelihood=self.model.likelihood,
            covar_module=self.model.covar_module,
        )

    def acquisition_function(self, fantasy_model: Optional[ScaMLGP] = None) -> Callable[[torch.Tensor], torch.Tensor]:
        """``fantasy_model``: the fantasy model of the pending evaluations where the caller has built it already
        (``model.fantasize_studies`` for many studies at once: the draws from ``gen`` are made there)."""
        model = self.model
        if fantasy_model is not None:
            model = fantasy_model
        elif self.max_pending_evaluations is not None and self.pending.shape[0] > 0:
            model = self.model.eval().fantasize(self.pending, self.num_fantasies, generator=self.gen)
        if self.acquisition in ("ei", "logei"):   # one best_f rule: the incumbent over the observed values
            Yf = self.Y[torch.isfinite(self.Y)]
            if Yf.numel() == 0:
                raise ValueError("EI needs at least one evaluation")
            return (ExpectedImprovement if self.acquisition == "ei" else LogExpectedImprovement)(model, float(Yf.min()))
        return UpperConfidenceBound(model, self.beta)

    def suggest(self) -> torch.Tensor:
        k = self.max_pending_evaluations
        if k is not None and self.pending.shape[0] >= k:
            raise OptimizerNotReady(f"{self.pending.shape[0]} evaluations are pending (max_pending_evaluations={k}): report one first")
        self.model.eval()
        af = self.acquisition_function()
        # (the graph path needs training data on the model: the prior-only model takes the torch branch of posterior())
        dev = af.model.device if (self.use_graph and af.model.n >= 1) else None
        x, _ = optimize_acqf(af, self.dim, self.raw_samples, self.num_restarts, self.af_max_iter, self.gen, graph_device=dev)
        if k is not None:
            self.pending = torch.cat([self.pending, x.reshape(1, -1)], 0)
        return x

    def joint_acquisition_function(self, q: int, X_pending: Optional[torch.Tensor] = None):
        """The joint Monte-Carlo acquisition function of ``suggest_batch``: qUCB for ``acquisition="ucb"``, qEI for ``"ei"`` (best_f: the
        incumbent over the observed values); its base samples come from ``gen``.  ``X_pending`` (p, D): evaluations that are running,
        appended to every batch and held fixed."""
        if self.acquisition == "logei":
            raise ValueError("a joint LogEI is not defined: suggest_batch takes acquisition='ucb' or 'ei'")
        if self.acquisition == "ei":
            Yf = self.Y[torch.isfinite(self.Y)]
            if Yf.numel() == 0:
                raise ValueError("EI needs at least one evaluation")
            return qExpectedImprovement(self.model, float(Yf.min()), self.num_mc_samples, self.gen, q=q, X_pending=X_pending,
                                        score_mode=self.joint_score_mode)
        return qUpperConfidenceBound(self.model, self.beta, self.num_mc_samples, self.gen, q=q, X_pending=X_pending, score_mode=self.joint_score_mode)

    def suggest_batch(self, q: int) -> torch.Tensor:
        """q points for q parallel workers, optimised AGAINST EACH OTHER: the maximiser (q, D) of the joint Monte-Carlo acquisition
        function over batches of q points (botorch's optimize_acqf(q = ...)), where q calls of ``suggest()`` condition every point on
        fantasies of the ones before it.  With ``max_pending_evaluations=k``: q <= k, and all q points become pending; with points
        already pending it raises (a joint acquisition function on a fantasy model is not defined here) unless the loop was built with
        ``joint_pending="joint"``: then the p pending points join every batch as fixed entries of the joint posterior (q + p <= k, and
        OptimizerNotReady once p >= k), and only the q new points are optimised.  ``report(x (q, D), y (q,))`` takes the results."""
        q, k, p = int(q), self.max_pending_evaluations, int(self.pending.shape[0])
        if q < 1:
            raise ValueError("suggest_batch takes q >= 1")
        if self.acquisition not in ("ucb", "ei"):
            raise ValueError("a joint LogEI is not defined: suggest_batch takes acquisition='ucb' or 'ei'")
        if p > 0 and self.joint_pending != "joint":
            raise NotImplementedError("suggest_batch with evaluations pending: the joint acquisition function is not defined on a fantasy model "
                                      "(joint_pending='joint' holds the pending points fixed in every batch instead)")
        if k is not None and p >= k:
            raise OptimizerNotReady(f"{p} evaluations are pending (max_pending_evaluations={k}): report one first")
        if k is not None and q + p > k:
            raise ValueError(f"suggest_batch({q}) exceeds max_pending_evaluations={k}" + (f" with {p} pending" if p else ""))
        self.model.eval()
        af = self.joint_acquisition_function(q, self.pending if p > 0 else None)
        # (the joint route for every q, q = 1 included: optimize_acqf(q=1) is the single-point path of the analytic functions)
        info: dict = {}
        X, _ = _optimize_acqf_joint(af, self.dim, q, self.raw_samples, self.num_restarts, self.af_max_iter, self.gen, 2.0, self.joint_opt_mode, info)
        self.last_suggest_info = info
        X = X.reshape(q, self.dim)
        if k is not None:
            self.pending = torch.cat([self.pending, X], 0)
        return X

    def run(self, objective: Callable[[torch.Tensor], float], n_steps: int):
        for _ in range(n_steps):
            x = self.suggest()
            self.report(x, objective(x))
        return self.X, self.Y


_NEEDS_LOCKSTEP = ("suggest_mode", ("lockstep", "device"), "suggest_mode='lockstep' or 'device': the sequential mode runs every study on its own")
# (mode, its values, what its value "batched" needs: (another mode, that mode's values that serve, the refusal's words))
_STUDIES_MODES = (
    ("suggest_mode", ("sequential", "lockstep", "device"), None),
    ("score_mode", ("per_study", "batched"), _NEEDS_LOCKSTEP),
    ("pending_mode", ("per_study", "batched"), _NEEDS_LOCKSTEP),
    ("fantasy_setup", ("per_study", "batched"),
     ("pending_mode", ("batched",), "pending_mode='batched': otherwise a study with pending evaluations runs on its own")),
)


def _check_modes(modes: Dict[str, str]) -> None:
    """``ScaMLGPBOStudies``'s mode strings against ``_STUDIES_MODES``, in its order."""
    for name, values, needs in _STUDIES_MODES:
        quoted = [repr(v) for v in values]
        if modes[name] not in values:
            raise ValueError(f"{name} must be {', '.join(quoted[:-1])} or {quoted[-1]}, got {modes[name]!r}")
        if needs is not None and modes[name] == "batched" and modes[needs[0]] not in needs[1]:
            raise ValueError(f"{name}='batched' needs {needs[2]}")


class _PartTimer:
    """``profile_parts`` (developer timing): called at a boundary between the parts of a suggest it synchronises, and the time since the
    last call goes to ``seconds[name]``.  Switched off it does nothing."""

    def __init__(self, on: bool):
        self.on, self.seconds, self.last = on, {}, None
        self()

    def __call__(self, name: Optional[str] = None) -> None:
        if not self.on:
            return
        torch.cuda.synchronize()
        now = time.perf_counter()
        if name is not None:
            self.seconds[name] = self.seconds.get(name, 0.0) + now - self.last
        self.last = now


class ScaMLGPBOStudies:
    """S independent Bayesian-optimisation studies against ONE fitted source stack, stepped in lock-step on one GPU -- the repeated
    runs behind a regret curve (scamlgp/benchmarking/local_runner.py:174-181 fans them out over a process pool, one study per core).

    ``studies[s]`` is a ``ScaMLGPBOLoop`` (its ``model``, ``X``, ``Y``, ``pending``, ``model.last_fit_info``: a study's record goes
    through ``results`` exactly as a single loop's does), built with ``seed=seeds[s]`` and the loop kwargs; given ``gp_likelihood`` /
    ``gp_kernel`` modules are copied per study (they hold the fitted state).  What is batched is the refit: ``report`` rebuilds every
    study's model and then runs the L-BFGS optimisations of ALL studies -- warm start plus restarts each -- in one launch
    (``utils.fit_targets_batched`` -> ``scaml_target_fit_batched_f64``), where one study's refit keeps 1 + restarts of the chip's 256 CUs
    busy for its whole latency.  Per study the starts, the optimiser and the best-of-restarts choice are the single loop's; study s
    draws its restart samples from ``fit_gens[s]`` (a ``torch.Generator`` seeded with ``seeds[s]``), its acquisition samples from
    ``studies[s].gen``.  A study whose shape the kernel does not take (n beyond its LDS, D > 16) is refitted as ``ScaMLGPBOLoop`` does
    it, on its own.  Studies may get out of step: a study with a pending or a failed (None / NaN) evaluation trains on fewer points than
    its neighbours.

    ``suggest_mode="sequential"`` (default): ``suggest`` runs the studies one after the other with the existing launches.
    ``suggest_mode="lockstep"``: per study the initial conditions of ``optimize_acqf`` as before (its own ``gen``, its own scoring pass:
    the same draws), then ONE box-constrained ``hyper.batched_lbfgs`` over the starts of all studies -- every objective evaluation is one
    grouped source pass and one batched acquisition launch for all of them (``utils.StudiesAcquisition``), captured into one HIP graph per
    ``suggest`` with ``use_graph`` --, one batched re-scoring of the end points, and per study the final choice of ``optimize_acqf``.  Each
    start is a problem of its own there (own history, step and stopping flag; ``optimize_acqf`` sums over a study's starts), so a
    start's path does not depend on the other studies.  A study the batched path does not take -- no training data yet, n > 96, D > 15,
    pending evaluations (a fantasy model) -- takes its own ``ScaMLGPBOLoop.suggest()`` in the same call.
    ``suggest_mode="device"``: ``"lockstep"`` with the optimiser itself on the device (``StudiesAcquisition.optimize`` ->
    ``scaml_studies_acqf_opt_f64``): the same initial conditions, the same per-start box-constrained L-BFGS, but its step is a kernel
    between the two evaluation launches, so no start waits for another, a start that has stopped is no longer evaluated and the host
    reads one status block per chunk of rounds.  The end points come back with their acquisition values (no re-scoring pass); the final
    choice and the fall-back of the studies the batch does not take are ``"lockstep"``'s.  ``last_suggest_info``: ``batched``,
    ``n_eval`` (rounds enqueued), ``n_calls``, ``evals_per_start`` and ``status`` per start.  ``num_studies=1`` is a legitimate use.

    ``score_mode`` (with ``"lockstep"`` or ``"device"``; ``"sequential"`` refuses ``"batched"``): ``"per_study"`` (default) -- stage 1 as
    described, every study scores its own candidates; ``"batched"`` -- every batched study draws its candidates from its own ``gen``
    (``acqf_draw_candidates``), ONE ``StudiesAcquisition.score`` call and one device -> host copy deliver all values (each table padded
    to whole strips of 16), then every study makes its picks from its own ``gen`` (``acqf_pick_initial_conditions``); the studies'
    factors come from one batched assemble and one batched Cholesky.  The draws, hence the generators' states, are the per-study
    mode's.  ``last_suggest_info["score_mode"]`` names the mode.  Not forwarded to the loops.

    ``pending_mode`` (with ``"lockstep"`` or ``"device"``; ``"sequential"`` refuses ``"batched"``): ``"per_study"`` (default) -- a study
    with pending evaluations takes its own ``ScaMLGPBOLoop.suggest()``, as described; ``"batched"`` -- it stays in the batch, with both
    ``score_mode``s: its acquisition function is built on its fantasy model as the single loop builds it (``fantasize`` from its own
    ``gen``, the set-up of the conditioned model per study), and ``utils.StudiesAcquisition`` evaluates it with the others, UCB / EI
    averaged over its fantasies (``scaml_target_fantasy_acqf_batched_f64`` and its siblings).  Whether a study stays is decided before
    its fantasies are drawn: n >= 1, n + p <= 96 and <= the stack's N, D <= 15, ``num_fantasies`` <= 64; any other study falls back as
    in the default mode.  Per study the order of the draws is the single loop's (fantasies, raw candidates, picks), so the generators
    end where a ``"per_study"`` twin's do; ``last_suggest_info`` has the keys it always had.  Not forwarded to the loops.

    One source stack PER study (the reference's protocol: ``benchmark_cls(seed=study_seed)`` / ``meta_data_seed=study_seed``,
    scamlgp/benchmarking/local_runner.py:51-65, 178-181 -- every study draws its own meta-tasks): ``source_gps`` may be a sequence of S
    dicts, as ``model.meta_fit_scamlgp_studies`` returns them (slices of one stack fitted in one call).  All three modes work: the
    batched refit takes its source terms per study anyway, and the grouped source pass reads study s's tasks only
    (``utils.StudiesAcquisition``).  A single dict keeps meaning "shared".

    ``fantasy_setup`` (with ``pending_mode="batched"``; anything else refuses ``"batched"``): ``"per_study"`` (default) -- the fantasy
    model of a study with pending evaluations is built by its own ``fantasize`` call, as described; ``"batched"`` -- the studies that
    stay in the batch and hold pending points get their fantasy models from ONE ``model.fantasize_studies`` call before any raw
    candidate is drawn (one grouped source pass, ``scaml_studies_condition_block_f64``, one batched Cholesky,
    ``scaml_studies_fantasy_condition_f64``, one status read-back; per study only the V launch of its n + p points is left).  Per study
    the order of the draws stays fantasies, raw candidates, picks, so every ``gen`` ends where a ``"per_study"`` twin's does; the
    fantasies are the same samples up to rounding (one factor of the joint block in place of the Schur complement's).
    ``last_suggest_info`` gains the key ``"fantasy_setup"`` in this mode (the default mode's record keeps exactly its keys); with
    ``profile_parts`` the part ``"setup"`` is timed apart from ``"stage1"``.
    Not forwarded to the loops."""

    def __init__(self, source_gps: Union[Dict[Hashable, SourceGP], Sequence[Dict[Hashable, SourceGP]]], dim: int, num_studies: int,
                 seeds: Optional[Sequence[int]] = None, suggest_mode: str = "sequential", score_mode: str = "per_study",
                 pending_mode: str = "per_study", fantasy_setup: str = "per_study", **loop_kwargs):
        _check_modes(dict(suggest_mode=suggest_mode, score_mode=score_mode, pending_mode=pending_mode, fantasy_setup=fantasy_setup))
        self.suggest_mode, self.score_mode, self.pending_mode, self.fantasy_setup = suggest_mode, score_mode, pending_mode, fantasy_setup
        self.profile_parts = False   # developer timing (tools/dev_studies_time.py): synchronise between the parts of a suggest and time them
        self.last_suggest_info: dict = {}
        S = int(num_studies)
        if S < 1:
            raise ValueError("num_studies must be a positive integer")
        seeds = list(range(S)) if seeds is None else [int(v) for v in seeds]
        if len(seeds) != S:
            raise ValueError(f"got {len(seeds)} seeds for {S} studies")
        if "seed" in loop_kwargs:
            raise TypeError("pass seeds=[...] (one per study), not seed=")
        self.dim, self.num_studies, self.seeds = dim, S, seeds
        # one dict: the stack shared by all studies; a sequence of S dicts: study s's own (model.meta_fit_scamlgp_studies)
        per_study = None if isinstance(source_gps, dict) else list(source_gps)
        if per_study is not None and len(per_study) != S:
            raise ValueError(f"got {len(per_study)} source stacks for {S} studies")
        self.studies = []
        for s in range(S):
            kw = dict(loop_kwargs)
            for name in ("gp_likelihood", "gp_kernel"):
                if kw.get(name) is not None:
                    kw[name] = copy.deepcopy(kw[name])
            self.studies.append(ScaMLGPBOLoop(source_gps if per_study is None else per_study[s], dim, seed=seeds[s], **kw))
        if self.studies[0].model._shard is not None:
            raise NotImplementedError("lock-step studies are not implemented for a task-sharded source stack (shard=True)")
        self.fit_gens = [torch.Generator().manual_seed(v) for v in seeds]

    def __len__(self) -> int:
        return self.num_studies

    def __getitem__(self, s: int) -> ScaMLGPBOLoop:
        return self.studies[s]

    def suggest(self) -> torch.Tensor:
        """(S, D): every study's next point (``ScaMLGPBOLoop.suggest``; OptimizerNotReady if a study has its full count pending)."""
        if self.suggest_mode == "sequential":
            return torch.stack([st.suggest() for st in self.studies])
        # as the sequential loop leaves it: the studies in front of one that is not ready have suggested (and recorded) their points
        blocked = [s for s, st in enumerate(self.studies)
                   if st.max_pending_evaluations is not None and st.pending.shape[0] >= st.max_pending_evaluations]
        if blocked:
            self._suggest_lockstep(self.studies[:blocked[0]])
            self.studies[blocked[0]].suggest()   # raises OptimizerNotReady
        return torch.stack(self._suggest_lockstep(self.studies))

    @staticmethod
    def _batched_study(st: ScaMLGPBOLoop) -> bool:
        """Does the batched acquisition take this study's step?  (An ordinary model with training data within the GRAD pass's limits;
        pending evaluations make it a fantasy model.)"""
        return (not (st.max_pending_evaluations is not None and st.pending.shape[0] > 0)) and st.model.supports_posterior_grad()

    def _takes_study(self, st: ScaMLGPBOLoop) -> bool:
        """``_batched_study``, and with ``pending_mode="batched"`` also a study whose pending evaluations make it a fantasy model the
        batched acquisition takes.  Asked BEFORE ``st.acquisition_function()`` draws the fantasies from ``st.gen``: a study that fell
        back afterwards would draw them twice."""
        if self._batched_study(st):
            return True
        p = st.pending.shape[0]
        if self.pending_mode != "batched" or st.max_pending_evaluations is None or p == 0:
            return False
        return _studies.takes(st.model, p, int(st.num_fantasies))

    def _fantasy_models(self, studies: Sequence[ScaMLGPBOLoop]) -> dict:
        """``fantasy_setup="batched"``: the fantasy models of the studies that stay in the batch and hold pending points, from ONE
        ``fantasize_studies`` call -- each study's fantasies drawn from its own ``gen`` before its raw candidates, as its own
        ``acquisition_function()`` would.  {position in ``studies``: model}; empty in the default mode."""
        if self.fantasy_setup != "batched":
            return {}
        take = [(i, st) for i, st in enumerate(studies) if self._takes_study(st) and not self._batched_study(st)]
        if not take:
            return {}
        models = fantasize_studies([st.model.eval() for _, st in take], [st.pending for _, st in take], [int(st.num_fantasies) for _, st in take],
                                   [st.gen for _, st in take])
        return {i: m for (i, _), m in zip(take, models)}

    def _suggest_lockstep(self, studies: Sequence[ScaMLGPBOLoop]):
        out = [None] * len(studies)
        mark = _PartTimer(self.profile_parts)
        fmodel = self._fantasy_models(studies)   # fantasy_setup="batched": {position: fantasy model}, all of them from one call
        if fmodel:
            mark("setup")
        batch, sa = self._stage1(studies, fmodel, out, mark)   # batch: (position, study, af, cand, vals, best0, x0)
        mark("stage1")
        self.last_suggest_info = dict(batched=[b[0] for b in batch], n_eval=0, n_iter=0, score_mode=self.score_mode)
        if self.fantasy_setup != "per_study":   # (the default mode's record keeps exactly the keys it had)
            self.last_suggest_info["fantasy_setup"] = self.fantasy_setup
        if self.profile_parts:
            # seconds: setup (fantasy_setup="batched"), stage1, packing (with the factors), rounds, stage3
            self.last_suggest_info["parts"] = mark.seconds
        if not batch:
            return out
        if sa is None:   # (score_mode="batched" has packed the studies for its scoring pass)
            sa = StudiesAcquisition([b[2] for b in batch])
            mark("packing")
        counts = [b[6].shape[0] for b in batch]
        X0, group = torch.cat([b[6] for b in batch], 0), sa.group_of(counts)
        xs, fs = (self._rounds_device if self.suggest_mode == "device" else self._rounds_host)(sa, X0, group, counts, studies[0])
        mark("rounds")
        out = self._final_choices(batch, out, xs, fs)
        mark("stage3")
        return out

    def _stage1(self, studies: Sequence[ScaMLGPBOLoop], fmodel: dict, out: list, mark):
        """Stage 1 of every study's ``optimize_acqf``.  A study the batch does not take makes its own ``suggest()`` into ``out``; every
        other one builds its acquisition function (on ``fmodel[position]`` where the batch has built its fantasy model) and draws its raw
        candidates from its own ``gen``.  ``score_mode="per_study"``: it scores and picks at once (``acqf_initial_conditions``).
        ``"batched"``: the studies' factors in two launches, then ONE scoring pass over all candidate tables and ONE device -> host copy,
        then every study's picks.  Returns (batch, the ``StudiesAcquisition`` the scoring pass has built or None)."""
        batch, drawn = [], []   # drawn: (position, study, af, cand) whose scoring is still to come
        for i, st in enumerate(studies):
            if not self._takes_study(st):
                out[i] = st.suggest()
                continue
            st.model.eval()
            af = st.acquisition_function(fmodel[i]) if i in fmodel else st.acquisition_function()   # (without a model from the batch: its own)
            if self.score_mode == "batched":
                drawn.append((i, st, af, acqf_draw_candidates(self.dim, st.raw_samples, st.gen)))
            else:
                batch.append((i, st, af) + acqf_initial_conditions(af, self.dim, st.raw_samples, st.num_restarts, st.gen))
        if not drawn:
            return batch, None
        mark("stage1")
        sa = StudiesAcquisition([d[2] for d in drawn], batched_factors=True)
        mark("packing")
        table, strips, first = sa.strip_table([d[3] for d in drawn])
        vals_all = sa.score(table, sa.group_of(strips))["value"].cpu()
        for (i, st, af, cand), o in zip(drawn, first):
            vals = vals_all[o:o + cand.shape[0]].clone()
            best0, pk = acqf_pick_initial_conditions(vals, st.num_restarts, st.gen)
            batch.append((i, st, af, cand, vals, best0, cand[pk]))
        return batch, sa

    def _rounds_device(self, sa, X0: torch.Tensor, group: torch.Tensor, counts, loop: ScaMLGPBOLoop):
        """The optimiser on the device: end points and THEIR values in one status read per chunk of rounds.  Returns (x, f) per study."""
        res = sa.optimize(X0, group, loop.af_max_iter, bounds=(0.0, 1.0))
        self.last_suggest_info.update(n_eval=res["n_eval"], n_calls=res["n_calls"], n_iter=int(res["stats"][:, 0].max()),
                                      evals_per_start=res["stats"][:, 1].tolist(), status=res["stats"][:, 2].tolist())
        return res["x"].cpu().split(counts), res["f"].cpu().split(counts)

    def _rounds_host(self, sa, X0: torch.Tensor, group: torch.Tensor, counts, loop: ScaMLGPBOLoop):
        """ONE ``hyper.batched_lbfgs`` on the host over the starts of all studies, every evaluation two library launches, then the end
        points of all studies re-scored in one evaluation.  Returns (x, f) per study."""
        B = X0.shape[0]
        vg = lambda X: sa.value_and_grad(X, group)   # noqa: E731
        if loop.use_graph:   # one capture per suggest() serves all studies: a single stream, two library launches
            vg = GraphedAcquisition(vg, B, self.dim, sa.device)
        t_eval = [0.0]

        def fun(x: torch.Tensor):
            t0 = time.perf_counter()
            v, g = vg(x)
            o = torch.cat([v.reshape(B, 1), g.reshape(B, self.dim)], 1).cpu()   # one device -> host copy per evaluation
            t_eval[0] += time.perf_counter() - t0   # (the copy has waited for the evaluation)
            return -o[:, 0], -o[:, 1:]

        res = hyper.batched_lbfgs(fun, X0, max_iter=loop.af_max_iter, bounds=(0.0, 1.0))
        fin = sa.value(res.x, group).cpu()
        self.last_suggest_info.update(n_eval=res.n_eval, n_iter=res.n_iter, eval_seconds=t_eval[0])
        return res.x.split(counts), fin.split(counts)

    @staticmethod
    def _final_choices(batch, out, xs_per_study, fin_per_study):
        for (i, st, af, cand, vals, best0, x0), xs, fs in zip(batch, xs_per_study, fin_per_study):
            x, _ = acqf_final_choice(cand, vals, best0, xs, fs)
            if st.max_pending_evaluations is not None:
                st.pending = torch.cat([st.pending, x.reshape(1, -1)], 0)
            out[i] = x
        return out

    def report(self, X: torch.Tensor, y) -> None:
        """One evaluation per study: X (S, D), y (S,) -- a tensor, or a sequence whose entries may be None / NaN (no objective value:
        the point stays out of that study's fit) -- then ONE refit of all studies.  ``X[s]`` need not be the point ``suggest`` returned
        for study s; the pending bookkeeping is ``ScaMLGPBOLoop.report``'s.  To leave a study's evaluation pending, report the others
        through ``report_some``."""
        xs = torch.as_tensor(X, dtype=torch.float64).reshape(-1, self.dim)
        ys = y.detach().cpu().reshape(-1).tolist() if isinstance(y, torch.Tensor) else list(y)
        if xs.shape[0] != self.num_studies or len(ys) != self.num_studies:
            raise ValueError(f"report() takes one point and one objective value per study ({self.num_studies}), got {xs.shape[0]} and {len(ys)}")
        self.report_some({s: (xs[s], ys[s]) for s in range(self.num_studies)})

    def report_some(self, evaluations: Dict[int, Tuple[torch.Tensor, object]]) -> None:
        """Evaluations of SOME studies, {study index: (x (D,) or (q, D), y float / None or (q,))}, then one refit of those studies;
        the others keep their models (and their pending points)."""
        idx = sorted(evaluations)
        for s in idx:
            self.studies[s].record(*evaluations[s])
        nrll = self.studies[0].num_restarts_log_likelihood
        fit_targets_batched([self.studies[s].model for s in idx], nrll, rng=[self.fit_gens[s] for s in idx])

    def run(self, objectives: Union[Callable[[torch.Tensor], Sequence[float]], Sequence[Callable[[torch.Tensor], float]]], n_steps: int):
        """``n_steps`` rounds of suggest -> evaluate -> report.  ``objectives``: one callable mapping the (S, D) points to S values, or
        S callables, one per study.  Returns ([X_s], [Y_s])."""
        for _ in range(n_steps):
            X = self.suggest()
            ys = objectives(X) if callable(objectives) else [f(x) for f, x in zip(objectives, X)]
            self.report(X, ys)
        return [st.X for st in self.studies], [st.Y for st in self.studies]
