"""Host-side mirror of ``scamlgp/model.py`` on top of the HIP hot path.

Same public names and argument meaning as the reference (``meta_fit_scamlgp``, ``ScaMLGP``,
``_compute_target_prior``, ``significant_weights_mask``), but the stack of source GPs is ONE batched
object: every source-side operation (marginal likelihood + gradient for all tasks x restarts,
Cholesky factors, posteriors at shared query points, the weighted prior sum) is a launch of
libscaml_hip.so over the whole ``(T, N, D)`` stack instead of a Python loop over gpytorch models
(``scamlgp/model.py:128, 176-188, 281``).  The target GP's own algebra (n <= ~80 points:
``scamlgp/model.py:359-384`` and gpytorch's exact prediction) stays in torch on the same device.

Deliberate deviations: tasks are fitted simultaneously from the same initial
values, so the reference's sequential warm-start chain (task t starts from task t-1's optimum,
``scamlgp/model.py:177-178``) is not reproduced; restarts are ranked by the training objective, not
by the eval-mode value the reference happens to compute (``scamlgp/utils.py:176-177``).
"""
from __future__ import annotations

import copy
import math
import warnings
from dataclasses import dataclass
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import torch

from . import dist as sdist
from . import hyper, ops, studies
from ._lib import KIND_MATERN52, KIND_RBF

_LOG_2PI = math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------------------
# data containers
# ---------------------------------------------------------------------------------------
class _CallableTensor(torch.Tensor):
    """The reference reads datasets both as ``data.X.shape`` (scamlgp/utils.py:117) and as
    ``data.X()`` (scamlgp/model.py:180): a tensor that returns itself when called serves both."""

    def __call__(self):
        return self.as_subclass(torch.Tensor)


class SupervisedDataset:
    """Minimal stand-in for botorch.utils.datasets.SupervisedDataset: X (n, d), Y (n, 1)."""

    def __init__(self, X: torch.Tensor, Y: torch.Tensor):
        self.X = torch.as_tensor(X).as_subclass(_CallableTensor)
        self.Y = torch.as_tensor(Y).as_subclass(_CallableTensor)


def validate_meta_data(meta_data: Dict[Hashable, SupervisedDataset]) -> None:
    """The checks of scamlgp/utils.py:112-136 with the same ValueError messages (callers match on them): at least
    one task; all tasks share batch shape and input dimension with the first one; one output column."""
    if not meta_data:
        raise ValueError("Empty meta data. Needs at least one source task.")
    tasks = iter(meta_data.items())
    first_id, first = next(tasks)
    batch_x, batch_y, dim = first.X.shape[:-2], first.Y.shape[:-2], first.X.shape[-1]
    if batch_x != batch_y:
        raise ValueError(f"The X and Y batch sizes of task {first_id} are not equal.")
    for tid, data in [(first_id, first), *tasks]:
        same = data.X.shape[:-2] == batch_x and data.Y.shape[:-2] == batch_y and data.X.shape[-1] == dim
        if not same:
            raise ValueError(f"Dimensions of tasks {first_id} and {tid} do not match.")
        n_out = data.Y.shape[-1]
        if n_out != 1:
            raise ValueError(f"The output dimension of task {tid} is {n_out} but must be one")


@dataclass(frozen=True)
class KernelSpec:
    """Shorthand for ``covar_module``: only the kernel family (RBF | Matern-5/2, ARD), reference priors."""
    kind: int = KIND_RBF


def _resolve_modules(likelihood, covar_module, D: int, default_kernel):
    """What the reference accepts as ``likelihood`` / ``covar_module`` (gpytorch modules, scamlgp/model.py:140-141,
    223-224) -> (GaussianLikelihood, ScaleKernel) holders of this package.  Also accepted: a HyperSpec as
    ``likelihood`` (all three parameter groups at once) and a KernelSpec as ``covar_module`` (family only)."""
    kind = covar_module.kind if isinstance(covar_module, (KernelSpec, hyper.ScaleKernel)) else KIND_RBF
    if isinstance(likelihood, hyper.HyperSpec):
        return hyper.modules_from_spec(likelihood, kind, D)
    if likelihood is not None and not isinstance(likelihood, hyper.GaussianLikelihood):
        raise TypeError(f"likelihood must be a GaussianLikelihood (or a HyperSpec), got {type(likelihood).__name__}")
    if covar_module is not None and not isinstance(covar_module, (KernelSpec, hyper.ScaleKernel)):
        raise TypeError(f"covar_module must be a ScaleKernel (or a KernelSpec), got {type(covar_module).__name__}")
    lik = likelihood if likelihood is not None else hyper.get_default_likelihood()
    if isinstance(covar_module, hyper.ScaleKernel):
        cov = covar_module
        if cov.base_kernel.ard_num_dims != D:
            raise ValueError(f"covar_module has ard_num_dims={cov.base_kernel.ard_num_dims} but the inputs have {D} dimensions")
    else:
        cov = default_kernel(hyper.MaternKernel if kind == KIND_MATERN52 else hyper.RBFKernel, D)
    return lik, cov


def standardize_fit(Y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """botorch Standardize(m=1): mean / unbiased std over dim -2, std < 1e-8 (or n = 1) -> 1."""
    m = Y.mean(dim=-2)
    if Y.shape[-2] < 2:
        s = torch.ones_like(m)
    else:
        s = Y.std(dim=-2)
        s = torch.where(s >= 1e-8, s, torch.ones_like(s))
    return m, s


class _OutcomeTransform:
    def __init__(self, mean: torch.Tensor, std: torch.Tensor):
        self.means, self.stdvs = mean.reshape(1, 1), std.reshape(1, 1)

    def untransform(self, Y: torch.Tensor, Yvar: Optional[torch.Tensor] = None):
        return self.means + self.stdvs * Y, None if Yvar is None else self.stdvs ** 2 * Yvar


class _MVN:
    def __init__(self, mean: torch.Tensor, cov: torch.Tensor):
        self.mean, self.covariance_matrix, self.lazy_covariance_matrix = mean, cov, cov

    @property
    def variance(self):
        return torch.diagonal(self.covariance_matrix, dim1=-2, dim2=-1)


class _Posterior:
    def __init__(self, mean: torch.Tensor, cov: torch.Tensor):
        self.mvn = _MVN(mean, cov)
        self.mean, self.variance = mean.unsqueeze(-1), self.mvn.variance.unsqueeze(-1)


# ---------------------------------------------------------------------------------------
# the stack of source GPs
# ---------------------------------------------------------------------------------------
class SourceGPStack:
    """All source GPs as one padded ``(T, N, D)`` problem on the device.

    Holds the data (per-task standardised targets, botorch ``Standardize`` semantics,
    scamlgp/model.py:185), the raw hyper-parameters ``(T, D+2)`` and, after ``refresh()``, the
    Cholesky factors / alpha / block inverses produced by the fused fit kernel."""

    def __init__(self, task_ids: Sequence[Hashable], X: Sequence[torch.Tensor], Y: Sequence[torch.Tensor],
                 kind: int = KIND_RBF, spec: Optional[hyper.HyperSpec] = None, device: Optional[torch.device] = None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.task_ids = list(task_ids)
        self.kind = int(kind)
        self.spec = spec or hyper.source_gp_spec()
        T = len(self.task_ids)
        self.D = int(X[0].shape[-1])
        ns = [int(x.shape[-2]) for x in X]
        self.N = max(ns)
        self.ragged = min(ns) != self.N
        Xp = torch.zeros(T, self.N, self.D, dtype=torch.float64)
        yp = torch.zeros(T, self.N, dtype=torch.float64)
        means, stds = torch.zeros(T, dtype=torch.float64), torch.ones(T, dtype=torch.float64)
        for t, (x, y) in enumerate(zip(X, Y)):
            y = torch.as_tensor(y, dtype=torch.float64).reshape(-1, 1).cpu()
            m, s = standardize_fit(y)
            means[t], stds[t] = m.squeeze(), s.squeeze()
            Xp[t, :ns[t]] = torch.as_tensor(x, dtype=torch.float64).cpu()
            yp[t, :ns[t]] = ((y - m) / s).squeeze(-1)
        self.X = Xp.to(self.device)
        self.y = yp.to(self.device)
        self.y_mean, self.y_std = means.to(self.device), stds.to(self.device)
        self.n_list = ns
        self.n_points = torch.tensor(ns, dtype=torch.int32, device=self.device) if self.ragged else None
        self.n_float = torch.tensor(ns, dtype=torch.float64, device=self.device)
        self.raw = self.spec.to_raw(self.spec.init_theta(self.D, device=self.device)).repeat(T, 1)
        self._fit = None
        self._rep_cache = {}
        self.shard: Optional[sdist.TaskShard] = None   # set by meta_fit_scamlgp(shard=True): this stack = tasks [lo, hi) of T_global

    # -- hyper-parameters -----------------------------------------------------------------
    @property
    def T(self) -> int:
        return len(self.task_ids)

    @property
    def theta(self) -> torch.Tensor:
        return self.spec.to_theta(self.raw)

    def set_theta(self, theta: torch.Tensor) -> None:
        self.raw = self.spec.to_raw(theta.to(self.device, torch.float64))
        self._fit = None

    # -- fused fit ------------------------------------------------------------------------
    def refresh(self) -> dict:
        """Factor all tasks at the current hyper-parameters (one launch) and cache L, alpha, W."""
        fit = ops.gp_fit_fused(self.X, self.y, self.theta, self.kind, n_points=self.n_points, want_linv=True)
        ops.raise_if_not_psd(fit["info"])
        # the explicit inverse factor: computed once per fit, it makes every later posterior a matrix product
        # (the role of gpytorch's prediction-strategy caches; scamlgp/model.py:128, :281 query fixed source GPs)
        # (only the block rows the posterior kernels read are written: lower_only)
        fit["Linv"] = ops.linv_batched(fit["L"], fit["Linv_diag"], n_points=self.n_points, lower_only=True)
        self._fit = fit
        return fit

    @property
    def fit(self) -> dict:
        return self._fit if self._fit is not None else self.refresh()

    def _replicated(self, reps: int):
        """The data of ``reps`` hyper-parameter sets per task, built once per ``reps`` (not per evaluation)."""
        c = self._rep_cache.get(reps)
        if c is None:
            c = dict(X=self.X.repeat(reps, 1, 1) if reps > 1 else self.X, y=self.y.repeat(reps, 1) if reps > 1 else self.y,
                     npts=None if self.n_points is None else self.n_points.repeat(reps), nflt=self.n_float.repeat(reps), out=None)
            self._rep_cache = {reps: c}   # one entry: the buffers of another batch size are released
        return c

    def objective(self, raw: torch.Tensor, reps: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """Negative training objective and its gradient w.r.t. the raw parameters for ``reps``
        hyper-parameter sets per task: raw (reps * T, D+2), problem b belongs to task b % T.
        objective = -(mll + sum log p(theta) / n)   (gpytorch ExactMarginalLogLikelihood with priors,
        A5 of SURVEY.md).  The marginal likelihood is the differentiable op ``ops.FusedMLL`` (one fused-fit
        launch forward, the analytic gradient kernels backward); constraint transform and priors are torch
        ops, and torch.autograd chains them -- "autograd stays in PyTorch" (scamlgp/utils.py:175, 190)."""
        c = self._replicated(reps)
        raw_ = raw.detach().requires_grad_(True)
        theta = self.spec.to_theta(raw_)
        mll = ops.fused_mll(c["X"], c["y"], theta, self.kind, c["npts"], c["out"])
        if self.N <= ops.fit_max_n():
            c["out"] = ops.FusedMLL.last   # reuse the factor buffers: backward always runs before the next forward here
        f = -(mll + self.spec.log_prior(theta) / c["nflt"])
        bad = ops.FusedMLL.last["info"] > 0
        (g,) = torch.autograd.grad(torch.where(bad, torch.zeros_like(f), f).sum(), raw_)
        f = torch.where(bad, torch.full_like(f, float("nan")), f.detach())
        return f, g

    def summed_mll_and_grad(self, theta_shared: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """sum_t MLL_t and sum_t dMLL_t/dtheta at ONE hyper-parameter vector shared by all tasks -- of this stack and,
        when the stack is a shard, of every rank's: local sums, then one fused all-reduce [sum MLL || sum grad]
        (BASELINE configs[3]: "RCCL all-reduce of the MLL hyper-gradient")."""
        th = theta_shared.to(self.device, torch.float64).reshape(1, -1).expand(self.T, -1).contiguous().requires_grad_(True)
        mll = ops.fused_mll(self.X, self.y, th, self.kind, self.n_points)
        (g,) = torch.autograd.grad(mll.sum(), th)
        return sdist.reduce_mll_and_grad(mll.detach(), g, self.shard)

    # -- posteriors -----------------------------------------------------------------------
    def posterior(self, xq: torch.Tensor, cov_first: int = 0, want_var: bool = True, VA: Optional[torch.Tensor] = None) -> dict:
        """Un-standardised posteriors of all tasks at xq (M, D): mean (T, M), var (T, M),
        cov (T, cov_first, M).  ``VA``: the cached V of the leading ``cov_first`` points (ops.source_posteriors)."""
        f = self.fit
        return ops.source_posteriors(xq.to(self.device, torch.float64), self.X, self.theta, self.kind, f["L"], f["Linv_diag"],
                                     f["alpha"], self.y_mean, self.y_std, n_points=self.n_points, want_var=want_var,
                                     cov_first=cov_first, Linv=f.get("Linv"), VA=VA)

    def raw_targets(self) -> torch.Tensor:
        """All source observations in original units, concatenated (scamlgp/model.py:264-270)."""
        out = []
        for t, n in enumerate(self.n_list):
            out.append(self.y_mean[t] + self.y_std[t] * self.y[t, :n])
        return torch.cat(out).unsqueeze(-1)

    def slice(self, lo: int, hi: int) -> "SourceGPStackSlice":
        """The stack over tasks [lo, hi) of this one: views of its tensors and factors, no copy (``SourceGPStackSlice``)."""
        return SourceGPStackSlice(self, lo, hi)


class SourceGPStackSlice(SourceGPStack):
    """Tasks [lo, hi) of a parent stack as a stack of its own: ``X``, ``y``, ``y_mean``, ``y_std``, ``n_float``, ``n_points``, ``raw`` and
    every entry of ``fit`` are the parent's tensors ``narrow``ed along the task axis (no copy; ``raw`` and ``fit`` follow the parent when
    it is refitted), ``N`` is the parent's padded N, ``task_ids`` / ``n_list`` / ``raw_targets()`` are the slice's own -- so a ScaMLGP on
    it standardises over ITS tasks' observations (scamlgp/model.py:264-273) and its source pass launches hi - lo tasks.  The
    hyper-parameters and factors belong to the parent: ``set_theta`` and ``refresh`` raise here.  ``parent`` and ``lo`` are what the
    grouped source pass of several slices needs (``utils.StudiesAcquisition``: the parent's arrays and a task base per study)."""

    def __init__(self, parent: SourceGPStack, lo: int, hi: int):
        if isinstance(parent, SourceGPStackSlice):
            raise TypeError("slice the parent stack (a slice of a slice would hide the arrays the factors live in)")
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= parent.T:
            raise ValueError(f"slice [{lo}, {hi}) of a stack of {parent.T} tasks")
        if parent.shard is not None:
            raise NotImplementedError("slices of a task-sharded source stack (shard=True) are not implemented")
        self.parent, self.lo, self.hi = parent, lo, hi
        T = hi - lo
        self.device, self.kind, self.spec, self.D, self.N = parent.device, parent.kind, parent.spec, parent.D, parent.N
        self.task_ids = parent.task_ids[lo:hi]
        self.n_list = parent.n_list[lo:hi]
        self.ragged = min(self.n_list) != self.N
        self.X, self.y = parent.X.narrow(0, lo, T), parent.y.narrow(0, lo, T)
        self.y_mean, self.y_std = parent.y_mean.narrow(0, lo, T), parent.y_std.narrow(0, lo, T)
        self.n_float = parent.n_float.narrow(0, lo, T)
        self.n_points = parent.n_points.narrow(0, lo, T) if self.ragged else None
        self._rep_cache = {}
        self._fit_view = (None, None)   # (the parent's fit dict, its narrowed twin)
        self.shard = None

    @property
    def raw(self) -> torch.Tensor:
        return self.parent.raw.narrow(0, self.lo, self.hi - self.lo)

    @raw.setter
    def raw(self, value) -> None:
        raise RuntimeError("a slice's hyper-parameters belong to its parent stack: set them on the parent")

    def set_theta(self, theta: torch.Tensor) -> None:
        raise RuntimeError("a slice's hyper-parameters belong to its parent stack: call set_theta on the parent")

    def refresh(self) -> dict:
        raise RuntimeError("a slice's factors belong to its parent stack: call refresh on the parent")

    @property
    def fit(self) -> dict:
        pf = self.parent.fit
        if self._fit_view[0] is not pf:
            Tp, T = self.parent.T, self.hi - self.lo
            view = {k: (v.narrow(0, self.lo, T) if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == Tp else v) for k, v in pf.items()}
            self._fit_view = (pf, view)
        return self._fit_view[1]

    def slice(self, lo: int, hi: int) -> "SourceGPStackSlice":
        return SourceGPStackSlice(self, lo, hi)   # (raises)


class SourceGP:
    """View of one task of a SourceGPStack with the attributes the reference touches on a
    SingleTaskGP: ``posterior(x).mvn``, ``outcome_transform.stdvs / untransform``, ``train_targets``."""

    def __init__(self, stack: SourceGPStack, index: int):
        self._stack, self._index = stack, index

    @property
    def outcome_transform(self) -> _OutcomeTransform:
        return _OutcomeTransform(self._stack.y_mean[self._index], self._stack.y_std[self._index])

    @property
    def train_targets(self) -> torch.Tensor:
        return self._stack.y[self._index, : self._stack.n_list[self._index]]

    @property
    def train_inputs(self):
        return (self._stack.X[self._index, : self._stack.n_list[self._index]],)

    def posterior(self, x: torch.Tensor) -> _Posterior:
        if x.dim() > 2:
            raise ValueError("SourceGP.posterior takes x (M, D): batched inputs go through ScaMLGP.posterior / forward")
        x2 = x.reshape(-1, x.shape[-1])
        M = x2.shape[0]
        p = self._stack.posterior(x2, cov_first=M)
        return _Posterior(p["mean"][self._index], p["cov"][self._index])


def _stack_of(source_gps: Sequence[SourceGP]) -> Tuple[SourceGPStack, List[int]]:
    stacks = {id(g._stack) for g in source_gps}
    if len(stacks) != 1:
        raise ValueError("all source GPs must come from one meta_fit_scamlgp call (one device-resident stack)")
    return source_gps[0]._stack, [g._index for g in source_gps]


# ---------------------------------------------------------------------------------------
# reference API
# ---------------------------------------------------------------------------------------
def _canonical_order(X: torch.Tensor, Y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """A task's observations in lexicographic order of (x_0, ..., x_{d-1}, y).  The reference sorts the meta
    evaluations before it builds the datasets (scamlgp/utils.py:72-109 ``sort_evaluations``) "to ensure that
    optimization runs are deterministic regardless of the order of input meta evaluations" -- the property its
    ``is_deterministic_with_shuffled_meta_data`` pins (scamlgp/testing.py:38-99); sorting here gives the kernels
    bit-identical stacks for shuffled inputs."""
    import numpy as np

    Xn = torch.as_tensor(X, dtype=torch.float64).reshape(-1, X.shape[-1]).cpu().numpy()
    Yn = torch.as_tensor(Y, dtype=torch.float64).reshape(-1, 1).cpu().numpy()
    order = np.lexsort(tuple(np.concatenate([Xn, Yn], 1).T[::-1]))
    return torch.from_numpy(Xn[order]), torch.from_numpy(Yn[order])


def meta_fit_scamlgp(
    meta_data: Dict[Hashable, SupervisedDataset],
    likelihood: Optional[hyper.GaussianLikelihood] = None,
    covar_module: Optional[hyper.ScaleKernel] = None,
    num_restarts_log_likelihood: int = 5,
    seed: Optional[int] = None,
    device: Optional[torch.device] = None,
    shard: bool = False,
    group=None,
    fit_options: Optional[dict] = None,
) -> Dict[Hashable, SourceGP]:
    """Train the source GPs on the given meta-data (scamlgp/model.py:138-189).

    ``fit_options`` is forwarded to ``optimize_marginal_likelihood`` (the reference forwards ``fit_gpytorch_options`` the same
    way, scamlgp/utils.py:139-175), e.g. ``{"driver": "device"}`` for the optimiser on the device.

    ``shard=True`` under an initialised torch.distributed group (one process per GPU): every rank is handed the SAME
    ``meta_data`` and keeps, fits and returns only its contiguous shard of the tasks (``dist.shard_range``); the
    tasks are independent, so the fit needs no collective.  A ScaMLGP built on such a dict all-reduces the one
    coupling of the path -- the weighted sums over tasks (scamlgp/model.py:129-134) -- across the ranks.

    ``likelihood`` / ``covar_module`` are templates, as in the reference (which deep-copies them per task): their
    constraints, priors and current values become every task's starting point.  Defaults: the reference's
    Gaussian likelihood and ScaleKernel(RBFKernel) with SingleTaskGP's priors.  All tasks and all restarts are
    optimised together on the GPU."""
    from .utils import optimize_marginal_likelihood

    if seed is not None:
        torch.manual_seed(seed=seed)
    validate_meta_data(meta_data)
    first = list(meta_data.values())[0]
    if first.X.dim() != 2:
        raise ValueError("batched (batch_shape x n x d) meta-data is not supported by the stacked GPU path")
    lik, cov = _resolve_modules(likelihood, covar_module, int(first.X.shape[-1]), hyper.get_kernel_source_gp)
    task_ids, data = list(meta_data.keys()), list(meta_data.values())
    ts = None
    if shard:
        ts = sdist.TaskShard(len(task_ids), group)
        if ts.hi == ts.lo:
            raise ValueError(f"rank {ts.rank} of {ts.world} would hold no task: shard fewer ranks than tasks")
        task_ids, data = task_ids[ts.local], data[ts.local]
    Xs, Ys = zip(*[_canonical_order(d.X(), d.Y()) for d in data])
    stack = SourceGPStack(task_ids, Xs, Ys, kind=cov.kind, spec=hyper.spec_from_modules(lik, cov), device=device)
    stack.shard = ts if ts is not None and ts.world > 1 else None
    optimize_marginal_likelihood(stack, num_restarts=num_restarts_log_likelihood, **(fit_options or {}))
    return {tid: SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}


def meta_fit_scamlgp_studies(
    meta_data_per_study: Sequence[Dict[Hashable, SupervisedDataset]],
    likelihood: Optional[hyper.GaussianLikelihood] = None,
    covar_module: Optional[hyper.ScaleKernel] = None,
    num_restarts_log_likelihood: int = 5,
    seed: Optional[int] = None,
    device: Optional[torch.device] = None,
    shard: bool = False,
    group=None,
    fit_options: Optional[dict] = None,
) -> List[Dict[Hashable, SourceGP]]:
    """``meta_fit_scamlgp`` for S studies that each bring their own meta-data (scamlgp/benchmarking/local_runner.py:51-65: every
    study of a configuration draws its own meta-tasks): ONE stack of S * T tasks, fitted by one ``optimize_marginal_likelihood`` call
    exactly as one large stack is (``fit_options={"driver": "device"}`` for the optimiser on the device), and S dicts of ``SourceGP``s
    on its slices (``SourceGPStack.slice``: study s = tasks [s T, (s + 1) T)).  A ``ScaMLGP`` on such a dict sees a T-task stack;
    ``bo.ScaMLGPBOStudies`` takes the list as its ``source_gps``.  The dicts need an equal number of tasks T and one input dimension;
    task ids need only be unique within a study.  ``shard=True`` is refused."""
    from .utils import optimize_marginal_likelihood

    if shard:
        raise NotImplementedError("per-study source stacks are not implemented for a task-sharded fit (shard=True)")
    studies = list(meta_data_per_study)
    if not studies:
        raise ValueError("Empty meta data. Needs at least one study.")
    if seed is not None:
        torch.manual_seed(seed=seed)
    for md in studies:
        validate_meta_data(md)
        if list(md.values())[0].X.dim() != 2:
            raise ValueError("batched (batch_shape x n x d) meta-data is not supported by the stacked GPU path")
    T, D = len(studies[0]), int(list(studies[0].values())[0].X.shape[-1])
    for s, md in enumerate(studies):
        if len(md) != T:
            raise ValueError(f"study {s} has {len(md)} source tasks but study 0 has {T}: the studies must have an equal number of tasks")
        d = int(list(md.values())[0].X.shape[-1])
        if d != D:
            raise ValueError(f"study {s} has input dimension {d} but study 0 has {D}")
    lik, cov = _resolve_modules(likelihood, covar_module, D, hyper.get_kernel_source_gp)
    ids = [(s, tid) for s, md in enumerate(studies) for tid in md]
    Xs, Ys = zip(*[_canonical_order(d.X(), d.Y()) for md in studies for d in md.values()])
    stack = SourceGPStack(ids, Xs, Ys, kind=cov.kind, spec=hyper.spec_from_modules(lik, cov), device=device)
    optimize_marginal_likelihood(stack, num_restarts=num_restarts_log_likelihood, **(fit_options or {}))
    out = []
    for s, md in enumerate(studies):
        sl = stack.slice(s * T, (s + 1) * T)
        sl.task_ids = list(md.keys())
        out.append({tid: SourceGP(sl, i) for i, tid in enumerate(sl.task_ids)})
    return out


def significant_weights_mask(weights: torch.Tensor, std_Y_vals: torch.Tensor, threshold: float) -> torch.Tensor:
    """Pruning criterion of scamlgp/model.py:192-215: task i is kept when its share of the scaled weights,
    w_i sigma_i / mean_j(w_j sigma_j), reaches ``threshold``."""
    scaled = weights * std_Y_vals
    return scaled * scaled.numel() / scaled.sum() >= threshold


def _compute_target_prior(x: torch.Tensor, source_gps: List[SourceGP], weights: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """scamlgp/model.py:108-135: mean = sum_i w_i mu_i(x) as (n, 1), cov = sum_i w_i^2 Sigma_i(x, x) (n, n),
    in original units.  One batched posterior launch + two weighted task sums."""
    if len(source_gps) != len(weights):
        raise ValueError(f"The number of source GPs, {len(source_gps)}, does not equal the number of weights, {len(weights)}")
    stack, idx = _stack_of(source_gps)
    if x.dim() > 2:
        raise ValueError("_compute_target_prior takes x (n, D): batched inputs go through ScaMLGP.posterior / forward")
    x2 = x.reshape(-1, x.shape[-1]).to(stack.device, torch.float64)
    M = x2.shape[0]
    p = stack.posterior(x2, cov_first=M)
    w_full = torch.zeros(stack.T, dtype=torch.float64, device=stack.device)
    w_full[idx] = weights.to(stack.device, torch.float64)
    active = torch.zeros(stack.T, dtype=torch.bool, device=stack.device)
    active[idx] = True
    mean = ops.weighted_task_sum(p["mean"], w_full, 1, active)
    cov = ops.weighted_task_sum(p["cov"], w_full, 2, active)
    return mean.unsqueeze(-1), cov


def _kernel_torch(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, kind: int) -> torch.Tensor:
    """os * k(x1 / l, x2 / l) in torch (target GP only: n <= ~80 rows)."""
    D = x1.shape[-1]
    a, b = x1 / theta[:D], x2 / theta[:D]
    d2 = (a.unsqueeze(-2) - b.unsqueeze(-3)).pow(2).sum(-1)
    if kind == KIND_RBF:
        k = torch.exp(-0.5 * d2)
    else:
        r = torch.sqrt(d2.clamp_min(1e-30))
        k = (1.0 + math.sqrt(5.0) * r + (5.0 / 3.0) * d2) * torch.exp(-math.sqrt(5.0) * r)
    return theta[D] * k


def psd_safe_cholesky(A: torch.Tensor, max_tries: int = 3) -> torch.Tensor:
    """linear_operator's psd_safe_cholesky in torch, for the target GP's n x n matrix (n <= ~80; the reference
    reaches it through scamlgp/utils.py:171-177 for the target fit as for the source fits): try as is; on failure
    add 1e-8, 1e-7, 1e-6 to the diagonal in turn (each try replaces the previous jitter); then NotPSDError.  NaN in
    A raises at once.  Differentiable (the jitter is a constant shift)."""
    if bool(torch.isnan(A).any()):
        raise ops.NotPSDError(f"cholesky_cpu: {int(torch.isnan(A).sum())} of {A.numel()} elements of the matrix are NaN.")
    L, info = torch.linalg.cholesky_ex(A)
    if not bool(info.any()):
        return L
    eye = torch.eye(A.shape[-1], dtype=A.dtype, device=A.device)
    for i in range(max_tries):
        jitter = 1e-8 * 10 ** i
        warnings.warn(f"A not p.d., added jitter of {jitter:.1e} to the diagonal", RuntimeWarning)
        L, info = torch.linalg.cholesky_ex(A + jitter * eye)
        if not bool(info.any()):
            return L
    raise ops.NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to {jitter:.1e}.")


def _split_batch(X: torch.Tensor, D: int):
    """X (..., q, D) -> (flat (M, D), batch_shape or None, q): botorch hands models ``batch_shape x q x d`` inputs
    (scamlgp/model.py:359-384 keeps the batch dimensions); the kernels take one flat list of M = prod(batch) * q points."""
    if X.dim() <= 2:
        return X.reshape(-1, D), None, X.reshape(-1, D).shape[0]
    return X.reshape(-1, D), tuple(X.shape[:-2]), int(X.shape[-2])


def _batch_blocks(cov: torch.Tensor, batch, q: int) -> torch.Tensor:
    """The per-batch q x q diagonal blocks of a joint (M, M) covariance, shaped (*batch, q, q)."""
    B = cov.shape[0] // q
    blocks = cov.reshape(B, q, B, q).diagonal(dim1=0, dim2=2).permute(2, 0, 1)
    return blocks.reshape(*batch, q, q)


class _LazyMVN:
    """``posterior(X).mvn``: mean (M,), variance (M,) at once; the joint (M, M) covariance only when asked for
    (an acquisition function over 1 000 candidates never needs it)."""

    def __init__(self, mean: torch.Tensor, variance: torch.Tensor, cov_fn):
        self.mean, self.variance, self._cov_fn, self._cov = mean, variance, cov_fn, None

    @property
    def covariance_matrix(self) -> torch.Tensor:
        if self._cov is None:
            self._cov = self._cov_fn()
        return self._cov

    lazy_covariance_matrix = covariance_matrix

    @property
    def stddev(self) -> torch.Tensor:
        return self.variance.clamp_min(0.0).sqrt()


class TargetPosterior:
    """What botorch's ``model.posterior(X)`` returns, reduced to what its callers read: ``.mean`` / ``.variance``
    as (M, 1) columns, ``.mvn.mean`` (M,), ``.mvn.variance`` (M,), ``.mvn.covariance_matrix`` (M, M)."""

    def __init__(self, mean: torch.Tensor, variance: torch.Tensor, cov_fn):
        self.mvn = _LazyMVN(mean, variance, cov_fn)

    mean = property(lambda self: self.mvn.mean.unsqueeze(-1))
    variance = property(lambda self: self.mvn.variance.unsqueeze(-1))

    def rsample(self, sample_shape: torch.Size = torch.Size(), generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """Joint samples ``(*sample_shape, *batch, M, 1)``: mean + L eps with L the jittered Cholesky of ``.mvn.covariance_matrix``
        (psd_safe_cholesky) and eps standard normal base samples drawn from ``generator`` (on the generator's device; default:
        torch's global one on the CPU), so that a seeded generator reproduces the samples."""
        mean = self.mvn.mean
        L = psd_safe_cholesky(self.mvn.covariance_matrix)
        gdev = generator.device if generator is not None else torch.device("cpu")
        eps = torch.randn(*torch.Size(sample_shape), *mean.shape, dtype=torch.float64, generator=generator, device=gdev).to(mean.device)
        return (mean + (L @ eps.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1)


class _StateCache:
    """Values computed from parameter tensors, kept per name until one of those tensors is replaced or modified in place.  An entry
    holds (tensor, version) pairs: the held references keep the objects alive, so identity cannot be faked by a recycled address."""

    def __init__(self) -> None:
        self._entries: dict = {}

    def get(self, name: str, tensors):
        """The value ``put`` under ``name`` if ``tensors`` are the very tensors it was computed from, unmodified since; else None."""
        held, value = self._entries.get(name, ((), None))
        same = len(held) == len(tensors) and all(h is t and v == t._version for (h, v), t in zip(held, tensors))
        return value if same else None

    def put(self, name: str, tensors, value):
        self._entries[name] = (tuple((t, t._version) for t in tensors), value)
        return value


class ScaMLGP:
    """Scalable meta-learning GP (scamlgp/model.py:218-384): target prior
    N(sum_i w_i mu_i, sum_i w_i^2 Sigma_i + k_t) over the posteriors of the source stack.

    Same constructor arguments and attributes as the reference class: ``likelihood`` / ``covar_module`` are the
    parameter-carrying modules (``hyper.GaussianLikelihood``, ``hyper.ScaleKernel``; the fitted ones of a previous
    model may be passed back in, scamlgp/optimizer.py:176-183), ``train_inputs``, ``train_targets``, ``weights``,
    ``source_gps``, ``source_means``, ``source_covs``, ``forward``, ``posterior``, ``train`` / ``eval``,
    ``state_dict`` / ``load_state_dict``."""

    def __init__(self, train_X: torch.Tensor, train_Y: torch.Tensor, source_gps: Dict[Hashable, SourceGP],
                 likelihood: Optional[hyper.GaussianLikelihood] = None, covar_module: Optional[hyper.ScaleKernel] = None,
                 weight_pruning_threshold: float = 1e-3, _fixed_transform: Optional[tuple] = None) -> None:
        self._weight_pruning_threshold = weight_pruning_threshold
        self.source_gps = source_gps
        gps = list(source_gps.values())
        self._stack, self._idx = _stack_of(gps)
        dev = self._stack.device
        self.device = dev
        self.train_X = torch.as_tensor(train_X, dtype=torch.float64).reshape(-1, self._stack.D).to(dev)
        self.train_Y = torch.as_tensor(train_Y, dtype=torch.float64).reshape(-1, 1).to(dev)
        self._idx_dev = torch.as_tensor(self._idx, dtype=torch.int64, device=dev)
        self._shard = self._stack.shard
        if self._shard is not None and len(gps) != self._stack.T:
            raise ValueError("a sharded source stack must be passed whole (every rank its full shard)")
        self.n, self.T = self.train_X.shape[0], (self._shard.n_tasks if self._shard is not None else len(gps))
        lik, cov = _resolve_modules(likelihood, covar_module, self._stack.D, hyper.get_default_kernel)
        self.likelihood, self.covar_module = lik.to(dev), cov.to(dev)
        self.kind = cov.kind
        self.spec = hyper.spec_from_modules(lik, cov)
        if _fixed_transform is None:
            # standardise w.r.t. ALL meta + target observations (scamlgp/model.py:264-276)
            self.has_transform = self.train_Y.numel() > 0
            if self._shard is None:
                m, s = standardize_fit(torch.cat([self._stack.raw_targets(), self.train_Y], dim=-2))
            else:   # the same statistics from all-reduced sums: no rank ever holds the other shards' observations
                m, s = sdist.standardize_fit_sharded(self._stack.raw_targets(), self.train_Y, self._shard)
            self.m_all, self.s_all = (m.squeeze(), s.squeeze()) if self.has_transform else (self.train_Y.new_zeros(()), self.train_Y.new_ones(()))
        else:   # condition_on_observations: the parent's transform, kept fixed (botorch's convention)
            self.has_transform = bool(_fixed_transform[2])
            self.m_all, self.s_all = _fixed_transform[0].clone(), _fixed_transform[1].clone()
        self._m_all_f, self._s_all_f = float(self.m_all), float(self.s_all)   # (one sync here instead of one per posterior call)
        self.outcome_transform = _OutcomeTransform(self.m_all, self.s_all) if self.has_transform else None
        self.train_inputs = (self.train_X,)
        self.train_targets = ((self.train_Y - self.m_all) / self.s_all).squeeze(-1)
        self._cache = _StateCache()                       # per parameter state: theta, pruned weights, training prior, Knn's factor
        self._stds_all = self._VA = self._tprob = None    # fixed for the model's lifetime, computed on first use
        # cached source posteriors at the target inputs, all tasks, no pruning (scamlgp/model.py:279-289)
        if self.n > 0:
            # (V of the training points: computed once here, reused by every later posterior / gradient call of this model)
            va = self._train_VA() if (self.n <= studies.MAX_N and self._stack.fit.get("Linv") is not None) else None
            p = self._stack.posterior(self.train_X, cov_first=self.n, VA=va)
            # (sharded: every rank contributes its tasks' columns, one all-reduce each -- n <= ~80, tiny)
            self.source_means = sdist.gather_task_axis(p["mean"][self._idx].transpose(0, 1).contiguous(), self._shard)   # (n, T)
            self.source_covs = sdist.gather_task_axis(p["cov"][self._idx].permute(1, 2, 0).contiguous(), self._shard)    # (n, n, T)
        self.raw_weights = torch.full((self.T,), 1.0 / self.T, dtype=torch.float64, device=dev)
        self.weights_prior = hyper.GammaPrior(1.0, 1.0)
        self.weights_lower_bound = 1e-10   # GreaterThan(1e-10, transform=None): a box bound for the optimiser
        self.training = True
        self.num_fantasies: Optional[int] = None   # F of a fantasy model (condition_on_observations with (F, p, 1) targets)

    @property
    def batch_shape(self) -> torch.Size:
        return torch.Size([self.num_fantasies]) if self.num_fantasies is not None else torch.Size()

    # the cached source posteriors at the training inputs: tensors, or -- a model from ``fantasize_studies`` -- a callable that cuts them
    # out of the batch's source pass on first read (a fantasy model is not fitted: only ``forward`` in training mode reads them)
    def _resolved(self, name: str) -> torch.Tensor:
        v = self.__dict__.get(name)
        if v is None:
            raise AttributeError(f"'ScaMLGP' object has no attribute '{name[1:]}' (a model without training data caches no source terms)")
        if callable(v):
            v = self.__dict__[name] = v()
        return v

    source_means = property(lambda self: self._resolved("_source_means"), lambda self, v: self.__dict__.__setitem__("_source_means", v))
    source_covs = property(lambda self: self._resolved("_source_covs"), lambda self, v: self.__dict__.__setitem__("_source_covs", v))

    @classmethod
    def _fantasy_of(cls, parent: "ScaMLGP", train_X: torch.Tensor, y_fant: torch.Tensor, VA: torch.Tensor, factor: dict,
                    source_means, source_covs) -> "ScaMLGP":
        """The fantasy model ``parent.fantasize`` would build for the pending points that close ``train_X`` (n + p, D), WITHOUT
        ``__init__``'s source launches (``fantasize_studies``): y_fant (F, p) the sampled outcomes in original units, ``VA`` its
        ``_train_VA()``, ``factor`` its target factor with alpha_f, the source terms as callables.  Everything else is what
        ``condition_on_observations`` leaves: copied modules, the parent's weights and transform kept fixed; ``spec`` is the parent's
        object (the constraints and priors are the same; a fantasy model is not fitted, so the init values are not used)."""
        new = cls.__new__(cls)
        F, n = int(y_fant.shape[0]), int(train_X.shape[0])
        new._weight_pruning_threshold = parent._weight_pruning_threshold
        new.source_gps, new._stack, new._idx, new._idx_dev, new._shard = parent.source_gps, parent._stack, parent._idx, parent._idx_dev, None
        new.device, new.n, new.T, new.kind, new.spec = parent.device, n, parent.T, parent.kind, parent.spec
        new.likelihood, new.covar_module = copy.deepcopy(parent.likelihood), copy.deepcopy(parent.covar_module)
        new.has_transform = parent.has_transform
        new.m_all, new.s_all = parent.m_all.clone(), parent.s_all.clone()
        new._m_all_f, new._s_all_f = parent._m_all_f, parent._s_all_f
        new.outcome_transform = _OutcomeTransform(new.m_all, new.s_all) if new.has_transform else None
        new.train_X = train_X
        new.train_inputs = (train_X,)
        new.train_Y = torch.cat([parent.train_Y.unsqueeze(0).expand(F, -1, -1), y_fant.unsqueeze(-1)], 1)   # (F, n + p, 1)
        new.train_targets = ((new.train_Y - new.m_all) / new.s_all).squeeze(-1).contiguous()                # (F, n + p)
        new._cache = _StateCache()
        new._stds_all, new._VA, new._tprob = parent._stds_all, VA, None
        new.source_means, new.source_covs = source_means, source_covs
        new.raw_weights = parent.raw_weights.detach().clone()
        new.weights_prior, new.weights_lower_bound = parent.weights_prior, parent.weights_lower_bound
        new.training = parent.training
        new.num_fantasies = F
        # equal parameters, equal derived values: the parent's constrained theta and pruned weights serve the copy's parameter state
        new._cache.put("theta", new._param_tensors(), parent.theta)
        new._cache.put("active", (new.weights,), parent._active_tasks())
        new._keep_target_factor(factor)
        return new

    # -- conditioning on new observations and fantasies (pending evaluations) ----------------------------------------------
    def condition_on_observations(self, X: torch.Tensor, Y: torch.Tensor) -> "ScaMLGP":
        """The model with (X (p, D), Y) appended to its target training set, Y (p, 1) or (F, p, 1) in original units: same
        hyper-parameters (copied modules), same weights, same source stack, the parent's outcome transform kept fixed (m_all / s_all
        are not refitted: botorch's convention), no refit.  Y (p, 1): an ordinary ScaMLGP.  Y (F, p, 1): a fantasy model of batch
        shape (F,) -- ``posterior(Xq)`` gives ``.mean`` / ``.variance`` (F, M, 1), the variance the same for every f; the acquisition
        functions average over the F fantasies (``fantasy_acqf``); ``mll`` and refitting raise."""
        if self._shard is not None:
            raise NotImplementedError("conditioning / fantasies are not implemented for a task-sharded source stack (shard=True)")
        if self.num_fantasies is not None:
            raise NotImplementedError("a fantasy model cannot be conditioned further")
        D = self._stack.D
        X = torch.as_tensor(X, dtype=torch.float64).to(self.device).reshape(-1, D)
        Y = torch.as_tensor(Y, dtype=torch.float64).to(self.device)
        p = X.shape[0]
        if Y.dim() == 1:
            Y = Y.unsqueeze(-1)
        if Y.dim() not in (2, 3) or tuple(Y.shape[-2:]) != (p, 1):
            raise ValueError(f"Y must be (p, 1) or (F, p, 1) with p = {p}, got {tuple(Y.shape)}")
        Y0 = Y[0] if Y.dim() == 3 else Y
        new = ScaMLGP(torch.cat([self.train_X, X]), torch.cat([self.train_Y, Y0]), self.source_gps,
                      likelihood=copy.deepcopy(self.likelihood), covar_module=copy.deepcopy(self.covar_module),
                      weight_pruning_threshold=self._weight_pruning_threshold, _fixed_transform=(self.m_all, self.s_all, self.has_transform))
        new.raw_weights = self.raw_weights.detach().clone()
        new.training = self.training
        if Y.dim() == 3:
            F = Y.shape[0]
            new.num_fantasies = int(F)
            new.train_Y = torch.cat([self.train_Y.unsqueeze(0).expand(F, -1, -1), Y], 1)            # (F, n + p, 1)
            new.train_targets = ((new.train_Y - new.m_all) / new.s_all).squeeze(-1).contiguous()   # (F, n + p)
        return new

    def fantasize(self, X: torch.Tensor, num_fantasies: int, generator: Optional[torch.Generator] = None,
                  observation_noise: bool = True) -> "ScaMLGP":
        """A fantasy model for pending evaluations at X (p, D): ``num_fantasies`` joint samples of the posterior at X (the (p, p)
        covariance of ``posterior(X).mvn.covariance_matrix``, plus the noise on its diagonal with ``observation_noise``), base samples
        from ``generator``, then ``condition_on_observations(X, samples)``.  Monte-Carlo integration over the pending outcomes inside
        the acquisition function (the "integrated acquisition" of Snoek et al., 2012, what botorch's ``fantasize`` serves).  The
        reference hands this step to blackboxopt, which is not available here, so which strategy it applies is not checked."""
        if self._shard is not None:
            raise NotImplementedError("fantasies are not implemented for a task-sharded source stack (shard=True)")
        X = torch.as_tensor(X, dtype=torch.float64).to(self.device).reshape(-1, self._stack.D)
        samples = self.posterior(X, observation_noise=observation_noise).rsample(torch.Size([int(num_fantasies)]), generator=generator)
        return self.condition_on_observations(X, samples)

    # -- parameters -------------------------------------------------------------------------
    @property
    def weights(self) -> torch.Tensor:
        return self.raw_weights

    @weights.setter
    def weights(self, value) -> None:
        self.raw_weights = torch.as_tensor(value, dtype=torch.float64).to(self.device)

    @property
    def raw_theta(self) -> torch.Tensor:
        """[raw lengthscales (D), raw outputscale, raw noise]: the modules' parameters as one vector."""
        cov, lik = self.covar_module, self.likelihood
        return torch.cat([cov.base_kernel.raw_lengthscale.reshape(-1), cov.raw_outputscale.reshape(1), lik.raw_noise.reshape(1)])

    @raw_theta.setter
    def raw_theta(self, value: torch.Tensor) -> None:
        v = torch.as_tensor(value, dtype=torch.float64).to(self.device).detach()
        D = self._stack.D
        self.covar_module.base_kernel._p.raw = v[:D].clone()
        self.covar_module._p.raw = v[D].clone()
        self.likelihood._p.raw = v[D + 1].clone()

    def _param_tensors(self):
        cov, lik = self.covar_module, self.likelihood
        return (cov.base_kernel.raw_lengthscale, cov.raw_outputscale, lik.raw_noise)

    @property
    def theta(self) -> torch.Tensor:
        """Constrained target hyper-parameters [lengthscales, outputscale, noise].  Cached per parameter state: an acquisition
        pass asks for them (and for the pruned weights below) on every call, each time a dozen element-wise launches for the
        same numbers -- a quarter of a scoring pass at configs[4] was such glue."""
        now = self._param_tensors()
        theta = self._cache.get("theta", now)
        return theta if theta is not None else self._cache.put("theta", now, self.spec.to_theta(self.raw_theta))

    def train(self):
        self.training = True
        return self

    def eval(self):
        self.training = False
        return self

    def state_dict(self) -> dict:
        return {"raw_theta": self.raw_theta.clone(), "raw_weights": self.raw_weights.clone()}

    def load_state_dict(self, sd: dict) -> None:
        self.raw_theta, self.raw_weights = sd["raw_theta"].clone(), sd["raw_weights"].clone()

    # -- model ------------------------------------------------------------------------------
    def _std_source_stds(self) -> torch.Tensor:
        if self._stds_all is None:
            self._stds_all = sdist.gather_task_axis(self._stack.y_std[self._idx], self._shard)
        return self._stds_all

    def _active_tasks(self):
        """Pruned weights as vectors over this rank's stack: w_full (T_stack,), active mask (bool)
        (scamlgp/model.py:365-372; the mask is decided on ALL T weights, each rank then takes its slice)."""
        w = key = self.weights
        c = self._cache.get("active", (key,))
        if c is not None:
            return c      # (same weights as last time: see `theta`)
        mask = significant_weights_mask(w, self._std_source_stds(), self._weight_pruning_threshold)
        if self._shard is not None:
            w, mask = w[self._shard.local], mask[self._shard.local]
        # (scatter instead of mask indexing: nothing here depends on a value read back by the host, so the whole
        #  acquisition pass can be captured into a HIP graph)
        idx = self._idx_dev
        w_full = torch.zeros(self._stack.T, dtype=torch.float64, device=self.device).scatter(0, idx, w)
        active = torch.zeros(self._stack.T, dtype=torch.bool, device=self.device).scatter(0, idx, mask)
        return self._cache.put("active", (key,), (w_full, active))

    def _source_prior(self, x: torch.Tensor, cov_first: int, train_first: bool = False):
        """sum_i w_i mu_i(x) (M,), sum_i w_i^2 Sigma_i (cov_first, M), sum_i w_i^2 var_i (M,) over the significant tasks
        of ALL ranks, in original units: one batched posterior launch over this rank's stack, the weighted task sums,
        and -- sharded -- ONE all-reduce of the fused buffer [mu_s || Sigma_s || var_s]."""
        w_full, active = self._active_tasks()
        # (the leading points of a joint evaluation are the model's training inputs: their V is computed once per model)
        va = self._train_VA() if (train_first and 0 < cov_first == self.n <= studies.MAX_N and x.shape[0] > self.n and self._stack.fit.get("Linv") is not None) else None
        p = self._stack.posterior(x, cov_first=cov_first, VA=va)
        mu_s, cov_s = ops.weighted_prior_reduce(p["mean"], p["cov"], w_full, active)
        var_s = ops.weighted_task_sum(p["var"], w_full, 2, active)
        mu_s, cov_s, var_s = sdist.fused_allreduce([mu_s, cov_s, var_s], self._shard)
        return mu_s, cov_s, var_s

    def forward(self, x: torch.Tensor) -> _MVN:
        """scamlgp/model.py:359-384.  Training: cached source terms at train_X; eval: pruned weights and a
        fresh batched source posterior at x.  Both in the standardised target space, plus k_t(x, x)."""
        x, batch, q = _split_batch(torch.as_tensor(x, dtype=torch.float64).to(self.device), self._stack.D)
        w = self.weights
        if self.training:
            mean = self.source_means @ w
            cov = self.source_covs @ w ** 2
        else:
            # = _compute_target_prior over the significant models (scamlgp/model.py:365-375), as stack-wide sums
            mean, cov, _ = self._source_prior(x, x.shape[0])
        if self.has_transform:
            mean = (mean - self.m_all) / self.s_all
            cov = cov / self.s_all ** 2
        cov = cov + _kernel_torch(x, x, self.theta, self.kind)
        if batch is not None and not self.training:   # (batch, q, D) input: independent q-point joints, one per batch element
            return _MVN(mean.reshape(*batch, q), _batch_blocks(cov, batch, q))
        return _MVN(mean, cov)

    __call__ = forward

    def mll(self, raw_theta: Optional[torch.Tensor] = None, raw_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Training objective (A9): [log N(y~ | mean, cov + sigma^2 I) + log priors] / n, differentiable in torch."""
        if self.num_fantasies is not None:
            raise NotImplementedError("a fantasy model is not fitted: it keeps its parent's hyper-parameters")
        rt = self.raw_theta if raw_theta is None else raw_theta
        w = self.raw_weights if raw_weights is None else raw_weights
        theta = self.spec.to_theta(rt)
        mean = (self.source_means @ w - self.m_all) / self.s_all
        cov = (self.source_covs @ w ** 2) / self.s_all ** 2 + _kernel_torch(self.train_X, self.train_X, theta, self.kind)
        cov = cov + theta[-1] * torch.eye(self.n, dtype=torch.float64, device=self.device)
        if 1 <= self.n <= ops.fit_max_n():
            # the library's jittered Cholesky + solves as ONE differentiable op: no host synchronisation (psd_safe_cholesky's
            # status check is one), so that the whole objective can be replayed from a HIP graph (utils._fit_target); a matrix
            # that is not positive definite even with jitter gives NaN instead of NotPSDError
            val = ops.gaussian_log_prob(cov, self.train_targets - mean)
        else:
            Lc = psd_safe_cholesky(cov)
            v = torch.linalg.solve_triangular(Lc, (self.train_targets - mean).unsqueeze(-1), upper=False)
            val = -0.5 * ((v * v).sum() + 2.0 * torch.log(torch.diagonal(Lc)).sum() + self.n * _LOG_2PI)
        val = val + self.spec.log_prior(theta) + self.weights_prior.log_prob(w).sum()
        return val / self.n

    def target_problem(self) -> Optional[ops.TargetFitProblem]:
        """The training set in the layouts of the library's target-fit kernel (built once; None if the kernel does not take
        this shape -- more target points than its LDS holds, D > 16 -- and the torch objective ``mll`` is all there is)."""
        if self._tprob is None:
            if self.num_fantasies is not None:
                raise NotImplementedError("a fantasy model is not fitted: it keeps its parent's hyper-parameters")
            if self.n < 1 or not ops.TargetFitProblem.supported(self.n, self.T, self._stack.D):
                return None
            self._tprob = ops.TargetFitProblem(self.source_means, self.source_covs, self.train_X, self.train_targets, self._m_all_f,
                                               self._s_all_f, self.spec, self.weights_prior, self.weights_lower_bound, self.kind)
        return self._tprob

    def mll_and_grad(self, z: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The training objective ``mll`` and its analytic gradient w.r.t. z = [raw_theta || raw_weights] for the rows of z
        (B, D + 2 + T) (default: the model's current parameters, B = 1): ONE launch of scaml_target_mll_f64 instead of torch
        autograd through ~100 small kernels.  Returns (value (B,), grad (B, P))."""
        prob = self.target_problem()
        if prob is None:
            raise ValueError("the target-fit kernel does not take this shape; use ScaMLGP.mll with torch autograd")
        if z is None:
            z = torch.cat([self.raw_theta, self.raw_weights]).unsqueeze(0)
        out = ops.target_mll(prob, z.to(self.device, torch.float64).reshape(-1, prob.P))
        return out["value"], out["grad"]

    def _joint(self, Xq: torch.Tensor, full: bool):
        """Standardised joint prior over cat(train_X, Xq) (A8, A10) from ONE source-posterior launch: mean (n + M,),
        the n x (n + M) covariance block (or the whole (n + M)^2 one with ``full``) and the query diagonal."""
        n, M = self.n, Xq.shape[0]
        xall = torch.cat([self.train_X, Xq], 0)
        first = n + M if full else n
        mu_s, cov_s, var_s = self._source_prior(xall, first)
        theta = self.theta
        mean = (mu_s - self.m_all) / self.s_all
        var_q = var_s[n:] / self.s_all ** 2 + theta[-2]
        cov = None
        if first > 0:
            cov = cov_s / self.s_all ** 2 + _kernel_torch(xall[:first], xall, theta, self.kind)
        return mean, cov, var_q, theta

    # -- posterior with input gradients (what the acquisition optimiser differentiates through) ------------------------------
    def supports_posterior_grad(self) -> bool:
        """The analytic input-gradient path needs training data within the fused covariance block (n <= 96), D <= 15 and the
        explicit inverse factors of the source stack (SourceGPStack.refresh caches them)."""
        return studies.takes(self)

    def _train_VA(self) -> torch.Tensor:
        """V = L^-1 K(X_t, train_X) of every source task (T, N, n): fixed for the model's lifetime (sources and training inputs are)."""
        if self._VA is None:
            st, f = self._stack, self._stack.fit
            self._VA = ops.source_posteriors(self.train_X, st.X, st.theta, st.kind, f["L"], f["Linv_diag"], f["alpha"], st.y_mean, st.y_std,
                                             n_points=st.n_points, want_var=False, keep_V=True, Linv=f["Linv"])["V"]
        return self._VA

    def _train_prior(self):
        """The weighted source sums at the training inputs (mu_s (n,), Sigma_s (n, n), var_s (n,)): per weight state."""
        w = self.weights
        c = self._cache.get("train_prior", (w,))
        return c if c is not None else self._cache.put("train_prior", (w,), self._source_prior(self.train_X, self.n))

    def _target_factor(self):
        """The jittered Cholesky of the target GP's training block Knn (+ alpha) at the current weights / hyper-parameters, or None
        if it has not been computed for this parameter state yet: it does not depend on the query points, and an acquisition
        optimisation scores hundreds of query batches against one parameter state."""
        return self._cache.get("factor", (self.weights,) + self._param_tensors())

    def _keep_target_factor(self, factor) -> None:
        self._cache.put("factor", (self.weights,) + self._param_tensors(), factor)

    def posterior_with_grad(self, X: torch.Tensor):
        """Target posterior mean / variance at X (Mq, D) in original units AND their gradients w.r.t. X: (mu (Mq,), var (Mq,),
        dmu (Mq, D), dvar (Mq, D)).  The reference gets these from torch autograd through ``model.posterior`` inside botorch's
        optimize_acqf (scamlgp/utils.py:215-224, SURVEY 3.3 HOT LOOP #4); here: one source pass with 16 columns per query point
        (value + D derivative right-hand sides through the same L^-1 product, scaml_posterior_linv_grad_f64), the weighted task
        sums, the target GP's value path (assemble / jittered Cholesky / solve / finish) and one contraction kernel
        (scaml_target_posterior_grad_f64) -- an L-BFGS-B evaluation over R starts scores R points instead of the (2 D + 1) R of a
        central-difference stencil, with exact gradients."""
        if not self.supports_posterior_grad():
            raise NotImplementedError(f"analytic posterior gradients need {studies.LIMITS}")
        if self.num_fantasies is not None:
            raise NotImplementedError("a fantasy model's acquisition gradient comes from fantasy_acqf (the acquisition-function classes)")
        Xq = torch.as_tensor(X, dtype=torch.float64).reshape(-1, self._stack.D).to(self.device).contiguous()
        cov_s, mean_s, var_s, xall, cov_g, mu_g, var_g = self._grad_pass(Xq)
        theta = self.theta
        full = ops.target_posterior_full(cov_s, mean_s, var_s, xall, theta, self.train_targets, self._m_all_f, self._s_all_f, self.kind,
                                         factor=self._target_factor())
        self._keep_target_factor(full["factor"])
        dmu, dvar = ops.target_posterior_grad(cov_g, mu_g, var_g, self.train_X, Xq, theta, full["alpha"], full["Z"], self._s_all_f,
                                              full["info"], self.kind)
        return full["mu"], full["var"], dmu, dvar

    def _grad_pass(self, Xq: torch.Tensor):
        """The source pass of ``posterior_with_grad`` at Xq (Mq, D): the joint prior over cat(train_X, Xq) for the target GP's value
        path (cov_s (n, n + Mq), mean_s, var_s (n + Mq,), xall) and the weighted GRAD-pass sums (cov_g (n, Mq * 16), mu_g, var_g)."""
        Mq, n = Xq.shape[0], self.n
        st, f = self._stack, self._stack.fit
        w_full, active = self._active_tasks()
        mu_t, cov_tt, var_t = self._train_prior()
        g = ops.source_posteriors_grad(Xq, self.train_X, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean, st.y_std, st.n_points,
                                       self._train_VA())
        mu_g, cov_g = ops.weighted_prior_reduce(g["mu"].reshape(st.T, Mq * 16), g["cov"], w_full, active)
        var_g = ops.weighted_task_sum(g["var"].reshape(st.T, Mq * 16), w_full, 2, active)
        mu_g, cov_g, var_g = sdist.fused_allreduce([mu_g, cov_g, var_g], self._shard)
        # the value columns next to the training block: the joint prior the target GP's value path takes
        cov_s = torch.cat([cov_tt, cov_g.reshape(n, Mq, 16)[:, :, 0]], 1)
        mean_s = torch.cat([mu_t, mu_g.reshape(Mq, 16)[:, 0]])
        var_s = torch.cat([var_t, var_g.reshape(Mq, 16)[:, 0]])
        xall = torch.cat([self.train_X, Xq], 0)
        return cov_s, mean_s, var_s, xall, cov_g, mu_g, var_g

    def joint_acqf(self, X: torch.Tensor, acqf: int, acqf_param: float, base_samples: torch.Tensor, want_grad: bool = False,
                   X_pending=None):
        """The joint Monte-Carlo acquisition function of B batches of q points, X (B, q, D): qEI (``acqf`` ops.ACQF_EI, acqf_param =
        best_f) or qUCB (ops.ACQF_UCB, beta) over the JOINT posterior of each batch, reparameterised with ``base_samples`` (S, q)
        -- (value (B,), d value / d X (B, q, D) or None).  The value pass at the B q points keeps their V; the joint GRAD pass
        (scaml_posterior_linv_grad_joint_f64) adds, per point, the covariances with its batch mates and their input derivatives; the
        weighted task sums, the assemble and Z = Knn^-1 Knq are those of ``posterior_with_grad`` (the training block's factor is cached);
        then ONE launch of scaml_target_qacqf_f64 factors every batch's q x q posterior covariance, draws the samples, evaluates the
        utility and carries the adjoint back through the factor to the inputs: no (B, S, q) tensor reaches memory.

        ``X_pending`` (p, D), or the dict ``joint_pending`` made of it: evaluations that are running (botorch's X_pending).  They join
        every batch behind its q points -- ``base_samples`` is (S, q + p), the utility's maximum runs over all q + p joint samples --
        and stay fixed: value (B,), gradient (B, q, D).  The pending points are the same in every batch, so they ride with the LEADING
        points of the source pass (Xa = cat(train_X, X_pending), Ma = n + p); the passes still see B q strips and
        scaml_target_qacqf_pending_f64 puts the (q + p) x (q + p) joint together.  None or p = 0: the path above, unchanged."""
        out = self.joint_acqf_full(X, acqf, acqf_param, base_samples, want_grad, X_pending)
        return out["value"], out["grad"]

    def joint_acqf_full(self, X: torch.Tensor, acqf: int, acqf_param: float, base_samples: torch.Tensor, want_grad: bool = False,
                        X_pending=None) -> dict:
        """``joint_acqf`` with the kernel's per-batch status: dict(value (B,), grad (B, q, D) or None, jitter (B,) -- the rung of the
        ladder 0, 1e-8, 1e-7, 1e-6 that made the batch's covariance positive definite --, info (B,) int32 -- 1: none did, the batch is
        NaN)."""
        if acqf not in (ops.ACQF_UCB, ops.ACQF_EI):   # (before anything is launched; the kernel refuses the same codes)
            raise ValueError("the joint acquisition function takes ops.ACQF_UCB or ops.ACQF_EI: a joint LogEI is not defined")
        kw = self.joint_acqf_inputs(X, base_samples, X_pending)
        B, q, D = kw.pop("shape")
        if B == 0:
            return dict(value=kw["Xq"].new_empty((0,)), grad=kw["Xq"].new_empty((0, q, D)) if want_grad else None,
                        jitter=kw["Xq"].new_empty((0,)), info=torch.empty(0, dtype=torch.int32, device=self.device))
        kernel = ops.target_qacqf_pending if "Xp" in kw else ops.target_qacqf
        out = kernel(acqf=acqf, acqf_param=acqf_param, want_grad=want_grad, **kw)
        out["grad"] = out["grad"].reshape(B, q, D) if want_grad else None
        return out

    def _joint_refusals(self) -> None:
        if self.num_fantasies is not None:
            raise NotImplementedError("the joint acquisition function is not defined on a fantasy model")
        if self._shard is not None:
            raise NotImplementedError("the joint acquisition function takes an unsharded source stack")
        if not self.supports_posterior_grad():
            raise NotImplementedError(f"the joint acquisition function needs {studies.LIMITS}")

    def joint_pending(self, X_pending: torch.Tensor) -> dict:
        """What ``joint_acqf(..., X_pending=)`` needs of a pending set X_pending (p, D) and what does not depend on the batches: the
        leading points of the source pass with the pending ones behind the training inputs (Xa (n + p, D), VA (T, N, n + p)), Zp (n, p) =
        Knn^-1 Knp, and the target posterior of the pending points among themselves in original units without observation noise
        (mu_p (p,), Sigma_pp (p, p)).  Computed for the model's current weights and hyper-parameters: an acquisition-function object
        calls this once and passes the dict with every evaluation."""
        self._joint_refusals()
        st, f = self._stack, self._stack.fit
        Xp = torch.as_tensor(X_pending, dtype=torch.float64).to(self.device).reshape(-1, st.D).contiguous()
        if Xp.shape[0] == 0:
            return dict(Xp=Xp)
        n, p = self.n, int(Xp.shape[0])
        if p >= ops.qacqf_max_q():
            raise NotImplementedError(f"the joint acquisition kernel takes q + p <= {ops.qacqf_max_q()} points: {p} pending leave no room for a batch")
        if n + p + 1 > studies.MAX_N or n + p + 1 > st.N:
            raise NotImplementedError(f"the joint acquisition function needs n + p + q <= {min(studies.MAX_N, st.N)}")
        Vp = ops.source_posteriors(Xp, st.X, st.theta, st.kind, f["L"], f["Linv_diag"], f["alpha"], st.y_mean, st.y_std, n_points=st.n_points,
                                   want_var=False, keep_V=True, Linv=f["Linv"])["V"]
        mvn = self.posterior(Xp).mvn
        xall = torch.cat([self.train_X, Xp], 0)
        mean_s, cov_s, var_s = self._source_prior(xall, n, train_first=True)
        factor = self._target_factor()
        if factor is not None and "alpha_f" not in factor:
            factor = dict(factor, alpha_f=factor["alpha"][0].unsqueeze(-1))
        blk = ops.target_fantasy_block(cov_s, mean_s, var_s, xall, self.theta, self.train_targets.unsqueeze(0), self._m_all_f, self._s_all_f,
                                       self.kind, factor=factor)
        return dict(Xp=Xp, Xa=xall, VA=torch.cat([self._train_VA(), Vp], -1).contiguous(), Zp=blk["Z"].contiguous(),
                    mu_p=mvn.mean.contiguous(), Sigma_pp=mvn.covariance_matrix.contiguous())

    def _joint_arguments(self, X: torch.Tensor, base_samples: torch.Tensor, X_pending=None):
        """The arguments of a joint evaluation, checked before anything batch-dependent is launched: X (B, q, D) and base_samples
        (S, q + p) on the device, and ``joint_pending``'s dict (None with no point pending).  The refusals of ``joint_acqf``."""
        self._joint_refusals()
        st = self._stack
        X = torch.as_tensor(X, dtype=torch.float64).to(self.device)
        if X.dim() != 3 or X.shape[-1] != st.D:
            raise ValueError("joint_acqf takes X (B, q, D)")
        B, q, D = X.shape
        n = self.n
        pend = None
        if X_pending is not None:
            pend = X_pending if isinstance(X_pending, dict) else self.joint_pending(X_pending)
            if pend["Xp"].shape[0] == 0:
                pend = None
        p = 0 if pend is None else int(pend["Xp"].shape[0])
        base_samples = torch.as_tensor(base_samples, dtype=torch.float64).to(self.device)
        if base_samples.dim() != 2 or base_samples.shape[1] != q + p or base_samples.shape[0] < 1:
            raise ValueError("base_samples must be (S, q)" if p == 0 else "base_samples must be (S, q + p)")
        if q > ops.qacqf_max_q() or base_samples.shape[0] > ops.qacqf_max_samples():
            raise NotImplementedError(f"the joint acquisition kernel takes q <= {ops.qacqf_max_q()} and at most {ops.qacqf_max_samples()} samples")
        if n + q > studies.MAX_N or n + q > st.N:
            raise NotImplementedError(f"the joint acquisition function needs n + q <= {min(studies.MAX_N, st.N)}")
        if p > 0 and q + p > ops.qacqf_max_q():
            raise NotImplementedError(f"the joint acquisition kernel takes q + p <= {ops.qacqf_max_q()} points, got q = {q} and {p} pending")
        if p > 0 and (n + p + q > studies.MAX_N or n + p + q > st.N):
            raise NotImplementedError(f"the joint acquisition function needs n + p + q <= {min(studies.MAX_N, st.N)}")
        return X, base_samples, pend

    def joint_acqf_inputs(self, X: torch.Tensor, base_samples: torch.Tensor, X_pending=None) -> dict:
        """Everything of ``joint_acqf`` in front of the acquisition kernel, for X (B, q, D): the keyword arguments of
        ``ops.target_qacqf`` by name (Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_g, mu_g, var_g, Xt, Xq, theta, base_samples,
        kind) and ``shape`` = (B, q, D).  They do not depend on the acquisition code or its parameter.  With p > 0 pending points
        (``X_pending``: (p, D) or ``joint_pending``'s dict): the keyword arguments of ``ops.target_qacqf_pending`` -- the same names,
        cov_g with n + p + q rows, base_samples (S, q + p), and Xp, Zp, mu_p, Sigma_pp."""
        st, f = self._stack, self._stack.fit
        X, base_samples, pend = self._joint_arguments(X, base_samples, X_pending)
        B, q, D = X.shape
        n = self.n
        Xq = X.reshape(B * q, D).contiguous()
        if B == 0:
            return dict(Xq=Xq, shape=(B, q, D))
        Mq = B * q
        w_full, active = self._active_tasks()
        mu_t, cov_tt, var_t = self._train_prior()
        VQ = ops.source_posteriors(Xq, st.X, st.theta, st.kind, f["L"], f["Linv_diag"], f["alpha"], st.y_mean, st.y_std, n_points=st.n_points,
                                   want_var=False, keep_V=True, Linv=f["Linv"])["V"]
        # (pending points are leading points: rows n .. n + p - 1 of every strip's covariance block, in front of the mates' rows)
        Xa, VA = (self.train_X, self._train_VA()) if pend is None else (pend["Xa"], pend["VA"])
        g = ops.source_posteriors_grad_joint(Xq, q, Xa, st.X, st.theta, st.kind, f["Linv"], f["alpha"], VA, VQ,
                                             st.y_mean, st.y_std, st.n_points)
        mu_g, cov_g = ops.weighted_prior_reduce(g["mu"].reshape(st.T, Mq * 16), g["cov"], w_full, active)
        var_g = ops.weighted_task_sum(g["var"].reshape(st.T, Mq * 16), w_full, 2, active)
        mu_g, cov_g, var_g = sdist.fused_allreduce([mu_g, cov_g, var_g], self._shard)
        # the value columns of the training rows next to the training block: the joint prior the target GP's value path takes
        cov_s = torch.cat([cov_tt, cov_g[:n].reshape(n, Mq, 16)[:, :, 0]], 1)
        mean_s = torch.cat([mu_t, mu_g.reshape(Mq, 16)[:, 0]])
        var_s = torch.cat([var_t, var_g.reshape(Mq, 16)[:, 0]])
        xall = torch.cat([self.train_X, Xq], 0)
        theta = self.theta
        factor = self._target_factor()
        if factor is not None and "alpha_f" not in factor:   # (cached by posterior(): one target vector, its alpha is the one column)
            factor = dict(factor, alpha_f=factor["alpha"][0].unsqueeze(-1))
        blk = ops.target_fantasy_block(cov_s, mean_s, var_s, xall, theta, self.train_targets.unsqueeze(0), self._m_all_f, self._s_all_f,
                                       self.kind, factor=factor)
        self._keep_target_factor(blk["factor"])
        kw = dict(Knq=blk["Knq"], Z=blk["Z"], alpha=blk["factor"]["alpha"][0], mean_q=blk["mean_q"], var_q=blk["var_q"], m_all=self._m_all_f,
                  s_all=self._s_all_f, info=blk["info"], cov_g=cov_g, mu_g=mu_g, var_g=var_g, Xt=self.train_X, Xq=Xq, theta=theta,
                  base_samples=base_samples, kind=self.kind, shape=(B, q, D))
        if pend is not None:
            kw.update(Xp=pend["Xp"], Zp=pend["Zp"], mu_p=pend["mu_p"], Sigma_pp=pend["Sigma_pp"])
        return kw

    def joint_acqf_opt_inputs(self, base_samples: torch.Tensor, X_pending=None) -> dict:
        """What the device optimiser of the joint acquisition (``ops.QAcqfOpt``, scaml_qacqf_opt_f64) is handed and what does not depend
        on the round: the arguments of ``joint_acqf_inputs``' launches by the C signature's names -- the source stack and the leading
        points (Xa, X, theta_s, Linv, alpha_s, y_mean, y_std, n_points_s, VA), w, active, the weighted source sums at the training
        inputs (mu_t, cov_tt, var_t), the target GP and the factor of its training block (Xt, theta_t, targets, L, Linv_diag, alpha_t,
        m_all, s_all, info), base_samples (S, q + p), kind_s, kind_t and, with p > 0 points pending (``X_pending``: (p, D) or
        ``joint_pending``'s dict), Xp, Zp, mu_p, Sigma_pp.  ``joint_acqf``'s refusals; the target factor of the current weights and
        hyper-parameters is computed here if no evaluation has cached it yet."""
        st, f = self._stack, self._stack.fit
        base_samples = torch.as_tensor(base_samples, dtype=torch.float64)
        if base_samples.dim() != 2:
            raise ValueError("base_samples must be (S, q + p)")
        pend = X_pending
        if X_pending is not None and not isinstance(X_pending, dict):
            self._joint_refusals()
            pend = self.joint_pending(X_pending)
        p = 0 if pend is None else int(pend["Xp"].shape[0])
        q = int(base_samples.shape[1]) - p
        if q < 1:
            raise ValueError("base_samples must be (S, q + p) with q >= 1")
        # (the refusals of a joint evaluation, on an empty set of batches of this q)
        _, base_samples, pend = self._joint_arguments(torch.empty(0, q, st.D, dtype=torch.float64), base_samples, pend)
        w_full, active = self._active_tasks()
        mu_t, cov_tt, var_t = self._train_prior()
        theta = self.theta
        factor = self._target_factor()
        if factor is None:
            factor = ops.target_fantasy_block(cov_tt, mu_t, var_t, self.train_X, theta, self.train_targets.unsqueeze(0), self._m_all_f,
                                              self._s_all_f, self.kind)["factor"]
            self._keep_target_factor(factor)
        Xa, VA = (self.train_X, self._train_VA()) if pend is None else (pend["Xa"], pend["VA"])
        kw = dict(Xa=Xa, X=st.X, theta_s=st.theta, Linv=f["Linv"], alpha_s=f["alpha"], y_mean=st.y_mean, y_std=st.y_std, n_points_s=st.n_points,
                  VA=VA, w=w_full, active=active.to(torch.uint8), mu_t=mu_t, cov_tt=cov_tt, var_t=var_t, Xt=self.train_X, theta_t=theta,
                  targets=self.train_targets, L=factor["L"], Linv_diag=factor["Linv_diag"], alpha_t=factor["alpha"][0],
                  m_all=self._m_all_f, s_all=self._s_all_f, info=factor["info"].reshape(-1)[:1], base_samples=base_samples,
                  kind_s=st.kind, kind_t=self.kind)
        if pend is not None:
            kw.update(Xp=pend["Xp"], Zp=pend["Zp"], mu_p=pend["mu_p"], Sigma_pp=pend["Sigma_pp"])
        return kw

    def joint_acqf_value(self, X: torch.Tensor, acqf: int, acqf_param: float, base_samples: torch.Tensor, X_pending=None) -> torch.Tensor:
        """``joint_acqf``'s value (B,) for X (B, q, D) WITHOUT its gradient, through a route of its own: what the scoring of an
        optimiser's raw candidates needs.  The batches are packed into strips of 16 columns (``ops.qacqf_value_pack``), the value-layout
        joint source pass (scaml_posterior_linv_cov_joint_f64) takes 16 points per strip -- the GRAD pass of ``joint_acqf`` one -- and
        gets the batch mates' covariances from the strip's own Gram tile, then the weighted task sums, the target's value path with the
        cached factor, and ONE launch of scaml_target_qacqf_value_f64 for all batches.  Same refusals, same ``X_pending`` (the pending
        points are leading points, ``joint_pending``'s dict is reused as it is), same base samples (S, q + p); the values are
        ``joint_acqf``'s up to the rounding of the two source passes."""
        return self.joint_acqf_value_full(X, acqf, acqf_param, base_samples, X_pending)["value"]

    def joint_acqf_value_full(self, X: torch.Tensor, acqf: int, acqf_param: float, base_samples: torch.Tensor, X_pending=None) -> dict:
        """``joint_acqf_value`` with the kernel's per-batch status: dict(value (B,), jitter (B,), info (B,) int32), as ``joint_acqf_full``."""
        if acqf not in (ops.ACQF_UCB, ops.ACQF_EI):   # (before anything is launched; the kernel refuses the same codes)
            raise ValueError("the joint acquisition function takes ops.ACQF_UCB or ops.ACQF_EI: a joint LogEI is not defined")
        kw = self.joint_acqf_value_inputs(X, base_samples, X_pending)
        B, q, D = kw.pop("shape")
        if B == 0:
            return dict(value=torch.empty(0, dtype=torch.float64, device=self.device), jitter=torch.empty(0, dtype=torch.float64, device=self.device),
                        info=torch.empty(0, dtype=torch.int32, device=self.device))
        return ops.target_qacqf_value(acqf=acqf, acqf_param=acqf_param, **kw)

    def joint_acqf_value_inputs(self, X: torch.Tensor, base_samples: torch.Tensor, X_pending=None) -> dict:
        """Everything of ``joint_acqf_value`` in front of the acquisition kernel, for X (B, q, D): the keyword arguments of
        ``ops.target_qacqf_value`` by name (Knq, Z, alpha, mean_q, var_q, m_all, s_all, info, cov_s, Xq, theta, base_samples, B, kind --
        Xq (Mp, D) the packed points, everything with a query axis at its Mp columns -- and Xp, Zp, mu_p, Sigma_pp with points pending)
        and ``shape`` = (B, q, D)."""
        st, f = self._stack, self._stack.fit
        X, base_samples, pend = self._joint_arguments(X, base_samples, X_pending)
        B, q, D = X.shape
        n = self.n
        if B == 0:
            return dict(shape=(B, q, D))
        Xq = ops.qacqf_value_pack(X)
        w_full, active = self._active_tasks()
        mu_t, cov_tt, var_t = self._train_prior()
        # (pending points are leading points: rows n .. n + p - 1 of the covariance block, in front of the mates' rows)
        Xa, VA = (self.train_X, self._train_VA()) if pend is None else (pend["Xa"], pend["VA"])
        g = ops.source_posteriors_cov_joint(Xq, B, q, Xa, st.X, st.theta, st.kind, f["Linv"], f["alpha"], VA, st.y_mean, st.y_std, st.n_points)
        mu_v, cov_v = ops.weighted_prior_reduce(g["mu"], g["cov"], w_full, active)
        var_v = ops.weighted_task_sum(g["var"], w_full, 2, active)
        # the training rows next to the training block: the joint prior the target GP's value path takes
        cov_s = torch.cat([cov_tt, cov_v[:n]], 1)
        mean_s = torch.cat([mu_t, mu_v])
        var_s = torch.cat([var_t, var_v])
        xall = torch.cat([self.train_X, Xq], 0)
        theta = self.theta
        factor = self._target_factor()
        if factor is not None and "alpha_f" not in factor:   # (cached by posterior(): one target vector, its alpha is the one column)
            factor = dict(factor, alpha_f=factor["alpha"][0].unsqueeze(-1))
        blk = ops.target_fantasy_block(cov_s, mean_s, var_s, xall, theta, self.train_targets.unsqueeze(0), self._m_all_f, self._s_all_f,
                                       self.kind, factor=factor)
        self._keep_target_factor(blk["factor"])
        kw = dict(Knq=blk["Knq"], Z=blk["Z"], alpha=blk["factor"]["alpha"][0], mean_q=blk["mean_q"], var_q=blk["var_q"], m_all=self._m_all_f,
                  s_all=self._s_all_f, info=blk["info"], cov_s=cov_v, Xq=Xq, theta=theta, base_samples=base_samples, B=B, kind=self.kind,
                  shape=(B, q, D))
        if pend is not None:
            kw.update(Xp=pend["Xp"], Zp=pend["Zp"], mu_p=pend["mu_p"], Sigma_pp=pend["Sigma_pp"])
        return kw

    def fantasy_acqf(self, X: torch.Tensor, acqf: int, acqf_param: float, want_grad: bool = False):
        """The acquisition function of a fantasy model, averaged over its fantasies, at X (M, D): (value (M,), d value / d X (M, D) or
        None).  ``acqf``: ops.ACQF_UCB (acqf_param = beta), ops.ACQF_EI or ops.ACQF_LOGEI (acqf_param = best_f).  The source pass at cat(X', Xq), the
        assemble and Z = Knn^-1 Knq are those of an ordinary model (the training block's factor and the F columns of alpha are computed
        once per parameter state and cached); then ONE launch of scaml_target_fantasy_acqf_f64 in place of the finish and gradient
        kernels: no per-fantasy work outside it."""
        if self.num_fantasies is None:
            raise ValueError("fantasy_acqf needs a fantasy model (ScaMLGP.fantasize)")
        if self.num_fantasies > studies.MAX_FANTASIES:
            raise NotImplementedError(f"the fantasy acquisition kernel takes at most {studies.MAX_FANTASIES} fantasies")
        Xq = torch.as_tensor(X, dtype=torch.float64).reshape(-1, self._stack.D).to(self.device).contiguous()
        n = self.n
        grad_inputs = None
        if want_grad:
            if not self.supports_posterior_grad():
                raise NotImplementedError(f"analytic acquisition gradients need {studies.LIMITS}")
            cov_s, mean_s, var_s, xall, cov_g, mu_g, var_g = self._grad_pass(Xq)
            grad_inputs = dict(cov_g=cov_g, mu_g=mu_g, var_g=var_g, Xt=self.train_X, Xq=Xq, theta=self.theta)
        else:
            if not 1 <= n <= ops.fit_max_n():
                raise NotImplementedError(f"the fantasy acquisition path takes 1 <= n <= {ops.fit_max_n()} training points")
            xall = torch.cat([self.train_X, Xq], 0)
            mean_s, cov_s, var_s = self._source_prior(xall, n, train_first=True)
        blk = ops.target_fantasy_block(cov_s, mean_s, var_s, xall, self.theta, self.train_targets, self._m_all_f, self._s_all_f, self.kind,
                                       factor=self._target_factor())
        self._keep_target_factor(blk["factor"])
        if Xq.shape[0] == 0:
            return Xq.new_empty((0,)), (Xq.new_empty((0, self._stack.D)) if want_grad else None)
        return ops.target_fantasy_acqf(blk["Knq"], blk["Z"], blk["alpha"], blk["mean_q"], blk["var_q"], self._m_all_f, self._s_all_f,
                                       blk["info"], acqf, acqf_param, 0.0, grad_inputs, self.kind)

    def _fantasy_posterior(self, Xq: torch.Tensor, batch, observation_noise: bool) -> TargetPosterior:
        """posterior() of a fantasy model at Xq (M, D): mean (F, M) from one product alpha^T Knq over all fantasies, the shared
        variance from scaml_target_finish_f64, the joint covariance (it does not depend on the targets either) only when read."""
        if batch is not None:
            raise ValueError("the posterior of a fantasy model takes X (M, D)")
        n, F = self.n, self.num_fantasies
        if not 1 <= n <= ops.fit_max_n():
            raise NotImplementedError(f"the fantasy posterior takes 1 <= n <= {ops.fit_max_n()} training points")
        xall = torch.cat([self.train_X, Xq], 0)
        mu_s, cov_s, var_s = self._source_prior(xall, n, train_first=True)
        theta = self.theta
        noise = float(theta[-1]) if observation_noise else 0.0
        blk = ops.target_fantasy_block(cov_s, mu_s, var_s, xall, theta, self.train_targets, self._m_all_f, self._s_all_f, self.kind,
                                       factor=self._target_factor(), var_noise_add=noise)
        self._keep_target_factor(blk["factor"])
        M = Xq.shape[0]
        mu = self.m_all + self.s_all * (blk["mean_q"] + blk["alpha"].transpose(0, 1) @ blk["Knq"])   # (F, M)
        mu = torch.where(blk["info"][0] > 0, torch.full_like(mu, float("nan")), mu)
        var = blk["var"].unsqueeze(0).expand(F, M)
        return TargetPosterior(mu, var, lambda: self._full_cov(Xq, observation_noise).unsqueeze(0).expand(F, M, M))

    def _full_cov(self, Xq: torch.Tensor, observation_noise: bool) -> torch.Tensor:
        """The joint (M, M) posterior covariance at Xq in original units: the Schur complement of the training block in the joint
        prior over cat(train_X, Xq) (a second source launch with the full query block)."""
        n = self.n
        _, cj, _, th = self._joint(Xq, full=True)
        S = cj[n:, n:]
        if n > 0:
            Lc2 = psd_safe_cholesky(cj[:n, :n] + th[-1] * torch.eye(n, dtype=torch.float64, device=self.device))
            V2 = torch.linalg.solve_triangular(Lc2, cj[:n, n:], upper=False)
            S = S - V2.transpose(0, 1) @ V2
        if observation_noise:
            S = S + th[-1] * torch.eye(S.shape[0], dtype=torch.float64, device=self.device)
        return self.s_all ** 2 * S

    def posterior(self, X: torch.Tensor, observation_noise: bool = False) -> TargetPosterior:
        """Target posterior at X (M, D) in original units (A10).  The source prior is evaluated ONCE at
        cat(train_X, X) -- train block, cross block and query diagonal -- instead of once per query as the
        reference does.  ``.mvn.covariance_matrix`` (the joint (M, M) covariance) costs a second
        launch with the full query block and is only computed when read.  X (M, D): M points, ``.mean`` (M, 1), joint (M, M)
        covariance.  X (*batch, q, D): ``.mean`` / ``.variance`` (*batch, q, 1), ``.mvn.covariance_matrix`` (*batch, q, q)."""
        Xq, batch, q = _split_batch(torch.as_tensor(X, dtype=torch.float64).to(self.device), self._stack.D)
        n = self.n
        if self.num_fantasies is not None:
            return self._fantasy_posterior(Xq, batch, observation_noise)
        if 1 <= n <= ops.fit_max_n():
            # the library's target-GP path: weighted source sums at cat(train_X, Xq), then assemble -> jittered Cholesky
            # (T = 1) -> solve -> finish: four launches, no host synchronisation, no torch arithmetic
            xall = torch.cat([self.train_X, Xq], 0)
            mu_s, cov_s, var_s = self._source_prior(xall, n, train_first=True)
            full = ops.target_posterior_full(cov_s, mu_s, var_s, xall, self.theta, self.train_targets, self._m_all_f, self._s_all_f, self.kind,
                                             observation_noise, factor=self._target_factor())
            self._keep_target_factor(full["factor"])
            mu_o, var_o = full["mu"], full["var"]
            # (a factorisation that fails even with jitter -- psd_safe_cholesky would raise NotPSDError -- comes back as NaN: the status
            #  stays on the device so that an acquisition-function evaluation never waits for the host)
        else:
            mean, cov, var_q, theta = self._joint(Xq, full=False)
            if n == 0:
                mu, var = mean, var_q
            else:
                Knn = cov[:, :n] + theta[-1] * torch.eye(n, dtype=torch.float64, device=self.device)
                Knq = cov[:, n:]
                Lc = psd_safe_cholesky(Knn)
                resid = (self.train_targets - mean[:n]).unsqueeze(-1)
                a = torch.cholesky_solve(resid, Lc).squeeze(-1)
                mu = mean[n:] + Knq.transpose(0, 1) @ a
                Vq = torch.linalg.solve_triangular(Lc, Knq, upper=False)
                var = var_q - (Vq * Vq).sum(0)
            if observation_noise:
                var = var + theta[-1]
            mu_o, var_o = self.m_all + self.s_all * mu, self.s_all ** 2 * var

        full_cov = lambda: self._full_cov(Xq, observation_noise)   # noqa: E731
        if batch is not None:
            # botorch's batch_shape x q x d convention (scamlgp/model.py:359-384 keeps the batch dimensions): mean / variance
            # (*batch, q, 1), covariance (*batch, q, q) -- one joint per batch element, NOT one joint over all points.  q = 1 (what
            # optimize_acqf sends to an analytic acquisition function) needs no joint at all.
            if q == 1:
                return TargetPosterior(mu_o.reshape(*batch, 1), var_o.reshape(*batch, 1), lambda: var_o.reshape(*batch, 1, 1))
            return TargetPosterior(mu_o.reshape(*batch, q), var_o.reshape(*batch, q), lambda: _batch_blocks(full_cov(), batch, q))
        return TargetPosterior(mu_o, var_o, full_cov)


def _fantasy_batch(models: Sequence[ScaMLGP], Xp: Sequence[torch.Tensor], Fs: Sequence[int], eps: torch.Tensor, own: bool) -> dict:
    """The device work of ``fantasize_studies`` for checked arguments: ``Xp[s]`` = cat(train_X, pending) of study s on the device, ``eps``
    (S, p_max, F_max) the draws (host or device), ``own``: the models sit on slices of one parent stack (``studies.source_stack`` finds
    the same).  Per study the V' launch, then the grouped value pass over the studies' X' strips, ``ops.studies_condition_block``,
    ``ops.potrf_batched``, ``ops.studies_fantasy_condition``.  Nothing is read back.  Returns dict(VA, pass (mu, var, cov), block (Knn,
    resid, mean_p), factor (``potrf_batched``'s dict), out (alpha_f, y_fant, mu_p), strip_base (host list) and the packed arrays by name)."""
    m0 = models[0]
    D, dev = m0._stack.D, m0.device
    ns, nps = [m.n for m in models], [int(x.shape[0]) for x in Xp]
    # V' per study, on its own stack object (step 1 of fantasize_studies)
    VA = []
    for m, x in zip(models, Xp):
        st, f = m._stack, m._stack.fit
        VA.append(ops.source_posteriors(x, st.X, st.theta, st.kind, f["L"], f["Linv_diag"], f["alpha"], st.y_mean, st.y_std,
                                        n_points=st.n_points, want_var=False, keep_V=True, Linv=f["Linv"])["V"].contiguous())
    # the batch (step 3): the studies' X' as query strips of 16 (filled up with a point of the box) and as leading points
    strips = [(n + 15) // 16 for n in nps]
    fill = torch.full((16, D), 0.5, dtype=torch.float64, device=dev)
    Xq = torch.cat([t for x, k in zip(Xp, strips) for t in (x, fill[:16 * k - x.shape[0]])], 0)
    a = studies.pack(models, VA, Xp)
    y = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence([m.train_targets for m in models], batch_first=True), (0, max(nps) - max(ns)))
    host = lambda vals: torch.tensor(vals, dtype=torch.int32).to(dev)   # noqa: E731
    base = [sum(strips[:s]) for s in range(len(models))]
    a.update(Xq=Xq, y=y, n_obs=host(ns), n_fant=host(Fs), strip_base=host(base), group=host([s for s, k in enumerate(strips) for _ in range(k)]),
             eps=eps.to(dev))
    src, own_kw = studies.source_stack(models, "fantasies are")
    fs = src.fit
    g = ops.source_posteriors_grouped(Xq, a["group"], a["Xt"], a["n_points"], a["VA_tab"], src.X, src.theta, src.kind, fs["Linv"], fs["alpha"],
                                      src.y_mean, src.y_std, src.n_points, **own_kw)
    blk = ops.studies_condition_block(g["mu"], g["cov"], a["strip_base"], a["w"], a["active"], a["Xt"], a["theta"], y, a["n_points"], a["n_obs"],
                                      a["m_all"], a["s_all"], m0.kind)
    fac = ops.potrf_batched(blk["Knn"], None, n_points=a["n_points"], want_linv=True)
    out = ops.studies_fantasy_condition(fac["L"], blk["resid"], blk["mean_p"], a["n_points"], a["n_obs"], fac["info"], a["eps"], a["n_fant"],
                                        a["m_all"], a["s_all"])
    return dict(VA=VA, strip_base=base, arrays=a, block=blk, factor=fac, out=out, **{"pass": g})


def fantasize_studies(models: Sequence[ScaMLGP], pending: Sequence[torch.Tensor], num_fantasies, generators: Sequence[Optional[torch.Generator]],
                      observation_noise: bool = True) -> List[ScaMLGP]:
    """``models[s].fantasize(pending[s], num_fantasies, generator=generators[s])`` for S studies at once: S fantasy models from a
    constant number of launches and ONE host round trip, where every ``fantasize`` call makes several dozen launches and three.

    ``models``: S ordinary ScaMLGP on one shared source stack, or on equal-T slices of one parent stack
    (``meta_fit_scamlgp_studies``) -- the rule of ``utils.StudiesAcquisition``; ``pending[s]`` (p_s, D) with p_s >= 1 and
    n_s + p_s <= 96; ``num_fantasies`` an int or one per study, at most 64; ``generators[s]`` as ``fantasize`` takes it.

    Everything follows from ONE Cholesky factor L' of the joint block K' over X' = cat(train_X, pending) (csrc/gp_studies_condition.h):
    the posterior at the pending points with observation noise has mean mean'_p + L_pn v, v = L_nn^-1 resid, and covariance
    L_pp L_pp^T, so the samples are mean'_p + L_pn v + L_pp eps_f and alpha_f = L'^-T [v ; eps_f].  The steps:
      1. per study the source-pass launch for V' = ``_train_VA`` of X'_s on the study's own stack -- the launch the conditioned model
         makes today, the same bits; these S asynchronous launches are the per-study device work that is left;
      2. per study ``eps_s = torch.randn(F, p_s, generator=...)`` with ``TargetPosterior.rsample``'s shape, dtype and device, so that a
         generator ends where a ``fantasize`` call leaves it;
      3. ONE value-mode grouped source pass over all studies' X' strips, ``ops.studies_condition_block``, ONE ``ops.potrf_batched``
         (ragged sizes, the jitter ladder per study), ``ops.studies_fantasy_condition``;
      4. one read-back of the studies' status: a block that fails on every rung raises ``ops.NotPSDError`` naming the study, as
         ``fantasize`` does through ``psd_safe_cholesky``; the jitter a study's block needed is in its model's ``last_condition_info``
         (its samples come from the jittered block);
      5. the models, without ``ScaMLGP.__init__``'s source launches (``ScaMLGP._fantasy_of``): ``_VA`` = V'_s, the study's slice of the
         factor with alpha_f kept as its target factor, ``source_means`` / ``source_covs`` cut out of the pass's outputs on first read.
    ``observation_noise=False`` is not implemented: L_pp L_pp^T is the covariance WITH the noise."""
    models, pending, generators = list(models), list(pending), list(generators)
    S = len(models)
    if S == 0:
        return []
    if len(pending) != S or len(generators) != S:
        raise ValueError(f"got {len(pending)} pending sets and {len(generators)} generators for {S} models")
    if not observation_noise:
        raise NotImplementedError("fantasize_studies samples with observation noise (the factor of the joint block holds it)")
    Fs = [int(num_fantasies)] * S if not isinstance(num_fantasies, (list, tuple)) else [int(v) for v in num_fantasies]
    if len(Fs) != S:
        raise ValueError(f"got {len(Fs)} fantasy counts for {S} models")
    _, own = studies.source_stack(models, "fantasies are")
    st0, dev = models[0]._stack, models[0].device
    Xp = []
    for s, m in enumerate(models):
        if m.num_fantasies is not None:
            raise NotImplementedError("a fantasy model cannot be conditioned further")
        x = torch.as_tensor(pending[s], dtype=torch.float64).to(dev).reshape(-1, st0.D)
        if x.shape[0] < 1 or not studies.takes(m, x.shape[0], Fs[s]):
            raise NotImplementedError(f"study {s}: fantasize_studies takes 1 <= n, p >= 1, n + p <= {studies.MAX_N} (and <= the stack's N), "
                                      f"D <= {studies.MAX_D} and at most {studies.MAX_FANTASIES} fantasies; use ScaMLGP.fantasize")
        Xp.append(torch.cat([m.train_X, x], 0))
    ns, nps = [m.n for m in models], [int(x.shape[0]) for x in Xp]
    # 2. the draws, one host table for the batch
    eps = torch.zeros(S, max(b - a for a, b in zip(ns, nps)), max(Fs), dtype=torch.float64)
    for s, gen in enumerate(generators):
        gdev = gen.device if gen is not None else torch.device("cpu")
        e = torch.randn(Fs[s], nps[s] - ns[s], dtype=torch.float64, generator=gen, device=gdev)
        eps[s, :nps[s] - ns[s], :Fs[s]] = e.transpose(0, 1).cpu()
    # 1. and 3. on the device
    b = _fantasy_batch(models, Xp, Fs, eps, bool(own))
    g, fac, out, VA, base = b["pass"], b["factor"], b["out"], b["VA"], b["strip_base"]
    # 4. the one round trip
    status = torch.cat([fac["info"].to(torch.float64), fac["jitter"]]).cpu()
    info, jitter = status[:S].to(torch.int64).tolist(), status[S:].tolist()
    bad = [s for s in range(S) if info[s] != 0]
    if bad:
        raise ops.NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to 1.0e-06 (the conditioned block of "
                              f"stud{'ies' if len(bad) > 1 else 'y'} {bad[:8]}{'...' if len(bad) > 8 else ''}).")
    # 5. the models
    fantasies = []
    for s, m in enumerate(models):
        n, F, c0 = nps[s], Fs[s], 16 * base[s]
        factor = studies.factor_slice(fac, s, n, alpha_f=out["alpha_f"][s, :n, :F].contiguous())
        rows = m._idx_dev   # (the model's tasks among the pass's rows: the stack's tasks, or the T slots of the study's slice)
        means = lambda rows=rows, c0=c0, n=n: g["mu"][rows, c0:c0 + n].transpose(0, 1).contiguous()              # noqa: E731  (n', T)
        covs = lambda rows=rows, c0=c0, n=n: g["cov"][rows, :n, c0:c0 + n].permute(1, 2, 0).contiguous()          # noqa: E731  (n', n', T)
        fm = ScaMLGP._fantasy_of(m, Xp[s], out["y_fant"][s, :n - ns[s], :F].transpose(0, 1), VA[s], factor, means, covs)
        fm.last_condition_info = dict(info=info[s], jitter=jitter[s])
        fantasies.append(fm)
    return fantasies
