"""What the batched studies paths share (``utils.StudiesAcquisition``, ``model.fantasize_studies``, ``bo.ScaMLGPBOStudies``): the limits
of the kernels behind them, the rule for which models may form a batch, the packing of the models into padded device arrays and a
study's slice of a batched factor.  Plain functions on ``ScaMLGP`` objects; nothing here calls the library."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

# The limits of the studies' kernels.  csrc/gp_studies_acqf.h defines the first three (STUDIES_ACQF_MAX_N, STUDIES_ACQF_MAX_D,
# STUDIES_FANTASY_MAX_F), ``scaml_posterior_max_n()`` answers the fourth; tests/test_dispatch.py and the grouped pass's GPU test hold
# these numbers to them.
MAX_N = 96           # training plus pending points per study: the GRAD pass's fused covariance block
MAX_D = 15           # input dimensions (the pass's 16 columns per query point: the value and D derivatives)
MAX_FANTASIES = 64   # fantasies per study
MAX_STACK_N = 512    # points per source task

LIMITS = f"1 <= n <= {MAX_N} training points and D <= {MAX_D}"   # (as the error messages word them)


def takes(model, pending: int = 0, fantasies: Optional[int] = None) -> bool:
    """Does the batched path take ``model``?  As it stands (``ScaMLGP.supports_posterior_grad``: 1 <= n <= MAX_N training -- on a
    fantasy model training and pending -- points, D <= MAX_D, a stack of N <= MAX_STACK_N on the GPU, at most MAX_FANTASIES fantasies);
    or, with ``fantasies`` given, as the ordinary model that is still to be conditioned on ``pending`` further points with that many
    fantasies: n + pending within MAX_N and within the stack's N (the points travel as query strips of the source pass), 1 <=
    ``fantasies`` <= MAX_FANTASIES.  Reads ``n``, ``num_fantasies``, ``device.type`` and ``_stack.D`` / ``_stack.N`` only."""
    st = model._stack
    if not (1 <= model.n and model.n + pending <= MAX_N and st.D <= MAX_D and st.N <= MAX_STACK_N and model.device.type == "cuda"):
        return False
    if fantasies is None:
        return model.num_fantasies is None or model.num_fantasies <= MAX_FANTASIES
    return model.num_fantasies is None and model.n + pending <= st.N and 1 <= fantasies <= MAX_FANTASIES


def source_stack(models: Sequence, what: str):
    """The rule for a batch: one source stack object shared by all models, or slices of one parent with an equal number of tasks T
    (``model.meta_fit_scamlgp_studies``); one kernel family; no task shard (``what`` words that refusal: "fantasies are").  Returns
    (source, own): the stack whose arrays the grouped source pass reads -- the shared one, or the parent -- and the pass's extra
    arguments, dict(task_base (G,) int32 on the device: the first task of study g, tasks_per_group = T) for slices, {} for a shared
    stack."""
    m0 = models[0]
    st0 = m0._stack
    parent = getattr(st0, "parent", None)
    shared = all(m._stack is st0 for m in models)
    own = (not shared) and parent is not None and all(getattr(m._stack, "parent", None) is parent and m._stack.T == st0.T for m in models)
    for m in models:
        if not (shared or own) or m.kind != m0.kind or m.T != m0.T:
            raise ValueError("the studies' models must share one source stack and one kernel family")
        if m._shard is not None:
            raise NotImplementedError(f"{what} not implemented for a task-sharded source stack (shard=True)")
    if not own:
        return st0, {}
    return parent, dict(task_base=torch.tensor([m._stack.lo for m in models], dtype=torch.int32).to(m0.device), tasks_per_group=st0.T)


def pack_parameters(models: Sequence):
    """(w (G, T) pruned weights, active (G, T) uint8, theta (G, D + 2)) of the models' current parameter states."""
    act = [m._active_tasks() for m in models]
    return torch.stack([a[0] for a in act]), torch.stack([a[1] for a in act]).to(torch.uint8), torch.stack([m.theta for m in models])


def pack(models: Sequence, VA: Sequence[torch.Tensor], Xp: Optional[Sequence[torch.Tensor]] = None) -> dict:
    """The models as the padded device arrays the batched kernels read, by name: w, active, theta (``pack_parameters``), Xt (G, n_max, D)
    zero-padded inputs, n_points (G,) int32, m_all, s_all (G,) the standardisers, VA_tab (G,) int64 the addresses of ``VA[g]``
    (contiguous; the caller keeps them alive).  ``Xp[g]``: the model's inputs where they are not its ``train_X`` -- the training set
    extended by pending points."""
    dev = models[0].device
    Xp = [m.train_X for m in models] if Xp is None else list(Xp)
    host = lambda vals, dt: torch.tensor(vals, dtype=dt).to(dev)   # noqa: E731
    w, active, theta = pack_parameters(models)
    return dict(w=w, active=active, theta=theta, Xt=torch.nn.utils.rnn.pad_sequence(Xp, batch_first=True),
                n_points=host([int(x.shape[0]) for x in Xp], torch.int32),
                m_all=host([m._m_all_f for m in models], torch.float64), s_all=host([m._s_all_f for m in models], torch.float64),
                VA_tab=host([v.data_ptr() for v in VA], torch.int64))


def factor_slice(f: dict, g: int, n: int, alpha_f: Optional[torch.Tensor] = None) -> dict:
    """Study g's slice, n points, of a batched factor ``f`` (``ops.target_factors_batched``, ``ops.potrf_batched(want_linv=True)``) in
    the layout a model keeps through ``_keep_target_factor``: its own ``ops.potrf_batched(Knn, resid, want_linv=True)``'s.  ``alpha_f``
    (n, F): a fantasy model's solutions -- kept under that name, column 0 as ``alpha``, no ``quad``."""
    cut = lambda key: f[key][g:g + 1]   # noqa: E731
    if alpha_f is None:
        alpha, quad, extra = cut("alpha")[:, :n].contiguous(), cut("quad"), {}
    else:
        alpha, quad, extra = alpha_f[:, 0].unsqueeze(0).contiguous(), None, dict(alpha_f=alpha_f)
    return dict(L=cut("L")[:, :n, :n].contiguous(), alpha=alpha, quad=quad, logdet=cut("logdet"), info=cut("info"), jitter=cut("jitter"),
                Linv_diag=cut("Linv_diag")[:, :(n + 15) // 16].contiguous(), **extra)
