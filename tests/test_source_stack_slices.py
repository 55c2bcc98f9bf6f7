"""``SourceGPStack.slice`` and ``meta_fit_scamlgp_studies``: what needs no launch runs on the CPU (views, the slice's own targets, the
refusals); the fit of S stacks as one and the batched refit on per-study stacks are marked ``gpu``."""
import numpy as np
import pytest
import torch

from scamlgp_amd import model as M, utils

CPU = torch.device("cpu")


def _parent(ns=(5, 3, 5, 1, 4, 5), D=2, seed=0, device=CPU):
    g = torch.Generator().manual_seed(seed)
    X = [torch.rand(n, D, dtype=torch.float64, generator=g) for n in ns]
    Y = [3.0 * t + torch.randn(n, 1, dtype=torch.float64, generator=g) for t, n in enumerate(ns)]
    return M.SourceGPStack([f"t{t}" for t in range(len(ns))], X, Y, device=device), X, Y


def _fake_fit(st):
    T, N = st.T, st.N
    z = lambda *s: torch.arange(int(np.prod(s)), dtype=torch.float64).reshape(s)   # noqa: E731
    return dict(L=z(T, N, N), alpha=z(T, N), Linv=z(T, N, N), Linv_diag=z(T, (N + 15) // 16, 16, 16), info=torch.zeros(T, dtype=torch.int32), note="kept")


def _same_storage(view, parent, lo):
    return view.data_ptr() == parent[lo:].data_ptr() and view.untyped_storage().data_ptr() == parent.untyped_storage().data_ptr()


def test_slice_tensors_share_storage_with_the_parent():
    st, _, _ = _parent()
    st._fit = _fake_fit(st)
    sl = st.slice(2, 5)
    assert isinstance(sl, M.SourceGPStack) and sl.parent is st and (sl.lo, sl.hi) == (2, 5)
    assert sl.T == 3 and sl.N == st.N == 5 and sl.D == st.D and sl.kind == st.kind and sl.spec is st.spec
    for name in ("X", "y", "y_mean", "y_std", "n_float", "raw", "n_points"):
        v, p = getattr(sl, name), getattr(st, name)
        assert v.shape == (3,) + tuple(p.shape[1:]) and _same_storage(v, p, 2), name
        assert v.is_contiguous(), name
    f = sl.fit
    for k, p in st.fit.items():
        if isinstance(p, torch.Tensor):
            assert f[k].shape == (3,) + tuple(p.shape[1:]) and _same_storage(f[k], p, 2), k
    assert f["note"] == "kept" and sl.fit is f                     # (one narrowed twin per parent fit)
    # (the CPU's vectorised sigmoid may differ from its scalar tail in the last bit: the same raw values at other offsets)
    torch.testing.assert_close(sl.theta, st.theta[2:5], rtol=1e-14, atol=0)
    # the parent refitted: the slice follows
    st.set_theta(st.theta * 1.5)
    assert _same_storage(sl.raw, st.raw, 2)
    torch.testing.assert_close(sl.theta, st.theta[2:5], rtol=1e-14, atol=0)
    st._fit = _fake_fit(st)
    assert sl.fit is not f and _same_storage(sl.fit["Linv"], st.fit["Linv"], 2)


def test_slice_own_bookkeeping():
    st, X, Y = _parent()
    sl = st.slice(2, 5)                                             # tasks of 5, 1, 4 points
    assert sl.task_ids == ["t2", "t3", "t4"] and sl.n_list == [5, 1, 4]
    assert sl.n_points is not None and sl.n_points.tolist() == [5, 1, 4]
    full = st.slice(0, 1)                                           # its one task fills the parent's N: no count table
    assert full.n_points is None and not full.ragged and full.N == 5
    even, _, _ = _parent(ns=(4, 4, 4, 4))
    assert even.n_points is None and even.slice(1, 3).n_points is None
    # raw_targets: the slice's own tasks' observations, in original units, and nothing else
    want = torch.cat([Y[t] for t in (2, 3, 4)])
    got = sl.raw_targets()
    assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-12)
    assert st.raw_targets().shape[0] == 23 and got.shape[0] == 10
    gp = M.SourceGP(sl, 1)
    assert gp.train_targets.shape == (1,) and gp.train_inputs[0].shape == (1, 2)


def test_a_slice_does_not_own_hyper_parameters_or_factors():
    st, _, _ = _parent()
    sl = st.slice(0, 2)
    with pytest.raises(RuntimeError, match="parent"):
        sl.set_theta(sl.theta)
    with pytest.raises(RuntimeError, match="parent"):
        sl.refresh()
    with pytest.raises(RuntimeError, match="parent"):
        utils.optimize_marginal_likelihood(sl, num_restarts=0, driver="device")
    with pytest.raises(TypeError):
        sl.slice(0, 1)
    for lo, hi in ((-1, 2), (2, 2), (3, 2), (0, 7)):
        with pytest.raises(ValueError):
            st.slice(lo, hi)


def _meta(T, D, n=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {f"m{t}": M.SupervisedDataset(torch.rand(n, D, dtype=torch.float64, generator=g), torch.randn(n, 1, dtype=torch.float64, generator=g))
            for t in range(T)}


def test_meta_fit_studies_refusals():
    with pytest.raises(ValueError, match="equal number of tasks"):
        M.meta_fit_scamlgp_studies([_meta(2, 3), _meta(3, 3)], device=CPU)
    with pytest.raises(ValueError, match="input dimension"):
        M.meta_fit_scamlgp_studies([_meta(2, 3), _meta(2, 4)], device=CPU)
    with pytest.raises(NotImplementedError, match="shard"):
        M.meta_fit_scamlgp_studies([_meta(2, 3), _meta(2, 3)], device=CPU, shard=True)
    with pytest.raises(ValueError, match="at least one"):
        M.meta_fit_scamlgp_studies([], device=CPU)
    with pytest.raises(ValueError, match="Empty meta data"):
        M.meta_fit_scamlgp_studies([_meta(2, 3), {}], device=CPU)
    bad = _meta(2, 3)
    bad["m1"] = M.SupervisedDataset(torch.rand(4, 3, dtype=torch.float64), torch.rand(4, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="output dimension"):
        M.meta_fit_scamlgp_studies([_meta(2, 3), bad], device=CPU)


def test_studies_take_one_dict_per_study_or_raise():
    from scamlgp_amd.bo import ScaMLGPBOStudies

    st, _, _ = _parent(ns=(4, 4, 4, 4))
    dicts = [{tid: M.SourceGP(sl, i) for i, tid in enumerate(sl.task_ids)} for sl in (st.slice(0, 2), st.slice(2, 4))]
    for n in (1, 3):
        with pytest.raises(ValueError, match="source stacks"):
            ScaMLGPBOStudies(dicts, dim=2, num_studies=n)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_meta_fit_studies_is_the_fit_of_one_large_stack():
    """S = 3 studies x T = 2 tasks (N = 24, D = 2, one task shorter) through ``meta_fit_scamlgp_studies`` and through ``meta_fit_scamlgp`` on
    the 6 tasks as one dict, same seed, device driver: the same stack, the same optimiser call -- equal hyper-parameters bit for bit;
    the returned dicts are slices [2 s, 2 s + 2) with the studies' own task ids."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    studies = []
    for s in range(3):
        md = {}
        for t in range(2):
            n = 24 if (s, t) != (1, 1) else 17
            X = torch.rand(n, 2, dtype=torch.float64, generator=g)
            md[f"task{t}"] = M.SupervisedDataset(X, torch.sin(4.0 * X.sum(-1, keepdim=True) + s) + 0.05 * torch.randn(n, 1, dtype=torch.float64, generator=g))
        studies.append(md)
    opts = dict(num_restarts_log_likelihood=1, seed=11, device=dev, fit_options=dict(driver="device", max_iter=15))
    per_study = M.meta_fit_scamlgp_studies(studies, **opts)
    flat = M.meta_fit_scamlgp({(s, tid): d for s, md in enumerate(studies) for tid, d in md.items()}, **opts)
    big = next(iter(flat.values()))._stack
    assert len(per_study) == 3
    parent = next(iter(per_study[0].values()))._stack.parent
    assert parent.T == 6 and torch.equal(parent.raw, big.raw) and torch.equal(parent.X, big.X)
    for s, gps in enumerate(per_study):
        assert list(gps) == ["task0", "task1"]
        sl = next(iter(gps.values()))._stack
        assert sl.parent is parent and (sl.lo, sl.hi) == (2 * s, 2 * s + 2) and [gp._index for gp in gps.values()] == [0, 1]
        assert (sl.n_points is not None) == (s == 1)
        m = M.ScaMLGP(torch.rand(3, 2, dtype=torch.float64, generator=g), torch.rand(3, 1, dtype=torch.float64, generator=g), gps)
        assert m.T == 2 and m.source_means.shape == (3, 2)


@pytest.mark.gpu
def test_batched_refit_takes_models_on_per_study_stacks():
    """``fit_targets_batched`` on three models, each on its own slice, against ``optimize_marginal_likelihood`` on twins of them one
    after the other with the same generators: the kernel runs the single call's instruction sequence per problem, so the fitted
    states are equal bit for bit (tests/test_studies_gpu.py holds the shared-stack case to the same)."""
    dev = torch.device("cuda:0")
    st, _, _ = _parent(ns=(20, 20, 20, 13, 20, 20), D=2, seed=3, device=dev)
    st.refresh()
    dicts = [{tid: M.SourceGP(sl, i) for i, tid in enumerate(sl.task_ids)} for sl in (st.slice(0, 2), st.slice(2, 4), st.slice(4, 6))]
    g = torch.Generator().manual_seed(4)
    data = [(torch.rand(n, 2, dtype=torch.float64, generator=g), torch.randn(n, 1, dtype=torch.float64, generator=g)) for n in (3, 7, 5)]
    batch = [M.ScaMLGP(x, y, d) for (x, y), d in zip(data, dicts)]
    single = [M.ScaMLGP(x, y, d) for (x, y), d in zip(data, dicts)]
    utils.fit_targets_batched(batch, 2, maxiter=30, rng=[torch.Generator().manual_seed(7 + i) for i in range(3)])
    for i, m in enumerate(single):
        with utils._rng_of(torch.Generator().manual_seed(7 + i)):
            utils.optimize_marginal_likelihood(m, 2, maxiter=30)
    for b, m in zip(batch, single):
        assert torch.equal(b.raw_theta, m.raw_theta) and torch.equal(b.raw_weights, m.raw_weights)
