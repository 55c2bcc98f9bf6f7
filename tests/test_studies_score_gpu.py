"""The batched stage 1 of the studies' acquisition optimiser on the MI355X: the value-only grouped source pass
(scaml_posterior_linv_grouped_f64 and its per-study-tasks twin), the strip scoring kernel (scaml_target_score_batched_f64), the
studies' factors in two launches (scaml_target_train_block_batched_f64 + one scaml_potrf_batched_f64), ``StudiesAcquisition.score``
and ``ScaMLGPBOStudies(score_mode="batched")``.

Stacks: T = 3, N = 32 Hartmann-6 tasks with a Matern-5/2 kernel, the golden RBF stack c1_branin_T4_N32_rbf, and one stack per study
(``meta_fit_scamlgp_studies`` over 2 studies of T = 3, N = 32, D = 2: the OWN pass).  A study's n is bounded by the stack's N.

Bounds.  BOUND = 1e-10 of max |ref| per quantity between the grouped pass (or ``score``) and the per-study path, the bound
tests/test_studies_acqf_gpu.py applies to the GRAD grouped pass; the strip kernel against ``ops.target_acqf_batched`` bit for bit (one
thread per output on both sides, no atomics); the factors under the componentwise bounds of tests/_target_bounds.py (POTRF residual
form g_{n+4} |L| |L^T|, the solve bound for alpha); rtol 1e-6 between the twins' chosen acquisition values
(tests/test_acqf_opt_gpu.py: RTOL_DRIVERS).  Every figure is printed before it is asserted (``pytest -s``);
profiles/studies_score_notes.md records them."""
import numpy as np
import pytest
import torch

from scamlgp_amd import _lib, hyper, model as M, ops, utils
from scamlgp_amd.bo import ScaMLGPBOStudies
from tests import _studies_score_problem as SP
from tests import _target_bounds as B
from tests._posterior_bounds import LD, gamma
from tests.test_acqf_opt_gpu import KW, RTOL_DRIVERS, _branin_gps, _obj
from tests.test_studies_acqf_gpu import BOUND, _afs, _hartmann_gps, _rel
from tests.test_studies_own_gpu import _study_models

pytestmark = pytest.mark.gpu
SENT = -12345.678


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


def _own_dicts(device):
    g = torch.Generator().manual_seed(5)
    studies = []
    for s in range(2):
        md = {}
        for t in range(3):
            X = torch.rand(32, 2, dtype=torch.float64, generator=g)
            md[f"task{t}"] = M.SupervisedDataset(X, torch.sin(4.0 * X.sum(-1, keepdim=True) + s + t) + 0.05 * torch.randn(32, 1, dtype=torch.float64, generator=g))
        studies.append(md)
    return M.meta_fit_scamlgp_studies(studies, num_restarts_log_likelihood=0, seed=11, device=device, fit_options=dict(driver="device", max_iter=15))


@pytest.fixture(scope="module")
def stacks(device):
    """name -> (one source dict per study, the studies' n, the target kernel); built once, never modified."""
    h, b = _hartmann_gps(device, T=3, N=32), _branin_gps(device)
    return dict(matern=([h] * 3, (1, 17, 32), hyper.MaternKernel), rbf=([b] * 3, (1, 17, 32), hyper.RBFKernel),
                own=(_own_dicts(device), (17, 32), hyper.MaternKernel))


def _fresh_models(stacks, name, seed=1):
    dicts, ns, kernel = stacks[name]
    return _study_models(dicts, ns, kernel, seed, prune=(1, 0))


def _table(models, strips, real_last, seed):
    """A candidate table: study g gets ``strips[g]`` strips, of whose last strip only ``real_last`` candidates are real (the rest
    is filler inside the box); a padding strip follows the first study's.  Returns (X (Mq, D) on the device, group per strip, rows: per
    study the indices of its real candidates, pad: the indices of the padding strip)."""
    dev, D = models[0].device, models[0]._stack.D
    g = torch.Generator().manual_seed(seed)
    group, rows, pad, o = [], [], None, 0
    for s_, c in enumerate(strips):
        group += [s_] * c
        rows.append(torch.arange(o, o + 16 * (c - 1) + real_last))
        o += 16 * c
        if s_ == 0:
            group.append(-1)
            pad = torch.arange(o, o + 16)
            o += 16
    X = torch.rand(o, D, dtype=torch.float64, generator=g)
    for s_, r in enumerate(rows):
        X[int(r[-1]) + 1:16 * ((int(r[-1]) + 16) // 16)] = 0.5
    return X.to(dev), torch.tensor(group, dtype=torch.int32, device=dev), rows, pad


@pytest.mark.parametrize("name", ["matern", "rbf", "own"])
def test_value_grouped_pass_matches_the_ungrouped_pass_per_study(stacks, name):
    models = _fresh_models(stacks, name)
    sa = utils.StudiesAcquisition(_afs(models, "ucb"))
    X, group, rows, pad = _table(models, (1, 2, 1)[:len(models)], 16, seed=2)
    src, f = sa.source, sa.source.fit
    T = sa.w.shape[1]
    cov_out = torch.full((T, sa.n_max, X.shape[0]), SENT, dtype=torch.float64, device=X.device)
    out = ops.source_posteriors_grouped(X, group, sa.Xt, sa.n_points, sa.VA_tab, src.X, src.theta, src.kind, f["Linv"], f["alpha"], src.y_mean,
                                        src.y_std, src.n_points, cov_out=cov_out, **sa._own)
    # the GRAD grouped pass at the same points: its column 0 is the same quantity
    gp = torch.repeat_interleave(group, 16)
    gg = ops.source_posteriors_grad_grouped(X, gp, sa.Xt, sa.n_points, sa.VA_tab, src.X, src.theta, src.kind, f["Linv"], f["alpha"], src.y_mean,
                                            src.y_std, src.n_points, **sa._own)
    gcov = gg["cov"].reshape(T, sa.n_max, X.shape[0], 16)
    torch.cuda.synchronize()
    for s_, m in enumerate(models):
        st, fs, n, r = m._stack, m._stack.fit, m.n, rows[s_].to(X.device)
        ref = ops.source_posteriors(torch.cat([m.train_X, X[r]]), st.X, st.theta, st.kind, fs["L"], fs["Linv_diag"], fs["alpha"], st.y_mean, st.y_std,
                                    n_points=st.n_points, cov_first=n, Linv=fs["Linv"], VA=m._train_VA())
        errs = dict(mu=_rel(out["mu"][:, r], ref["mean"][:, n:]), var=_rel(out["var"][:, r], ref["var"][:, n:]),
                    cov=_rel(out["cov"][:, :n][:, :, r], ref["cov"][:, :, n:]))
        grad = dict(mu=_rel(out["mu"][:, r], gg["mu"][:, r, 0]), var=_rel(out["var"][:, r], gg["var"][:, r, 0]),
                    cov=_rel(out["cov"][:, :n][:, :, r], gcov[:, :n][:, :, r, 0]))
        print(f"{name} study {s_} (n = {n}): against the ungrouped pass {errs}; against column 0 of the GRAD grouped pass {grad}")
        assert max(errs.values()) <= BOUND and max(grad.values()) <= BOUND, (name, s_, errs, grad)
        assert bool((cov_out[:, n:][:, :, r] == SENT).all()), "rows a >= n_g of a strip must stay untouched"
        assert bool((cov_out[:, :n][:, :, r] != SENT).all())
    pad = pad.to(X.device)
    assert not bool(out["mu"][:, pad].any()) and not bool(out["var"][:, pad].any())          # a padding strip: zeros,
    assert bool((cov_out[:, :, pad] == SENT).all())                                            # and no row of cov written


@pytest.mark.parametrize("T, D", [(9, 6), (3, 2)])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("acqf", [0, 1])
def test_strip_kernel_equals_the_batched_acquisition_bit_for_bit(device, T, D, kind, acqf):
    """n = 1, 15, 16, 17, 33 and a failed study, one and three strips per study, a padding strip, a pruned task holding NaN, NaN past
    every n, one candidate with a NaN coordinate (tests/_studies_score_problem.py): the same device inputs in both layouts."""
    prob = SP.Problem(T, D, kind, seed=500 + T + D + kind, strips=(1, 3, 1, 3, 3, 1))
    dt = dict(group=torch.int32, n_points=torch.int32, info=torch.int32, active=torch.uint8)
    up = lambda a: [torch.from_numpy(a[k]).to(device=device, dtype=dt.get(k, torch.float64)) for k in SP.ORDER]   # noqa: E731
    strip = ops.target_score_batched(*up(prob.arrays(acqf, "value")), acqf, kind, want_posterior=True)
    query = ops.target_acqf_batched(*up(prob.arrays(acqf, "grad")), acqf, kind, want_grad=False, want_posterior=True)
    torch.cuda.synchronize()
    for k in ("value", "mu", "var"):
        a, b = strip[k].cpu().numpy(), query[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), (k, int((a != b).sum()))
    val = strip["value"].cpu().numpy()
    studies = np.repeat(prob.group, 16)
    assert not val[studies < 0].any() and np.isnan(val[studies == SP.FAILED]).all() and np.isnan(val[prob.nan_q])
    live = (studies >= 0) & (studies != SP.FAILED) & (np.arange(prob.Mq) != prob.nan_q)
    assert np.isfinite(val[live]).all()
    for q in np.nonzero(live)[0][::7]:
        np.testing.assert_allclose(val[q], prob.reference(acqf, int(q))[0], rtol=1e-9)


def _with_duplicates(m):
    """A model on m's source dict whose second half of the training inputs repeats the first, with a slightly NEGATIVE noise in its
    cached theta (tests/_failpath_cases.py: duplicate_stack): Knn fails at jitter 0 and 1e-8 and factors at 1e-7, whatever the kernel."""
    X = m.train_X.clone()
    n = X.shape[0]
    X[n // 2:] = X[:n - n // 2]
    d = M.ScaMLGP(X.cpu(), m.train_Y.cpu(), m.source_gps, covar_module=hyper.get_default_kernel(hyper.MaternKernel, X.shape[1]))
    d.weights = m.weights.clone()
    d.raw_theta = m.raw_theta.clone()
    th = d.theta.clone()
    th[-1] = -5e-8
    d._cache.put("theta", d._param_tensors(), th)
    assert float(d.theta[-1]) == -5e-8
    return d.eval()


@pytest.mark.parametrize("name", ["matern", "own"])
def test_batched_factors_agree_with_each_models_own(stacks, name):
    def build():
        ms = _fresh_models(stacks, name, seed=3)
        return ms + [_with_duplicates(ms[-1])]

    own, bat = build(), build()
    for m in own:                                    # the model's own factor, through posterior
        m.posterior(m.train_X[:1])
    assert all(m._target_factor() is None for m in bat)
    taken, fall = utils.StudiesAcquisition._factors_batched(bat)
    torch.cuda.synchronize()
    assert taken == bat
    for i, (mo, mb) in enumerate(zip(own, bat)):
        fo, fb = mo._target_factor(), mb._target_factor()
        assert fb is not None and fb["L"].shape == fo["L"].shape and fb["Linv_diag"].shape == fo["Linv_diag"].shape
        n = mo.n
        info_o, info_b, jit_o, jit_b = int(fo["info"][0]), int(fb["info"][0]), float(fo["jitter"][0]), float(fb["jitter"][0])
        print(f"{name} model {i} (n = {n}): info {info_b} / {info_o}, jitter {jit_b} / {jit_o}")
        assert info_b == info_o == 0 and jit_b == jit_o
        assert jit_o == (1e-7 if i == len(own) - 1 else 0.0)
        # Knn as the model's own path assembles it, from its own weighted sums
        mu_t, cov_tt, var_t = mo._train_prior()
        Knn, resid = torch.empty(n, n, dtype=torch.float64, device=mo.device), torch.empty(n, dtype=torch.float64, device=mo.device)
        _lib.check_rc(_lib.lib.scaml_target_assemble_f64(cov_tt.data_ptr(), mu_t.data_ptr(), var_t.data_ptr(), mo.train_X.data_ptr(), mo.theta.data_ptr(),
                                                         mo.train_targets.data_ptr(), mo._m_all_f, mo._s_all_f, n, 0, mo._stack.D, mo.kind, Knn.data_ptr(),
                                                         resid.data_ptr(), None, None, None, torch.cuda.current_stream().cuda_stream), "assemble")
        # the batched assemble: Knn exactly the single assemble's (the factorisation reads the lower triangle; the upper one mirrors it),
        # resid up to the scatter of the source means it is built from (1e-11 of max |resid|: tests/test_studies_acqf_gpu.py SCATTER_MAX)
        Kb = fall["Knn"][i, :n, :n]
        d_knn, d_res = _rel(torch.tril(Kb), torch.tril(Knn)), _rel(fall["resid"][i, :n], resid)
        print(f"   batched assemble against the single one: Knn {d_knn:.3e} (must be 0), resid {d_res:.3e}")
        assert torch.equal(torch.tril(Kb), torch.tril(Knn)) and torch.equal(Kb, Kb.T) and d_res <= 1e-11
        Lb, Lo = fb["L"][0].cpu().numpy(), fo["L"][0].cpu().numpy()
        for tag, L_ in (("batched", Lb), ("own", Lo)):
            LLt, q = B.potrf_reference(L_, Knn.cpu().numpy(), jit_o)
            err = np.abs(LLt - q.ref)
            print(f"   {tag} L L^T against Knn + jitter I: largest error / bound {float((err / np.maximum(q.bound, 1e-300)).max()):.3e}")
            assert bool((err <= q.bound).all()), (name, i, tag)
        # L L^T against the model's L L^T: each within its residual bound of the same matrix
        Pb, Po = LD(np.tril(Lb)) @ LD(np.tril(Lb)).T, LD(np.tril(Lo)) @ LD(np.tril(Lo)).T
        bound = gamma(n + 4) * (np.abs(np.tril(Lb)) @ np.abs(np.tril(Lb)).T + np.abs(np.tril(Lo)) @ np.abs(np.tril(Lo)).T)
        print(f"   L L^T batched against own: largest difference / bound {float((np.abs(Pb - Po) / np.maximum(bound, 1e-300)).max()):.3e}")
        assert bool((np.abs(Pb - Po) <= bound).all())
        # alpha: each under the solve bound of its own factor and right-hand side; the two right-hand sides differ by the scatter of
        # the source means (LDS float atomics), the two references by the perturbation of the factor
        ab, ao = fb["alpha"][0].cpu().numpy(), fo["alpha"][0].cpu().numpy()
        qo = B.solve_reference(Lo, resid.cpu().numpy()[:, None], n)
        assert bool((np.abs(LD(ao[:, None]) - qo.ref) <= qo.bound).all())
        Li = B.inverse_lower(np.tril(Lo))
        Kinv = np.abs((Li.T @ Li).astype(np.float64))
        pert = Kinv @ (2.0 * float(gamma(n + 4)) * (np.abs(np.tril(Lo)) @ np.abs(np.tril(Lo)).T) @ np.abs(ao) + 1e-11 * np.abs(resid.cpu().numpy()).max())
        bound_a = 2.0 * qo.bound[:, 0].astype(np.float64) + pert
        print(f"   alpha batched against own: largest difference / bound {float((np.abs(ab - ao) / np.maximum(bound_a, 1e-300)).max()):.3e}, "
              f"relative {float(np.abs(ab - ao).max() / np.abs(ao).max()):.3e}")
        assert bool((np.abs(ab - ao) <= bound_a).all())


@pytest.mark.parametrize("name", ["matern", "rbf", "own"])
@pytest.mark.parametrize("which", ["ucb", "ei"])
def test_score_matches_every_studys_own_acquisition(stacks, name, which):
    """48 candidates per study, 40 real and 8 filler, plus a padding strip: ``StudiesAcquisition.score`` (factors batched) against each
    study's ``af(cand)``."""
    models = _fresh_models(stacks, name, seed=4)
    afs = _afs(models, which)
    sa = utils.StudiesAcquisition(afs, batched_factors=True)
    X, group, rows, pad = _table(models, (3,) * len(models), 8, seed=6)
    out = sa.score(X, group, want_posterior=True)
    torch.cuda.synchronize()
    models = _fresh_models(stacks, name, seed=4)      # the reference: the same models again, with factors of their own
    afs = _afs(models, which)
    for s_, (af, m) in enumerate(zip(afs, models)):
        r = rows[s_].to(X.device)
        assert r.numel() == 40
        post = m.posterior(X[r])
        errs = dict(value=_rel(out["value"][r], af(X[r])), mu=_rel(out["mu"][r], post.mean.reshape(-1)), var=_rel(out["var"][r], post.variance.reshape(-1)))
        print(f"{name} {which} study {s_} (n = {m.n}): score against the study's own path {errs}")
        assert max(errs.values()) <= BOUND, (name, which, s_, errs)
    assert not bool(out["value"][pad.to(X.device)].any())


def test_score_chunks_under_its_workspace_cap(stacks, monkeypatch):
    models = _fresh_models(stacks, "rbf", seed=4)
    sa = utils.StudiesAcquisition(_afs(models, "ucb"), batched_factors=True)
    X, group, rows, pad = _table(models, (3, 3, 3), 16, seed=8)
    whole = sa.score(X, group)["value"]
    calls = []
    plain = ops.target_score_batched
    monkeypatch.setattr(ops, "target_score_batched", lambda *a, **k: (calls.append(a[0].shape[1]), plain(*a, **k))[1])
    monkeypatch.setattr(utils.StudiesAcquisition, "SCORE_COV_CAP_BYTES", 4 * sa.w.shape[1] * sa.n_max * 16 * 8)   # four strips per chunk
    parts = sa.score(X, group)["value"]
    assert calls == [64, 64, 32] and _rel(parts, whole) <= BOUND


def test_batched_score_mode_next_to_a_per_study_twin(device, monkeypatch):
    """Two ``ScaMLGPBOStudies(suggest_mode="device")`` that differ only in ``score_mode``, same seeds, same reported data: S = 3,
    2 steps, raw_samples = 64, num_restarts = 4, study 0 starts without data.  The picked candidate indices are what
    ``bo.acqf_pick_initial_conditions`` returns on either side (every call of a ``suggest`` is recorded, the fall-back study's too)."""
    from scamlgp_amd import bo

    picked = []
    pick = bo.acqf_pick_initial_conditions
    monkeypatch.setattr(bo, "acqf_pick_initial_conditions", lambda *a, **k: (lambda r: (picked.append(r), r)[1])(pick(*a, **k)))
    gps = _branin_gps(device)
    S, DIM, seeds = 3, 2, [31, 32, 33]
    bat = ScaMLGPBOStudies(gps, DIM, S, seeds=seeds, suggest_mode="device", score_mode="batched", **KW)
    twin = ScaMLGPBOStudies(gps, DIM, S, seeds=seeds, suggest_mode="device", score_mode="per_study", **KW)
    g = torch.Generator().manual_seed(0)
    init = {s: torch.rand(2 + 3 * s, DIM, dtype=torch.float64, generator=g) for s in (1, 2)}
    for side in (bat, twin):
        side.report_some({s: (x, [_obj(r) for r in x]) for s, x in init.items()})
    for step in range(2):
        picked.clear()
        Xb = bat.suggest()
        picks_b = list(picked)
        picked.clear()
        Xt = twin.suggest()
        picks_t = list(picked)
        ib, it = bat.last_suggest_info, twin.last_suggest_info
        assert ib["score_mode"] == "batched" and it["score_mode"] == "per_study"
        assert ib["batched"] == it["batched"] == ([1, 2] if step == 0 else [0, 1, 2])
        # (study 0 is the only fall-back and comes first on either side, so the calls line up study by study)
        assert len(picks_b) == S and picks_b == picks_t, (step, picks_b, picks_t)
        assert set(it) - {"score_mode"} == {"batched", "n_eval", "n_iter", "n_calls", "evals_per_start", "status"} and set(ib) == set(it)
        for s in range(S):
            assert torch.equal(bat[s].gen.get_state(), twin[s].gen.get_state()), (step, s)
            if s not in ib["batched"]:
                continue
            af = twin[s].acquisition_function()
            v = af(torch.stack([Xb[s], Xt[s]]).to(device)).cpu()
            print(f"step {step} study {s}: chosen value, batched {float(v[0]):.12f}, per study {float(v[1]):.12f}")
            assert abs(float(v[0]) - float(v[1])) <= RTOL_DRIVERS * max(abs(float(v[0])), abs(float(v[1])))
        ys = [_obj(x) for x in Xt]
        bat.report(Xt, ys)
        twin.report(Xt, ys)
