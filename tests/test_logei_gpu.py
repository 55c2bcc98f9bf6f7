"""LogEI (acquisition code 17) on the MI355X: the elementwise transform (7o) on the whole 50-digit table inside the a-priori bounds of
tests/_logei_bounds.py; the fantasy kernel (7f) against that module's long-double reference fed the entry point's own arrays, every
element inside its counted first-order bound (tests/_logei_bounds.fantasy_reference); the studies' batched evaluation against each
study's own path (tests/test_studies_acqf_gpu.py's bound) with the bit-for-bit identities of the existing codes; the behaviour the feature is for -- where EI and its
gradient are exactly 0, LogEI has a slope and the device optimiser moves --; and the BO loops with acquisition="logei"."""
import math

import numpy as np
import pytest
import torch

from scamlgp_amd import _lib, hyper, model as M, ops, utils
from scamlgp_amd.bo import ScaMLGPBOStudies
from tests import _fantasy_bounds as FB
from tests import _logei_bounds as LB
from tests._posterior_bounds import LD
from tests.test_acqf_opt_gpu import KW, _branin_gps, _obj
from tests.test_studies_acqf_gpu import BOUND, _hartmann_gps, _models, _rel

pytestmark = pytest.mark.gpu
LOGEI = ops.ACQF_LOGEI


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


def test_codes():
    assert (ops.ACQF_UCB, ops.ACQF_EI, ops.ACQF_LOGEI) == (0, 1, 17)


@pytest.mark.parametrize("v", [0.37, 1e-9, 5e-10, 0.0, -0.01], ids=["above", "on", "tiny", "zero", "negative"])
def test_transform_on_the_table(device, v):
    t = LB.table()
    par = 0.25
    mu = par - t["u"] * math.sqrt(max(v, 1e-9))   # the whole table, u = -1e8 included
    A, Amu, Av = ops.acqf_transform(torch.from_numpy(mu).to(device), torch.full((mu.size,), v, dtype=torch.float64, device=device), LOGEI, par)
    r = LB.transform(par, mu, v)
    for name, got in (("A", A), ("Amu", Amu), ("Av", Av)):
        got = got.cpu().numpy()
        err, bound = np.abs(LD(got) - r[name]), r["E_" + name]
        print(f"v = {v}: {name} error / bound {float((err / np.where(bound > 0, bound, 1)).max()):.3f}")
        assert np.isfinite(got).all() and (err <= bound).all(), name
    assert bool((Av == 0.0).all()) == (v <= 1e-9)
    A1, none1, none2 = ops.acqf_transform(torch.from_numpy(mu).to(device), torch.full((mu.size,), v, dtype=torch.float64, device=device), LOGEI, par,
                                          want_factors=False)
    assert none1 is None and none2 is None and torch.equal(A1, A)


def test_transform_ucb_ei_nan_and_refusals(device):
    mu = torch.tensor([0.3, -0.2, float("nan"), 5.0], dtype=torch.float64, device=device)
    var = torch.tensor([0.5, 2.0, 1.0, 1e-12], dtype=torch.float64, device=device)
    A, Amu, Av = ops.acqf_transform(mu, var, ops.ACQF_UCB, 9.0)
    assert torch.allclose(A[:2], torch.sqrt(9.0 * var[:2]) - mu[:2], rtol=1e-15) and bool((Amu == -1.0).all())
    A, Amu, Av = ops.acqf_transform(mu, var, ops.ACQF_EI, 0.1)
    assert float(Av[3]) == 0.0 and float(A[3]) == 0.0 and float(A[0]) > 0
    A, Amu, Av = ops.acqf_transform(mu, var, LOGEI, 0.1)
    assert bool(torch.isnan(A[2])) and bool(torch.isfinite(A[[0, 1, 3]]).all()) and float(Av[3]) == 0.0
    out = torch.full((4,), 7.0, dtype=torch.float64, device=device)
    for code in (0x10, 0x12, 2, 3, -1):
        rc = _lib.lib.scaml_acqf_transform_f64(mu.data_ptr(), var.data_ptr(), 0.1, 4, code, out.data_ptr(), None, None, None)
        assert rc == _lib.E_BADARG
    assert _lib.lib.scaml_acqf_transform_f64(None, None, 0.1, 0, LOGEI, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- (7f) --------------------------------------------------------------------------------------------------------------------
def _call(a, device, code, info=None):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)   # noqa: E731
    n, M, D = a["n"], a["M"], a["D"]
    gi = dict(cov_g=t(a["cov_g"]), mu_g=t(a["mu_g"]), var_g=t(a["var_g"]), Xt=t(a["Xt"]), Xq=t(a["Xq"]), theta=t(a["theta"]))
    inf = None if info is None else torch.tensor([info], dtype=torch.int32, device=device)
    v, g = ops.target_fantasy_acqf(t(a["Knq"]), t(a["Z"]), t(a["alpha"]), t(a["mean_q"]), t(a["var_q"]), a["m"], a["s"], inf, code, a["param"],
                                   noise_add=a["noise_add"], grad_inputs=gi, kind=a["kind"])
    return v.cpu(), g.cpu()


def _hold(label, a, ref, value, grad, gmask=None):
    LB.hold(label, a, ref, value.numpy(), grad.numpy(), gmask)
    for name, got in (("value", value), ("grad", grad)):
        q = ref[name]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(q.bound > 0, np.abs(LD(got.numpy()) - q.ref) / np.where(q.bound > 0, q.bound, 1), 0)
        print(f"{label} {name}: largest error / bound {float(np.nanmax(r)):.3f}, largest bound / scale {float(np.nanmax(q.bound) / q.scale):.2e}")


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (8, 63, 3, 6), (65, 63, 130, 6), (96, 64, 3, 15)], ids=str)
def test_fantasy_kernel(device, shape, kind):
    a = FB.inputs(*shape, kind, FB.EI)
    ref = LB.fantasy_reference(a)
    for info in (None, 0):
        value, grad = _call(a, device, LOGEI, info)
        _hold(f"{shape} kind {kind} info {info}", a, ref, value, grad)
    value, grad = _call(a, device, LOGEI, 2)
    assert bool(torch.isnan(value).all()) and bool(torch.isnan(grad).all())


@pytest.mark.parametrize("kind", [0, 1])
def test_fantasy_kernel_where_ei_is_dead(device, kind):
    """Every u_f <= -40: the library's EI and its gradient are exactly 0; LogEI is finite with a non-zero gradient, inside its bound."""
    a = FB.tail_inputs("deep", kind)
    ref = LB.fantasy_reference(a)
    assert float(ref["u"].max()) <= -40.0
    v_ei, g_ei = _call(a, device, ops.ACQF_EI)
    assert not bool(v_ei.any()) and not bool(g_ei.any())
    value, grad = _call(a, device, LOGEI)
    _hold(f"deep tail kind {kind}", a, ref, value, grad)
    assert bool((grad.abs().max(1).values > 0).all()) and float(value.max()) < -700.0


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("mode", ["neg", "tiny", "zero"])
def test_fantasy_kernel_clamp(device, mode, kind):
    """On the 1e-9 floor the partial d A / d v is exactly absent: the clamped queries' gradient does not move by a bit with var_g."""
    a = FB.clamp_inputs(mode, FB.EI, kind)
    ref = LB.fantasy_reference(a)
    assert (ref["v"][list(FB.CLAMPED_Q)] <= 1e-9).all()
    value, g1 = _call(a, device, LOGEI)
    _hold(f"clamp {mode} kind {kind}", a, ref, value, g1)
    _, g2 = _call(dict(a, var_g=3.0 * a["var_g"] + 1.0), device, LOGEI)
    q = list(FB.CLAMPED_Q)
    assert torch.equal(g1[q], g2[q]) and bool((g1[1] != g2[1]).all())


def test_fantasy_kernel_nonfinite_query(device):
    a = FB.nonfinite_inputs((8, 63, 3, 6), 1, FB.EI, float("nan"))
    clean = FB.inputs(8, 63, 3, 6, 1, FB.EI)
    value, grad = _call(a, device, LOGEI)
    v0, g0 = _call(clean, device, LOGEI)
    gmask = np.zeros((a["M"], a["D"]), dtype=bool)
    gmask[-1] = True
    _hold("non-finite query", a, LB.fantasy_reference(clean), value, grad, gmask)
    assert bool(torch.isnan(grad[-1]).all()) and torch.equal(grad[:-1], g0[:-1]) and torch.equal(value[:-1], v0[:-1])


# ---- the studies' batched evaluation (7g) / (7i) / (7k) and the optimiser ---------------------------------------------------------
def _logei_afs(models, shift=0.05):
    return [utils.LogExpectedImprovement(m, float(m.train_Y.min()) - shift * i) for i, m in enumerate(models)]


def test_batched_evaluation_matches_each_study(device):
    """G = 3 studies, n = (1, 17, 40): the batched evaluation with code 17 against each study's own LogExpectedImprovement
    ((5d) + (7o)), tests/test_studies_acqf_gpu.py's bound; the strip scoring (7i) gives (7g)'s values bit for bit."""
    models = _models(_hartmann_gps(device), (1, 17, 40), hyper.MaternKernel, seed=11)
    counts = (4, 3, 2)
    g = torch.Generator().manual_seed(12)
    Xs = [torch.rand(c, 6, dtype=torch.float64, generator=g).to(device) for c in counts]
    afs = _logei_afs(models)
    sa = utils.StudiesAcquisition(afs)
    assert sa.acqf == LOGEI
    out = sa.evaluate(torch.cat(Xs), sa.group_of(counts))
    torch.cuda.synchronize()
    for k in ("value", "grad"):
        for s, (af, x, chunk) in enumerate(zip(afs, Xs, out[k].split(list(counts)))):
            v, gr = af.value_and_grad(x)
            err = _rel(chunk, v if k == "value" else gr)
            print(f"study {s} (n = {models[s].n}) {k}: {err:.3e}")
            assert err <= BOUND
            assert _rel(af(x), v) <= BOUND
    with pytest.raises(TypeError):
        utils.StudiesAcquisition([afs[0], utils.ExpectedImprovement(models[1], 0.0)])


def test_fantasy_studies_match_each_study(device):
    """(7k): studies of F = 1 (ordinary), 2 and 64 fantasies in one launch against each study's own (7f) path."""
    models = _models(_hartmann_gps(device), (5, 14, 16), hyper.MaternKernel, seed=21)
    g = torch.Generator().manual_seed(22)
    pend = [None, torch.rand(3, 6, dtype=torch.float64, generator=g), torch.rand(1, 6, dtype=torch.float64, generator=g)]
    fant = [m if p is None else m.fantasize(p, F, generator=torch.Generator().manual_seed(23 + F))
            for m, p, F in zip(models, pend, (1, 2, 64))]
    afs = _logei_afs(fant)
    counts = (2, 3, 2)
    Xs = [torch.rand(c, 6, dtype=torch.float64, generator=g).to(device) for c in counts]
    sa = utils.StudiesAcquisition(afs)
    assert sa.fantasy
    out = sa.evaluate(torch.cat(Xs), sa.group_of(counts))
    plain = utils.StudiesAcquisition(afs[:1]).evaluate(Xs[0], torch.zeros(counts[0], dtype=torch.int32, device=device))
    torch.cuda.synchronize()
    for k in ("value", "grad"):
        chunks = out[k].split(list(counts))
        for s, (af, x) in enumerate(zip(afs, Xs)):
            v, gr = af.value_and_grad(x)
            err = _rel(chunks[s], v if k == "value" else gr)
            print(f"study {s} (F = {fant[s].num_fantasies}) {k}: {err:.3e}")
            assert err <= BOUND
        assert _rel(chunks[0], plain[k]) <= 1e-11    # the F = 1 study next to (7g): the source pass's scatter only


# ---- (7k) at F = 1 / 2 / 64 with n' = 1 / 17 / 96: each study's own path, the identities on one source pass, non-finite queries ------
MIX = ((1, 0, None), (14, 3, 2), (92, 4, 64))   # (n, pending points, fantasies): n' = 1, 17, 96


@pytest.fixture(scope="module")
def case(device):
    base = _models(_hartmann_gps(device, T=2, N=96), [n for n, _, _ in MIX], hyper.RBFKernel, seed=42, prune=(1, 0))
    assert all(bool(torch.isfinite(m.theta).all()) for m in base)
    g = torch.Generator().manual_seed(42)
    D = base[0]._stack.D
    models = [m if not p else m.fantasize(torch.rand(p, D, dtype=torch.float64, generator=g), F, generator=g).eval() for m, (n, p, F) in zip(base, MIX)]
    afs = [utils.LogExpectedImprovement(m, float(m.train_Y.min()) - 0.05 * i) for i, m in enumerate(models)]
    G = len(models)
    sa = utils.StudiesAcquisition(afs)
    assert sa.fantasy and sa.acqf == ops.ACQF_LOGEI and sa.n_fant.tolist() == [1, 2, 64] and sa.n_points.tolist() == [1, 17, 96]
    X = torch.rand(16 * G, D, dtype=torch.float64, generator=g).to(device)   # a strip of 16 per study
    group = sa.group_of([16] * G)
    st, f = sa.source, sa.source.fit
    src = ops.source_posteriors_grad_grouped(X, group, sa.Xt, sa.n_points, sa.VA_tab, st.X, st.theta, st.kind, f["Linv"], f["alpha"], st.y_mean,
                                             st.y_std, st.n_points)
    return dict(afs=afs, sa=sa, X=X, group=group, src=src, G=G, D=D)


def _fantasy_launch(c, X):
    sa, src = c["sa"], c["src"]
    return ops.target_fantasy_acqf_batched(src["mu"], src["var"], src["cov"], c["group"], X, sa.w, sa.active, sa.Xt, sa.theta, sa.L, sa.Linv_diag,
                                           sa.alpha_f, sa.n_fant, sa.n_points, sa.m_all, sa.s_all, sa.info, sa.acqf_param, sa.acqf, sa.kind)


def test_each_study_against_its_own_path(case):
    out = case["sa"].evaluate(case["X"], case["group"])
    torch.cuda.synchronize()
    for k in ("value", "grad"):
        for s, (af, x, chunk) in enumerate(zip(case["afs"], case["X"].split(16), out[k].split(16))):
            v, gr = af.value_and_grad(x)
            err = _rel(chunk, v if k == "value" else gr)
            print(f"study {s} (n' = {af.model.n}, F = {af.model.num_fantasies}) {k}: {err:.3e}")
            assert bool(torch.isfinite(chunk).all()) and err <= BOUND


def test_identities_on_one_source_pass(case, device):
    sa, src, X, G = case["sa"], case["src"], case["X"], case["G"]
    mixed = _fantasy_launch(case, X)
    assert bool(torch.isfinite(mixed["value"]).all()) and bool(torch.isfinite(mixed["grad"]).all())
    # the F = 1 study's rows of the same pass under (7g), with the arrays of the study alone
    sa1 = utils.StudiesAcquisition(case["afs"][:1])
    assert not sa1.fantasy and sa1.acqf == ops.ACQF_LOGEI
    T, nm = sa.w.shape[1], sa1.n_max
    cov = src["cov"].reshape(T, sa.n_max, 16 * G, 16)[:, :nm, :16].reshape(T, nm, -1).contiguous()
    tail1 = (sa1.w, sa1.active, sa1.Xt, sa1.theta, sa1.L, sa1.Linv_diag, sa1.alpha, sa1.n_points, sa1.m_all, sa1.s_all, sa1.info, sa1.acqf_param,
             sa1.acqf, sa1.kind)
    plain = ops.target_acqf_batched(src["mu"][:, :16].contiguous(), src["var"][:, :16].contiguous(), cov, sa1.group_of([16]), X[:16].contiguous(), *tail1)
    assert torch.equal(mixed["value"][:16], plain["value"]) and torch.equal(mixed["grad"][:16], plain["grad"])
    # (7i): column 0 of that pass as one strip, per candidate (7g)'s value
    cov0 = src["cov"].reshape(T, sa.n_max, 16 * G, 16)[:, :nm, :16, 0].contiguous()
    strip = ops.target_score_batched(src["mu"][:, :16, 0].contiguous(), src["var"][:, :16, 0].contiguous(), cov0,
                                     torch.zeros(1, dtype=torch.int32, device=device), X[:16].contiguous(), *tail1)
    assert torch.equal(strip["value"], plain["value"])
    # (7k)'s strips: the log-domain average of the strip kernel is the query kernel's, F = 1, 2 and 64
    covs = src["cov"].reshape(T, sa.n_max, 16 * G, 16)[..., 0].contiguous()
    strips = ops.target_fantasy_score_batched(src["mu"][..., 0].contiguous(), src["var"][..., 0].contiguous(), covs,
                                              torch.arange(G, dtype=torch.int32, device=device), X, sa.w, sa.active, sa.Xt, sa.theta, sa.L,
                                              sa.Linv_diag, sa.alpha_f, sa.n_fant, sa.n_points, sa.m_all, sa.s_all, sa.info, sa.acqf_param, sa.acqf,
                                              sa.kind)
    torch.cuda.synchronize()
    assert torch.equal(strips["value"], mixed["value"])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_query_coordinate(case, bad):
    X, D = case["X"], case["D"]
    clean = _fantasy_launch(case, X)
    Xb = X.clone()
    rows = [3, 16 + 5, 32 + 15]   # one point of each study
    for i, r in enumerate(rows):
        Xb[r, (i * 2) % D] = bad
    out = _fantasy_launch(case, Xb)
    torch.cuda.synchronize()
    keep = torch.ones(X.shape[0], dtype=torch.bool, device=X.device)
    keep[rows] = False
    assert bool(torch.isnan(out["value"][rows]).all()) and bool(torch.isnan(out["grad"][rows]).all())
    assert torch.equal(out["value"][keep], clean["value"][keep]) and torch.equal(out["grad"][keep], clean["grad"][keep])


def test_logei_moves_where_ei_cannot(device):
    """A tiny stack (T = 2, N = 16, D = 2), a target of n = 6 and best_f so far below the model that u <= -40 at every start
    (asserted from model.posterior): ExpectedImprovement and its gradient are exact zeros and the device optimiser leaves every start
    where it began; with LogExpectedImprovement no start's value decreases and at least one start moves and gains."""
    D = 2
    g = torch.Generator().manual_seed(32)
    Xs = [torch.rand(16, D, dtype=torch.float64, generator=g) for _ in range(2)]
    stack = M.SourceGPStack(["a", "b"], Xs, [torch.sin(3.0 * x.sum(-1, keepdim=True) + 0.3 * t) for t, x in enumerate(Xs)], kind=0, device=device)
    stack.set_theta(torch.tensor([[0.7, 0.9, 1.0, 4e-3], [0.8, 0.6, 1.2, 2e-3]], dtype=torch.float64))
    stack.refresh()
    gps = {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}
    X = torch.rand(6, D, dtype=torch.float64, generator=g)
    Y = torch.sin(3.0 * X.sum(-1, keepdim=True))
    model = M.ScaMLGP(X, Y, gps, covar_module=hyper.get_default_kernel(hyper.MaternKernel, D)).eval()
    x0 = (0.2 + 0.6 * torch.rand(4, D, dtype=torch.float64, generator=g)).to(device)
    mvn = model.posterior(x0).mvn
    sigma = mvn.variance.clamp_min(1e-9).sqrt()
    best_f = float((mvn.mean - 45.0 * sigma).min())
    assert float((-(mvn.mean - best_f) / sigma).max()) <= -40.0
    ei, logei = utils.ExpectedImprovement(model, best_f), utils.LogExpectedImprovement(model, best_f)
    v, gr = ei.value_and_grad(x0)
    assert not bool(v.any()) and not bool(gr.any())
    group = torch.zeros(4, dtype=torch.int32, device=device)
    # (the call suggest_mode="device" makes for its starts, bo.ScaMLGPBOStudies.suggest; made here so that the starts are known)
    ends = {name: utils.StudiesAcquisition([af]).optimize(x0, group, 20, bounds=(0.0, 1.0))["x"].cpu() for name, af in (("ei", ei), ("logei", logei))}
    assert torch.equal(ends["ei"], x0.cpu())
    v0, v1 = logei(x0).cpu(), logei(ends["logei"].to(device)).cpu()
    moved = (ends["logei"] != x0.cpu()).any(1)
    print(f"LogEI at the starts {v0.tolist()}, at the ends {v1.tolist()}")
    assert bool((v1 >= v0).all()) and bool((moved & (v1 > v0)).any())


@pytest.mark.parametrize("mode,extra", [("sequential", {}), ("lockstep", {}), ("device", dict(max_pending_evaluations=2, pending_mode="batched", num_fantasies=8))])
def test_bo_studies_with_logei(device, mode, extra):
    gps = _branin_gps(device)
    kw = dict(KW, acquisition="logei")
    st = ScaMLGPBOStudies(gps, 2, 2, seeds=[71, 72], suggest_mode=mode, **kw, **extra)
    with pytest.raises(ValueError):
        st[0].acquisition_function()     # "ei"'s rule: no evaluation yet
    g = torch.Generator().manual_seed(3)
    init = {s: torch.rand(3 + s, 2, dtype=torch.float64, generator=g) for s in range(2)}
    st.report_some({s: (x, [_obj(r) for r in x]) for s, x in init.items()})
    for step in range(3):
        X = st.suggest()
        assert X.shape == (2, 2) and bool(((X >= 0.0) & (X <= 1.0)).all())
        afs = [st[s].acquisition_function() for s in range(2)]   # (with pending evaluations: on the study's fantasy model)
        assert all(isinstance(af, utils.LogExpectedImprovement) for af in afs)
        assert all((af.model.num_fantasies is not None) == bool(extra) for af in afs)
        vals = torch.stack([af(X[s:s + 1].to(device)).cpu() for s, af in enumerate(afs)])
        assert bool(torch.isfinite(vals).all())
        if not extra:
            if mode == "lockstep":   # the lock-step evaluation against each study's own value_and_grad
                sa = utils.StudiesAcquisition(afs)
                out = sa.evaluate(X.to(device), sa.group_of((1, 1)))
                for s, af in enumerate(afs):
                    x = X[s:s + 1].to(device)
                    v, gr = af.value_and_grad(x)
                    # a suggested point is (nearly) stationary: the gradient is what cancellation leaves of its two terms, so the
                    # bound is taken of THEIR magnitude, |Amu| |dmu| + |Av| |dvar|, not of the gradient's own
                    mu, var, dmu, dvar = af.model.posterior_with_grad(x)
                    _, Amu, Av = ops.acqf_transform(mu, var, LOGEI, af.best_f)
                    scale = float((Amu.abs().unsqueeze(-1) * dmu.abs() + Av.abs().unsqueeze(-1) * dvar.abs()).max())
                    assert _rel(out["value"][s:s + 1], v) <= BOUND
                    assert float((out["grad"][s:s + 1] - gr).abs().max()) <= BOUND * scale
        st.report(X, [_obj(x) for x in X])
