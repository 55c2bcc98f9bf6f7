"""sa_block<R, Params> of csrc/gp_studies_acqf.h on the MI355X through its four entry points -- scaml_target_acqf_batched_f64 (7g),
scaml_target_score_batched_f64 (7i), scaml_target_fantasy_acqf_batched_f64 and scaml_target_fantasy_score_batched_f64 (7k) -- against
the long-double reference of tests/_studies_bounds.py, every element of value, grad, mu_out and var_out held to its a-priori fp64
bound (capped at 1e-8 of the output's largest reference magnitude in its group), on the input sets that module lists: the smallest
shapes at which the body branches, none of the workload's.  Every output buffer holds a sentinel and one guard row more than the
call may write; what the contract says is not read holds NaN.  The chain runs the real pipeline of a lock-step suggest on the ragged
golden stack, each stage's reference fed the device's own upstream outputs.  Each test prints the largest error / bound and
bound / scale seen so far per entry point and output (profiles/studies_bounds_notes.md records them)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from scamlgp_amd import _lib, ops
from tests import _posterior_bounds as P
from tests import _posterior_variant_bounds as V
from tests import _studies_bounds as SB
from tests import _target_bounds as B
from tests import test_target_bounds_gpu as TG
from tests._studies_bounds import ACQ, ACQS, EI, FAMILY, KINDS, LOGEI, UCB

pytestmark = pytest.mark.gpu

_p = TG._p
ORDER = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha", "n_points", "m_all", "s_all", "info", "acqf_param")
ORDER_F = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha_f", "n_fant", "n_points", "m_all", "s_all",
           "info", "acqf_param")
DTYPES = dict(group=torch.int32, n_points=torch.int32, n_fant=torch.int32, info=torch.int32, active=torch.uint8)
NAMES = dict(acqf="scaml_target_acqf_batched_f64", score="scaml_target_score_batched_f64", fantasy="scaml_target_fantasy_acqf_batched_f64",
             fantasy_score="scaml_target_fantasy_score_batched_f64")


class Device(TG.Device):
    """tests/test_target_bounds_gpu.Device with the backend interface of tests/_studies_bounds.py: be.run(entry, a, grad, post)."""

    def run(self, entry, a, grad, post):
        Mq, D = a["Xq"].shape
        strips, fant = entry in ("score", "fantasy_score"), entry.startswith("fantasy")
        assert not (fant and post)
        ins = [self.up(a[k], DTYPES.get(k, torch.float64)) for k in (ORDER_F if fant else ORDER)]
        value = self.out(Mq)
        gr = self.out(Mq, D) if grad and not strips else None
        mu, var = (self.out(Mq), self.out(Mq)) if post else (None, None)
        dims = (Mq, a["G"], a["n_max"]) + ((a["F_max"],) if fant else ())
        tail = (a["T"], D, a["kind"], a["acqf"])
        outs = {"acqf": (value, gr, mu, var), "score": (value, mu, var), "fantasy": (value, gr), "fantasy_score": (value,)}[entry]
        fn = getattr(self.lib, NAMES[entry])
        _lib.check_rc(fn(*[_p(x) for x in ins], *dims, *tail, *[_p(x) for x in outs], self.stream), NAMES[entry])
        torch.cuda.synchronize()
        t = lambda x: None if x is None else self.take(x)   # noqa: E731
        return dict(value=t(value), grad=t(gr), mu=t(mu), var=t(var))


def _show():
    for line in SB.report():
        print(line)


FAM = pytest.mark.parametrize("kind", KINDS, ids=["rbf", "matern"])
ACQF = pytest.mark.parametrize("acqf", ACQS, ids=[ACQ[x] for x in ACQS])


@FAM
@ACQF
@pytest.mark.parametrize("name", sorted(SB.ORDINARY_SETS))
def test_ordinary_sets_within_bound(name, kind, acqf, device):
    """(7g) with every output and with grad / mu_out / var_out NULL, (7i) on column 0 re-laid as strips."""
    a = SB.ORDINARY_SETS[name](kind, acqf)
    be = Device(device)
    SB.check_set(be, a, f"studies-{name}-{FAMILY[kind]}-{ACQ[acqf]}", tag="clean")
    if acqf == UCB:
        SB.check_junk_columns(be, a, f"studies-{name}-{FAMILY[kind]}")
    _show()


@FAM
@ACQF
@pytest.mark.parametrize("name", sorted(SB.FANTASY_SETS))
def test_fantasy_sets_within_bound(name, kind, acqf, device):
    """Both entries of (7k): F_g from 1 to 64 under F_max = 64 and 9, F = 1 next to F = 64 in one launch, (96, 64) as a strip."""
    a = SB.FANTASY_SETS[name](kind, acqf)
    be = Device(device)
    SB.check_set(be, a, f"studies-{name}-{FAMILY[kind]}-{ACQ[acqf]}", tag="clean")
    if acqf == UCB:
        SB.check_junk_columns(be, a, f"studies-{name}-{FAMILY[kind]}")
    _show()


@FAM
@ACQF
def test_clamps(kind, acqf, device):
    """var = -0.01, 5e-10, exactly 0, beta = 0: within the bounds, and the clamped partial exactly absent from the gradient."""
    SB.check_clamp(Device(device), kind, acqf)
    _show()


@FAM
@pytest.mark.parametrize("acqf", [EI, LOGEI], ids=["ei", "logei"])
@pytest.mark.parametrize("mode", ["span", "deep"])
def test_ei_tails(mode, kind, acqf, device):
    SB.check_tail(Device(device), mode, kind, acqf)
    _show()


@FAM
def test_refusals_and_non_finite_queries(kind, device):
    """info != 0, n_points / n_fant out of range: NaN for that group only; a NaN query coordinate: NaN in that query's outputs; once per
    entry point, the others within their bounds."""
    be = Device(device)
    a = SB.set_T8(kind, EI)
    SB.check_refusals(be, a, f"studies-T8-{FAMILY[kind]}", victim=2)
    SB.check_nonfinite(be, a, f"studies-T8-{FAMILY[kind]}-nanq", q=3)
    f = SB.set_FB(kind, LOGEI)
    SB.check_refusals(be, f, f"studies-FB-{FAMILY[kind]}", victim=0)
    SB.check_nonfinite(be, f, f"studies-FB-{FAMILY[kind]}-nanq", q=1)
    _show()


# ---- the chain: the real pipeline of a lock-step suggest, every stage's reference fed the device's own upstream outputs ------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_ragged_T4_N48_matern.npz")
CHAIN_NS, CHAIN_PENDING, CHAIN_F = (1, 17, 40), 3, 5      # study 1: 14 observed + 3 pending points, 5 fantasies
CHAIN_COUNTS = (2, 2, 2)                                   # query points per study, then a padding row


@contextlib.contextmanager
def _outputscale(value):
    """tests/_posterior_bounds.py states its bounds for stacks whose outputscale is its constant OS; the golden stack has another."""
    old = P.OS, V.OS
    P.OS = V.OS = value
    try:
        yield
    finally:
        P.OS, V.OS = old


@FAM
def test_chain_within_its_bounds(kind, device):
    """The ragged golden stack (T = 4, N = 48, Matern-5/2) under studies of n = (1, 17, 40), the second with 3 pending points and
    F = 5: (1) the grouped GRAD and value source passes (5e) / (5f) and the value pass at the studies' training points under the bounds
    of tests/_posterior_variant_bounds.py / tests/_posterior_bounds.py; (2) the training blocks (7j) and one scaml_potrf_batched_f64
    under those of tests/_target_bounds.py; (3) the solve for alpha_f; (4) the four entry points on all of that, UCB, EI and LogEI,
    under the bounds of tests/_studies_bounds.py.  `kind`: the family of the studies' target kernels."""
    be = Device(device)
    lib, stream, fam = be.lib, be.stream, FAMILY[kind]
    d = np.load(GOLDEN)
    inp = {k: d[k] for k in ("X", "y", "theta", "n_points", "y_mean", "y_std")}
    kind_s, (T, N, D), G, n_max = int(d["kind"]), d["X"].shape, len(CHAIN_NS), max(CHAIN_NS)
    os_s = float(inp["theta"][0, D])
    assert (inp["theta"][:, D] == os_s).all()
    rng = np.random.default_rng([20261021, 9, kind])
    # ---- set-up: the source fit, L^-1, and V of every study's training points (covered by tests/test_posterior_bounds_gpu.py)
    X, y, theta = (be.up(inp[k]) for k in ("X", "y", "theta"))
    npts, ym, ysd = be.up(inp["n_points"], torch.int32), be.up(inp["y_mean"]), be.up(inp["y_std"])
    fit = ops.gp_fit_fused(X, y, theta, kind_s, n_points=npts, want_linv=True)
    assert not bool((fit["info"] != 0).any())
    Linv = ops.linv_batched(fit["L"], fit["Linv_diag"], n_points=npts)
    src = (_p(X), _p(theta), _p(Linv), _p(fit["alpha"]), _p(ym), _p(ysd), _p(npts))
    Xt = rng.uniform(size=(G, n_max, D))
    Xt_d = be.up(Xt)
    VA = []
    for g, n in enumerate(CHAIN_NS):
        va = torch.zeros(T, N, n, dtype=torch.float64, device=device)
        _lib.check_rc(lib.scaml_posterior_linv_f64(_p(Xt_d[g, :n].contiguous()), *src, T, N, n, D, kind_s, None, None, _p(va), 0, stream),
                      "scaml_posterior_linv_f64")
        VA.append(va)
    VA_tab = torch.tensor([v.data_ptr() for v in VA], dtype=torch.int64, device=device)
    n_a = be.up(np.array(CHAIN_NS, dtype=np.int32), torch.int32)
    arr = dict(inp, alpha=fit["alpha"].cpu().numpy(), Linv=Linv.cpu().numpy(), L=fit["L"].cpu().numpy(), Linv_diag=fit["Linv_diag"].cpu().numpy(),
               Xa=Xt, VA=[v.cpu().numpy() for v in VA])
    # ---- stage 1: the grouped passes
    group_q = np.array([g for g, c in enumerate(CHAIN_COUNTS) for _ in range(c)] + [-1], dtype=np.int32)
    Mq = len(group_q)
    Xq = rng.uniform(size=(Mq, D))
    group_s = np.array(list(range(G)) + [-1], dtype=np.int32)
    Xs = rng.uniform(size=(16 * len(group_s), D))
    for g in range(G):
        Xs[16 * g:16 * g + CHAIN_COUNTS[g]] = Xq[group_q == g]

    def grouped(fn, Xp, group, W):
        M = Xp.shape[0]
        outs = [torch.full((T + 1, *s), SB.SENTINEL, dtype=torch.float64, device=device) for s in ((M * W,), (M * W,), (n_max, M * W))]
        Xp_d, group_d = be.up(Xp), be.up(group, torch.int32)      # (held until the launch has run)
        _lib.check_rc(getattr(lib, fn)(_p(Xp_d), _p(group_d), _p(Xt_d), _p(n_a), _p(VA_tab), *src, T, N, M, G, n_max, D, kind_s,
                                       *[_p(o) for o in outs], stream), fn)
        torch.cuda.synchronize()
        assert all(bool((o[T] == SB.SENTINEL).all()) for o in outs), f"{fn} wrote past the last task slot's slice"
        return dict(zip(("mu", "var", "cov"), (o[:T].cpu().numpy() for o in outs)))

    with _outputscale(os_s):
        cq = V._v("5e", T, N, D, kind_s, Mq=Mq, Ma=CHAIN_NS, group=tuple(int(x) for x in group_q), ragged=0)
        gq = grouped("scaml_posterior_linv_grad_grouped_f64", Xq, group_q, 16)
        V.check_case(cq, dict(arr, Xq=Xq), gq, " chain")
        cs = V._v("5f", T, N, D, kind_s, Mq=len(Xs), Ma=CHAIN_NS, group=tuple(int(x) for x in group_s), ragged=0)
        gs = grouped("scaml_posterior_linv_grouped_f64", Xs, group_s, 1)
        V.check_case(cs, dict(arr, Xq=Xs), gs, " chain")
        # the source terms at the studies' training points: the value pass (5c') per study
        means_t, covs_p = np.zeros((G, T, n_max)), np.zeros((G, T, n_max * (n_max + 1) // 2))
        terms = []
        for g, n in enumerate(CHAIN_NS):
            val = P._c("linv_cov", T, N, n, D, kind_s, Ma=n, ragged=0, std=True)
            mu, var, cov = be.out(T, n), be.out(T, n), be.out(T, n, n)
            _lib.check_rc(lib.scaml_posterior_linv_cov_f64(_p(Xt_d[g, :n].contiguous()), *src, _p(VA[g]), T, N, n, n, D, kind_s, _p(mu), _p(var), _p(cov),
                                                           0, stream), "scaml_posterior_linv_cov_f64")
            got = dict(mu=be.take(mu), var=be.take(var), cov=be.take(cov))
            ainp = dict(inp, Xq=Xt[g, :n])
            for t in range(T):
                P.check_task(val, ainp, dict(arr, Xq=Xt[g, :n], VA=arr["VA"][g]), t, {k: x[t] for k, x in got.items()})
            ia, ib = np.tril_indices(n)
            means_t[g, :, :n] = got["mu"]
            covs_p[g, :, :n * (n + 1) // 2] = got["cov"][:, ia, ib]
            terms.append(got)
    # ---- stage 2: the training blocks (7j) and ONE potrf
    w = 0.2 + rng.uniform(size=(G, T))
    active = np.ones((G, T), dtype=np.uint8)
    active[1, 2], w[1, 2] = 0, 0.0      # one task pruned in one study only
    theta_t = np.concatenate([0.4 + rng.uniform(size=(G, D)), 0.5 + rng.uniform(size=(G, 1)), 0.05 + 0.1 * rng.uniform(size=(G, 1))], 1)      # (noise >= 0.05: the caps of stage 4 need the conditioning)
    m_all, s_all = np.full(G, 40.0) + rng.uniform(size=G), np.full(G, 30.0) + rng.uniform(size=G)
    yt = np.sin(3.0 * Xt.sum(-1)) + 0.2 * rng.normal(size=(G, n_max))
    n_pts = np.array(CHAIN_NS, dtype=np.int32)
    dev = {k: be.up(x, DTYPES.get(k, torch.float64)) for k, x in dict(means_t=means_t, covs_p=covs_p, Xt=Xt, yt=yt, n_points=n_pts, m_all=m_all, s_all=s_all,
                                                                     w=w, active=active, theta=theta_t).items()}
    Knn, resid = be.out(G, n_max, n_max), be.out(G, n_max)
    _lib.check_rc(lib.scaml_target_train_block_batched_f64(*[_p(dev[k]) for k in ("means_t", "covs_p", "Xt", "yt", "n_points", "m_all", "s_all", "w", "active",
                                                                                  "theta")], G, n_max, T, D, kind, _p(Knn), _p(resid), stream),
                  "scaml_target_train_block_batched_f64")
    Knn_h, resid_h = be.take(Knn), be.take(resid)
    f = ops.potrf_batched(Knn[:G].contiguous(), resid[:G].contiguous(), n_points=dev["n_points"], want_linv=True)
    torch.cuda.synchronize()
    L, W, alpha, info, jitter = (f[k].cpu().numpy() for k in ("L", "Linv_diag", "alpha", "info", "jitter"))
    assert not info.any() and not jitter.any(), (info, jitter)
    label = f"studies-chain-{fam}"
    for g, n in enumerate(CHAIN_NS):
        ia, ib = np.tril_indices(n)
        full = np.zeros((T, n, n))
        full[:, ia, ib] = covs_p[g, :, :n * (n + 1) // 2]
        full = full + np.tril(full, -1).transpose(0, 2, 1)
        tb = SB.train_block_reference(means_t[g, :, :n], full, Xt[g, :n], yt[g, :n], m_all[g], s_all[g], w[g], active[g], theta_t[g], kind)
        SB.within(f"{label} study {g}", ("studies_chain", fam, "Knn"), np.tril(Knn_h[g, :n, :n]), tb["Knn"])
        SB.within(f"{label} study {g}", ("studies_chain", fam, "resid"), resid_h[g, :n], tb["resid"])
        LLt, q = B.potrf_reference(L[g, :n, :n], Knn_h[g, :n, :n], 0.0)
        SB.within(f"{label} study {g}", ("studies_chain", fam, "L L^T"), LLt, q)
        SB.within(f"{label} study {g}", ("studies_chain", fam, "alpha"), alpha[g, :n], B._col(B.solve_reference(L[g, :n, :n], resid_h[g, :n, None], n)))
    # ---- stage 3: alpha_f of the study with pending points: the fantasised outcomes differ in the pending rows
    g, n = 1, CHAIN_NS[1]
    R = np.repeat(resid_h[g, :n, None], CHAIN_F, axis=1)
    R[n - CHAIN_PENDING:] += 0.3 * rng.normal(size=(CHAIN_PENDING, CHAIN_F))
    Lg, Wg = np.ascontiguousarray(L[g, :n, :n]), np.ascontiguousarray(W[g, :(n + 15) // 16])
    af = be.solve(Lg[None], Wg[None], R[None], None, False)[0]
    SB.within(f"{label} study {g}", ("studies_chain", fam, "alpha_f"), af, B.solve_reference(Lg, R, n))
    alpha_f = np.zeros((G, n_max, CHAIN_F))
    alpha_f[:, :, 0] = alpha
    alpha_f[g, :n] = af
    # ---- stage 4: the four entry points on the device's own upstream outputs
    common = dict(w=w, active=active, Xt=Xt, theta=theta_t, L=L, Linv_diag=W, n_points=n_pts, m_all=m_all, s_all=s_all, info=info.astype(np.int32),
                  G=G, n_max=n_max, T=T, D=D, kind=kind)
    for acqf in ACQS:
        aq = dict(common, name="chain", mu=gq["mu"].reshape(T, Mq, 16), var=gq["var"].reshape(T, Mq, 16), cov=gq["cov"], group=group_q, Xq=Xq, Mq=Mq,
                  acqf=acqf, alpha=np.ascontiguousarray(alpha_f[:, :, 0]), acqf_param=np.array([4.0, 5.0, 6.0]))
        if acqf != UCB:
            mu64 = SB.posterior64(aq)[0]
            aq["acqf_param"] = np.array([mu64[group_q == s].mean() + 0.1 for s in range(G)])
        as_ = dict(aq, mu=gs["mu"], var=gs["var"], cov=gs["cov"], group=group_s, Xq=Xs, Mq=len(Xs))
        fq = dict(aq, alpha_f=alpha_f, n_fant=np.array([1, CHAIN_F, 1], dtype=np.int32), F_max=CHAIN_F)
        fs = dict(as_, alpha_f=alpha_f, n_fant=fq["n_fant"], F_max=CHAIN_F)
        for entry, a, grad, post in (("acqf", aq, True, True), ("score", as_, False, True), ("fantasy", fq, True, False), ("fantasy_score", fs, False, False)):
            a = {k: x for k, x in a.items() if not (k == "alpha" and "alpha_f" in a)}
            SB.hold(f"{label}-{ACQ[acqf]}", entry, a, SB.reference(a), be.run(entry, a, grad=grad, post=post), table="studies_chain")
    _show()
