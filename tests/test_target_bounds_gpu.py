"""The kernels downstream of the source pass (scaml_weighted_task_sum_f64, scaml_weighted_prior_reduce_f64, scaml_target_assemble_f64,
scaml_potrf_batched_f64 at T = 1, scaml_cho_solve_batched_f64, scaml_solve_lt_batched_f64, scaml_target_finish_f64,
scaml_target_posterior_grad_f64) through the C ABI against a long-double reference that consumes the DEVICE's own upstream outputs,
each output element held to the a-priori forward error bound of tests/_target_bounds.py (capped at 1e-8 of the quantity's scale), on
the input sets that module lists.  Every output buffer holds a sentinel and one guard row / slice more than the call may write;
padding past n_t that the contract says is not read holds NaN.  Each test prints the largest error / bound and bound / scale seen so
far per kernel and output (profiles/target_bounds_notes.md records them)."""
import numpy as np
import pytest
import torch

from scamlgp_amd import _lib, ops
from tests import _posterior_bounds as P
from tests import _target_bounds as B
from tests import test_studies_acqf_emul as SE
from tests._posterior_bounds import KIND_MATERN52, KIND_RBF, SENTINEL

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else t.data_ptr()


class Device:
    """The backend interface of tests/_target_bounds.py on the C ABI: numpy in, numpy out, every output through a guarded buffer."""
    name = "device"

    def __init__(self, device):
        self.dev, self.lib = device, _lib.lib

    def up(self, a, dtype=torch.float64):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dtype)

    def out(self, *shape):
        """A buffer of shape[0] + 1 rows full of the sentinel: the last row is the guard."""
        return torch.full((shape[0] + 1, *shape[1:]), SENTINEL, dtype=torch.float64, device=self.dev)

    @staticmethod
    def take(buf):
        assert bool((buf[-1] == SENTINEL).all()), "the call wrote past the end of its output"
        return buf[:-1].cpu().numpy()

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def wsum(self, inp, w, active, power):
        T, length = inp.shape
        i, wd, ad, o = self.up(inp), self.up(w), self.up(active, torch.uint8), self.out(length)
        _lib.check_rc(self.lib.scaml_weighted_task_sum_f64(_p(i), _p(wd), _p(ad), T, length, power, _p(o), self.stream), "scaml_weighted_task_sum_f64")
        return self.take(o)

    def prior_reduce(self, mu, cov, w, active):
        T = w.shape[0]
        M = (mu if mu is not None else cov).shape[-1]
        Ma = 0 if cov is None else cov.shape[1]
        md, cd, wd, ad = self.up(mu), self.up(cov), self.up(w), self.up(active, torch.uint8)
        mo, co = (None if mu is None else self.out(M)), (None if cov is None else self.out(Ma * M))
        _lib.check_rc(self.lib.scaml_weighted_prior_reduce_f64(_p(md), _p(cd), _p(wd), _p(ad), T, M, Ma, _p(mo), _p(co), self.stream),
                      "scaml_weighted_prior_reduce_f64")
        return (None if mo is None else self.take(mo)), (None if co is None else self.take(co).reshape(Ma, M))

    def assemble(self, a):
        n, M, D = a["n"], a["M"], a["D"]
        ins = [self.up(a[k]) for k in ("cov_s", "mean_s", "var_s", "Xall", "theta", "y")]
        Knn, resid = self.out(n, n), self.out(n)
        Knq, mean_q, var_q = (self.out(n, M), self.out(M), self.out(M)) if M else (None, None, None)
        _lib.check_rc(self.lib.scaml_target_assemble_f64(*[_p(x) for x in ins], float(a["m"]), float(a["s"]), n, M, D, a["kind"], _p(Knn), _p(resid),
                                                         _p(Knq), _p(mean_q), _p(var_q), self.stream), "scaml_target_assemble_f64")
        got = dict(Knn=self.take(Knn), resid=self.take(resid))
        if M:
            got.update(Knq=self.take(Knq), mean_q=self.take(mean_q), var_q=self.take(var_q))
        return got

    def potrf(self, Knn, resid):
        n = Knn.shape[0]
        NB = (n + 15) // 16
        A, y = self.up(Knn[None]), self.up(resid[None])
        L, alpha, W = self.out(1, n, n), self.out(1, n), self.out(1, NB, 16, 16)
        scal = torch.full((3,), SENTINEL, dtype=torch.float64, device=self.dev)      # quad, logdet, jitter_used
        info = torch.full((1,), -7, dtype=torch.int32, device=self.dev)
        _lib.check_rc(self.lib.scaml_potrf_batched_f64(_p(A), _p(y), None, None, 1, n, _p(L), _p(alpha), scal[0:].data_ptr(), scal[1:].data_ptr(),
                                                       _p(info), scal[2:].data_ptr(), _p(W), _lib.FIT_STORE_L | _lib.FIT_ZERO_UPPER, self.stream),
                      "scaml_potrf_batched_f64")
        return dict(L=self.take(L)[0], alpha=self.take(alpha)[0], W=self.take(W)[0], info=int(info.cpu()[0]), jitter=float(scal.cpu()[2]))

    def solve(self, L, W, Bs, n_points, lt):
        T, N, R = Bs.shape
        Ld, Wd, Bd, nd = self.up(L), self.up(W), self.up(Bs), self.up(n_points, torch.int32)
        X = self.out(T, N, R)
        fn = self.lib.scaml_solve_lt_batched_f64 if lt else self.lib.scaml_cho_solve_batched_f64
        _lib.check_rc(fn(_p(Ld), _p(Wd), _p(Bd), _p(nd), T, N, R, _p(X), self.stream), "scaml_cho_solve_batched_f64")
        return self.take(X)

    def _fit(self, fc, inp):
        X, y, theta = (self.up(inp[k]) for k in ("X", "y", "theta"))
        npts = self.up(inp["n_points"], torch.int32)
        fit = ops.gp_fit_fused(X, y, theta, fc.kind, n_points=npts, want_linv=True)
        live = torch.tensor([n > 0 for n in P.counts(fc, inp)], device=self.dev)
        assert not bool((fit["info"] != 0)[live].any())
        return X, theta, npts, fit

    def fit(self, fc, inp):
        fit = self._fit(fc, inp)[3]
        return dict(L=fit["L"].cpu().numpy(), Linv_diag=fit["Linv_diag"].cpu().numpy())

    def finish(self, a, info):
        n, M = a["n"], a["M"]
        ins = [self.up(a[k]) for k in ("Knq", "Z", "alpha", "mean_q", "var_q")]
        inf = None if info is None else torch.tensor([info], dtype=torch.int32, device=self.dev)
        mu, var = self.out(M), self.out(M)
        _lib.check_rc(self.lib.scaml_target_finish_f64(*[_p(x) for x in ins], float(a["m"]), float(a["s"]), float(a["noise_add"]), _p(inf), n, M,
                                                       _p(mu), _p(var), self.stream), "scaml_target_finish_f64")
        return self.take(mu), self.take(var)

    def tgrad(self, a, info):
        n, Mq, D = a["n"], a["Mq"], a["D"]
        width = a["Xq"].shape[1]      # (the D = 16 call brings the buffers of D = 15)
        ins = [self.up(a[k]) if (n or k in ("mu_g", "var_g", "Xq", "theta")) else None for k in ("cov_g", "mu_g", "var_g", "Xt", "Xq", "theta", "alpha", "Z")]
        inf = None if info is None else torch.tensor([info], dtype=torch.int32, device=self.dev)
        dmu, dvar = self.out(Mq, width), self.out(Mq, width)
        rc = self.lib.scaml_target_posterior_grad_f64(*[_p(x) for x in ins], float(a["s"]), _p(inf), n, Mq, D, a["kind"], _p(dmu), _p(dvar), self.stream)
        return rc, self.take(dmu), self.take(dvar)

    def source_passes(self, val, inp, grad, ginp):
        """The value pass (scaml_posterior_linv_cov_f64 at cat(Xt, Xq)) and the GRAD pass (scaml_posterior_linv_grad_f64 at Xq) of the chain
        on one device fit, as tests/test_posterior_bounds_gpu.py calls them."""
        lib, T, N, D, Ma = self.lib, val.T, val.N, val.D, val.Ma
        X, theta, npts, fit = self._fit(val, inp)
        L, W, alpha = fit["L"], fit["Linv_diag"], fit["alpha"]
        Linv = ops.linv_batched(L, W, n_points=npts)
        ym, ysd = self.up(inp["y_mean"]), self.up(inp["y_std"])
        Xall, Xq, Xa = self.up(inp["Xq"]), self.up(ginp["Xq"]), self.up(ginp["Xa"])
        VA = torch.empty(T, N, Ma, dtype=torch.float64, device=self.dev)
        _lib.check_rc(lib.scaml_posterior_linv_f64(_p(Xa), _p(X), _p(theta), _p(Linv), _p(alpha), _p(ym), _p(ysd), _p(npts), T, N, Ma, D, val.kind,
                                                   None, None, _p(VA), 0, self.stream), "scaml_posterior_linv_f64")
        M, Mq = val.M, grad.M
        mu, var, cov = self.out(T, M), self.out(T, M), self.out(T, Ma, M)
        _lib.check_rc(lib.scaml_posterior_linv_cov_f64(_p(Xall), _p(X), _p(theta), _p(Linv), _p(alpha), _p(ym), _p(ysd), _p(npts), _p(VA), T, N, M, Ma, D,
                                                       val.kind, _p(mu), _p(var), _p(cov), 0, self.stream), "scaml_posterior_linv_cov_f64")
        gmu, gvar, gcov = self.out(T, Mq, 16), self.out(T, Mq, 16), self.out(T, Ma, 16 * Mq)
        _lib.check_rc(lib.scaml_posterior_linv_grad_f64(_p(Xq), _p(Xa), _p(X), _p(theta), _p(Linv), _p(alpha), _p(ym), _p(ysd), _p(npts), _p(VA), T, N, Mq,
                                                        Ma, D, val.kind, _p(gmu), _p(gvar), _p(gcov), 0, self.stream), "scaml_posterior_linv_grad_f64")
        arr = dict(inp, L=L.cpu().numpy(), Linv_diag=W.cpu().numpy(), alpha=alpha.cpu().numpy(), Linv=Linv.cpu().numpy(), VA=VA.cpu().numpy())
        return dict(arr=arr, value=dict(mu=self.take(mu), var=self.take(var), cov=self.take(cov)),
                    grad=dict(mu=self.take(gmu), var=self.take(gvar), cov=self.take(gcov)))


def _show(*prefixes):
    for pre in prefixes:
        for line in B.report(pre):
            print(line)


@pytest.mark.parametrize("T", B.WSUM_T)
def test_weighted_sum_within_its_bound(T, device):
    """Every length, power and mask for one T (the prior reduce at T = 5): a masked task is skipped whatever it holds, every task masked
    gives exact zeros, nothing is written past `len`."""
    B.check_wsum(Device(device), T)
    _show("weighted_task_sum", "weighted_prior_reduce")


@pytest.mark.parametrize("case", B.ASSEMBLE_CASES, ids=B.assemble_id)
def test_assemble_potrf_solve_within_their_bounds(case, device):
    """The assemble; then on ITS Knn / resid the POTRF (T = 1, residual form, alpha under the solve bound) and on that factor and the
    assembled Knq the solve (R = M).  A NaN query coordinate: NaN in exactly that column of Knq, everything else within its bound."""
    B.check_assemble(Device(device), case)
    _show("target_assemble", "potrf(T=1)", "cho_solve(target)")


@pytest.mark.parametrize("case", B.SOLVE_CASES, ids=B.solve_id)
def test_solve_within_its_bound(case, device):
    """scaml_cho_solve_batched_f64 / scaml_solve_lt_batched_f64 on a device fit beyond the target sizes, against the long-double inverse
    of the device's L alone; rows at or past n_t exactly zero."""
    B.check_solve(Device(device), case)
    _show("cho_solve", "solve_lt")


@pytest.mark.parametrize("shape", B.FINISH_SHAPES, ids=lambda s: f"n{s[0]}-M{s[1]}")
def test_finish_within_its_bound(shape, device):
    B.check_finish(Device(device), *shape)
    _show("target_finish")


@pytest.mark.parametrize("case", B.TGRAD_CASES, ids=B.tgrad_id)
def test_target_gradient_within_its_bound(case, device):
    """info NULL / 0 / > 0 (NaN), and for Mq = 3 a query with a NaN and with an infinite coordinate and finite mu_g / var_g / cov_g: NaN
    in every entry of that query's dmu / dvar, the other queries within their bounds (include/scaml_gp.h (5d))."""
    B.check_tgrad(Device(device), case)
    _show("target_posterior_grad")


def test_target_gradient_refuses_d_16(device):
    B.check_tgrad_toolarge(Device(device))


@pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])
def test_chain_within_its_bounds(kind, device):
    """The real pipeline end to end -- source value and GRAD passes, weighted sums, assemble, POTRF, solve, finish, gradient -- every
    stage's reference fed the device's own upstream outputs: the layout contracts between the stages."""
    B.check_chain(Device(device), kind)
    _show("chain")


@pytest.mark.parametrize("kind", [KIND_RBF, KIND_MATERN52], ids=["rbf", "matern"])
def test_batched_acquisition_gives_nan_for_a_non_finite_query(kind, device):
    """scaml_target_acqf_batched_f64 (include/scaml_gp.h (7g)) on the synthetic studies of tests/test_studies_acqf_emul.py, whose
    source-pass columns are finite whatever the query holds: one NaN coordinate gives NaN in that query's value, every entry of its
    gradient, mu_out and var_out; the other queries are bit for bit those of the clean call (the result is a pure function of the
    inputs); nothing is written past the outputs."""
    be = Device(device)
    prob = SE.Problem(6, kind, seed=11)
    q = SE.LOW_VAR_Q + 1
    order = ("mu", "var", "cov", "group", "Xq", "w", "active", "Xt", "theta", "L", "Linv_diag", "alpha", "n_points", "m_all", "s_all", "info", "acqf_param")
    dtypes = dict(group=torch.int32, n_points=torch.int32, info=torch.int32, active=torch.uint8)

    def run(acqf, poison):
        a = prob.arrays(acqf)
        Mq, D = a["Xq"].shape
        if poison:
            a["Xq"][q, 2] = np.nan
        ins = [be.up(a[k], dtypes.get(k, torch.float64)) for k in order]
        outs = [be.out(Mq), be.out(Mq, D), be.out(Mq), be.out(Mq)]
        _lib.check_rc(be.lib.scaml_target_acqf_batched_f64(*[_p(x) for x in ins], Mq, prob.G, prob.n_max, SE.T, D, kind, acqf, *[_p(x) for x in outs],
                                                           be.stream), "scaml_target_acqf_batched_f64")
        return dict(zip(("value", "grad", "mu", "var"), (be.take(x) for x in outs)))

    for acqf in (0, 1):
        good, bad = run(acqf, False), run(acqf, True)
        others = np.arange(good["value"].shape[0]) != q
        for k in ("value", "grad", "mu", "var"):
            assert np.isfinite(good[k][q]).all(), k
            assert np.isnan(bad[k][q]).all(), (k, bad[k][q])
            assert np.array_equal(bad[k][others], good[k][others]), k
