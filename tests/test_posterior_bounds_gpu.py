"""The source-posterior kernels (scaml_posterior_batched_f64, scaml_posterior_linv_f64, scaml_posterior_cov_f64,
scaml_posterior_linv_cov_f64, scaml_posterior_linv_grad_f64, scaml_linv_batched_f64 and its lower-only variant) against a
long-double reference that consumes the DEVICE's own L / Linv_diag / Linv / alpha / V / VA, each output element held to the
a-priori forward error bound of tests/_posterior_bounds.py (capped at 1e-8 of the quantity's scale) -- at the shapes where the
kernels branch: odd and even N, 2 / 9 / 16 / 17 / 32 row blocks, nine tasks (second XCD round, workgroups past the last task),
M = 1 and partial strips, D off the MFMA k-step, Ma in {0, 1, 16, 17, 96}, ragged tasks down to one and zero points, and a query
point with a NaN coordinate.  The entry points are called with output buffers that hold a sentinel and one task slice more than
the call may write."""
import numpy as np
import pytest
import torch

from scamlgp_amd import _lib, ops
from tests import _posterior_bounds as B
from tests._posterior_bounds import CASES, SENTINEL

pytestmark = pytest.mark.gpu


def _dev(a, device, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _out(device, T, *shape):
    """An output buffer of T + 1 task slices full of the sentinel: slice T is the guard no call may touch."""
    return torch.full((T + 1, *shape), SENTINEL, dtype=torch.float64, device=device)


def _take(buf, T):
    assert bool((buf[T] == SENTINEL).all()), "the call wrote past the last task's slice"
    return buf[:T].cpu().numpy()


def _ok(rc, what):
    _lib.check_rc(rc, what)


def _run(c, device):
    """Fit on the device, call the case's entry point; returns (inputs, arrays for the reference, outputs by name (T, ...))."""
    lib, stream = _lib.lib, torch.cuda.current_stream().cuda_stream
    inp = B.make_inputs(c)
    T, N, M, D, Ma = c.T, c.N, c.M, c.D, c.Ma
    X, y, theta = (_dev(inp[k], device) for k in ("X", "y", "theta"))
    npts = _dev(inp["n_points"], device, torch.int32)
    ym, ysd = _dev(inp["y_mean"], device), _dev(inp["y_std"], device)
    fit = ops.gp_fit_fused(X, y, theta, c.kind, n_points=npts, want_linv=True)
    live = torch.tensor([n > 0 for n in B.counts(c, inp)], device=device)
    assert not bool((fit["info"] != 0)[live].any())
    L, W, alpha = fit["L"], fit["Linv_diag"], fit["alpha"]
    arr = dict(inp, L=L.cpu().numpy(), Linv_diag=W.cpu().numpy(), alpha=alpha.cpu().numpy())
    if c.kern.startswith("linvmat"):
        out = _out(device, T, N, N)
        fn = lib.scaml_linv_batched_lower_f64 if c.kern == "linvmat_lower" else lib.scaml_linv_batched_f64
        _ok(fn(_p(L), _p(W), _p(npts), T, N, _p(out), stream), "scaml_linv_batched_f64")
        return inp, arr, dict(Linv=_take(out, T))
    Linv = ops.linv_batched(L, W, n_points=npts)
    arr["Linv"] = Linv.cpu().numpy()
    Xq = _dev(inp["Xq"], device)
    flags = _lib.POST_XQ_PER_TASK if c.per_task else 0

    def leading_V(Xlead):      # V of the Ma leading points, as the callers of the covariance passes produce it
        VA = torch.empty(T, N, Ma, dtype=torch.float64, device=device)
        _ok(lib.scaml_posterior_linv_f64(_p(Xlead), _p(X), _p(theta), _p(Linv), _p(alpha), _p(ym), _p(ysd), _p(npts), T, N, Ma, D, c.kind,
                                         None, None, _p(VA), flags, stream), "scaml_posterior_linv_f64")
        return VA

    if c.kern in ("subst", "subst_mean", "linv"):
        mean_only = c.kern == "subst_mean"
        mu = _out(device, T, M)
        var, V = (None, None) if mean_only else (_out(device, T, M), _out(device, T, N, M))
        if c.kern == "linv":
            rc = lib.scaml_posterior_linv_f64(_p(Xq), _p(X), _p(theta), _p(Linv), _p(alpha), _p(ym), _p(ysd), _p(npts), T, N, M, D, c.kind,
                                              _p(mu), _p(var), _p(V), flags, stream)
        else:
            rc = lib.scaml_posterior_batched_f64(_p(Xq), _p(X), _p(theta), None if mean_only else _p(L), None if mean_only else _p(W), _p(alpha),
                                                 _p(ym), _p(ysd), _p(npts), T, N, M, D, c.kind, _p(mu), _p(var), _p(V),
                                                 flags | (_lib.POST_MEAN_ONLY if mean_only else 0), stream)
        _ok(rc, "scaml_posterior_*_f64")
        got = dict(mu=_take(mu, T))
        if not mean_only:
            got.update(var=_take(var, T), V=_take(V, T))
        return inp, arr, got
    if c.kern == "cov":
        V = torch.empty(T, N, M, dtype=torch.float64, device=device)
        _ok(lib.scaml_posterior_batched_f64(_p(Xq), _p(X), _p(theta), _p(L), _p(W), _p(alpha), _p(ym), _p(ysd), _p(npts), T, N, M, D, c.kind,
                                            None, None, _p(V), flags, stream), "scaml_posterior_batched_f64")
        arr["V"] = V.cpu().numpy()
        cov = _out(device, T, Ma, M)
        _ok(lib.scaml_posterior_cov_f64(_p(Xq), _p(theta), _p(V), _p(ysd), T, N, M, Ma, D, c.kind, _p(cov), flags, stream), "scaml_posterior_cov_f64")
        return inp, arr, dict(cov=_take(cov, T))
    if c.kern == "linv_cov":
        VA = leading_V(Xq[:, :Ma].contiguous() if c.per_task else Xq[:Ma].contiguous())
        arr["VA"] = VA.cpu().numpy()
        mu, var, cov = _out(device, T, M), _out(device, T, M), _out(device, T, Ma, M)
        _ok(lib.scaml_posterior_linv_cov_f64(_p(Xq), _p(X), _p(theta), _p(Linv), _p(alpha), _p(ym), _p(ysd), _p(npts), _p(VA), T, N, M, Ma, D,
                                             c.kind, _p(mu), _p(var), _p(cov), flags, stream), "scaml_posterior_linv_cov_f64")
        return inp, arr, dict(mu=_take(mu, T), var=_take(var, T), cov=_take(cov, T))
    assert c.kern == "grad"
    Xa = VA = cov = None
    if Ma:
        Xa = _dev(inp["Xa"], device)
        VA = leading_V(Xa)
        arr["VA"] = VA.cpu().numpy()
        cov = _out(device, T, Ma, 16 * M)
    mu, var = _out(device, T, M, 16), _out(device, T, M, 16)
    _ok(lib.scaml_posterior_linv_grad_f64(_p(Xq), _p(Xa), _p(X), _p(theta), _p(Linv), _p(alpha), _p(ym), _p(ysd), _p(npts), _p(VA), T, N, M, Ma, D,
                                          c.kind, _p(mu), _p(var), _p(cov), 0, stream), "scaml_posterior_linv_grad_f64")
    got = dict(mu=_take(mu, T), var=_take(var, T))
    if Ma:
        got["cov"] = _take(cov, T)
    return inp, arr, got


@pytest.mark.parametrize("case", CASES, ids=B.case_id)
def test_posterior_within_its_forward_error_bound(case, device):
    """Every output element of every task within its bound (tests/_posterior_bounds.py states the model); rows >= n_t of V and the
    GRAD columns past D exactly zero; nothing written outside the outputs; n_t = 0 gives the prior exactly; a query point with a
    NaN coordinate gives NaN in its own mu / var / cov and leaves the other queries of its strip within their bounds (its column of
    V is NaN from the substitution kernel and unspecified from the explicit-inverse pass, include/scaml_gp.h (5) / (5c))."""
    inp, arr, got = _run(case, device)
    for t in range(case.T):
        B.check_task(case, inp, arr, t, {k: v[t] for k, v in got.items()}, v_nan=case.kern == "subst")
    for key, (err, cap) in sorted(B.RATIOS.items()):
        if key[0] == case.kern and key[1] == ("rbf" if case.kind == B.KIND_RBF else "matern"):
            print(f"{B.case_id(case)} {key[2]}: largest error / bound so far {err:.3e}, largest bound / scale {cap:.3e}")
