"""CPU checks of the value-only joint q-point acquisition kernel (csrc/gp_qacqf.h: qa_batch<true, true>, the body of
scaml_target_qacqf_value_kernel, include/scaml_gp.h (7r)) and of the column map of its value layout (csrc/gp_qacqf_columns.h) through
a host build of the same sources (tests/host_emul/qacqf_value_emul.cpp).

  the column map for q = 1 .. 8: injective, the padding columns its complement, the Python helper equal to the header's;
  (7r) against the host builds of (7p) and (7q) on the SAME numbers fed in both layouts: value, jitter and info bit for bit (the
  padding columns of the value layout hold NaN here: nothing of them is read);
  (7r) against torch fp64 of the definition (tests/_qacqf_ref.py) at 1e-9 max|ref| -- the figure of tests/test_qacqf_emul.py, with its
  estimate q^2 u cond = 7e-11 at q = 8, cond = 1e4 --, on joint posteriors from that file's ``tail_inputs`` recipe (cond(Sigma) = 100
  by construction, asserted <= 1e4 with the tie and kink margins on the reference alone), no sample left out;
  the NaN rules and the LDS footprints at the limits.
Measured worst ratios: profiles/qacqf_value_notes.md."""
import ctypes
import math

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from scamlgp_amd import ops
from tests import _qacqf_ref as R
from tests._host_emul import DP, IP, build, ptr as _p
from tests.test_qacqf_emul import Problem, run_batch, tail_inputs
from tests.test_qacqf_pending_emul import acqf_param, pending_inputs, pending_problem, run_pending

NAN = float("nan")
_I, _F = ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """(the value-only build, (7q)'s build, (7p)'s build)"""
    lib = build(tmp_path_factory, "qacqf_value_emul")
    lib.emul_qacqf_value.restype = _I
    lib.emul_qacqf_value.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 8 + [_I, _F] + [_I] * 8 + [DP, DP, IP]
    for f in (lib.emul_qav_column, lib.emul_qav_columns):
        f.restype = _I
    lib.emul_qav_column.argtypes, lib.emul_qav_columns.argtypes = [_I] * 3, [_I] * 2
    lib.emul_qav_batch_of.restype, lib.emul_qav_batch_of.argtypes = _I, [_I] * 4
    lib.emul_qacqf_value_lds_doubles.restype, lib.emul_qacqf_value_lds_doubles.argtypes = ctypes.c_longlong, [_I] * 4
    lib.emul_posterior_linv_lds_doubles.restype, lib.emul_posterior_linv_lds_doubles.argtypes = ctypes.c_longlong, [_I] * 2
    lib.emul_qacqf_value_plan.restype, lib.emul_qacqf_value_plan.argtypes = None, [_I] * 5 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.emul_posterior_jointv_plan.restype, lib.emul_posterior_jointv_plan.argtypes = None, [_I] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    pend = build(tmp_path_factory, "qacqf_pending_emul")
    pend.emul_qacqf_pending.restype = _I
    pend.emul_qacqf_pending.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 11 + [_I, _F] + [_I] * 7 + [DP, DP, DP, IP]
    ref = build(tmp_path_factory, "qacqf_emul")
    ref.emul_qacqf.restype = _I
    ref.emul_qacqf.argtypes = [DP] * 5 + [_F, _F, IP] + [DP] * 7 + [_I, _F] + [_I] * 6 + [DP, DP, DP, IP]
    return lib, pend, ref


# ---- the column map ---------------------------------------------------------------------------------------------------------------
PAD_PER_STRIP = {1: 0, 2: 0, 3: 1, 4: 0, 5: 1, 6: 4, 7: 2, 8: 0}


@pytest.mark.parametrize("q", range(1, 9))
def test_column_map(emul, q):
    lib = emul[0]
    bps = 16 // q
    assert 16 - bps * q == PAD_PER_STRIP[q]
    for B in sorted({1, bps - 1, bps, bps + 1, 3 * bps} - {0}):
        Mp = lib.emul_qav_columns(B, q)
        assert Mp == 16 * -(-B // bps) == ops.qacqf_value_columns(B, q)
        cols = [[lib.emul_qav_column(b, j, q) for j in range(q)] for b in range(B)]
        flat = [c for row in cols for c in row]
        assert len(set(flat)) == B * q and min(flat) >= 0 and max(flat) < Mp            # injective, inside the Mp columns
        assert all(row[j] == row[0] + j and row[0] // 16 == row[-1] // 16 for row in cols for j in range(q))   # consecutive, no batch straddles a strip
        assert torch.equal(ops.qacqf_value_column_map(B, q), torch.tensor(cols, dtype=torch.int64))
        # the padding columns are the complement, and a column's batch is the inverse of the map
        owner = {c: b for b, row in enumerate(cols) for c in row}
        for c in range(Mp):
            assert lib.emul_qav_batch_of(c // 16, c % 16, q, B) == owner.get(c, -1), (B, q, c)
        X = torch.arange(B * q * 2, dtype=torch.float64).reshape(B, q, 2) + 1.0
        packed = ops.qacqf_value_pack(X)
        assert packed.shape == (Mp, 2) and torch.equal(packed[flat], X.reshape(-1, 2))
        pad = sorted(set(range(Mp)) - set(flat))
        assert bool((packed[pad] == 0.5).all())


# ---- the same numbers in both layouts ----------------------------------------------------------------------------------------------
def to_value_layout(inp, B, q, rows, fill=NAN):
    """The arrays of (7p) / (7q) (``kernel_inputs`` / ``pending_inputs``: a column per point, cov_g with 16 columns per point) in the
    value layout: a point's column from the map, its covariance column 16 j of cov_g, ``fill`` in the padding columns."""
    cols = ops.qacqf_value_column_map(B, q).reshape(-1)
    Mq, Mp = B * q, ops.qacqf_value_columns(B, q)
    out = {k: v for k, v in inp.items() if isinstance(v, torch.Tensor)}

    def spread(a):   # (..., Mq) -> (..., Mp)
        z = torch.full(a.shape[:-1] + (Mp,), fill, dtype=torch.float64)
        z[..., cols] = a.detach()
        return z
    for k in ("Knq", "Z", "mean_q", "var_q"):
        out[k] = spread(inp[k])
    out["cov_s"] = spread(inp["cov_g"].detach().reshape(rows, Mq, 16)[:, :, 0])
    out["Xq"] = spread(inp["Xq"].detach().T).T.contiguous()
    return out


def run_value(lib, v, m, s, B, q, p, eps, acqf, par, kind, info=None):
    a = {k: np.ascontiguousarray(t.detach().numpy(), dtype=np.float64) for k, t in v.items() if isinstance(t, torch.Tensor)}
    n, Mp = a["Knq"].shape
    D = a["Xq"].shape[1]
    value, jit = np.full(B, 7.0), np.full(B, 7.0)
    info_out = np.full(B, 7, dtype=np.int32)
    e = np.ascontiguousarray(eps.numpy())
    pend = [_p(a[k]) if p > 0 else None for k in ("Xp", "Zp", "mu_p", "Sigma_pp")]
    rc = lib.emul_qacqf_value(_p(a["Knq"]), _p(a["Z"]), _p(a["alpha"]), _p(a["mean_q"]), _p(a["var_q"]), m, s,
                              _p(info) if info is not None else None, _p(a["cov_s"]), _p(a["Xq"]), _p(a["theta"]), _p(e), *pend, acqf, par,
                              n, Mp, B, q, p, eps.shape[0], D, kind, _p(value), _p(jit), _p(info_out))
    assert rc == 0
    return torch.from_numpy(value), torch.from_numpy(jit), torch.from_numpy(info_out)


def with_hard_batches(prob, inp, q):
    """Batch 1 made to need a rung of the ladder and batch 2 made to fail all four, through var_q (the diagonal of Sigma) alone, so
    that the same numbers go into both layouts: the LAST pivot of batch 1 is moved to -5e-8 (it fails at 0 and at 1e-8; a jitter j
    raises it by at least j, so 1e-7 passes), the first pivot of batch 2 to about -s^2."""
    inp = dict(inp)
    vq = inp["var_q"].detach().clone()
    with torch.no_grad():
        _, Sigma = prob.joint(prob.X[1])
    C = torch.linalg.cholesky(Sigma)
    vq[1 * q + q - 1] -= (float(C[-1, -1]) ** 2 + 5e-8) / prob.s ** 2
    vq[2 * q] = -1.0
    inp["var_q"] = vq
    return inp


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
@pytest.mark.parametrize("S", [1, 7, 300, 512])
@pytest.mark.parametrize("q", [1, 2, 3, 8])
def test_bits_of_7p(emul, q, S, acqf):
    lib, _, ref = emul
    B, D, n, kind = 4, 3, 9, (q + S) % 2
    prob = Problem(B, q, D, n, kind, seed=13 * q + S + acqf)
    eps = torch.randn(S, q, dtype=torch.float64, generator=torch.Generator().manual_seed(q + S))
    inp = with_hard_batches(prob, prob.kernel_inputs(), q)
    par = acqf_param(prob, acqf)
    v0, _, jit0, info0 = run_batch(ref, inp, prob, eps, acqf, par)
    assert info0.tolist() == [0, 0, 1, 0] and float(jit0[0]) == 0.0 and float(jit0[1]) > 0.0 and float(jit0[3]) == 0.0
    assert math.isnan(float(v0[2])) and bool(torch.isfinite(v0[[0, 1, 3]]).all())
    v, jit, info = run_value(lib, to_value_layout(inp, B, q, n + q), prob.m, prob.s, B, q, 0, eps, acqf, par, kind)
    for got, want in ((v, v0), (jit, jit0), (info, info0)):
        assert np.array_equal(got.numpy(), want.numpy(), equal_nan=True)
    assert np.array_equal(np.isnan(v.numpy()), np.isnan(v0.numpy()))


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
@pytest.mark.parametrize("q,p,D,n,S,kind", [(2, 1, 2, 17, 300, 1), (1, 7, 15, 17, 512, 0), (3, 5, 15, 88, 7, 0)])
def test_bits_of_7q(emul, q, p, D, n, S, kind, acqf):
    lib, pend, _ = emul
    B = 7   # q = 3: two strips, the second with two batches
    prob = pending_problem(B, q, p, D, n, kind, seed=11 * (q + p) + n + acqf)
    eps = torch.randn(S, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(q + p + S))
    inp = pending_inputs(prob, q, p)
    vq = inp["var_q"].detach().clone()
    vq[2 * q] = -1.0   # batch 2 fails on every rung
    inp["var_q"] = vq
    par = acqf_param(prob, acqf)
    v0, _, jit0, info0 = run_pending(pend, inp, prob, q, p, eps, acqf, par)
    assert info0.tolist() == [0, 0, 1, 0, 0, 0, 0] and math.isnan(float(v0[2])) and int(torch.isfinite(v0).sum()) == B - 1
    v, jit, info = run_value(lib, to_value_layout(inp, B, q, n + p + q), prob.m, prob.s, B, q, p, eps, acqf, par, kind)
    for got, want in ((v, v0), (jit, jit0), (info, info0)):
        assert np.array_equal(got.numpy(), want.numpy(), equal_nan=True)


# ---- against the definition in torch fp64 -------------------------------------------------------------------------------------------
WORST = {"ratio": 0.0}


def _ratio(got, ref, what):
    """|got - ref| against 1e-9 max|ref|; the ratio is printed before it is asserted."""
    tol = 1e-9 * float(ref.abs().max())
    err = float((got - ref).abs().max())
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: err {err:.3e} tol {tol:.3e} ratio {ratio:.3g} (worst so far {WORST['ratio']:.3g})")
    assert ratio <= 1.0, what


def inputs_of_joints(joints, q, D, kind, seed):
    """Value-layout inputs of (7r) under which batch b's joint posterior is EXACTLY the given (mu_b, Sigma_b), up to the rounding of one
    sum: one training point with Knq = Z = 0 (nothing is subtracted), s = 1, m = 0, mean_q = mu, var_q = diag(Sigma), and the mate rows
    of cov_s = Sigma_jk - os k_t(x_j, x_k) for random points x."""
    B, n = len(joints), 1
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(B, q, D, dtype=torch.float64, generator=g)
    theta = torch.cat([0.5 + torch.rand(D, dtype=torch.float64, generator=g), torch.tensor([1.3, 0.04], dtype=torch.float64)])
    cols, Mp = ops.qacqf_value_column_map(B, q), ops.qacqf_value_columns(B, q)
    out = dict(Knq=torch.zeros(n, Mp, dtype=torch.float64), Z=torch.zeros(n, Mp, dtype=torch.float64), alpha=torch.ones(n, dtype=torch.float64),
               mean_q=torch.full((Mp,), NAN, dtype=torch.float64), var_q=torch.full((Mp,), NAN, dtype=torch.float64),
               cov_s=torch.full((n + q, Mp), NAN, dtype=torch.float64), Xq=ops.qacqf_value_pack(X), theta=theta)
    for b, (mu, Sigma) in enumerate(joints):
        K = R.kernel(X[b], X[b], theta, kind)
        out["mean_q"][cols[b]] = mu
        out["var_q"][cols[b]] = torch.diagonal(Sigma)
        out["cov_s"][n:, cols[b]] = (Sigma - K).T   # row n + k, column of point j: P_jk - os k_t(x_j, x_k)
    return out


@pytest.mark.parametrize("acqf", [R.ACQF_EI, R.ACQF_UCB])
@pytest.mark.parametrize("S", [1, 7, 300, 512])
@pytest.mark.parametrize("q", [1, 2, 3, 8])
def test_against_the_definition(emul, q, S, acqf):
    lib = emul[0]
    B, D, kind = 16 // q + 1, 2, (q + S) % 2   # (two strips)
    eps = tail_inputs(q, S, acqf, seed=1000 * q + S + acqf)[2]
    par = None
    joints = []
    for b in range(B):
        mu, Sigma, _, pb = tail_inputs(q, S, acqf, seed=1000 * q + S + acqf + 50 * b)
        par = pb if par is None else max(par, pb)   # (qEI: best_f above every batch's means)
        joints.append((mu, Sigma))
    v_ref = []
    for mu, Sigma in joints:
        R.assert_well_posed(mu, Sigma, eps, acqf, par)
        v_ref.append(R.mc_value(mu, Sigma, eps, acqf, par))
    v_ref = torch.stack(v_ref)
    assert float(v_ref.abs().min()) > 0
    v, jit, info = run_value(lib, inputs_of_joints(joints, q, D, kind, seed=q + S), 0.0, 1.0, B, q, 0, eps, acqf, par, kind)
    assert not info.any() and not jit.any()
    _ratio(v, v_ref, f"q={q} S={S} acqf={acqf} value / definition")


def test_against_the_definition_with_points_pending(emul):
    """(q, p) = (3, 5): the 8 x 8 joint of the recipe, its leading 3 entries the moving points (given through the value layout), the
    other 5 the pending set (mixed block through rows n + k of cov_s, Zp = 0; Sigma_pp, mu_p as given)."""
    lib = emul[0]
    q, p, S, D, kind, n = 3, 5, 300, 2, 1, 1
    for acqf in (R.ACQF_EI, R.ACQF_UCB):
        mu, Sigma, eps, par = tail_inputs(q + p, S, acqf, seed=77 + acqf)
        R.assert_well_posed(mu, Sigma, eps, acqf, par)
        v_ref = R.mc_value(mu, Sigma, eps, acqf, par).reshape(1)
        inp = inputs_of_joints([(mu[:q], Sigma[:q, :q])], q, D, kind, seed=5)
        Xp = torch.rand(p, D, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
        cols = ops.qacqf_value_column_map(1, q)[0]
        mates = inp["cov_s"][n:]
        mixed = torch.full((p, mates.shape[1]), NAN, dtype=torch.float64)
        mixed[:, cols] = Sigma[q:, :q] - R.kernel(Xp, inp["Xq"][cols], inp["theta"], kind)   # row n + k, column of point j
        inp["cov_s"] = torch.cat([inp["cov_s"][:n], mixed, mates], 0)
        inp.update(Xp=Xp, Zp=torch.zeros(n, p, dtype=torch.float64), mu_p=mu[q:].clone(), Sigma_pp=Sigma[q:, q:].clone())
        v, jit, info = run_value(lib, inp, 0.0, 1.0, 1, q, p, eps, acqf, par, kind)
        assert not info.any() and not jit.any()
        _ratio(v, v_ref, f"q={q} p={p} S={S} acqf={acqf} value / definition")


# ---- NaN rules, footprints -----------------------------------------------------------------------------------------------------------
def test_nan_rules(emul):
    lib, pend, _ = emul
    B, q, p = 6, 3, 2   # (five batches in the first strip, one in the second)
    prob = pending_problem(B, q, p, 2, 5, 0, seed=2)
    eps = torch.randn(16, q + p, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    inp = pending_inputs(prob, q, p)
    val = to_value_layout(inp, B, q, 5 + p + q)
    run = lambda a, acqf=R.ACQF_EI, par=0.5, info=None: run_value(lib, a, prob.m, prob.s, B, q, p, eps, acqf, par, 0, info)   # noqa: E731
    v0, jit0, info0 = run(val)
    assert bool(torch.isfinite(v0).all()) and not info0.any()
    assert torch.equal(v0, run_pending(pend, inp, prob, q, p, eps, R.ACQF_EI, 0.5)[0])
    # two calls: bit for bit
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(run(val), (v0, jit0, info0)))
    # a failed target factorisation: everything is NaN
    v, jit, info = run(val, info=np.ones(1, dtype=np.int32))
    assert bool(torch.isnan(v).all()) and bool(torch.isnan(jit).all()) and bool((info == 1).all())
    cols = ops.qacqf_value_column_map(B, q)
    # a NaN / infinite coordinate of a batch's own point: that batch is NaN, the others are bit for bit what they were
    for b, bad_value in ((1, NAN), (5, float("inf"))):
        bad = dict(val)
        bad["Xq"] = val["Xq"].clone()
        bad["Xq"][cols[b, 1], 1] = bad_value
        v = run(bad)[0]
        assert math.isnan(float(v[b]))
        assert all(float(v[o]) == float(v0[o]) for o in range(B) if o != b)
    # a NaN in a batch's own inputs
    for name, idx in (("Knq", (3, int(cols[4, 0]))), ("Z", (0, int(cols[4, 2]))), ("mean_q", (int(cols[4, 1]),)), ("var_q", (int(cols[4, 0]),)),
                      ("cov_s", (5 + p + 1, int(cols[4, 2]))), ("cov_s", (5 + 1, int(cols[4, 0])))):
        bad = dict(val)
        bad[name] = val[name].clone()
        bad[name][idx] = NAN
        v = run(bad)[0]
        assert math.isnan(float(v[4])), name
        assert all(float(v[o]) == float(v0[o]) for o in range(B) if o != 4), name
    # a NaN anywhere in the shared pending set: every batch is NaN (Sigma_pp: an entry of the upper triangle, which is not read)
    for name, idx in (("Xp", (1, 0)), ("Zp", (4, 1)), ("mu_p", (0,)), ("Sigma_pp", (0, 1))):
        bad = dict(val)
        bad[name] = val[name].detach().clone()
        bad[name][idx] = NAN
        assert bool(torch.isnan(run(bad, R.ACQF_UCB, 4.0)[0]).all()), name


def test_plans_and_footprints(emul):
    lib = emul[0]
    out = (ctypes.c_longlong * 3)()
    for n, q, p in ((88, 3, 5), (88, 1, 7), (88, 7, 1), (88, 8, 0), (95, 1, 0)):   # n + p + q = 96, q + p <= 8
        lib.emul_qacqf_value_plan(5, n, q, p, 512, out)
        assert (out[0], out[1]) == (5, 256)
        assert out[2] == lib.emul_qacqf_value_lds_doubles(n, q, p, 512) and out[2] * 8 <= 160 * 1024   # the largest shapes fit the LDS
    # the source pass: the Gram tile's image behind (5c')'s carve, a workgroup per (task rounded up to 8, strip)
    for N, D in ((512, 15), (512, 6), (96, 15), (32, 2)):
        lib.emul_posterior_jointv_plan(3, N, D, 48, out)
        assert (out[0], out[1]) == (8 * 3, 512)
        assert out[2] == lib.emul_posterior_linv_lds_doubles(N, D) + 256 and out[2] * 8 <= 160 * 1024
    # N = 96 with Ma = 89 and N = 32 with Ma = 17: nas = NB leading images fill the K_*^T strip, the Gram image lies behind it
    for N, Ma in ((96, 89), (32, 17)):
        nb, nas = (N + 15) // 16, (Ma + 15) // 16
        assert nas == nb and (nas + 1) * 256 == nb * 256 + 256
