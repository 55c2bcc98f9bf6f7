"""CPU checks of the P-variable box instance of the device L-BFGS (csrc/gp_qacqf_opt.h: the optimiser step of scaml_qacqf_opt_f64 with
its slot table, and the gather of a round) through a single-threaded host build of the same source
(tests/host_emul/qacqf_opt_emul.cpp: test infrastructure, never part of the library).  The state machine of ONE start is
``hyper.batched_lbfgs(bounds=...)`` run on that start alone: fed the same (f, g) it has the same iteration count, evaluation count,
stop reason and -- the sums run in the same order, no product is contracted -- the same accepted points, bit for bit.  What only
the device has (two variables per lane, the lane broadcasts across the two) is tests/test_qacqf_opt_step_gpu.py's."""
import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests._host_emul import ptr
from tests._qacqf_opt_cases import F64, FAILED, RUNNING, accepted_points, coupled_hartmann, drive, host_alone, load_emul, quadratic


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return load_emul(tmp_path_factory)


def _same_as_host(emul, fun, x0, bounds, **kw):
    for b in range(x0.shape[0]):
        fun_b = (lambda x, idx=None, b=b: fun(x, [b]))
        ref, path, reason = host_alone(lambda x: fun_b(x), x0[b:b + 1], bounds, **kw)
        res = drive(emul, fun_b, x0[b:b + 1].numpy(), bounds=tuple(np.asarray(v) for v in bounds), **kw)
        assert res["stats"][0, :3].tolist() == [ref.n_iter, ref.n_eval, reason], (b, res["stats"][0].tolist(), ref.n_iter, ref.n_eval, reason)
        pts = accepted_points(res)
        assert len(pts) == len(path), (b, len(pts), len(path))
        for (it, xr, _, _), xe in zip(path, pts):
            np.testing.assert_array_equal(xe, xr.numpy(), err_msg=f"start {b}, iteration {it}")
        np.testing.assert_array_equal(res["x"][0], ref.x[0].numpy())
        if reason != FAILED:
            assert res["f"][0] == -float(ref.f[0])      # the maximised value at the accepted point


@pytest.mark.parametrize("P", [1, 24, 63, 64, 65, 120, 128])
def test_iterates_match_the_host_optimiser_on_the_separable_quadratic(emul, P):
    fun, x0 = quadratic(P, 3)
    _same_as_host(emul, fun, x0, (0.0, 1.0), max_iter=200, gtol=1e-10, ftol=0.0)
    res = drive(emul, fun, x0.numpy(), gtol=1e-10, ftol=0.0)
    assert (res["x"] >= 0.0).all() and (res["x"] <= 1.0).all()


def test_iterates_match_the_host_optimiser_on_the_coupled_hartmann_blocks(emul):
    fun, x0 = coupled_hartmann(4)
    _same_as_host(emul, fun, x0, (0.0, 1.0), max_iter=60)
    # (P,) bounds
    lo, hi = torch.full((24,), 0.1, dtype=F64), torch.linspace(0.6, 1.2, 24, dtype=F64)
    _same_as_host(emul, fun, x0[:2], (lo, hi), max_iter=40)


def test_a_start_outside_the_box_is_projected(emul):
    fun, x0 = quadratic(65, 3)
    res = drive(emul, fun, x0.numpy(), gtol=1e-10, ftol=0.0)
    assert (x0[-1] < 0).any() and (x0[-1] > 1).any()
    np.testing.assert_array_equal(res["asked"][0][1][2], x0[-1].clamp(0.0, 1.0).numpy())   # the first point evaluated is the projected start


def test_a_nan_start_fails_with_status_4(emul):
    fun, x0 = quadratic(65, 3)
    x0[1, 64] = float("nan")
    res = drive(emul, fun, x0.numpy(), gtol=1e-10, ftol=0.0)
    assert res["stats"][1, :3].tolist() == [0, 1, FAILED] and res["f"][1] == -np.inf
    clean = drive(emul, fun, np.nan_to_num(x0.numpy(), nan=0.5), gtol=1e-10, ftol=0.0)
    for b in (0, 2):   # the other starts are what they are without it
        np.testing.assert_array_equal(res["x"][b], clean["x"][b])
        assert res["stats"][b].tolist() == clean["stats"][b].tolist()


@pytest.mark.parametrize("fill", [0.0, np.nan])
def test_chunking_does_not_change_the_state(emul, fill):
    fun, x0 = coupled_hartmann(5)
    kw = dict(max_iter=30, history=4, state_fill=fill)
    one = drive(emul, fun, x0.numpy(), per_call=1, **kw)
    assert len(set(one["stats"][:, 1].tolist())) > 1          # the starts stop at different rounds
    for per_call in (3, 1 + 30 * 20):
        res = drive(emul, fun, x0.numpy(), per_call=per_call, **kw)
        for k in ("x", "f", "stats", "state"):
            np.testing.assert_array_equal(res[k], one[k], err_msg=k)
        if fill == 0.0:
            assert res["state"].tobytes() == one["state"].tobytes()


@pytest.mark.parametrize("per_call", [1, 3])
def test_compaction_leaves_every_start_the_bytes_of_the_run_that_never_compacts(emul, per_call):
    fun, x0 = coupled_hartmann(5)
    kw = dict(max_iter=30, history=4, per_call=per_call)
    plain = drive(emul, fun, x0.numpy(), **kw)
    comp = drive(emul, fun, x0.numpy(), compact=True, **kw)
    assert len(comp["tables"][-1]) < 5                         # starts did leave the table
    for table in comp["tables"][1:]:
        assert all(plain["stats"][b, 1] > 0 for b in table)
    assert comp["state"].tobytes() == plain["state"].tobytes()
    for k in ("x", "f", "stats"):
        np.testing.assert_array_equal(comp[k], plain[k], err_msg=k)
    # a stopped start is asked for nothing after the chunk in which it stopped
    asked = np.zeros(5, dtype=int)
    for slots, _ in comp["asked"]:
        asked[slots] += 1
    assert (asked >= comp["stats"][:, 1]).all() and (asked - comp["stats"][:, 1] < per_call).all()


def test_a_start_absent_from_the_table_is_not_touched(emul):
    fun, x0 = coupled_hartmann(5)
    res = drive(emul, fun, x0.numpy(), subset=[0, 3, 4], max_iter=20, state_fill=7.0, out_fill=-3.0)
    for b in (1, 2):
        assert (res["state"][b] == 7.0).all() and (res["x"][b] == -3.0).all() and res["f"][b] == -3.0 and (res["stats"][b] == -3).all()
    full = drive(emul, fun, x0.numpy(), max_iter=20)
    for b in (0, 3, 4):
        np.testing.assert_array_equal(res["x"][b], full["x"][b])
        assert res["stats"][b].tolist() == full["stats"][b].tolist() and res["stats"][b, 2] != RUNNING


def test_a_reversed_table_gives_the_same_result_per_start(emul):
    fun, x0 = quadratic(65, 4)
    kw = dict(max_iter=40, gtol=1e-10, ftol=0.0, per_call=3)
    fwd = drive(emul, fun, x0.numpy(), **kw)
    for compact in (False, True):
        rev = drive(emul, fun, x0.numpy(), reverse=True, compact=compact, **kw)
        assert rev["tables"][0].tolist() == [3, 2, 1, 0]
        assert rev["state"].tobytes() == fwd["state"].tobytes()
        for k in ("x", "f", "stats"):
            np.testing.assert_array_equal(rev[k], fwd[k], err_msg=k)


def test_python_state_stride_matches_header(emul):
    from scamlgp_amd import ops

    assert emul.emul_qacqf_opt_max_p() == 128
    for P in (1, 15, 63, 64, 65, 120, 128):
        for history in range(1, 17):
            assert ops.studies_acqf_opt_state_doubles(P, history) == emul.emul_qacqf_opt_state_doubles(P, history)


@pytest.mark.parametrize("n,Mq,D,extra", [(1, 1, 1, 1), (5, 6, 3, 2), (12, 1, 2, 4), (1, 7, 15, 0), (9, 16, 6, 8)])
def test_the_gather_is_the_four_concatenations(emul, n, Mq, D, extra):
    """column 0 of every point's 16 of mu_g, var_g and of the training rows of cov_g behind the training block; the points behind
    the training inputs (ScaMLGP.joint_acqf_inputs' four torch.cat)."""
    gen = torch.Generator().manual_seed(n * 100 + Mq)
    r = lambda *s: torch.rand(*s, dtype=F64, generator=gen)   # noqa: E731
    mu_g, var_g, cov_g, Xq = r(Mq * 16), r(Mq * 16), r(n + extra, Mq * 16), r(Mq, D)
    mu_t, var_t, cov_tt, Xt = r(n), r(n), r(n, n), r(n, D)
    want = dict(cov_s=torch.cat([cov_tt, cov_g[:n].reshape(n, Mq, 16)[:, :, 0]], 1), mean_s=torch.cat([mu_t, mu_g.reshape(Mq, 16)[:, 0]]),
                var_s=torch.cat([var_t, var_g.reshape(Mq, 16)[:, 0]]), xall=torch.cat([Xt, Xq], 0))
    got = dict(mean_s=np.full(n + Mq, np.nan), var_s=np.full(n + Mq, np.nan), cov_s=np.full((n, n + Mq), np.nan), xall=np.full((n + Mq, D), np.nan))
    ins = [np.ascontiguousarray(t.numpy()) for t in (mu_g, var_g, cov_g, Xq, mu_t, var_t, cov_tt, Xt)]
    outs = [got[k] for k in ("mean_s", "var_s", "cov_s", "xall")]
    emul.emul_qacqf_opt_gather(*[ptr(a) for a in ins], *[ptr(a) for a in outs], n, Mq, D, 0)
    # the round's launch writes the right-hand parts only
    assert np.isnan(got["mean_s"][:n]).all() and np.isnan(got["cov_s"][:, :n]).all() and np.isnan(got["xall"][:n]).all()
    np.testing.assert_array_equal(got["mean_s"][n:], want["mean_s"][n:].numpy())
    emul.emul_qacqf_opt_gather(*[ptr(a) for a in ins], *[ptr(a) for a in outs], n, Mq, D, 1)
    for k in got:
        np.testing.assert_array_equal(got[k], want[k].numpy(), err_msg=k)
