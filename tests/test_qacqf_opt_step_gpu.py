"""scaml_qacqf_opt_step_f64 (include/scaml_gp.h (7t)) on the MI355X next to the single-threaded host build of the same header
(tests/host_emul/qacqf_opt_emul.cpp), round by round, on (f, g) computed on the host and copied in.

The claim is BIT EQUALITY of every state word after every round.  Both sides get identical inputs; the arithmetic is +, -, x, /, sqrt,
min and max, all correctly rounded in fp64; contraction is off; the order of additions is the same (variable 0 first, ascending: on
the device lanes 0 .. 63 of a lane's first variable, then of its second).  What only the device has -- two variables per lane, the
broadcasts across the two, the slot table in flight -- is what can break it; the first differing word and its round are printed."""
import numpy as np
import pytest
import torch

from scamlgp_amd import ops
from tests._host_emul import ptr
from tests._qacqf_opt_cases import RUNNING, box, coupled_hartmann, load_emul, quadratic

pytestmark = pytest.mark.gpu
OPTS = dict(max_iter=15, history=4, max_ls=20, gtol=1e-9, ftol=0.0, c1=1e-4)
B = 5


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return load_emul(tmp_path_factory)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_same_bits(what, rnd, dev, host):
    d, h = _bits(dev).reshape(-1), _bits(host).reshape(-1)
    bad = np.nonzero(d != h)[0]
    if bad.size:
        w = int(bad[0])
        print(f"{what}: round {rnd}: {bad.size} words differ, the first is word {w}: device {np.asarray(dev).reshape(-1)[w]!r} "
              f"({int(d[w]):#018x}), host {np.asarray(host).reshape(-1)[w]!r} ({int(h[w]):#018x})")
    assert bad.size == 0, (what, rnd, int(bad[0]))


def _lockstep(emul, device, fun, x0, per_call=None, reverse=False, subset=None, gtol=None):
    """Both sides from the same starts, one evaluation at a time; every array compared after every launch.  ``per_call``: the stopped
    starts leave the table every so many rounds (None: the table never changes)."""
    opts = OPTS if gtol is None else dict(OPTS, gtol=gtol)
    x0 = np.ascontiguousarray(x0.numpy(), dtype=np.float64)
    nB, P = x0.shape
    lo, hi = box((0.0, 1.0), P)
    H = opts["history"]
    stride = ops.studies_acqf_opt_state_doubles(P, H)
    order = list(range(nB)) if subset is None else list(subset)
    slots = np.asarray(order[::-1] if reverse else order, dtype=np.int32)
    # host side (sentinel fill: what is not written must not be written on either side)
    h = dict(state=np.full((nB, stride), 3.0), Xq=np.zeros((nB, P)), x=np.full((nB, P), -7.0), f=np.full(nB, -7.0), stats=np.full((nB, 4), -7, dtype=np.int32),
             value=np.zeros(nB), grad=np.zeros((nB, P)))
    t = lambda a, dt=torch.float64: torch.from_numpy(np.array(a)).to(dt).to(device)   # noqa: E731
    d = dict(state=t(h["state"]), Xq=t(h["Xq"]), x=t(h["x"]), f=t(h["f"]), stats=t(h["stats"], torch.int32), x0=t(x0), lo=t(lo), hi=t(hi))

    def step(mode, value=None, grad=None):
        k = int(slots.shape[0])
        emul.emul_qacqf_opt_step(ptr(h["value"]), ptr(h["grad"]), ptr(slots), ptr(x0), ptr(lo), ptr(hi), ptr(h["state"]), ptr(h["Xq"]), ptr(h["x"]),
                                 ptr(h["f"]), ptr(h["stats"]), nB, k, P, mode, opts["max_iter"], H, opts["max_ls"], opts["gtol"], opts["ftol"], opts["c1"])
        ops.qacqf_opt_step(d["state"], mode, d["lo"], d["hi"], d["Xq"][:k], d["x"], d["f"], d["stats"], x0=d["x0"],
                           value=None if value is None else t(value), grad=None if grad is None else t(grad), slots=t(slots, torch.int32), **opts)

    def compare(rnd):
        k = int(slots.shape[0])
        _assert_same_bits("state", rnd, d["state"].cpu().numpy(), h["state"])
        _assert_same_bits("Xq", rnd, d["Xq"][:k].cpu().numpy(), h["Xq"][:k])
        _assert_same_bits("x", rnd, d["x"].cpu().numpy(), h["x"])
        _assert_same_bits("f", rnd, d["f"].cpu().numpy(), h["f"])
        np.testing.assert_array_equal(d["stats"].cpu().numpy(), h["stats"])

    step(0)
    compare(0)
    budget = 1 + opts["max_iter"] * opts["max_ls"]
    rnd, smallest = 0, int(slots.shape[0])
    while rnd < budget:
        rnd += 1
        k = int(slots.shape[0])
        pts = d["Xq"][:k].cpu().numpy()                    # what the DEVICE asks for (bit-equal to the host's: compared above)
        fv, gv = fun(torch.from_numpy(pts.copy()), slots.tolist())
        h["value"][:k], h["grad"][:k] = -fv.numpy(), -gv.numpy()
        step(1, h["value"][:k], h["grad"][:k])
        compare(rnd)
        running = [b for b in slots.tolist() if h["stats"][b, 2] == RUNNING]
        if not running:
            break
        if per_call is not None and rnd % per_call == 0 and len(running) < k:
            slots = np.asarray(running, dtype=np.int32)
            smallest = int(slots.shape[0])
            step(2)
            compare(rnd)
    return dict(state=d["state"].cpu().numpy(), x=d["x"].cpu().numpy(), f=d["f"].cpu().numpy(), stats=d["stats"].cpu().numpy(), rounds=rnd, smallest=smallest)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 120, 128])
def test_every_state_word_equals_the_host_build_on_the_separable_quadratic(emul, device, P):
    fun, x0 = quadratic(P, B)
    res = _lockstep(emul, device, fun, x0)
    print(f"P = {P}: {res['rounds']} rounds, status {res['stats'][:, 2].tolist()}, evaluations {res['stats'][:, 1].tolist()}")
    assert (res["stats"][:, 2] != RUNNING).all() and (res["x"] >= 0.0).all() and (res["x"] <= 1.0).all()


def test_every_state_word_equals_the_host_build_on_the_coupled_hartmann_blocks(emul, device):
    fun, x0 = coupled_hartmann(B)
    res = _lockstep(emul, device, fun, x0)
    print(f"P = 24: {res['rounds']} rounds, status {res['stats'][:, 2].tolist()}, evaluations {res['stats'][:, 1].tolist()}")
    assert (res["stats"][:, 2] != RUNNING).all()


@pytest.mark.parametrize("P", [65, 120])
def test_compaction_and_a_reversed_table_cross_the_slot_boundary_with_the_same_bytes(emul, device, P):
    # (gtol 1e-2: the starts converge at different rounds, 8 .. 12 evaluations, so that the table does shrink)
    fun, x0 = quadratic(P, B)
    plain = _lockstep(emul, device, fun, x0, gtol=1e-2)
    assert len(set(plain["stats"][:, 1].tolist())) > 1 and (plain["stats"][:, 2] == 1).all()
    for kw in (dict(per_call=3), dict(per_call=1, reverse=True), dict(reverse=True)):
        res = _lockstep(emul, device, fun, x0, gtol=1e-2, **kw)
        assert ("per_call" not in kw) or res["smallest"] < B, kw
        assert res["state"].tobytes() == plain["state"].tobytes(), kw
        for k in ("x", "f", "stats"):
            np.testing.assert_array_equal(res[k], plain[k], err_msg=f"{k} {kw}")


def test_a_start_absent_from_the_table_is_not_touched(emul, device):
    fun, x0 = quadratic(65, B)
    res = _lockstep(emul, device, fun, x0, subset=[4, 0, 2])
    for b in (1, 3):
        assert (res["state"][b] == 3.0).all() and (res["x"][b] == -7.0).all() and res["f"][b] == -7.0 and (res["stats"][b] == -7).all()


def test_a_nan_start_fails_and_the_others_do_not_see_it(emul, device):
    fun, x0 = quadratic(65, B)
    x0[1, 64] = float("nan")
    res = _lockstep(emul, device, fun, x0)
    assert res["stats"][1, :3].tolist() == [0, 1, 4] and res["f"][1] == -np.inf
    assert (res["stats"][[0, 2, 3, 4], 2] != 4).all()
