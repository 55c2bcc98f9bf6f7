"""The sixteen later instances of gp_posterior_linv_kernel -- the grouped GRAD pass (5e) / (5e') with atomic and with ordered sums,
the grouped value pass (5f) / (5f'), the joint GRAD pass (5g) and the joint value pass (5h) -- against the long-double reference of
tests/_posterior_variant_bounds.py, every output element of every task slot held to its a-priori bound (capped at 1e-8 of the
quantity's scale in its source task).  Every case is a chain: fit, L^-1 and the value pass that produces VA (and VQ) run on the
device, and the reference is fed those arrays as the device produced them.  Shapes: N = 17 / 32 / 129 / 144 / 272 / 512 (two blocks
and six idle waves, nas == NB, the first block of the second serpentine round, the vector loads, the third round, the limit), nine
task slots, group tables with padding entries, OWN task bases that overlap and leave the arrays, q = 1 .. 8 with and without
padding columns.  The output buffers hold a sentinel and one task slice more than the call may write: a whole guard slice stands
behind the last row and the last column of the last slot.  The ordered-sum instances are reached with
scaml_debug_grouped_ordered_sums (include/scaml_gp_debug.h)."""
import numpy as np
import pytest
import torch

from scamlgp_amd import _lib, ops
from tests import _posterior_variant_bounds as V
from tests._posterior_variant_bounds import CASES, SENTINEL

pytestmark = pytest.mark.gpu


def _dev(a, device, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _out(device, T, *shape):
    return torch.full((T + 1, *shape), SENTINEL, dtype=torch.float64, device=device)


def _take(buf, T):
    assert bool((buf[T] == SENTINEL).all()), "the call wrote past the last task slot's slice"
    return buf[:T].cpu().numpy()


@pytest.fixture
def ordered_sums():
    """Sets scaml_debug_grouped_ordered_sums and puts the value found at the first call back."""
    found = []

    def set_mode(mode):
        prev = _lib.lib.scaml_debug_grouped_ordered_sums(mode)
        found.append(prev)
        return prev

    yield set_mode
    if found:
        _lib.lib.scaml_debug_grouped_ordered_sums(found[0])


class _Chain:
    """Fit, L^-1 and the value passes of one case on the device; call() runs the case's entry point into fresh sentinel buffers."""

    def __init__(self, c, device):
        self.c, self.device = c, device
        self.lib, self.stream = _lib.lib, torch.cuda.current_stream().cuda_stream
        inp = self.inp = V.make_inputs(c)
        self.X, self.y, self.theta = (_dev(inp[k], device) for k in ("X", "y", "theta"))
        self.npts = _dev(inp["n_points"], device, torch.int32)
        self.ym, self.ysd = _dev(inp["y_mean"], device), _dev(inp["y_std"], device)
        fit = ops.gp_fit_fused(self.X, self.y, self.theta, c.kind, n_points=self.npts, want_linv=True)
        counts = [c.N] * c.Tsrc if inp["n_points"] is None else [int(v) for v in inp["n_points"]]
        assert not bool((fit["info"] != 0)[torch.tensor([n > 0 for n in counts], device=device)].any())
        self.alpha = fit["alpha"]
        self.Linv = ops.linv_batched(fit["L"], fit["Linv_diag"], n_points=self.npts)
        self.Xa = _dev(inp["Xa"], device)
        self.arr = dict(inp, alpha=self.alpha.cpu().numpy(), Linv=self.Linv.cpu().numpy())
        if c.grouped:
            self.VA = []
            for g in range(c.G):
                Vall = self.value_V(self.Xa[g, :c.Ma[g]].contiguous())      # (Tsrc, N, Ma_g): the group's slots pick their source tasks
                va = torch.zeros(c.T, c.N, c.Ma[g], dtype=torch.float64, device=device)
                for t in range(c.T):
                    src = V.source_of(c, g, t)
                    if src is not None:
                        va[t] = Vall[src]
                self.VA.append(va)
            self.VA_tab = torch.tensor([v.data_ptr() for v in self.VA], dtype=torch.int64, device=device)
            self.arr["VA"] = [v.cpu().numpy() for v in self.VA]
            self.group = torch.tensor(c.group, dtype=torch.int32, device=device)
            self.n_a = torch.tensor(c.Ma, dtype=torch.int32, device=device)
            self.task_base = torch.tensor(c.task_base, dtype=torch.int32, device=device) if c.own else None
        else:
            self.VA = self.value_V(self.Xa)
            self.arr["VA"] = self.VA.cpu().numpy()
        self.set_queries(inp["Xq"])

    def value_V(self, pts):
        """V of the points pts under every source task, from the existing value pass (5c)."""
        c, m = self.c, pts.shape[0]
        out = torch.empty(c.Tsrc, c.N, m, dtype=torch.float64, device=self.device)
        _lib.check_rc(self.lib.scaml_posterior_linv_f64(_p(pts), _p(self.X), _p(self.theta), _p(self.Linv), _p(self.alpha), _p(self.ym), _p(self.ysd),
                                                        _p(self.npts), c.Tsrc, c.N, m, c.D, c.kind, None, None, _p(out), 0, self.stream),
                      "scaml_posterior_linv_f64")
        return out

    def set_queries(self, Xq):
        self.Xq = _dev(Xq, self.device)
        if self.c.fam == "5g":
            self.VQ = self.value_V(self.Xq)
            self.arr["VQ"] = self.VQ.cpu().numpy()

    def call(self):
        c, lib, s = self.c, self.lib, self.stream
        W = 16 if c.grad else 1
        mu, var, cov = _out(self.device, c.T, c.M * W), _out(self.device, c.T, c.M * W), _out(self.device, c.T, c.rows, c.M * W)
        src = (_p(self.X), _p(self.theta), _p(self.Linv), _p(self.alpha), _p(self.ym), _p(self.ysd), _p(self.npts))
        if c.grouped:
            fn = {"5e": "scaml_posterior_linv_grad_grouped", "5f": "scaml_posterior_linv_grouped"}[c.fam[:2]] + ("_own_f64" if c.own else "_f64")
            args = (_p(self.Xq), _p(self.group), _p(self.Xa), _p(self.n_a), _p(self.VA_tab), *src, c.T, c.N, c.Mq, c.G, c.rows, c.D, c.kind,
                    _p(mu), _p(var), _p(cov))
            rc = getattr(lib, fn)(*args, *((_p(self.task_base), c.Tsrc) if c.own else ()), s)
        elif c.fam == "5g":
            fn = "scaml_posterior_linv_grad_joint_f64"
            rc = lib.scaml_posterior_linv_grad_joint_f64(_p(self.Xq), _p(self.Xa), *src, _p(self.VA), _p(self.VQ), c.T, c.N, c.Mq, c.Ma, c.q, c.D, c.kind,
                                                         _p(mu), _p(var), _p(cov), 0, s)
        else:
            fn = "scaml_posterior_linv_cov_joint_f64"
            assert c.M == lib.scaml_qacqf_value_columns(c.B, c.q)
            rc = lib.scaml_posterior_linv_cov_joint_f64(_p(self.Xq), _p(self.Xa), *src, _p(self.VA), c.T, c.N, c.M, c.Ma, c.B, c.q, c.D, c.kind,
                                                        _p(mu), _p(var), _p(cov), 0, s)
        _lib.check_rc(rc, fn)
        return dict(mu=_take(mu, c.T), var=_take(var, c.T), cov=_take(cov, c.T))

    def check(self, got, label=""):
        V.check_case(self.c, self.arr, got, label)


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)


@pytest.mark.parametrize("case", CASES, ids=V.case_id)
def test_variant_within_its_forward_error_bound(case, device, ordered_sums):
    """Every element of every task slot within its bound; rows a >= Ma_g of cov, and everything of a padding unit but its zeros in
    mu / var, untouched; the mate rows of a padding column of (5h) exact zeros; every other element written.  (5e) / (5e') with
    det: the same through the ordered-sum instance, whose two calls agree bit for bit in mu, var and cov and whose cov has the bits
    of the atomic instance's (both add the waves' tiles in a fixed order)."""
    ch = _Chain(case, device)
    assert ordered_sums(0) in (0, 1)
    got = ch.call()
    ch.check(got)
    if case.det:
        assert ordered_sums(1) == 0
        first, second = ch.call(), ch.call()
        assert ordered_sums(0) == 1
        assert _same_bits(first, second), "two calls of the ordered-sum instance differ"
        assert np.array_equal(first["cov"].view(np.int64), got["cov"].view(np.int64)), "cov of the ordered-sum instance differs from the atomic instance's"
        ch.check(first, " ordered")


# the query point that gets a NaN coordinate: a unit of a live group whose slots read real tasks; (5g) / (5h): point 1 of batch 1
NAN_POINT = {"5e": 3, "5e'": 1, "5f": 17, "5f'": 17, "5g": 4, "5h": 4}
NAN_CASES = [(f, det) for f in NAN_POINT for det in ((False, True) if f[:2] == "5e" else (False,))]


@pytest.mark.parametrize("fam,det", NAN_CASES, ids=[f + ("-ordered" if d else "") for f, d in NAN_CASES])
def test_nan_query_stays_in_its_own_outputs(fam, det, device, ordered_sums):
    """A NaN coordinate gives NaN in that point's own mu / var and column (GRAD: strip) of cov -- its mate rows included.  Every other
    element of cov has the bits of the clean call, every other mu / var is within its bound (bit-equal for the ordered sums).  Left
    out, as include/scaml_gp.h leaves them: the mate rows of the point's batch mates that pair them with it."""
    c = next(x for x in CASES if x.fam == fam and x.N == 129)
    ordered_sums(1 if det else 0)
    ch = _Chain(c, device)
    clean = ch.call()
    ch.check(clean)
    jn = NAN_POINT[fam]
    col = V.qav_column(jn // c.q, jn % c.q, c.q) if fam == "5h" else jn
    Xn = ch.inp["Xq"].copy()
    Xn[col, c.D - 1] = np.nan
    vq_clean = getattr(ch, "VQ", None)
    ch.set_queries(Xn)
    if vq_clean is not None:      # the other columns of VQ do not see the NaN; the reference keeps the clean call's arrays
        keep = [j for j in range(c.Mq) if j != jn]
        assert torch.equal(ch.VQ[:, :, keep], vq_clean[:, :, keep])
    ch.arr["Xq"], ch.arr["VQ"] = ch.inp["Xq"], None if vq_clean is None else vq_clean.cpu().numpy()
    got = ch.call()
    W = 16 if c.grad else 1
    own = np.zeros(c.M * W, dtype=bool)
    own[col * W:col * W + W] = True
    paired = np.zeros((c.rows, c.M * W), dtype=bool)      # mate rows of the batch mates that involve the NaN point
    if c.q:
        mates = [(jn // c.q) * c.q + r for r in range(c.q) if r != jn % c.q]
        for m in mates:
            mc = V.qav_column(m // c.q, m % c.q, c.q) if fam == "5h" else m
            paired[c.Ma + jn % c.q, mc * W:mc * W + W] = True
    g = (c.group[jn] if c.grad else c.group[jn // 16]) if c.grouped else 0
    patched = {k: v.copy() for k, v in got.items()}
    for t in range(c.T):
        if V.source_of(c, g, t) is None:
            continue
        written = V.reference(c, ch.arr, t)["cov"][1]
        for name in ("mu", "var"):
            assert np.isnan(got[name][t][own]).all(), f"{fam} slot {t} {name}: the NaN point's own entries are {got[name][t][own]}"
            patched[name][t][own] = clean[name][t][own]
        mine = written & own[None, :]
        assert mine.any() and np.isnan(got["cov"][t][mine]).all(), f"{fam} slot {t}: the NaN point's own part of cov is not NaN"
        patched["cov"][t][mine | paired] = clean["cov"][t][mine | paired]
    assert np.array_equal(patched["cov"].view(np.int64), clean["cov"].view(np.int64)), "cov outside the NaN point's own part changed"
    if det:
        assert _same_bits(patched, clean)
    ch.check(patched, " nan")
