"""The bounds of tests/_posterior_variant_bounds.py, checked without a device: they admit honest fp64 arithmetic in each variant's own
formulation (expanded-form distances in phase 1, coordinate differences in the epilogues, the group / src / mate indexing on the
flat arrays the entry points take, the packing of csrc/gp_qacqf_columns.h) on every input set of
tests/test_posterior_variant_bounds_gpu.py, every cap holds from the reference alone, and every planted fault below is rejected.
The first failing element of each fault is in profiles/posterior_variant_bounds_notes.md."""
import numpy as np
import pytest

from tests import _posterior_bounds as B
from tests import _posterior_variant_bounds as V
from tests import test_posterior_bounds as PB
from tests._posterior_variant_bounds import CASES, OS, SENTINEL


def _take(a, idx):
    """Flat read as the kernel addresses the array; an index a planted stride fault pushes past the end wraps instead of faulting."""
    return np.asarray(a).ravel().take(np.asarray(idx), mode="wrap")


def _value_V(c, arr, src, pts):
    """The value pass's V (N, m) of the points pts under source task src: tril(Linv) K_*^T, zeros in rows >= n."""
    n = c.N if arr["n_points"] is None else int(arr["n_points"][src])
    out = np.zeros((c.N, len(pts)))
    il = 1.0 / arr["theta"][src, :c.D]
    out[:n] = np.tril(arr["Linv"][src, :n, :n]) @ PB._columns64(arr["X"][src, :n], il, c.kind, pts, False, True)
    return out


def standin(c, arr, t, fault=None):
    """Slot t's outputs of case c's entry point in plain fp64 numpy, in sentinel-filled arrays; `fault` plants one fault."""
    N, D, q = c.N, c.D, c.q
    W = 16 if c.grad else 1
    mu, var = np.full(c.M * W, SENTINEL), np.full(c.M * W, SENTINEL)
    cov = np.full((c.rows, c.M * W), SENTINEL)
    small = None if arr["y_std"] is None else int(np.argmin(arr["y_std"]))
    d_ = np.arange(D)
    for col0, g, rows_q in V.units(c):
        sl = slice(col0, col0 + 16)
        slot, src = t, t
        if c.grouped and not 0 <= g < c.G:
            mu[sl] = var[sl] = 0.0
            continue
        if c.own:
            if fault == "out_at_src":      # slot t holds what the slot whose source task is t computed
                slot = t - c.task_base[g]
                if not 0 <= slot < c.T:
                    continue
            else:
                src = t + c.task_base[g]
            if not 0 <= src < c.Tsrc:
                mu[sl] = var[sl] = 0.0
                continue
        at = lambda what: slot if fault == what + "_at_slot" else src      # noqa: E731
        n = N if arr["n_points"] is None else int(arr["n_points"][at("n")])
        ys = 1.0 if arr["y_std"] is None else arr["y_std"][at("ys")]
        ym = 0.0 if arr["y_mean"] is None else arr["y_mean"][src]
        il = 1.0 / arr["theta"][src, :D]
        P, al = arr["X"][src, :n], arr["alpha"][at("alpha"), :n]
        pts = arr["Xq"][rows_q]
        xq = pts[0] if c.grad else pts
        C = PB._columns64(P, il, c.kind, xq, c.grad, True)
        Vv = np.tril(arr["Linv"][src, :n, :n]) @ C
        if fault == "drop_blocks":      # row blocks kb >= 8 (the second serpentine round on) contribute nothing
            Vv[128:] = 0.0
        value = np.eye(16)[0] if c.grad else np.ones(16)
        mu_u = ys * (C.T @ al) + ym * value
        s = (Vv * (Vv[:, :1] if c.grad else Vv)).sum(0)
        var_u = ys * ys * (OS - s)
        if c.grad:
            var_u[1:] = -2.0 * ys * ys * s[1:]
        # the leading rows: the group's points and V, read as the kernel strides them
        Ma = c.Ma[g] if c.grouped else c.Ma
        a_, r_ = np.arange(Ma), np.arange(n)
        if c.grouped:
            sx = Ma if fault == "xa_stride" else c.rows
            sv = c.rows if fault == "va_stride" else Ma
            Xlead = _take(arr["Xa"], ((g * sx + a_)[:, None]) * D + d_[None, :])
            VA = _take(arr["VA"][g], ((slot * N + r_)[:, None]) * sv + a_[None, :])
        else:
            Xlead, VA = arr["Xa"], arr["VA"][slot, :n, :Ma]
        cov_u = np.full((c.rows, 16), SENTINEL)
        cov_u[:Ma] = ys * ys * (PB._columns64(Xlead, il, c.kind, xq, c.grad, False) - VA.T @ Vv)
        if c.fam == "5g":
            j = rows_q[0]
            mate0 = j if fault == "mate0_strip" else (j // q) * q
            sq = 16 * c.Mq if fault == "vq_stride" else c.Mq
            VQ = _take(arr["VQ"], ((slot * N + r_)[:, None]) * sq + mate0 + np.arange(q)[None, :])
            Xm = _take(arr["Xa"] if fault == "mate_from_xa" else arr["Xq"], ((mate0 + np.arange(q))[:, None]) * D + d_[None, :])
            rows_m = ys * ys * (PB._columns64(Xm, il, c.kind, xq, True, False) - VQ.T @ Vv)
            if fault == "own_full":      # the point's own mate row with the full derivative of var
                rows_m[j % q, 1:] *= 2.0
            cov_u[Ma:] = rows_m
        if c.fam == "5h":
            G = Vv.T @ Vv
            if fault == "gram_image":      # the image before the Gram tile's: the last tile of the leading rows
                nas = (Ma + 15) // 16
                VAp = np.zeros((n, 16 * nas))
                VAp[:, :Ma] = VA
                G = (VAp.T @ Vv)[16 * (nas - 1):]
            qs = pts * il
            strip = col0 // 16
            live = sum(V.qav_batch_of(strip, b * q, q, c.B) >= 0 for b in range(V.qav_bps(q)))
            for cc in range(16):
                if V.qav_batch_of(strip, cc, q, c.B) < 0:
                    if fault != "pad_unwritten":
                        cov_u[Ma:Ma + q, cc] = 0.0
                    continue
                mb = (cc // q + 1) % live if fault == "neighbour_batch" else cc // q
                for i in range(mb * q, mb * q + q):
                    d2 = ((qs[i] - qs[cc]) ** 2).sum()
                    kv = PB._k64(np.array([d2]), c.kind, True)[0][0]
                    cov_u[Ma + i % q, cc] = ys * ys * (kv - G[i, cc])
        if fault == "small_1e-7" and src == small:
            mu_u, var_u = mu_u * (1 + 1e-7), var_u * (1 + 1e-7)
            cov_u = np.where(cov_u == SENTINEL, SENTINEL, cov_u * (1 + 1e-7))
        mu[sl], var[sl], cov[:, sl] = mu_u, var_u, cov_u
    return dict(mu=mu, var=var, cov=cov)


_HOST = {}


def host_arrays(c):
    """The case's inputs with the host stand-in of the device fit and of the value passes that produce VA and VQ."""
    if c in _HOST:
        return _HOST[c]
    arr = V.make_inputs(c)
    arr.update(B.host_fit(B.Case("linv", c.Tsrc, c.N, c.Mq, c.D, c.kind, 0, c.ragged, bool(c.std), False, False, c.c, c.noise), arr))
    if c.grouped:
        arr["VA"] = []
        for g in range(c.G):
            va = np.zeros((c.T, c.N, c.Ma[g]))
            for t in range(c.T):
                src = V.source_of(c, g, t)
                if src is not None:
                    va[t] = _value_V(c, arr, src, arr["Xa"][g, :c.Ma[g]])
            arr["VA"].append(va)
    else:
        arr["VA"] = np.stack([_value_V(c, arr, t, arr["Xa"]) for t in range(c.T)])
        if c.fam == "5g":
            arr["VQ"] = np.stack([_value_V(c, arr, t, arr["Xq"]) for t in range(c.T)])
    _HOST[c] = arr
    return arr


@pytest.mark.parametrize("case", CASES, ids=V.case_id)
def test_bound_admits_fp64_arithmetic(case):
    """Honest fp64 in the variant's formulation is inside the bound on every input set of the GPU file, and the sentinel / padding
    contracts the reference states are the stand-in's."""
    arr = host_arrays(case)
    slots = [standin(case, arr, t) for t in range(case.T)]
    V.check_case(case, arr, {k: np.stack([s[k] for s in slots]) for k in slots[0]}, " host")


def test_caps_hold_on_every_set_from_the_reference_alone():
    """CAP is a condition on the inputs: every bound of every set is within 1e-8 of its quantity's scale, no kernel involved."""
    for case in CASES:
        arr = host_arrays(case)
        for t in range(case.T):
            V.cap_check(case, arr, t)


def _first(fam, **kw):
    return next(c for c in CASES if c.fam == fam and all(getattr(c, k) == v for k, v in kw.items()))


# fault, case, slot, the first failing element (profiles/posterior_variant_bounds_notes.md quotes the messages)
FAULTS = [
    ("xa_stride", _first("5e", N=129), 0, " cov[0, 48]"),         # Xa read at stride Ma_g instead of Ma_max
    ("va_stride", _first("5e", N=129), 0, " cov[0, 16]"),         # VA at row stride Ma_max instead of Ma_g
    ("xa_stride", _first("5f", N=129), 0, " cov[0, 16]"),
    ("va_stride", _first("5f", N=129), 0, " cov[0, 16]"),
    ("n_at_slot", _first("5e'", N=129), 0, " var[0]"),            # OWN: n_points read at the slot instead of src (alpha is zero past n)
    ("ys_at_slot", _first("5e'", N=129), 0, " mu[0]"),            # OWN: y_std at the slot
    ("alpha_at_slot", _first("5e'", N=129), 0, " mu[0]"),         # OWN: alpha at the slot
    ("out_at_src", _first("5e'", N=129), 0, " mu"),               # OWN: the outputs written at src
    ("n_at_slot", _first("5f'", N=129), 0, " var[0]"),
    ("out_at_src", _first("5f'", N=129), 1, " mu"),
    ("mate0_strip", _first("5g", N=129), 0, " cov[15, 16]"),      # mate0 = strip instead of (strip / q) * q
    ("vq_stride", _first("5g", N=129), 0, " cov[15, 0]"),         # VQ at row stride M instead of M / 16
    ("own_full", _first("5g", N=129), 0, " cov[15, 1]"),          # a point's own mate row with the full derivative of var
    ("mate_from_xa", _first("5g", N=129), 0, " cov[15, 0]"),      # the mate's coordinates taken from Xa
    ("neighbour_batch", _first("5h", N=129), 0, " cov[17, 0]"),   # the mate taken from the neighbouring batch
    ("pad_unwritten", _first("5h", N=129), 0, " cov"),            # a padding column's mate rows left unwritten
    ("gram_image", _first("5h", N=129), 0, " cov[17, 0]"),        # the Gram tile read at image nas - 1
    ("gram_image", _first("5h", N=32), 0, " cov[24, 0]"),
]


@pytest.mark.parametrize("fault,case,slot,where", FAULTS, ids=[f"{f[0]}-{V.case_id(f[1])}" for f in FAULTS])
def test_rejects_planted_fault(fault, case, slot, where):
    arr = host_arrays(case)
    V.check_slot(case, arr, slot, standin(case, arr, slot))            # the unfaulted stand-in passes
    with pytest.raises(AssertionError) as e:
        V.check_slot(case, arr, slot, standin(case, arr, slot, fault))
    print(str(e.value))
    assert where in str(e.value), str(e.value)


@pytest.mark.parametrize("case", CASES, ids=V.case_id)
def test_dropped_row_blocks_show_from_n_129_on(case):
    """The contribution of row blocks kb >= 8 -- the second round of the serpentine schedule on -- dropped from V: no set with
    N < 129 can see it (the outputs are the same bits), every set with N >= 129 rejects it."""
    arr = host_arrays(case)
    if case.N < 129:
        for t in range(case.T):
            clean, faulty = standin(case, arr, t), standin(case, arr, t, "drop_blocks")
            assert all(np.array_equal(clean[k], faulty[k]) for k in clean)
        return
    caught = 0
    for t in range(case.T):
        try:
            V.check_slot(case, arr, t, standin(case, arr, t, "drop_blocks"))
        except AssertionError as e:
            caught += 1
            if caught == 1:
                print(str(e))
    assert caught, f"{V.case_id(case)}: the dropped row blocks went unnoticed"


@pytest.mark.parametrize("case", [c for c in CASES if c.std == 2], ids=V.case_id)
def test_small_task_fault_is_rejected_where_the_whole_tensor_rule_passes_it(case):
    """A relative 1e-7 on all outputs of the one source task whose y_std is smallest (30 times below the others): the per-element
    bounds reject it; the route-against-route rule of the existing files -- 1e-9 of the largest entry of the whole tensor -- lets the
    same cov and var through, computed here once on the same arrays."""
    arr = host_arrays(case)
    small = int(np.argmin(arr["y_std"]))
    rejected, seen = 0, False
    clean_all, faulty_all = [], []
    for t in range(case.T):
        clean, faulty = standin(case, arr, t), standin(case, arr, t, "small_1e-7")
        clean_all.append(clean), faulty_all.append(faulty)
        if any(V.source_of(case, g, t) == small for _, g, _ in V.units(case)):
            seen = True
            with pytest.raises(AssertionError) as e:
                V.check_slot(case, arr, t, faulty)
            rejected += 1
            print(str(e.value))
            with pytest.raises(AssertionError) as e:      # the covariances alone: what the whole-tensor rule holds to 1e-6 relative
                V.check_slot(case, arr, t, dict(clean, cov=faulty["cov"]))
            assert " cov[" in str(e.value)
            print(str(e.value))
    assert seen and rejected, f"{V.case_id(case)}: no slot reads the small task"
    for name in ("var", "cov"):
        a, b = np.stack([x[name] for x in clean_all]), np.stack([x[name] for x in faulty_all])
        wr = a != SENTINEL
        assert (a[wr] != b[wr]).any()
        assert np.abs(a[wr] - b[wr]).max() <= 1e-9 * np.abs(a[wr]).max(), f"{name}: the whole-tensor rule notices"
