"""Long-double reference, a-priori forward error bounds and shared assertions for the sixteen later instances of
gp_posterior_linv_kernel (csrc/gp_posterior.hip): the grouped GRAD pass (5e) / (5e') with atomic and with ordered sums, the grouped
value pass (5f) / (5f'), the joint GRAD pass (5g) and the joint value pass (5h).

The construction is that of tests/_posterior_bounds.py: the reference consumes exactly the arrays the entry point is handed, in the
entry point's layout (Linv, alpha, VA and VQ as the device -- or, without one, the host stand-in -- produced them), and next to each
reference element stands its bound.  mu, var, their derivative columns and V with its bound E_V come from that module's
task_reference itself (kern "grad" / "linv", called with the unit's source task and query points), so these lines are that module's
by construction; the `cov` line is restated here once (_cov_line) because its rows are no longer the head of Xq:

  leading rows a < Ma_g     cov line with the group's own Xa[g], VA_tab[g], Ma_g; OWN: the source arrays at src = task_base[g] + slot
  (5g) mate row Ma + r      cov line, value and GRAD col, with VA_a -> column b q + r of VQ (an input: no error term), x_a -> Xq[b q + r]
  (5h) mate row Ma + r      both operands are the kernel's:  E = ys^2 (E_K(x_m, x_c) + |V_m|^T E_V,c + E_V,m^T |V_c| + E_V,m^T E_V,c
                            + g_{N+4} |V_m|^T |V_c| + u (|os k| + |V_m^T V_c|)) + 2 u |cov|

Statement counts of the sites that differ from the base pass, read off the kernel:
  * the epilogue's df with a mate's coordinates (JOINT): `xab[xa0 + d] * invl[d] - xqs[d * 16 + c]` -- the statement of the leading
    rows with another pointer: two scaled coordinates of 2 u each and the difference's own rounding, what the GRAD col line counts.
  * the JOINTV epilogue: df = xqs[i] - xqs[c] from two scaled coordinates in LDS, d2 by fma, kernel_from_sqdist, `ys * ys * (kv - G)`:
    one subtraction and two products, the u (|os k| + |G|) + 2 u |cov| of the cov line.  E_d2 (expanded form) covers the difference form.
  * the Gram tile is four more MFMAs per row block on the V block and the same fixed-order sum over the waves as the other tiles:
    an inner product of N terms, g_{N+4}.
  * the DET sums: eight shares added in wave order in place of the LDS atomics -- the same N + 3 additions in another order, inside
    g_{N+4}: the ordered and the atomic instances share one bound.

Contracts stated by the reference (`written` masks): rows a >= Ma_g of a group's strips of cov are untouched; a padding entry of
`group` (negative or >= G) and an OWN slot whose src falls outside 0 .. Tsrc - 1 give zeros in mu / var and no row of cov; the mate
rows of a padding column of (5h) are exact zeros; every other element is written.

CAP = 1e-8 of the quantity's largest reference magnitude in the (source) task stays a condition on the inputs.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import _posterior_bounds as B
from tests._posterior_bounds import CAP, KIND_MATERN52, KIND_RBF, LD, OS, SENTINEL, U, Quantity, Ratios, assert_within, columns, gamma  # noqa: F401
from tests._posterior_bounds import _kernel, inverse_lower  # noqa: F401  (the building blocks, for the stand-ins)

_Fields = namedtuple("_Fields", "fam T Tsrc N D kind Mq Ma group task_base q B ragged std c noise det twin")


class VCase(_Fields):
    """One input set.  fam: 5e / 5e' / 5f / 5f' / 5g / 5h.  Grouped: Ma = (Ma_g), group per query point (5e) or per strip (5f), Mq
    query points; joint: Ma leading points, B batches of q.  The aliases let _posterior_bounds.case_id / assert_within name the case."""
    __slots__ = ()
    kern = property(lambda s: s.fam)
    M = property(lambda s: qav_columns(s.B, s.q) if s.fam == "5h" else s.Mq)
    per_task = nanq = False
    grad = property(lambda s: s.fam in ("5e", "5e'", "5g"))
    grouped = property(lambda s: s.fam[:2] in ("5e", "5f"))
    own = property(lambda s: s.fam.endswith("'"))
    G = property(lambda s: len(s.Ma) if s.grouped else 1)
    rows = property(lambda s: max(s.Ma) if s.grouped else s.Ma + s.q)      # the row count of cov


def _v(fam, T, N, D, kind, Mq=0, Ma=(), group=(), task_base=None, Tsrc=None, q=0, B=0, ragged=None, std=False, c=0.5, noise=1e-2,
       det=False, twin=False):
    return VCase(fam, T, Tsrc or T, N, D, kind, Mq or B * q, Ma, group, task_base, q, B, ragged, std, c, noise, det, twin)


R, MT = KIND_RBF, KIND_MATERN52
# N: 17 two blocks, six idle waves | 32 nas == NB for (5h) | 129 odd, NB = 9: the first block of the second serpentine round | 144 even:
# the vector loads | 272 NB = 17: third round | 512 the limit.  T = 9: second XCD round.
# std = 2: task 0's y_std 30 times below the smallest of the others.
CASES = [
    _v("5e", 9, 17, 1, R, Mq=5, Ma=(1, 17, 9), group=(0, 2, -1, 1, 2), ragged=0, std=True, c=0.3, det=True),
    _v("5e", 3, 129, 5, MT, Mq=5, Ma=(1, 16, 96), group=(2, 0, 3, 1, 2), ragged=0, det=True),
    _v("5e", 2, 272, 15, R, Mq=3, Ma=(17, 33), group=(1, 0, 1), std=2, det=True),
    _v("5e", 2, 512, 4, MT, Mq=2, Ma=(96, 5), group=(0, 1), ragged=0, det=True),
    _v("5e'", 2, 129, 5, R, Mq=5, Ma=(17, 1, 96, 16), group=(0, 1, 2, 3, 1), task_base=(3, 0, 1, 4), Tsrc=5, ragged=0, std=2, det=True),
    _v("5e'", 9, 17, 1, MT, Mq=3, Ma=(1, 9), group=(0, 1, 0), task_base=(9, 0), Tsrc=18, c=0.3, det=True),
    _v("5e'", 2, 272, 4, MT, Mq=2, Ma=(33, 17), group=(1, 0), task_base=(2, 0), Tsrc=4),
    _v("5f", 9, 17, 1, R, Mq=48, Ma=(17, 1), group=(1, -1, 0), c=0.3),
    _v("5f", 3, 129, 5, MT, Mq=32, Ma=(96, 16), group=(0, 1), ragged=0, std=2),
    _v("5f", 2, 144, 4, R, Mq=16, Ma=(33,), group=(0,)),
    _v("5f", 2, 512, 15, MT, Mq=16, Ma=(17,), group=(0,)),
    _v("5f'", 2, 129, 5, R, Mq=64, Ma=(17, 1, 96, 16), group=(0, 1, 2, 3), task_base=(3, 0, 1, 4), Tsrc=5, ragged=0, std=2),
    _v("5f'", 2, 129, 5, MT, Mq=64, Ma=(17, 1, 96, 16), group=(0, 1, 2, 3), task_base=(3, 0, 1, 4), Tsrc=5, ragged=0, std=2),
    _v("5g", 9, 17, 1, R, Ma=1, q=1, B=3, c=0.3),
    _v("5g", 2, 17, 4, MT, Ma=9, q=8, B=2),
    _v("5g", 3, 129, 5, R, Ma=15, q=3, B=2, ragged=0, std=2),
    _v("5g", 2, 144, 4, MT, Ma=88, q=8, B=2),
    _v("5g", 2, 272, 15, R, Ma=17, q=2, B=2, twin=True),
    _v("5g", 2, 512, 5, MT, Ma=16, q=4, B=2, ragged=0),
    _v("5h", 2, 32, 2, R, Ma=24, q=8, B=3),
    _v("5h", 3, 129, 5, MT, Ma=17, q=3, B=6, ragged=0, std=2),
    _v("5h", 2, 144, 4, R, Ma=16, q=5, B=4),
    _v("5h", 2, 144, 4, MT, Ma=16, q=6, B=4),
    _v("5h", 2, 144, 4, R, Ma=16, q=7, B=4),
    _v("5h", 2, 272, 15, MT, Ma=94, q=2, B=9),
    _v("5h", 2, 512, 5, R, Ma=17, q=4, B=5, ragged=0),
]


def case_id(c: VCase) -> str:
    s = B.case_id(c)
    return s + (f"-q{c.q}-B{c.B}" if c.q else "") + ("-own" if c.own else "")


# ---- the packing of csrc/gp_qacqf_columns.h ----------------------------------------------------------------------------------------
def qav_bps(q):
    return 16 // q


def qav_column(b, j, q):
    return 16 * (b // qav_bps(q)) + (b % qav_bps(q)) * q + j


def qav_columns(Bn, q):
    return 16 * ((Bn + qav_bps(q) - 1) // qav_bps(q))


def qav_batch_of(strip, c, q, Bn):
    return -1 if (c // q >= qav_bps(q) or strip * qav_bps(q) + c // q >= Bn) else strip * qav_bps(q) + c // q


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_inputs(c: VCase) -> dict:
    """make_inputs' conventions of tests/_posterior_bounds.py for the Tsrc source tasks and the Mq query points (the first on a
    training point of task 0, the second 1e-7 away from another), then the variant's own arrays: Xa (G, Ma_max, D) or (Ma, D), for
    (5h) the query points packed into Mp columns (finite padding columns)."""
    base = B.Case("linv", c.Tsrc, c.N, c.Mq, c.D, c.kind, 0, c.ragged, bool(c.std), False, False, c.c, c.noise)
    inp = B.make_inputs(base)
    rng = np.random.default_rng([7, c.Tsrc, c.N, c.D, c.Mq])
    if c.std == 2:
        inp["y_std"][0] = inp["y_std"].min() / 30.0      # (task 0 has all N points in every set)
    if c.twin:      # two mates of batch 1 coincide exactly
        inp["Xq"][c.q + 1] = inp["Xq"][c.q]
    if c.grouped:
        Xa = rng.uniform(size=(c.G, c.rows, c.D))
    else:
        Xa = rng.uniform(size=(c.Ma, c.D))
    Xa.reshape(-1, c.D)[0] = inp["X"][0, 1]
    inp["Xa"] = Xa
    if c.fam == "5h":
        Xp = rng.uniform(size=(c.M, c.D))
        for b in range(c.B):
            for j in range(c.q):
                Xp[qav_column(b, j, c.q)] = inp["Xq"][b * c.q + j]
        inp["Xq"] = Xp
    return inp


def source_of(c: VCase, g: int, t: int):
    """The source task slot t of group g reads, or None for a padding unit."""
    if g < 0 or g >= c.G:
        return None
    src = t + (c.task_base[g] if c.own else 0)
    return src if 0 <= src < c.Tsrc else None


def units(c: VCase):
    """(first column, group, rows of Xq) of every workgroup's strip of 16 columns."""
    if c.grad:
        return [(16 * j, c.group[j] if c.grouped else 0, [j]) for j in range(c.Mq)]
    return [(16 * s, c.group[s] if c.grouped else 0, list(range(16 * s, 16 * s + 16))) for s in range(c.M // 16)]


def lead_points(c: VCase, arr: dict, g: int):
    """(Xa, Ma) of group g."""
    if c.grouped:
        return arr["Xa"][g, :c.Ma[g]], c.Ma[g]
    return arr["Xa"], c.Ma


# ---- reference and bound -------------------------------------------------------------------------------------------------------------
def _cov_line(Xrows, l, kind, pts, grad, A, V, EV, ys2, g, E_A=None):
    """The cov line of tests/_posterior_bounds.py for the rows Xrows against the unit's columns: A (n, rows) the rows' V -- an input
    (E_A None) or computed by the kernel with bound E_A."""
    cols = [columns(Xrows, l, kind, p, True) for p in pts] if grad else [columns(Xrows, l, kind, pts, False)]
    K, E_K = np.concatenate([x[0] for x in cols], 1), np.concatenate([x[1] for x in cols], 1)
    aA, aV = np.abs(A), np.abs(V)
    dot = A.T @ V
    cov = ys2 * (K - dot)
    E_dot = aA.T @ EV + g * (aA.T @ aV)
    if E_A is not None:
        E_dot = E_dot + E_A.T @ aV + E_A.T @ EV
    return cov, ys2 * (E_K + E_dot + U * (np.abs(K) + np.abs(dot))) + 2 * U * np.abs(cov)


def reference(c: VCase, arr: dict, t: int) -> dict:
    """name -> (Quantity, written) over slot t's slice of mu / var (M [, 16]) and cov (rows, M [* 16]).  Unwritten elements keep the
    sentinel; a padding unit's mu / var have reference and bound 0 (exact zeros)."""
    W = 16 if c.grad else 1
    ncol = c.M * W
    g_ = gamma(c.N + 4)
    ref = {k: np.zeros(s, dtype=LD) for k, s in (("mu", (ncol,)), ("var", (ncol,)), ("cov", (c.rows, ncol)))}
    bnd = {k: np.zeros(v.shape, dtype=LD) for k, v in ref.items()}
    src_of = {k: np.full(v.shape, -1) for k, v in ref.items()}
    written = dict(mu=np.ones(ncol, dtype=bool), var=np.ones(ncol, dtype=bool), cov=np.zeros((c.rows, ncol), dtype=bool))
    for col0, g, rows_q in units(c):
        src = source_of(c, g, t)
        if src is None:
            continue
        sl = slice(col0, col0 + 16)
        pts = arr["Xq"][rows_q]
        n = c.N if arr["n_points"] is None else int(arr["n_points"][src])
        base = B.Case("grad" if c.grad else "linv", c.Tsrc, c.N, len(rows_q), c.D, c.kind, 0, None, False, False, False, c.c, c.noise)
        r = B.task_reference(base, dict(arr, Xq=pts), src)
        for name in ("mu", "var"):
            ref[name][sl], bnd[name][sl] = r[name].ref.reshape(-1), r[name].bound.reshape(-1)
            src_of[name][sl] = src
        V, EV = r["V"].ref[:n], r["V"].bound[:n]
        l = arr["theta"][src, :c.D]
        ys = 1.0 if arr["y_std"] is None else float(arr["y_std"][src])
        ys2 = LD(ys) * LD(ys)
        Xa, Ma = lead_points(c, arr, g)
        A = LD((arr["VA"][g] if c.grouped else arr["VA"])[t, :n, :Ma])
        ref["cov"][:Ma, sl], bnd["cov"][:Ma, sl] = _cov_line(Xa, l, c.kind, pts, c.grad, A, V, EV, ys2, g_)
        written["cov"][:Ma, sl] = True
        src_of["cov"][:, sl] = src
        if c.fam == "5g":
            j = rows_q[0]
            mates = (j // c.q) * c.q + np.arange(c.q)
            A = LD(arr["VQ"][t, :n][:, mates])
            ref["cov"][Ma:, sl], bnd["cov"][Ma:, sl] = _cov_line(arr["Xq"][mates], l, c.kind, pts, True, A, V, EV, ys2, g_)
            written["cov"][Ma:, sl] = True
        if c.fam == "5h":
            full, E_full = _cov_line(pts, l, c.kind, pts, False, V, V, EV, ys2, g_, E_A=EV)      # (16, 16): element (mate, column)
            written["cov"][Ma:, sl] = True      # a padding column: exact zeros
            for cc in range(16):
                if qav_batch_of(col0 // 16, cc, c.q, c.B) < 0:
                    continue
                m0 = (cc // c.q) * c.q
                ref["cov"][Ma:, col0 + cc], bnd["cov"][Ma:, col0 + cc] = full[m0:m0 + c.q, cc], E_full[m0:m0 + c.q, cc]
    out = {}
    for name in ref:
        scale = np.zeros(ref[name].shape)
        val = np.zeros(ref[name].shape, dtype=bool)
        val[..., 0::W] = True
        for src in np.unique(src_of[name][src_of[name] >= 0]):
            here = src_of[name] == src
            ys = 1.0 if arr["y_std"] is None else float(arr["y_std"][src])
            scale[here & val] = B._scale(ref[name][here & val]) if name == "mu" else OS * ys * ys
            if c.grad:      # value columns and derivative columns are different quantities: each gets its own scale
                scale[here & ~val] = B._scale(ref[name][here & ~val & written[name]])
        out[name] = (Quantity(ref[name], bnd[name], scale), written[name])
    return out


def check_case(c: VCase, arr: dict, got: dict, label: str = ""):
    """check_slot for every slot of got (name -> (T, ...)), then one line per output with the case's own largest error / bound and
    bound / scale (for profiles/posterior_variant_bounds_notes.md: the figures are for the record and feed no tolerance)."""
    mine, B.RATIOS = B.RATIOS, Ratios()
    try:
        for t in range(c.T):
            check_slot(c, arr, t, {k: v[t] for k, v in got.items()})
        for (_, _, name), (err, cap) in sorted(B.RATIOS.items()):
            print(f"RATIO {case_id(c)}{label} {name}: largest error / bound {err:.3e}, largest bound / scale {cap:.3e}")
    finally:
        B.RATIOS = mine


def check_slot(c: VCase, arr: dict, t: int, got: dict):
    """Every element of slot t's outputs: unwritten ones keep the sentinel, GRAD columns past D are exact zeros, every other one is
    within its bound (and the bound within the cap).  (5g): a point's own mate row is its variance and HALF of its derivative."""
    refs = reference(c, arr, t)
    for name, (q, written) in refs.items():
        a = np.asarray(got[name]).reshape(q.ref.shape)
        assert (a[~written] == SENTINEL).all(), f"{case_id(c)} slot {t} {name}: an element the call may not write was written"
        assert not (a[written] == SENTINEL).any(), f"{case_id(c)} slot {t} {name}: an element the call must write keeps the sentinel"
        if c.grad:
            dead = np.zeros(a.shape[-1], dtype=bool)
            for col in range(1 + c.D, 16):
                dead[col::16] = True
            assert (a[..., dead][written[..., dead]] == 0).all(), f"{case_id(c)} slot {t} {name}: GRAD columns 1 + D .. 15 are not exactly zero"
        assert_within(c, t, name, np.where(written, a, 0.0), q)
    if c.fam == "5g":
        cov, var = np.asarray(got["cov"]).reshape(c.rows, -1), np.asarray(got["var"]).reshape(-1)
        Ec, Ev = refs["cov"][0].bound, refs["var"][0].bound
        half = np.where(np.arange(16) == 0, 1.0, 0.5)
        for j in range(c.Mq):
            sl, row = slice(16 * j, 16 * j + 16), c.Ma + j % c.q
            err = np.abs(LD(cov[row, sl]) - half * LD(var[sl]))
            assert (err <= Ec[row, sl] + half * Ev[sl]).all(), \
                f"{case_id(c)} slot {t}: point {j}'s own mate row is not var and half of var's derivative: {cov[row, sl]} against {var[sl]}"


def cap_check(c: VCase, arr: dict, t: int):
    """The cap from the reference alone: every bound at most CAP of its quantity's scale."""
    for name, (q, written) in reference(c, arr, t).items():
        over = written & ~(q.bound <= CAP * q.scale)
        assert not over.any(), (f"{case_id(c)} slot {t} {name}{list(np.argwhere(over)[0])}: the bound {float(q.bound[over].max()):.3e} exceeds {CAP} "
                                f"of the scale {float(q.scale[over].max()):.3e} -- the input set is ill-chosen")
