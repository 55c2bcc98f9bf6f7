"""CPU checks of the fused fit's per-wave tile schedule (csrc/gf_schedule.hpp) through a host build of the same header
(tests/host_emul/fit_schedule_emul.cpp).  The kernel works the schedule out once per attempt and then trusts it in every
phase of every panel iteration, so for every kernel instance (NB 16-blocks, WU update waves) and every wave it must
be exactly the tile order the kernel has always used: tile t of the lower triangle, numbered column-major, sits in
slot t // WU of wave t % WU.  What the GPU does with it is tests/test_fit_schedule_gpu.py's."""
import ctypes

import numpy as np
import pytest

from tests._host_emul import build

INSTANCES = [(2, 1), (4, 3), (8, 3), (8, 7), (16, 7)]   # SCAML_INSTANTIATE list of csrc/gp_fit_fused.hip
UP = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "fit_schedule_emul")
    lib.emul_fit_schedule_words.restype, lib.emul_fit_schedule_words.argtypes = None, [ctypes.c_int] * 3 + [UP]
    lib.emul_fit_schedule_off.restype, lib.emul_fit_schedule_off.argtypes = ctypes.c_int, [ctypes.c_int] * 2
    lib.emul_fit_schedule_slo.restype, lib.emul_fit_schedule_slo.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    lib.emul_fit_schedule_layout.restype, lib.emul_fit_schedule_layout.argtypes = None, [UP]
    return lib


@pytest.fixture(scope="module")
def layout(emul):
    out = np.zeros(6, dtype=np.uint32)
    emul.emul_fit_schedule_layout(out.ctypes.data_as(UP))
    slots, idx_lane, col_lane, none, pitch, block_bytes = (int(v) for v in out)
    return dict(slots=slots, idx_lane=idx_lane, col_lane=col_lane, none=none, pitch=pitch, block_bytes=block_bytes)


def _words(emul, NB, WU, wave):
    out = np.zeros(64, dtype=np.uint32)
    emul.emul_fit_schedule_words(NB, WU, wave, out.ctypes.data_as(UP))
    return [int(v) for v in out]


def _tiles(NB):
    """(block column, block row) of the lower triangle in column-major order: the numbering of the kernel's tiles."""
    return [(j, i) for j in range(NB) for i in range(j, NB)]


def test_layout_fits_the_kernel(layout):
    # 20 accumulator tiles per wave (csrc/tile_regs.inc), pitch 17 doubles (FIT_PP of csrc/gp_fit_params.h): one block row
    # of a column buffer is 16 * 17 * 8 bytes; the three lane ranges do not overlap and end inside the 64 lanes
    assert layout["slots"] == 20 and layout["pitch"] == 17 and layout["block_bytes"] == 16 * 17 * 8
    assert layout["idx_lane"] >= layout["slots"] and layout["col_lane"] >= layout["idx_lane"] + layout["slots"]
    assert layout["col_lane"] + max(nb for nb, _ in INSTANCES) + 1 <= 64
    assert layout["none"] == 0xFFFFFFFF


@pytest.mark.parametrize("NB,WU", INSTANCES)
def test_every_tile_exactly_once_in_column_major_order(emul, layout, NB, WU):
    tiles = _tiles(NB)
    NT = len(tiles)
    slots = -(-NT // WU)
    assert slots <= layout["slots"]
    seen = {}
    for wave in range(WU):
        w = _words(emul, NB, WU, wave)
        mine = []
        for s in range(layout["slots"]):
            t = s * WU + wave
            word, idx = w[s], w[layout["idx_lane"] + s]
            if t >= NT:
                # no tile: both lanes carry the sentinel (only the wave's last slot, or slots the instance never dispatches)
                assert word == layout["none"] and idx == layout["none"], (wave, s)
                assert s >= slots - 1
                continue
            j, i = idx & 0xFF, idx >> 8
            assert (j, i) == tiles[t], (wave, s)
            assert (j, i) not in seen, (wave, s, seen.get((j, i)))
            seen[(j, i)] = (wave, s)
            # packed byte offsets: block column in the low half, block row in the high half, each inside its field and
            # inside a column buffer of NB block rows
            colb, rowb = word & 0xFFFF, word >> 16
            assert colb == 16 * j * layout["pitch"] * 8 and rowb == 16 * i * layout["pitch"] * 8
            assert colb <= 32640 and rowb <= 32640 and rowb < NB * layout["block_bytes"]
            assert word != layout["none"]
            mine.append(j * NB + i)   # column-major key
        # the wave's slots walk the triangle in column-major order
        assert mine == sorted(mine) and len(set(mine)) == len(mine)
    assert sorted(seen) == sorted(tiles)   # the whole lower triangle, nothing else


@pytest.mark.parametrize("NB,WU", INSTANCES)
def test_column_slot_ranges_match_the_closed_form(emul, layout, NB, WU):
    tiles = _tiles(NB)
    NT = len(tiles)
    for wave in range(WU):
        w = _words(emul, NB, WU, wave)
        owned = [tiles[t] for t in range(wave, NT, WU)]   # slot -> tile
        slo = [w[layout["col_lane"] + c] for c in range(NB + 1)]
        for c in range(NB + 1):
            off = c * NB - c * (c - 1) // 2                      # first tile of column c
            assert emul.emul_fit_schedule_off(NB, c) == off
            closed = 0 if off - wave <= 0 else -(-(off - wave) // WU)   # ceil((off - wave) / WU), clamped at 0
            assert slo[c] == closed == emul.emul_fit_schedule_slo(NB, WU, wave, c), (wave, c)
            # ... which is the number of the wave's tiles left of column c
            assert slo[c] == sum(1 for (j, _) in owned if j < c)
        assert slo[0] == 0 and slo[NB] == len(owned) and slo == sorted(slo)
        for c in range(NB):
            # the wave's tiles of column c are the contiguous slots [slo(c), slo(c + 1)), at most ceil(NB / WU) of them
            assert [s for s, (j, _) in enumerate(owned) if j == c] == list(range(slo[c], slo[c + 1]))
            assert slo[c + 1] - slo[c] <= -(-NB // WU)
            # the diagonal tile is the first of its column: in the wave's first slot of the column or with another wave
            rows = [i for (j, i) in owned if j == c]
            assert c not in rows[1:]
        # lanes the kernel never reads hold zero
        assert all(v == 0 for v in w[layout["col_lane"] + NB + 1:])
