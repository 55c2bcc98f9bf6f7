// gf_schedule.hpp -- the per-wave tile schedule of the fused fit (csrc/gp_fit_fused.hip).
//
// The lower triangle of an NB x NB block matrix is cut into NT = NB (NB + 1) / 2 tiles, numbered column-major:
// column j starts at tile off(j) = j NB - j (j - 1) / 2 and holds the block rows j .. NB - 1.  Update wave w of WU
// owns the tiles t = s WU + w, slot s.  Which (block row, block column) a slot holds never changes during the
// kernel, so each wave works it out ONCE per attempt instead of walking the columns again in every phase of every
// panel iteration.  The schedule of one wave is 64 words, one per lane of a VGPR:
//   lanes 0 .. 19              slot s: the LDS byte offsets of the tile's block column and block row inside a column
//                              buffer (16 j PP 8 and 16 i PP 8, each <= 32 640: 16 bits apiece), or GF_SCHED_NONE
//                              where the wave has no tile in that slot (t >= NT)
//   lanes 20 .. 39             slot s: block column | block row << 8 (GF_SCHED_NONE where empty)
//   lanes 40 .. 40 + NB        column c: slo(c), the first slot of this wave at or right of column c; the wave's tiles
//                              of column c are the slots [slo(c), slo(c + 1)), slo(NB) = number of tiles it owns
// Plain C++, no HIP builtins: compiled for the device by the kernel and for the host by tests/host_emul/.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GF_SCHED_HD __host__ __device__ inline
#else
#define GF_SCHED_HD inline
#endif

namespace scaml {

constexpr int GF_SCHED_SLOTS = 20;              // accumulator tiles per wave (csrc/tile_regs.inc)
constexpr int GF_SCHED_IDX_LANE = 20;           // first lane of the (column, row) indices
constexpr int GF_SCHED_COL_LANE = 40;           // first lane of slo(c)
constexpr unsigned GF_SCHED_NONE = 0xffffffffu;  // no tile in this slot
constexpr int GF_SCHED_PITCH = 17;              // doubles per row of an LDS column buffer (PP of the kernel)
constexpr unsigned GF_SCHED_BLOCK_BYTES = 16u * GF_SCHED_PITCH * 8u;   // one block row of a column buffer

// first tile of column j
GF_SCHED_HD int gf_sched_off(int NB, int j) { return j * NB - j * (j - 1) / 2; }

// number of tiles of this wave in front of column j (the closed form the kernel used to evaluate per phase)
GF_SCHED_HD int gf_sched_slo(int NB, int WU, int wave, int j) {
  const int o = gf_sched_off(NB, j) - wave;
  return o <= 0 ? 0 : (o + WU - 1) / WU;
}

// tile t -> block column j (block row i = j + (t - off(j))), by the walk over the columns; -1 when t >= NT
GF_SCHED_HD int gf_sched_column_of(int NB, int t) {
  int j = 0, r = t;
  while (j < NB && r >= NB - j) { r -= NB - j; ++j; }
  return j < NB ? j : -1;
}

// word `lane` of the schedule of update wave `wave`
GF_SCHED_HD unsigned gf_sched_word(int NB, int WU, int wave, int lane) {
  if (lane < 2 * GF_SCHED_SLOTS) {
    const int s = lane < GF_SCHED_IDX_LANE ? lane : lane - GF_SCHED_IDX_LANE;
    const int t = s * WU + wave;
    const int j = gf_sched_column_of(NB, t);
    if (j < 0) return GF_SCHED_NONE;
    const int i = j + (t - gf_sched_off(NB, j));
    if (lane < GF_SCHED_IDX_LANE) return (unsigned)j * GF_SCHED_BLOCK_BYTES | ((unsigned)i * GF_SCHED_BLOCK_BYTES) << 16;
    return (unsigned)j | (unsigned)i << 8;
  }
  const int c = lane - GF_SCHED_COL_LANE;
  if (c >= 0 && c <= NB) return (unsigned)gf_sched_slo(NB, WU, wave, c);
  return 0u;
}

}  // namespace scaml
