// Host build of the fused fit's per-wave tile schedule (csrc/gf_schedule.hpp) for tests/test_fit_schedule.py: the header is
// plain C++, so the words the kernel keeps in the lanes of a VGPR are computed here by the very same functions.
// Test infrastructure, never part of the library.
#include "gf_schedule.hpp"

extern "C" {

// the 64 schedule words of update wave `wave` of instance (NB, WU), one per lane
void emul_fit_schedule_words(int NB, int WU, int wave, unsigned* out64) {
  for (int lane = 0; lane < 64; ++lane) out64[lane] = scaml::gf_sched_word(NB, WU, wave, lane);
}

int emul_fit_schedule_off(int NB, int j) { return scaml::gf_sched_off(NB, j); }
int emul_fit_schedule_slo(int NB, int WU, int wave, int j) { return scaml::gf_sched_slo(NB, WU, wave, j); }

// layout constants: slots, first index lane, first column lane, sentinel, pitch, bytes per block row
void emul_fit_schedule_layout(unsigned* out6) {
  out6[0] = (unsigned)scaml::GF_SCHED_SLOTS;
  out6[1] = (unsigned)scaml::GF_SCHED_IDX_LANE;
  out6[2] = (unsigned)scaml::GF_SCHED_COL_LANE;
  out6[3] = scaml::GF_SCHED_NONE;
  out6[4] = (unsigned)scaml::GF_SCHED_PITCH;
  out6[5] = scaml::GF_SCHED_BLOCK_BYTES;
}

}  // extern "C"
