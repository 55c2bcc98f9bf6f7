// gp_fit_fused_full.hip -- the full-tile instances gp_fit_fused_kernel<16, 7, kind, true> of csrc/gp_fit_fused.hip (FULL, see
// gp_fit_attempt there), in a translation unit of their own: the same source, only the list of explicit instantiations at its
// end differs.
#define SCAML_FIT_FULL_TU
#include "gp_fit_fused.hip"
