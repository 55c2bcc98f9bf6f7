// Host build of the launcher's dispatch rules (csrc/gp_dispatch.h) for tests/_dispatch.py: the header is plain C++, so the plan
// a test asks for is computed by the very functions csrc/scaml_host.cpp launches from.  Each plan comes back as its fields in
// declaration order.  Test infrastructure, never part of the library.
#define __device__   // (csrc/gp_posterior_params.h marks one member function for the device)
#include "gp_dispatch.h"

extern "C" {

long long emul_lds_limit() { return (long long)scaml::LDS_LIMIT; }
int emul_linv_target_workgroups() { return scaml::LINV_TARGET_WORKGROUPS; }
int emul_fit_class(int N) { return scaml::fit_class(N); }
int emul_fit_class_max_d(int N) { return scaml::fit_class_max_d(N); }

void emul_fit_plan(int T, int N, int D, int cus, long long* out5) {
  const scaml::FitPlan p = scaml::fit_plan(T, N, D, cus);
  const long long v[5] = {p.variant, p.nb, p.wu, p.block, (long long)p.lds_doubles};
  for (int i = 0; i < 5; ++i) out5[i] = v[i];
}

void emul_blocked_plan(int T, int N, int D, int cus, int mode, long long workspace_bytes, int no_retry, long long* out11) {
  const scaml::BlockedPlan p = scaml::blocked_plan(T, N, D, cus, mode, workspace_bytes, no_retry != 0);
  const long long v[11] = {p.path, p.t8, p.parts, (long long)p.lds_coop, (long long)p.flag_bytes, (long long)p.need,
                           p.nt,   p.solve_small_d, p.rounds, (long long)p.lds_solve, (long long)p.lds_syrk};
  for (int i = 0; i < 11; ++i) out11[i] = v[i];
}

void emul_grad_plan(int T, int N, int D, int cus, int mode, int no_split, int ragged, int aligned16, long long* out9) {
  const scaml::GradPlan p = scaml::grad_plan(T, N, D, cus, mode, no_split != 0, ragged != 0, aligned16 != 0);
  const long long v[9] = {p.single, p.sc, p.nbt, p.dma, p.split, p.grid_x, p.grid_y, p.block, (long long)p.lds_doubles};
  for (int i = 0; i < 9; ++i) out9[i] = v[i];
}

void emul_target_fit_plan(int n, int T, int D, int mode, int batched, long long* out2) {
  const scaml::TargetFitPlan p = batched ? scaml::target_fit_batched_plan(n, T, D, mode) : scaml::target_fit_plan(n, T, D, mode);
  out2[0] = p.use_mfma;
  out2[1] = (long long)p.lds_doubles;
}

void emul_posterior_plan(int N, int D, long long* out2) {
  const scaml::PosteriorPlan p = scaml::posterior_plan(N, D);
  out2[0] = p.waves;
  out2[1] = p.xl;
}

// the studies' limits (csrc/gp_studies_acqf.h): training + pending points, input dimensions, fantasies
void emul_studies_limits(long long* out3) {
  out3[0] = scaml::STUDIES_ACQF_MAX_N;
  out3[1] = scaml::STUDIES_ACQF_MAX_D;
  out3[2] = scaml::STUDIES_FANTASY_MAX_F;
}

int emul_strip_solve_waves(int np) { return scaml::strip_solve_waves(np); }
int emul_linv_groups(int T, int nb, int waves) { return scaml::linv_groups(T, nb, waves); }

}  // extern "C"
