// art_kernels_nolicm.hip -- the kernels compiled without MachineLICM (build.py adds
// -disable-machine-licm to this translation unit only): the helper kernel (init_one / finalize_one,
// the streamed pipeline's helper duty), the integrator for every geometry but flat's (GR, boundary
// layer, isotropic, RK4 with saveat) and the one-wave-per-ray tail kernel. MachineLICM hoists the
// loop bodies' polynomial and tableau constants (exp, sincos, acos, atan2, the Vern6 coefficients:
// ~150 v_mov_b32) out of the loops into registers live across them:
//   * the helper kernel then spilled 74-95 VGPRs to scratch at 2 waves per SIMD, and a persistent
//     helper using scratch stalled the next launch on another queue for seconds;
//   * the GR integrator spilled 60 VGPRs (226 without the pass, no spill): its bulk launch runs
//     3.4% faster without it, the lone tail ray 2% (profiles/r06q_gr_licm.jsonl).
// The flat integrator keeps the pass (art_kernels.hip): without it it spills nothing either but
// rematerialises the constants inside the step loop and runs 3% slower
// (profiles/r06o_ab_device_licm_off_everywhere.jsonl). The pass moves instructions and changes no
// arithmetic: the outputs are bit-identical (profiles/r06n_bitident_licm.log).
#include <hip/hip_runtime.h>

#include <atomic>

#include "art_core.h"
#include "art_event.h"
#include "art_internal.h"
#include "art_step.h"
#include "art_ray_io.h"
#include "art_propagate.h"
#include "art_tail.h"
#include "art_helper.h"
#include "art_sample.h"
#include "art_eval_math.h"

namespace art {

// the helper instantiation of the integrator's geometry (launch_propagate, launch_integrator_streamed)
HFn pick_helper(const KParams& P) {
  const int geom = geom_of(P);
  return geom == GEOM_FLAT ? helper_kernel<GEOM_FLAT> : (geom == GEOM_GR ? helper_kernel<GEOM_GR> : helper_kernel<GEOM_ANY>);
}
int helper_waves_per_simd(const KParams& P) {
  // 2 when the build for these parameters fits 2 waves per SIMD without scratch (read once per build)
  static std::atomic<int> cached[3];
  const HFn fn = pick_helper(P);
  const int g = fn == helper_kernel<GEOM_FLAT> ? 1 : (fn == helper_kernel<GEOM_GR> ? 2 : 0);
  int w = cached[g].load(std::memory_order_relaxed);
  if (!w) {
    hipFuncAttributes a{};
    const bool ok = hipFuncGetAttributes(&a, (const void*)fn) == hipSuccess;
    (void)hipGetLastError();
    w = (ok && a.localSizeBytes == 0 && a.numRegs > 0 && a.numRegs <= 256) ? 2 : 1;
    cached[g].store(w, std::memory_order_relaxed);
  }
  return w;
}

// The integrator and tail instantiations compiled here, without MachineLICM (art_kernels_nolicm.hip):
// every geometry but flat's Vern6/RK4 integrator. GR: the bulk launch 235.2-236.7 -> 227.3-228.7
// ms per 10^6 rays, the lone tail ray 7.69 -> 7.54 us per attempt (no spills: 256 VGPRs + 60 spilled
// -> 226), bit-identical (profiles/r06q_gr_licm.jsonl); the flat integrator stays in art_kernels.hip,
// 3% faster with the pass (profiles/r06o_ab_device_licm_off_everywhere.jsonl).
KFn nl_propagate(int integ, int geom, bool save, int don, int wps) {
#define ART_NL(I, G, S, D, W, C) \
  if (integ == I && geom == G && save == S && don == D && wps == W) return propagate_kernel<I, G, S, D, W, C>;
  ART_BUILDS_NL(ART_NL)  // (the list: art_launch_plan.h)
#undef ART_NL
  return nullptr;
}
// (the cyclotron-observing Vern6 integrators, SegOut::cyc_tau: GR and the general geometry)
KFn nl_propagate_cyc(int geom, int don) {
#define ART_NL(I, G, S, D, W, C) \
  if (geom == G && don == D) return propagate_kernel<I, G, S, D, W, C>;
  ART_BUILDS_NL_CYC(ART_NL)
#undef ART_NL
  return nullptr;
}
TFn nl_tail(int geom) {
#define ART_NL(G) \
  if (geom == G) return tail_kernel<G>;
  ART_BUILDS_TAIL(ART_NL)
#undef ART_NL
  return nullptr;
}
static_assert(GEOM_ANY == LP_GEOM_ANY && GEOM_FLAT == LP_GEOM_FLAT && GEOM_GR == LP_GEOM_GR && ART_WAVES_PER_SIMD == LP_WPS &&
                  BLOCK == LP_BLOCK && HOT_BLOCKS == LP_HOT_BLOCKS,
              "art_launch_plan.h plans with the kernels' own constants");

// the sampler's builds, compiled here without MachineLICM (art_kernels_nolicm.hip)
SFn nl_sample(int wps, bool blocks) {
  return wps == 3 ? (blocks ? sample_kernel<3, true> : sample_kernel<3, false>)
                  : (blocks ? sample_kernel<2, true> : sample_kernel<2, false>);
}
SHFn nl_sample_halo(int wps, bool blocks) {
  return wps == 3 ? (blocks ? sample_kernel<3, true, true, double> : sample_kernel<3, false, true, double>)
                  : (blocks ? sample_kernel<2, true, true, double> : sample_kernel<2, false, true, double>);
}
MFn nl_eval_math(int fn) { return pick_eval_math<1>(fn); }

}  // namespace art
