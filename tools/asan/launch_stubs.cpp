// launch_stubs.cpp -- TEST INFRASTRUCTURE ONLY: the kernel launch wrappers of
// art_internal.h for the host-only sanitizer build of the C boundary's host units (capi_main.cpp). No GPU
// exists there, so every launch reports hipErrorNoDevice.
#include "../../adiabatic_raytracer_amd/csrc/art_internal.h"

namespace art {
int persistent_blocks(const void*, int64_t, int, int) { return 1; }
size_t claim_order_bytes(int64_t) { return 0; }
hipError_t launch_propagate(const KParams&, int64_t, const SegIn&, const SegOut&, int32_t, unsigned long long*,
                            unsigned long long*, hipStream_t, const LaunchPlanIn&, LaunchPlan*, hipEvent_t, hipEvent_t,
                            hipStream_t, const HotSide&) {
  return hipErrorNoDevice;
}
hipError_t launch_integrator_streamed(const KParams&, int64_t, const SegIn&, const SegOut&, int32_t, unsigned long long*,
                                      unsigned long long*, int, hipStream_t, LaunchPlan*) { return hipErrorNoDevice; }
hipError_t launch_helpers(const KParams&, int64_t, const SegIn&, const SegOut&, int, int64_t, int, unsigned long long*,
                          hipStream_t) {
  return hipErrorNoDevice;
}
int64_t small_tail_limit() { return 0; }
int geom_of(const KParams&) { return 0; }  // (GEOM_ANY: the launch plan's input)
int helper_waves_per_simd(const KParams&) { return 2; }
HFn pick_helper(const KParams&) { return nullptr; }
KFn nl_propagate(int, int, bool, int, int) { return nullptr; }
KFn nl_propagate_cyc(int, int) { return nullptr; }
TFn nl_tail(int) { return nullptr; }
SFn nl_sample(int, bool) { return nullptr; }
SHFn nl_sample_halo(int, bool) { return nullptr; }
hipError_t launch_sample(const KParams&, double, uint64_t, int64_t, int64_t, double*, double*, double*, double*, int32_t*,
                         int32_t*, unsigned long long*, hipStream_t, int, const HaloK*) { return hipErrorNoDevice; }
hipError_t launch_prob(const KParams&, int64_t, const double*, const double*, const double*, int64_t, const int64_t*,
                       double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_flux(const KParams&, int64_t, const double*, const double*, const int32_t*, const int8_t*,
                       const double*, int32_t, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_flux_phi(int64_t, const double*, const int8_t*, const double*, int32_t, double, double, double*, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_sky_map(int64_t, const double*, const double*, const double*, const int8_t*, const double*,
                          const SkyAxes&, int, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_sky_map_segments(const KParams&, int64_t, const double*, const double*, const double*, const int32_t*,
                                   const int8_t*, const double*, const double*, const SkyAxes&, int, int, double*,
                                   int32_t*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_eval_rhs(const KParams&, int64_t, const double*, const double*, const double*, const int8_t*, double*,
                           hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_eval_hamiltonian(const KParams&, int64_t, const double*, const double*, const double*, const double*,
                                   double*, double*, double*, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_event_weight(const KParams&, int64_t, const double*, const double*, const double*, double, double,
                               double, double*, hipStream_t, const HaloK*) { return hipErrorNoDevice; }
hipError_t launch_eval_condition(const KParams&, int64_t, const double*, const double*, double*, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_eval_cyclotron(const KParams&, int64_t, const double*, const double*, const double*, double*, double*,
                                 hipStream_t) { return hipErrorNoDevice; }
size_t tree_scan_bytes(int64_t) { return 0; }
hipError_t launch_tree_roots(const KParams&, const TreeRules&, int64_t, const double*, const double*, const double*,
                             const int8_t*, TreeState*, TreeEv*, int32_t*, int32_t*, int32_t*, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_tree_pack(const TreeRules&, int64_t, int64_t, const int32_t*, const int32_t*, const int32_t*, int32_t*,
                            TreeState*, const TreeEv*, const TreeBatch&, double, double, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_tree_step(const KParams&, const TreeRules&, int64_t, int64_t, const int32_t*, TreeState*, TreeEv*,
                            const TreeBatch&, art_tree_node*, int32_t*, int32_t*, int32_t*, void*, size_t, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_tree_finish(const TreeRules&, int64_t, const TreeState*, int32_t*, int32_t*, int32_t*, int64_t*, void*,
                              size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_tree_flatten(int64_t, const art_tree_node*, const int64_t*, int64_t, art_tree_node*, hipStream_t) {
  return hipErrorNoDevice;
}
size_t event_scan_bytes(int64_t) { return 0; }
hipError_t launch_event_scan(int64_t, const art_tree_node*, bool, int32_t*, void*, size_t, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_event_gather(int64_t, const art_tree_node*, const int32_t*, int64_t, const double*, int64_t,
                               const TreeBatch&, int32_t*, double, double, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_event_rows(const EventRowsArgs&, const SkyAxes&, int, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_event_moments(const EventRowsArgs&, const EventMomentsArgs&, const SkyAxes&, int, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_event_reweight(const KParams&, const KParams&, const EventRowsArgs&, const EventReweightArgs&,
                                 const SkyAxes&, int, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_event_halo_scan(const EventRowsArgs&, const EventHaloScanArgs&, const SkyAxes&, int, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_event_replicates(const EventRowsArgs&, const EventReplicatesArgs&, const SkyAxes&, int, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_event_grid(const EventRowsArgs&, const EventGridArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_event_spectrum(const EventRowsArgs&, const EventSpectrumArgs&, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_exact_histogram(int64_t, const int32_t*, const double*, int, int64_t*, double*, bool, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_exact_finish(int64_t, const int64_t*, double*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_event_exact(const EventRowsArgs&, const EventExactArgs&, const SkyAxes&, int, int, hipStream_t) {
  return hipErrorNoDevice;
}
hipError_t launch_event_origin(const EventRowsArgs&, const EventOriginArgs&, const SkyAxes&, int, const OriginAxes&, int, hipStream_t) {
  return hipErrorNoDevice;
}
MFn nl_eval_math(int) { return nullptr; }
hipError_t launch_eval_math(int, int, int64_t, const double*, const double*, double*, double*, hipStream_t) {
  return hipErrorNoDevice;
}
}  // namespace art
