// art_event_haloscan.h -- the halo scan (art_event_halo_scan_device): one run drawn and weighted under
// a base halo model reweighted to a list of target models. With a halo model the sampler takes only
// the proposal scale vp and the integrator sees the drawn speed through erg, so v0 and v_NS enter in
// one place: the factor F that event_weight_halo multiplies sln_prob by (art_halo.h, halo_factor).
// Two runs with the same seed and the same vp therefore draw the same events, grow the same forests
// and write the same rows but for column 7, and a target model h seen from the base run b is one
// scalar per event, exact for every tree:
//   R_h(u) = F_h / F_b = (v0_b/v0_h)³ exp(|u + v_b|²/v0_b² - |u + v_h|²/v0_h²),   u = C_KM vifty
// (art_halo.h, halo_ratio; the s²/vp² term cancels). The power of a final row under h is the run's own
// column 8 * column 7 times R_h of its event, in the run's own bins.
//
// Three kernels: the ratios per event and model, the bins, and the second moments per model (pass A
// and the group-by are art_event_moments.h's). They take their records through art_event_record.h and
// are compiled only in art_kernels.hip (ART_EVENT_KERNELS).
#pragma once
#include "art_core.h"
#include "art_event_moments.h"
#include "art_halo.h"

namespace art {

// art_event_halo_scan_out::totals, per model
enum { HS_TOT_SUM_AXION = 0, HS_TOT_SUM_PHOTON, HS_TOT_RATIO, HS_TOT_RATIO_SQ, HS_TOT_MISPLACED, HS_TOT_COUNT };

}  // namespace art

#ifdef ART_EVENT_KERNELS
namespace art {

// One lane per event: R[k n_events + e] for every model from the event's three vifty components (SoA,
// coalesced), and Σ_e R and Σ_e R² per model, summed per wave and added once per wave.
__global__ __launch_bounds__(256) void event_halo_ratio_kernel(const int64_t n, const EventHaloScanArgs h) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = e < n;
  double u[3] = {0.0, 0.0, 0.0};
  if (live) {
    u[0] = h.vifty[e] * C_KM;
    u[1] = h.vifty[n + e] * C_KM;
    u[2] = h.vifty[2 * n + e] * C_KM;
  }
  for (int k = 0; k < h.n_k; ++k) {
    double R = 0.0;
    if (live) {
      R = halo_ratio(u, h.base, h.models[k]);
      h.R[k * n + e] = R;
    }
    wave_add(&h.totals[k * HS_TOT_COUNT + HS_TOT_RATIO], R);
    wave_add(&h.totals[k * HS_TOT_COUNT + HS_TOT_RATIO_SQ], R * R);
  }
}

// One lane per node record. A final record of its own tree's range takes its bins and its event's
// values once (event_record, art_event_record.h); then per model its power, the run's own p_r =
// column 8 * column 7 (exp(-τ) included with the cyclotron fields) times R of its event, goes to
// flux[k], sky[k] and the totals. The misplaced records are counted per model.
__global__ __launch_bounds__(256) void event_halo_bins_kernel(const EventRowsArgs a, const EventHaloScanArgs h,
                                                              const SkyAxes A, const int cos_axis) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const EventRecord rec = event_record(a, h.node_start, i, h.nbins, h.sky != nullptr, A, cos_axis);
  const bool fin = rec.state == RECORD_FINAL;
  const int sp = rec.species, fb = rec.fb, sb = rec.sb;
  const double pr = rec.power;
  const int64_t e = rec.e;
  const double bad = wave_sum(rec.state == RECORD_MISPLACED ? 1.0 : 0.0);
  for (int k = 0; k < h.n_k; ++k) {
    double pw = 0.0;
    if (fin) {
      pw = pr * h.R[k * a.n_events + e];
      if (fb >= 0) unsafeAtomicAdd(&h.flux[(int64_t)k * 2 * h.nbins + sp * h.nbins + fb], pw);
      if (sb >= 0) unsafeAtomicAdd(&h.sky[k * h.sky_size + sb], pw);
    }
    if (h.Pw && i < a.n_nodes) h.Pw[k * a.n_nodes + i] = pw;
    wave_add(&h.totals[k * HS_TOT_COUNT + HS_TOT_SUM_AXION], sp == 0 ? pw : 0.0);
    wave_add(&h.totals[k * HS_TOT_COUNT + HS_TOT_SUM_PHOTON], sp == 0 ? 0.0 : pw);
    lane0_add(&h.totals[k * HS_TOT_COUNT + HS_TOT_MISPLACED], bad);
  }
}

// The second moments per model: moment_scan_tables (art_event_moments.h) over the powers the bins
// kernel left in Pw; a_e and the bins are the run's own for every model.
__global__ __launch_bounds__(256) void event_halo_moments_kernel(const EventRowsArgs a, const EventMomentsArgs m,
                                                                 const EventHaloScanArgs h) {
  moment_scan_tables(a, m, h);
}

hipError_t launch_event_halo_scan(const EventRowsArgs& a, const EventHaloScanArgs& h, const SkyAxes& A, int cos_axis,
                                  hipStream_t s) {
  if (a.n_events <= 0) return hipSuccess;
  hipLaunchKernelGGL(event_halo_ratio_kernel, dim3((unsigned)((a.n_events + 255) / 256)), dim3(256), 0, s, a.n_events, h);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(event_halo_bins_kernel, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a, h, A, cos_axis);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (!h.mtotals) return hipSuccess;
  return launch_scan_moments(event_halo_moments_kernel, a, h, A, cos_axis, s);
}

}  // namespace art
#endif  // ART_EVENT_KERNELS
