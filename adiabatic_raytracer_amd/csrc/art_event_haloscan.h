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
// and the group-by are art_event_moments.h's). They need art_kernels.hip's np_hist_bin, sky_bin_of,
// EventLoad and event_row, and art_event_moments.h's entries, and are compiled only there
// (ART_EVENT_HALOSCAN_KERNELS).
#pragma once
#include "art_core.h"
#include "art_event_moments.h"
#include "art_halo.h"

namespace art {

// art_event_halo_scan_out::totals, per model
enum { HS_TOT_SUM_AXION = 0, HS_TOT_SUM_PHOTON, HS_TOT_RATIO, HS_TOT_RATIO_SQ, HS_TOT_MISPLACED, HS_TOT_COUNT };

}  // namespace art

#ifdef ART_EVENT_HALOSCAN_KERNELS
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
    double s1 = R, s2 = R * R;
    for (int off = warpSize / 2; off > 0; off >>= 1) {
      s1 += __shfl_down(s1, off);
      s2 += __shfl_down(s2, off);
    }
    if ((threadIdx.x & (warpSize - 1)) == 0 && s1 != 0.0) {
      unsafeAtomicAdd(&h.totals[k * HS_TOT_COUNT + HS_TOT_RATIO], s1);
      unsafeAtomicAdd(&h.totals[k * HS_TOT_COUNT + HS_TOT_RATIO_SQ], s2);
    }
  }
}

// One lane per node record. A final record in its own tree's range takes its bins and its event's
// values once, by event_row(row = nullptr), np_hist_bin and sky_bin_of, so it falls into the bins
// event_rows_kernel puts it in; then per model its power, the run's own p_r = column 8 * column 7
// (exp(-τ) included with the cyclotron fields) times R of its event, goes to flux[k], sky[k] and the
// totals. A record inside the forest's range whose `tree` is another tree's is counted (misplaced).
__global__ __launch_bounds__(256) void event_halo_bins_kernel(const EventRowsArgs a, const EventHaloScanArgs h,
                                                              const SkyAxes A, const int cos_axis) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool fin = false;
  int sp = 0, fb = -1, sb = -1;
  double pr = 0.0, bad = 0.0;
  int64_t e = 0;
  if (i < a.n_nodes) {
    const art_tree_node& nd = a.nodes[i];
    e = nd.tree;
    if (!(e >= 0 && e < a.n_events && h.node_start[e] <= i && i < h.node_start[e + 1])) {
      if (h.node_start[0] <= i && i < h.node_start[a.n_events]) bad = 1.0;
    } else if (nd.is_final != 0) {
      fin = true;
      const EventLoad E{a, e};
      double tau = 0.0;
      if (a.cyc_slot) {
        const int64_t j = a.cyc_slot[i];
        if (j >= 0 && j < a.cyc_n) tau = a.cyc_tau[j];
      }
      const EventRowBins Bn = event_row(nd, E, a.event_offset, a.mass_a, tau, a.cyc_slot != nullptr, EVENT_COLS_SHORT,
                                        (double*)nullptr);
      sp = Bn.species;
      pr = Bn.power;
      if (h.nbins > 0) fb = np_hist_bin(Bn.phi, h.nbins);
      if (h.sky) sb = sky_bin_of(A, cos_axis ? Bn.cos_theta : Bn.theta, Bn.phi, Bn.dw, sp);
    }
  }
  for (int off = warpSize / 2; off > 0; off >>= 1) bad += __shfl_down(bad, off);
  for (int k = 0; k < h.n_k; ++k) {
    double pw = 0.0;
    if (fin) {
      pw = pr * h.R[k * a.n_events + e];
      if (fb >= 0) unsafeAtomicAdd(&h.flux[(int64_t)k * 2 * h.nbins + sp * h.nbins + fb], pw);
      if (sb >= 0) unsafeAtomicAdd(&h.sky[k * h.sky_size + sb], pw);
    }
    if (h.Pw && i < a.n_nodes) h.Pw[k * a.n_nodes + i] = pw;
    double ta = sp == 0 ? pw : 0.0, tp = sp == 0 ? 0.0 : pw;  // Σ power of axions, of photons
    for (int off = warpSize / 2; off > 0; off >>= 1) {
      ta += __shfl_down(ta, off);
      tp += __shfl_down(tp, off);
    }
    if ((threadIdx.x & (warpSize - 1)) == 0) {
      if (ta != 0.0) unsafeAtomicAdd(&h.totals[k * HS_TOT_COUNT + HS_TOT_SUM_AXION], ta);
      if (tp != 0.0) unsafeAtomicAdd(&h.totals[k * HS_TOT_COUNT + HS_TOT_SUM_PHOTON], tp);
      if (bad != 0.0) unsafeAtomicAdd(&h.totals[k * HS_TOT_COUNT + HS_TOT_MISPLACED], bad);
    }
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
#endif  // ART_EVENT_HALOSCAN_KERNELS
