// art_event_replicates.h -- the jackknife replicates (art_event_replicates_device): the first-moment tables of
// a chunk kept per GROUP of events, g = (event_offset + tree) mod R, so that the error of any function of the
// tables follows from the R leave-one-group-out estimates (trees.jackknife). Per set k (one for the plain run,
// one per coupling or halo model of a scan) and group g: the flux table, the sky map and the two species' totals,
// with the powers and bins of the call the set belongs to --
//   kind 0  p_r = column 8 * column 7 (event_row's power, exp(-τ) included with the cyclotron fields),
//   kind 1  reweight_power(W_k, B_k, cyclotron, τ, sln_prob) of art_event_reweight.h, W_k and B_k the `weights` and
//           `back` that art_event_reweight_device hands out,
//   kind 2  p_r R[k, event], R the `ratio` that art_event_halo_scan_device hands out --
// and per group alone the events n_g, a_g = Σ_e ((attempts[e] - 1) + e's final photon rows), whose sum over the
// groups is f_inx, and the records that lie in the range of a tree other than their own (skipped, as in the moments).
//
// One kernel, one lane per node record and per event. The kernel needs art_kernels.hip's np_hist_bin, sky_bin_of,
// EventLoad and event_row and art_event_reweight.h's reweight_power, and is compiled only there
// (ART_EVENT_REPLICATES_KERNELS). No LDS table: R flux tables and R sky maps rarely fit the 8192 doubles a block may
// take, so every table is added to in HBM.
#pragma once
#include "art_core.h"
#include "art_event_reweight.h"

namespace art {

constexpr int REPLICATES_MIN_GROUPS = 2, REPLICATES_MAX_GROUPS = 64, REPLICATES_MAX_SETS = 32;
enum { REP_KIND_RUN = 0, REP_KIND_COUPLING, REP_KIND_HALO, REP_KIND_COUNT };
// art_event_replicates_out::groups, per group
enum { REP_GRP_EVENTS = 0, REP_GRP_A, REP_GRP_MISPLACED, REP_GRP_COUNT };

// the group of the event with the global id `id` (any sign: a misplaced record's `tree` is arbitrary)
__host__ __device__ inline int replicate_group(int64_t id, int R) {
  const int64_t m = id % R;
  return (int)(m < 0 ? m + R : m);
}

}  // namespace art

#ifdef ART_EVENT_REPLICATES_KERNELS
namespace art {

// One lane per node record and per event (n = max(n_nodes, n_events) lanes).
//   As an event, lane i adds 1 and attempts[i] - 1 to its group's n_g and a_g.
//   As a record, a final record in its own tree's range takes its bins and its event's values once, by
//   event_row(row = nullptr), np_hist_bin and sky_bin_of, so it falls into the bins event_rows_kernel puts it in;
//   a photon adds 1 to its group's a_g; then per set its power goes to flux[k][g], sky[k][g] and totals[k][g].
// The per-group counts go through a block-private LDS table of 3 R doubles, flushed once per block. The totals are
// summed over the runs of lanes of one group in a wave -- the records of a tree are neighbours, so a wave holds few
// runs -- with a segmented __shfl_down, and added once per run.
__global__ __launch_bounds__(256) void event_replicates_kernel(const EventRowsArgs a, const EventReplicatesArgs r,
                                                               const SkyAxes A, const int cos_axis) {
  __shared__ double sh_grp[REP_GRP_COUNT * REPLICATES_MAX_GROUPS];
  const int R = r.n_groups;
  for (int q = threadIdx.x; q < REP_GRP_COUNT * R; q += blockDim.x) sh_grp[q] = 0.0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.n_events) {
    const int ge = replicate_group(a.event_offset + i, R);
    atomicAdd(&sh_grp[ge * REP_GRP_COUNT + REP_GRP_EVENTS], 1.0);
    if (a.attempts) atomicAdd(&sh_grp[ge * REP_GRP_COUNT + REP_GRP_A], (double)((int64_t)a.attempts[i] - 1));
  }
  bool fin = false;
  int sp = 0, fb = -1, sb = -1, g = -1;
  double pr = 0.0, tau = 0.0, sln = 0.0;
  int64_t e = 0;
  if (i < a.n_nodes) {
    const art_tree_node& nd = a.nodes[i];
    e = nd.tree;
    if (!(e >= 0 && e < a.n_events && r.node_start[e] <= i && i < r.node_start[e + 1])) {
      if (r.node_start[0] <= i && i < r.node_start[a.n_events])
        atomicAdd(&sh_grp[replicate_group(a.event_offset + e, R) * REP_GRP_COUNT + REP_GRP_MISPLACED], 1.0);
    } else {
      g = replicate_group(a.event_offset + e, R);
      if (nd.is_final != 0) {
        fin = true;
        const EventLoad E{a, e};
        if (a.cyc_slot) {
          const int64_t j = a.cyc_slot[i];
          if (j >= 0 && j < a.cyc_n) tau = a.cyc_tau[j];
        }
        const EventRowBins Bn = event_row(nd, E, a.event_offset, a.mass_a, tau, a.cyc_slot != nullptr, EVENT_COLS_SHORT,
                                          (double*)nullptr);
        sp = Bn.species;
        pr = Bn.power;
        sln = E.sln_prob();
        if (r.nbins > 0) fb = np_hist_bin(Bn.phi, r.nbins);
        if (r.sky) sb = sky_bin_of(A, cos_axis ? Bn.cos_theta : Bn.theta, Bn.phi, Bn.dw, sp);
        if (sp == 1) atomicAdd(&sh_grp[g * REP_GRP_COUNT + REP_GRP_A], 1.0);
      }
    }
  }
  // the runs of one group among a wave's lanes: `seg` counts the run heads up to this lane, so it does not fall
  // along the wave and equal numbers are neighbours, which the segmented sum below needs
  const int lane = threadIdx.x & (warpSize - 1);
  const int g_prev = __shfl_up(g, 1);
  const bool head = lane == 0 || g_prev != g;
  const unsigned long long heads = __ballot(head);
  const int seg = __popcll(heads & (~0ull >> (63 - lane)));
  for (int k = 0; k < r.n_k; ++k) {
    double pw = 0.0;
    if (fin) {
      if (r.kind == REP_KIND_RUN) pw = pr;
      else if (r.kind == REP_KIND_COUPLING)
        pw = reweight_power(r.node_factor[k * a.n_nodes + i], r.event_factor[k * a.n_events + e], a.cyc_slot != nullptr,
                            tau, sln);
      else pw = pr * r.event_factor[k * a.n_events + e];
      const int64_t kg = (int64_t)k * R + g;
      if (fb >= 0) unsafeAtomicAdd(&r.flux[kg * 2 * r.nbins + sp * r.nbins + fb], pw);
      if (sb >= 0) unsafeAtomicAdd(&r.sky[kg * r.sky_size + sb], pw);
    }
    double ta = sp == 0 ? pw : 0.0, tp = sp == 0 ? 0.0 : pw;  // Σ power of axions, of photons
    for (int off = 1; off < warpSize; off <<= 1) {
      const double oa = __shfl_down(ta, off), op = __shfl_down(tp, off);
      const int os = __shfl_down(seg, off);
      if (lane + off < warpSize && os == seg) {
        ta += oa;
        tp += op;
      }
    }
    if (head && g >= 0) {
      const int64_t kg = (int64_t)k * R + g;
      if (ta != 0.0) unsafeAtomicAdd(&r.totals[kg * 2], ta);
      if (tp != 0.0) unsafeAtomicAdd(&r.totals[kg * 2 + 1], tp);
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < REP_GRP_COUNT * R; q += blockDim.x)
    if (sh_grp[q] != 0.0) unsafeAtomicAdd(&r.groups[q], sh_grp[q]);
}

hipError_t launch_event_replicates(const EventRowsArgs& a, const EventReplicatesArgs& r, const SkyAxes& A, int cos_axis,
                                   hipStream_t s) {
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(event_replicates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, r, A, cos_axis);
  return hipGetLastError();
}

}  // namespace art
#endif  // ART_EVENT_REPLICATES_KERNELS
