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
// One kernel, one lane per node record and per event. The kernel takes its records through art_event_record.h and
// is compiled only in art_kernels.hip (ART_EVENT_KERNELS). No LDS table: R flux tables and R sky maps rarely fit the
// 8192 doubles a block may take, so every table is added to in HBM.
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

#ifdef ART_EVENT_KERNELS
namespace art {

// The power of a final record in set k of a call whose sets are of `kind` (Set: EventReplicatesArgs or
// EventSpectrumArgs): pr the run's own power, i and e the record and its event, tau and sln read by kind 1 only. The
// operations, and their order, are reweight_power's and pr * F.
template <class Set>
__device__ inline double set_power(const EventRowsArgs& a, const Set& r, int k, int64_t i, int64_t e, double pr, double tau,
                                   double sln) {
  if (r.kind == REP_KIND_RUN) return pr;
  if (r.kind == REP_KIND_COUPLING)  // (each kind loads its own factors: a load shared by two branches stays pending
                                    // on the way round them, and the wait for it also waits for the set's atomic adds)
    return reweight_power(r.node_factor[k * a.n_nodes + i], r.event_factor[k * a.n_events + e], a.cyc_slot != nullptr, tau,
                          sln);
  return pr * r.event_factor[k * a.n_events + e];
}

// One lane per node record and per event (n = max(n_nodes, n_events) lanes).
//   As an event, lane i adds 1 and attempts[i] - 1 to its group's n_g and a_g.
//   As a record, a final record of its own tree's range takes its bins and its event's values once (event_record,
//   art_event_record.h) and a misplaced one adds 1 to the count of the group its `tree` names;
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
  const EventRecord rec = event_record(a, r.node_start, i, r.nbins, r.sky != nullptr, A, cos_axis);
  const bool fin = rec.state == RECORD_FINAL;
  const int sp = rec.species, fb = rec.fb, sb = rec.sb;
  const int64_t e = rec.e;
  const int g = rec.state >= RECORD_OWN ? replicate_group(a.event_offset + e, R) : -1;
  if (rec.state == RECORD_MISPLACED)
    atomicAdd(&sh_grp[replicate_group(a.event_offset + e, R) * REP_GRP_COUNT + REP_GRP_MISPLACED], 1.0);
  if (fin && sp == 1) atomicAdd(&sh_grp[g * REP_GRP_COUNT + REP_GRP_A], 1.0);
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
      pw = set_power(a, r, k, i, e, rec.power, rec.tau, rec.sln);
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
#endif  // ART_EVENT_KERNELS
