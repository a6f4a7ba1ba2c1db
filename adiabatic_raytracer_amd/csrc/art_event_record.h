// art_event_record.h -- what the event kernels share on the device (art_event_moments.h, _reweight.h, _haloscan.h,
// _replicates.h, _grid.h, _spectrum.h): which node record counts and into which bins, a tree's range, the first term
// of a_e and the wave sum. Device only: art_kernels.hip includes it once, below np_hist_bin (art_ray_io.h), sky_bin_of
// and event_row (art_event_rows.h) and above those six headers.
//
// THE RECORD RULE. Tree e owns the records [node_start[e], node_start[e + 1]), and every per-tree walk -- the
// moments' group-by, the scans' weights, the grid's wave -- takes the records of that range for e's. So a record
// counts only where its `tree` names the range it lies in: then it is `own`, and `final` with is_final != 0, when it
// takes its event's values, its power and its bins once through event_row(row = nullptr), np_hist_bin and sky_bin_of,
// the calls event_rows_kernel makes, so that a row falls into the same bins in every table. A record inside the
// forest, [node_start[0], node_start[n_events]), whose `tree` names another range is `misplaced`: no walk would
// reach it under its own event and the walk of the range it lies in would take it for the wrong one, so it is kept
// out of every table (skipped) and counted, and the caller fails on the count rather than publish sums that miss a
// row. Records beyond the forest are spare capacity: neither counted nor skipped.
// event_rows_kernel (art_kernels.hip) has another rule, stated there.
#pragma once
#include "art_core.h"
#include "art_event_rows.h"
#include "art_internal.h"

namespace art {

// event_row's source of its event's values: each is loaded from HBM where its column is written
struct EventLoad {
  const EventRowsArgs& a;
  const int64_t e;
  __device__ double x(int c) const { return a.x[c * a.n_events + e]; }
  __device__ double k(int c) const { return a.k_init[c * a.n_events + e]; }
  __device__ double cos_w() const { return a.weight5[e]; }
  __device__ double sln_prob() const { return a.weight5[2 * a.n_events + e]; }
  __device__ double vel_eng() const { return a.weight5[4 * a.n_events + e]; }
  __device__ double back_prob() const { return a.back[e].prob; }
  __device__ double back_weight() const { return a.back[e].weight; }
  __device__ double back_count() const { return (double)a.back_counts[e]; }
  __device__ double count() const { return (double)a.counts[e]; }
  __device__ double info() const { return (double)a.infos[e]; }
};

// the cyclotron optical depth of record i's last segment: its re-run's, 0 without one
__device__ inline double event_tau(const EventRowsArgs& a, int64_t i) {
  if (!a.cyc_slot) return 0.0;
  const int64_t j = a.cyc_slot[i];
  return j >= 0 && j < a.cyc_n ? a.cyc_tau[j] : 0.0;
}

// Record i by the rule above. e is the record's `tree` whatever the state; the other fields are a final record's:
// fb the flux bin of nbins (-1: none, or nbins == 0), sb the flat sky bin (-1: none, or !want_sky), power event_row's,
// tau and sln its event_tau and its event's sln_prob. Inlined: a caller pays for the fields it reads only (without
// the bins no acos, no atan2, no search). node_start is not read for i >= a.n_nodes (it may be null without records).
enum { RECORD_NONE = 0, RECORD_MISPLACED, RECORD_OWN, RECORD_FINAL };
struct EventRecord {
  int state = RECORD_NONE;
  int64_t e = 0;
  int species = 0, fb = -1, sb = -1;
  double power = 0.0, tau = 0.0, sln = 0.0;
};
__device__ __forceinline__ EventRecord event_record(const EventRowsArgs& a, const int64_t* node_start, int64_t i,
                                                    int nbins, bool want_sky, const SkyAxes& A, int cos_axis) {
  EventRecord rec;
  if (i >= a.n_nodes) return rec;
  const art_tree_node& nd = a.nodes[i];
  const int64_t e = rec.e = nd.tree;
  if (!(e >= 0 && e < a.n_events && node_start[e] <= i && i < node_start[e + 1])) {
    if (node_start[0] <= i && i < node_start[a.n_events]) rec.state = RECORD_MISPLACED;
    return rec;
  }
  rec.state = RECORD_OWN;
  if (nd.is_final == 0) return rec;
  rec.state = RECORD_FINAL;
  const EventLoad E{a, e};
  rec.tau = event_tau(a, i);
  const EventRowBins B = event_row(nd, E, a.event_offset, a.mass_a, rec.tau, a.cyc_slot != nullptr, EVENT_COLS_SHORT,
                                   (double*)nullptr);
  rec.species = B.species;
  rec.power = B.power;
  rec.sln = E.sln_prob();
  if (nbins > 0) rec.fb = np_hist_bin(B.phi, nbins);
  if (want_sky) rec.sb = sky_bin_of(A, cos_axis ? B.cos_theta : B.theta, B.phi, B.dw, B.species);
  return rec;
}

// the records of tree e, its range cut to the records there are: their number, *first the first (0 without node_start)
__device__ inline int64_t tree_range(const int64_t* node_start, int64_t n_nodes, int64_t e, int64_t* first) {
  *first = 0;
  if (!node_start) return 0;
  int64_t s0 = node_start[e], s1 = node_start[e + 1];
  s0 = s0 < 0 ? 0 : (s0 > n_nodes ? n_nodes : s0);
  s1 = s1 < s0 ? s0 : (s1 > n_nodes ? n_nodes : s1);
  *first = s0;
  return s1 - s0;
}

// the first term of a_e = (attempts[e] - 1) + e's final photon rows, the event's part of f_inx
__device__ inline int64_t event_attempts_m1(const EventRowsArgs& a, int64_t e) {
  return a.attempts ? (int64_t)a.attempts[e] - 1 : 0;
}

// The sum of v over the wave, in lane 0, and the add of a non-zero one to *dst once per wave. The order of the adds
// and the skipped zero are part of the results.
__device__ inline double wave_sum(double v) {
  for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}
__device__ inline void lane0_add(double* dst, double sum) {
  if ((threadIdx.x & (warpSize - 1)) == 0 && sum != 0.0) unsafeAtomicAdd(dst, sum);
}
__device__ inline void wave_add(double* dst, double v) { lane0_add(dst, wave_sum(v)); }

}  // namespace art
