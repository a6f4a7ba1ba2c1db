// art_event_moments.h -- the second moments of the binned event power (art_event_moments_device): the
// Monte-Carlo errors of the flux table, the sky map and the totals. The independent unit of a run is
// the EVENT (one sampled conversion point); the rows of one event, the leaves of one forward tree,
// are correlated. So per event e and bin b the content X_{e,b} = Σ power of e's final rows in b is
// formed first, and Q_b = Σ_e X_{e,b}², C_b = Σ_e X_{e,b} a_e are what the tables take, with
// a_e = (attempts[e] - 1) + (final photon rows of e), the event's part of f_inx.
//
// The per-tree group-by is written once as __host__ __device__ functions over one tree's list of
// MomentEntry: the kernels below and a host build for the CPU tests (tools/eventmoments.cpp) compile
// the same source. The kernels themselves need art_kernels.hip's np_hist_bin, sky_bin_of, EventLoad
// and event_row and are compiled only there (ART_EVENT_MOMENTS_KERNELS).
#pragma once
#include "art_core.h"

namespace art {

// art_event_moments_out::totals
enum { EM_TOT_EVENTS = 0, EM_TOT_A1, EM_TOT_A2, EM_TOT_Q_AXION, EM_TOT_Q_PHOTON, EM_TOT_C_AXION, EM_TOT_C_PHOTON,
       EM_TOT_BAD, EM_TOT_COUNT };

// What pass A leaves of one node record, 16 B. flux: the flat flux bin species * nbins + bin of a
// final node, or for one the flux table does not count MOMENT_AXION / MOMENT_PHOTON (its species is
// still needed: the totals take every final row), or MOMENT_NONE for a record that is not a final
// node of its tree's range. sky: the flat sky bin, -1 for not counted.
constexpr int32_t MOMENT_NONE = -1, MOMENT_AXION = -2, MOMENT_PHOTON = -3;
struct alignas(16) MomentEntry {
  int32_t flux, sky;
  double power;
};
enum { MOMENT_KEY_FLUX = 0, MOMENT_KEY_SKY, MOMENT_KEY_SPECIES };

__host__ __device__ inline bool moment_final(const MomentEntry& t) { return t.flux != MOMENT_NONE; }
__host__ __device__ inline int moment_species(const MomentEntry& t, int nbins) {
  return t.flux >= 0 ? (t.flux >= nbins ? 1 : 0) : (t.flux == MOMENT_PHOTON ? 1 : 0);
}
// the group an entry belongs to in table `which`, -1 for none
__host__ __device__ inline int moment_key(const MomentEntry& t, int which, int nbins) {
  if (!moment_final(t)) return -1;
  if (which == MOMENT_KEY_FLUX) return t.flux >= 0 ? t.flux : -1;
  if (which == MOMENT_KEY_SKY) return t.sky;
  return moment_species(t, nbins);
}

// The group-by of one tree: t[0, c) are its records' entries in node order. When entry j is the FIRST
// of its group in table `which`, returns the group's key and its content X, the powers of the group
// summed in node order; -1 otherwise, so every (tree, key) group is reported by exactly one j.
__host__ __device__ inline int moment_group(const MomentEntry* t, int64_t c, int64_t j, int which, int nbins, double* X) {
  const int key = moment_key(t[j], which, nbins);
  if (key < 0) return -1;
  for (int64_t i = 0; i < j; ++i)
    if (moment_key(t[i], which, nbins) == key) return -1;
  double x = t[j].power;
  for (int64_t i = j + 1; i < c; ++i)
    if (moment_key(t[i], which, nbins) == key) x += t[i].power;
  *X = x;
  return key;
}

// moment_group with the powers taken from pw[0, c), the tree's records' powers at another coupling
// (art_event_reweight.h), in the place of the entries' own: the same groups, keys and order of adds
__host__ __device__ inline int moment_group_scaled(const MomentEntry* t, const double* pw, int64_t c, int64_t j, int which,
                                                   int nbins, double* X) {
  const int key = moment_key(t[j], which, nbins);
  if (key < 0) return -1;
  for (int64_t i = 0; i < j; ++i)
    if (moment_key(t[i], which, nbins) == key) return -1;
  double x = pw[j];
  for (int64_t i = j + 1; i < c; ++i)
    if (moment_key(t[i], which, nbins) == key) x += pw[i];
  *X = x;
  return key;
}

// the final photon rows among a tree's entries: with attempts - 1 the event's a_e
__host__ __device__ inline int64_t moment_photon_rows(const MomentEntry* t, int64_t c, int nbins) {
  int64_t m = 0;
  for (int64_t i = 0; i < c; ++i)
    if (moment_final(t[i]) && moment_species(t[i], nbins) == 1) ++m;
  return m;
}

}  // namespace art

#ifdef ART_EVENT_MOMENTS_KERNELS
namespace art {

// record i lies in the range of its own tree: node_start[tree] <= i < node_start[tree + 1]
__device__ inline bool moment_in_own_range(const EventMomentsArgs& m, int64_t n_events, int64_t i, int64_t tree) {
  return tree >= 0 && tree < n_events && m.node_start[tree] <= i && i < m.node_start[tree + 1];
}

// Pass A, one lane per node record: the entry of a final node that lies in its own tree's range --
// bins and power by event_row(row = nullptr), np_hist_bin and sky_bin_of, as event_rows_kernel takes
// them, so a row is in the same bin in the first and in the second moments. A record inside some
// tree's range whose `tree` is another is counted in totals[7] and gets no entry.
__global__ __launch_bounds__(256) void event_moments_entries_kernel(const EventRowsArgs a, const EventMomentsArgs m,
                                                                   const SkyAxes A, const int cos_axis) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double bad = 0.0;
  if (i < a.n_nodes) {
    const art_tree_node& nd = a.nodes[i];
    const int64_t e = nd.tree;
    MomentEntry t{MOMENT_NONE, -1, 0.0};
    if (!moment_in_own_range(m, a.n_events, i, e)) {
      if (m.node_start[0] <= i && i < m.node_start[a.n_events]) bad = 1.0;
    } else if (nd.is_final != 0) {
      const EventLoad E{a, e};
      double tau = 0.0;
      if (a.cyc_slot) {
        const int64_t j = a.cyc_slot[i];
        if (j >= 0 && j < a.cyc_n) tau = a.cyc_tau[j];
      }
      const EventRowBins B = event_row(nd, E, a.event_offset, a.mass_a, tau, a.cyc_slot != nullptr, EVENT_COLS_SHORT,
                                       (double*)nullptr);
      const int fb = m.nbins > 0 ? np_hist_bin(B.phi, m.nbins) : -1;
      t.flux = fb >= 0 ? B.species * m.nbins + fb : (B.species ? MOMENT_PHOTON : MOMENT_AXION);
      t.sky = m.sky_sq ? sky_bin_of(A, cos_axis ? B.cos_theta : B.theta, B.phi, B.dw, B.species) : -1;
      t.power = B.power;
    }
    m.entries[i] = t;
  }
  for (int off = warpSize / 2; off > 0; off >>= 1) bad += __shfl_down(bad, off);
  if ((threadIdx.x & (warpSize - 1)) == 0 && bad != 0.0) unsafeAtomicAdd(&m.totals[EM_TOT_BAD], bad);
}

// the entries of tree e: its range cut to the records there are
__device__ inline const MomentEntry* moment_tree(const EventMomentsArgs& m, int64_t n_nodes, int64_t e, int64_t* c,
                                                 int64_t* first) {
  if (!m.node_start) {
    *c = 0, *first = 0;
    return m.entries;
  }
  int64_t s0 = m.node_start[e], s1 = m.node_start[e + 1];
  s0 = s0 < 0 ? 0 : (s0 > n_nodes ? n_nodes : s0);
  s1 = s1 < s0 ? s0 : (s1 > n_nodes ? n_nodes : s1);
  *c = s1 - s0, *first = s0;
  return m.entries + s0;
}

// Pass B, one lane per node record and per event (grid-stride). The lane of the first row of an
// (event, bin) group sums the group over its tree's entries (small cached reads) and adds X² and
// X a_e to the tables in HBM, once per group; the same for the two species, into the totals. Lane
// i < n_events also adds event i's 1, a_e and a_e². The totals are summed per lane, then per wave,
// and added once per wave.
__global__ __launch_bounds__(256) void event_moments_kernel(const EventRowsArgs a, const EventMomentsArgs m) {
  double tot[EM_TOT_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
    const int64_t i = i0 + threadIdx.x;
    if (i < a.n_events) {
      int64_t c, first;
      const MomentEntry* t = moment_tree(m, a.n_nodes, i, &c, &first);
      const double ae = (double)((a.attempts ? (int64_t)a.attempts[i] - 1 : 0) + moment_photon_rows(t, c, m.nbins));
      tot[EM_TOT_EVENTS] += 1.0;
      tot[EM_TOT_A1] += ae;
      tot[EM_TOT_A2] += ae * ae;
    }
    if (i >= a.n_nodes || !moment_final(m.entries[i])) continue;
    const int64_t e = a.nodes[i].tree;  // (an entry is final only in its own tree's range)
    int64_t c, first;
    const MomentEntry* t = moment_tree(m, a.n_nodes, e, &c, &first);
    const int64_t j = i - first;
    if (j < 0 || j >= c) continue;
    double ae = -1.0, X;
    for (int which = MOMENT_KEY_FLUX; which <= MOMENT_KEY_SPECIES; ++which) {
      const int key = moment_group(t, c, j, which, m.nbins, &X);
      if (key < 0) continue;
      if (ae < 0.0) ae = (double)((a.attempts ? (int64_t)a.attempts[e] - 1 : 0) + moment_photon_rows(t, c, m.nbins));
      if (which == MOMENT_KEY_FLUX) {
        unsafeAtomicAdd(&m.flux_sq[key], X * X);
        unsafeAtomicAdd(&m.flux_xa[key], X * ae);
      } else if (which == MOMENT_KEY_SKY) {
        unsafeAtomicAdd(&m.sky_sq[key], X * X);
        unsafeAtomicAdd(&m.sky_xa[key], X * ae);
      } else {
        tot[EM_TOT_Q_AXION + key] += X * X;
        tot[EM_TOT_C_AXION + key] += X * ae;
      }
    }
  }
  for (int q = 0; q < EM_TOT_BAD; ++q) {
    double t = tot[q];
    for (int off = warpSize / 2; off > 0; off >>= 1) t += __shfl_down(t, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && t != 0.0) unsafeAtomicAdd(&m.totals[q], t);
  }
}

// Pass B of a scan (the coupling scan's and the halo scan's moments kernels), one lane per node
// record and per event: event_moments_kernel's group-by over pass A's entries -- the bins and a_e are
// the run's own for every k -- with the powers of set k, r.Pw[k n_nodes + record], in the place of the
// entries' own. Scan: r.n_k sets, r.Pw, r.sky_size and the tables r.flux_sq, r.flux_xa, r.sky_sq,
// r.sky_xa and r.mtotals, set k's part at k times the usual size.
template <class Scan>
__device__ inline void moment_scan_tables(const EventRowsArgs& a, const EventMomentsArgs& m, const Scan& r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double ev[3] = {0.0, 0.0, 0.0};  // events, a_e, a_e²
  if (i < a.n_events) {
    int64_t c, first;
    const MomentEntry* t = moment_tree(m, a.n_nodes, i, &c, &first);
    const double ae = (double)((a.attempts ? (int64_t)a.attempts[i] - 1 : 0) + moment_photon_rows(t, c, m.nbins));
    ev[0] = 1.0, ev[1] = ae, ev[2] = ae * ae;
  }
  const MomentEntry* t = nullptr;
  int64_t c = 0, first = 0, j = -1;
  double ae = 0.0;
  if (i < a.n_nodes && moment_final(m.entries[i])) {
    const int64_t e = a.nodes[i].tree;  // (an entry is final only in its own tree's range)
    t = moment_tree(m, a.n_nodes, e, &c, &first);
    j = i - first;
    if (j < 0 || j >= c) j = -1;
    else ae = (double)((a.attempts ? (int64_t)a.attempts[e] - 1 : 0) + moment_photon_rows(t, c, m.nbins));
  }
  for (int k = 0; k < r.n_k; ++k) {
    double tot[EM_TOT_BAD] = {ev[0], ev[1], ev[2], 0.0, 0.0, 0.0, 0.0};
    if (j >= 0) {
      const double* pw = r.Pw + k * a.n_nodes + first;
      double X;
      for (int which = MOMENT_KEY_FLUX; which <= MOMENT_KEY_SPECIES; ++which) {
        const int key = moment_group_scaled(t, pw, c, j, which, m.nbins, &X);
        if (key < 0) continue;
        if (which == MOMENT_KEY_FLUX) {
          unsafeAtomicAdd(&r.flux_sq[(int64_t)k * 2 * m.nbins + key], X * X);
          unsafeAtomicAdd(&r.flux_xa[(int64_t)k * 2 * m.nbins + key], X * ae);
        } else if (which == MOMENT_KEY_SKY) {
          unsafeAtomicAdd(&r.sky_sq[k * r.sky_size + key], X * X);
          unsafeAtomicAdd(&r.sky_xa[k * r.sky_size + key], X * ae);
        } else {
          tot[EM_TOT_Q_AXION + key] = X * X;
          tot[EM_TOT_C_AXION + key] = X * ae;
        }
      }
    }
    for (int q = 0; q < EM_TOT_BAD; ++q) {
      double v = tot[q];
      for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
      if ((threadIdx.x & (warpSize - 1)) == 0 && v != 0.0) unsafeAtomicAdd(&r.mtotals[k * EM_TOT_COUNT + q], v);
    }
  }
}

// The moments tail of a scan's launch (host code; launch_event_reweight's and launch_event_halo_scan's): pass A
// over the run's own records, then `kernel`, the scan's __global__ wrapper of moment_scan_tables.
template <class Scan>
hipError_t launch_scan_moments(void (*kernel)(EventRowsArgs, EventMomentsArgs, Scan), const EventRowsArgs& a, const Scan& r,
                               const SkyAxes& A, int cos_axis, hipStream_t s) {
  EventMomentsArgs m{};
  m.node_start = r.node_start; m.nbins = r.nbins; m.entries = r.entries;
  m.sky_sq = r.sky_sq;   // (pass A reads it as "there is a sky table" only)
  m.totals = r.mtotals;  // (pass A's misplaced records: slot 7 of the first set)
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(event_moments_entries_kernel, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a, m, A,
                       cos_axis);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, m, r);
  return hipGetLastError();
}

hipError_t launch_event_moments(const EventRowsArgs& a, const EventMomentsArgs& m, const SkyAxes& A, int cos_axis,
                                hipStream_t s) {
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  if (n <= 0) return hipSuccess;
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(event_moments_entries_kernel, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a, m, A,
                       cos_axis);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(event_moments_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, a, m);
  return hipGetLastError();
}

}  // namespace art
#endif  // ART_EVENT_MOMENTS_KERNELS
