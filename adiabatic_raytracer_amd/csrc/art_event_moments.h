// art_event_moments.h -- the second moments of the binned event power (art_event_moments_device): the
// Monte-Carlo errors of the flux table, the sky map and the totals. The independent unit of a run is
// the EVENT (one sampled conversion point); the rows of one event, the leaves of one forward tree,
// are correlated. So per event e and bin b the content X_{e,b} = Σ power of e's final rows in b is
// formed first, and Q_b = Σ_e X_{e,b}², C_b = Σ_e X_{e,b} a_e are what the tables take, with
// a_e = (attempts[e] - 1) + (final photon rows of e), the event's part of f_inx.
//
// The per-tree group-by is written once as __host__ __device__ functions over one tree's list of
// MomentEntry: the kernels below and a host build for the CPU tests (tools/eventmoments.cpp) compile
// the same source. The kernels themselves take their records through art_event_record.h and are
// compiled only in art_kernels.hip (ART_EVENT_KERNELS).
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

#ifdef ART_EVENT_KERNELS
namespace art {

// Pass A, one lane per node record, of the moments, of the scans' moments and (BINS = false: no acos, no atan2, no
// bin search) of the spectrum: the entry of a final record of its own tree's range (event_record, art_event_record.h),
// so a row is in the same bin in the first and in the second moments. A misplaced record is counted in *misplaced and
// gets no entry.
template <bool BINS>
__global__ __launch_bounds__(256) void event_entries_kernel(const EventRowsArgs a, const int64_t* node_start,
                                                            MomentEntry* entries, const int nbins, const int sky,
                                                            double* misplaced, const SkyAxes A, const int cos_axis) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const EventRecord rec = event_record(a, node_start, i, BINS ? nbins : 0, BINS && sky, A, cos_axis);
  if (i < a.n_nodes) {
    MomentEntry t{MOMENT_NONE, -1, 0.0};
    if (rec.state == RECORD_FINAL) {
      t.flux = rec.fb >= 0 ? rec.species * nbins + rec.fb : (rec.species ? MOMENT_PHOTON : MOMENT_AXION);
      t.sky = rec.sb;
      t.power = rec.power;
    }
    entries[i] = t;
  }
  wave_add(misplaced, rec.state == RECORD_MISPLACED ? 1.0 : 0.0);
}

// pass A's launch (host code): nothing without records
template <bool BINS>
hipError_t launch_event_entries(const EventRowsArgs& a, const int64_t* node_start, MomentEntry* entries, int nbins,
                                bool sky, double* misplaced, const SkyAxes& A, int cos_axis, hipStream_t s) {
  if (a.n_nodes <= 0) return hipSuccess;
  hipLaunchKernelGGL(event_entries_kernel<BINS>, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a, node_start,
                     entries, nbins, (int)sky, misplaced, A, cos_axis);
  return hipGetLastError();
}

// the entries of tree e: its range cut to the records there are
__device__ inline const MomentEntry* moment_tree(const EventMomentsArgs& m, int64_t n_nodes, int64_t e, int64_t* c,
                                                 int64_t* first) {
  *c = tree_range(m.node_start, n_nodes, e, first);
  return m.entries + *first;
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
      const double ae = (double)(event_attempts_m1(a, i) + moment_photon_rows(t, c, m.nbins));
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
      if (ae < 0.0) ae = (double)(event_attempts_m1(a, e) + moment_photon_rows(t, c, m.nbins));
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
  for (int q = 0; q < EM_TOT_BAD; ++q) wave_add(&m.totals[q], tot[q]);
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
    const double ae = (double)(event_attempts_m1(a, i) + moment_photon_rows(t, c, m.nbins));
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
    else ae = (double)(event_attempts_m1(a, e) + moment_photon_rows(t, c, m.nbins));
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
    for (int q = 0; q < EM_TOT_BAD; ++q) wave_add(&r.mtotals[k * EM_TOT_COUNT + q], tot[q]);
  }
}

// The moments tail of a scan's launch (host code; launch_event_reweight's and launch_event_halo_scan's): pass A
// over the run's own records (its misplaced records: slot 7 of the first set), then `kernel`, the scan's __global__
// wrapper of moment_scan_tables.
template <class Scan>
hipError_t launch_scan_moments(void (*kernel)(EventRowsArgs, EventMomentsArgs, Scan), const EventRowsArgs& a, const Scan& r,
                               const SkyAxes& A, int cos_axis, hipStream_t s) {
  EventMomentsArgs m{};
  m.node_start = r.node_start; m.nbins = r.nbins; m.entries = r.entries;
  const hipError_t e = launch_event_entries<true>(a, r.node_start, r.entries, r.nbins, r.sky_sq != nullptr,
                                                  &r.mtotals[EM_TOT_BAD], A, cos_axis, s);
  if (e != hipSuccess) return e;
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, m, r);
  return hipGetLastError();
}

hipError_t launch_event_moments(const EventRowsArgs& a, const EventMomentsArgs& m, const SkyAxes& A, int cos_axis,
                                hipStream_t s) {
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  if (n <= 0) return hipSuccess;
  const hipError_t e = launch_event_entries<true>(a, m.node_start, m.entries, m.nbins, m.sky_sq != nullptr,
                                                  &m.totals[EM_TOT_BAD], A, cos_axis, s);
  if (e != hipSuccess) return e;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(event_moments_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, a, m);
  return hipGetLastError();
}

}  // namespace art
#endif  // ART_EVENT_KERNELS
