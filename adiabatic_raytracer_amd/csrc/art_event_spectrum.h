// art_event_spectrum.h -- the event power spectrum (art_event_spectrum_device): the DISTRIBUTION of the per-event
// power X_{e,s}, the quantity whose sums every product of a run is and whose squares the moments take. Per set k (one
// for the plain run, one per coupling or halo model of a scan, the powers by kind as art_event_replicates.h's) and
// species s it keeps
//   a histogram over bins that need no range: bin = bits(X) >> (52 - m) for a finite X > 0, the top 11 + m bits of the
//     IEEE-754 pattern, 2^m bins per octave, 2047 << m bins from the subnormals to the largest finite double --
//     count, Σ X and Σ X² per bin;
//   totals (8): events, events with finite X > 0, with X == 0, bad (negative, NaN, infinite; kept out of every table
//     and list), S = Σ X, Q = Σ X², misplaced records (the first set's first entry only), reserved;
//   the T events with the largest finite X > 0 and their global ids, ordered by (X descending, id ascending), carried
//     in and out, so that the list after any number of calls is a function of the multiset of (X, id) seen.
//
// X_{e,s} is the moments' (art_event_moments.h): the powers of e's final rows of species s summed in node order, the
// double moment_group(..., MOMENT_KEY_SPECIES) and moment_group_scaled return. The bin rule, the order of the list,
// the merge and the per-tree sum are __host__ __device__ functions: the kernels below and a host build for the CPU
// tests (tools/eventspectrum.cpp) compile the same source. The kernels take their records through art_event_record.h
// (pass A is the moments', without the bins) and are compiled only in art_kernels.hip (ART_EVENT_KERNELS).
#pragma once
#include "art_core.h"
#include "art_event_moments.h"
#include "art_event_replicates.h"

namespace art {

constexpr int SPECTRUM_MAX_SUB_BITS = 4, SPECTRUM_MAX_TOP = 256, SPECTRUM_MAX_SETS = REPLICATES_MAX_SETS;
// art_event_spectrum_out::totals, per set and species
enum { SP_TOT_EVENTS = 0, SP_TOT_POSITIVE, SP_TOT_ZEROS, SP_TOT_BAD, SP_TOT_SUM, SP_TOT_SUM_SQ, SP_TOT_MISPLACED,
       SP_TOT_RESERVED, SP_TOT_COUNT };

__host__ __device__ inline int64_t spectrum_bins(int m) { return (int64_t)2047 << m; }

__host__ __device__ inline uint64_t spectrum_bits(double x) { return __builtin_bit_cast(uint64_t, x); }
__host__ __device__ inline double spectrum_value(uint64_t bits) { return __builtin_bit_cast(double, bits); }

// finite and > 0: the patterns 1 .. 0x7fefffffffffffff (a set sign bit, 0, inf and every NaN lie outside)
__host__ __device__ inline bool spectrum_positive(uint64_t bits) { return bits - 1 < 0x7fefffffffffffffull; }

// the bin of x with m sub-octave bits, -1 for an x that is not finite or <= 0. Monotone in x; the lower edge of bin b
// is the double with the pattern b << (52 - m).
__host__ __device__ inline int spectrum_bin(double x, int m) {
  const uint64_t b = spectrum_bits(x);
  return spectrum_positive(b) ? (int)(b >> (52 - m)) : -1;
}

// The order of the top list: (bits a, id a) comes BEFORE (bits b, id b). For finite X > 0 the pattern is monotone in
// X, so this is (X descending, id ascending); the padding (0, -1) comes after every entry.
__host__ __device__ inline bool spectrum_before(uint64_t ba, int64_t ia, uint64_t bb, int64_t ib) {
  return ba > bb || (ba == bb && ia < ib);
}

// In a list sorted by spectrum_before: the entries that come before (kb, ki), with or_equal also those equal to it.
__host__ __device__ inline int spectrum_rank(const uint64_t* lb, const int64_t* li, int n, uint64_t kb, int64_t ki,
                                             bool or_equal) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    const bool in = spectrum_before(lb[mid], li[mid], kb, ki) || (or_equal && lb[mid] == kb && li[mid] == ki);
    if (in) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The place in the merged list of entry i of sorted list a (first = true) or of sorted list b (first = false):
// equal entries of a come before those of b, so the places of the na + nb entries are a permutation of 0 .. na + nb.
__host__ __device__ inline int spectrum_place(const uint64_t* ab, const int64_t* ai, int na, const uint64_t* bb,
                                              const int64_t* bi, int nb, int i, bool first) {
  return first ? i + spectrum_rank(bb, bi, nb, ab[i], ai[i], false) : i + spectrum_rank(ab, ai, na, bb[i], bi[i], true);
}

// The best T of two sorted lists into (ob, oi), padded with (0, -1); the outputs must not overlap the inputs.
__host__ __device__ inline void spectrum_merge(const uint64_t* ab, const int64_t* ai, int na, const uint64_t* bb,
                                               const int64_t* bi, int nb, int T, uint64_t* ob, int64_t* oi) {
  for (int q = na + nb < T ? na + nb : T; q < T; ++q) ob[q] = 0, oi[q] = -1;
  for (int i = 0; i < na; ++i) {
    const int q = spectrum_place(ab, ai, na, bb, bi, nb, i, true);
    if (q < T) ob[q] = ab[i], oi[q] = ai[i];
  }
  for (int i = 0; i < nb; ++i) {
    const int q = spectrum_place(ab, ai, na, bb, bi, nb, i, false);
    if (q < T) ob[q] = bb[i], oi[q] = bi[i];
  }
}

// X_{e,s} of one tree for both species: t[0, c) are its records' entries in node order and power(j) the power of
// record j, read for final entries only. The first row of a species sets X, the later ones are added in node order:
// the adds of moment_group and moment_group_scaled, so the same double. No row of a species: 0.
template <class Power>
__host__ __device__ inline void spectrum_event_power(const MomentEntry* t, int64_t c, const Power& power, double X[2]) {
  bool have_a = false, have_p = false;  // (scalars, not arrays indexed by the species: no scratch on the device)
  double xa = 0.0, xp = 0.0;
  for (int64_t j = 0; j < c; ++j) {
    if (!moment_final(t[j])) continue;
    const double p = power(j);
    if (moment_species(t[j], 0) == 1) {
      if (have_p) xp += p;
      else xp = p, have_p = true;
    } else {
      if (have_a) xa += p;
      else xa = p, have_a = true;
    }
  }
  X[0] = xa, X[1] = xp;
}

}  // namespace art

#ifdef ART_EVENT_KERNELS
namespace art {

// Pass A is art_event_moments.h's without the bins (event_entries_kernel<false>): the entry of a final record of its
// own tree's range holds its species (MOMENT_AXION / MOMENT_PHOTON) and the run's power; the misplaced records are
// counted in totals[6] of the first set's first entry.

// the power of record j of the tree at `first` in set k, by kind (set_power, art_event_replicates.h)
struct SpectrumPower {
  const EventRowsArgs& a;
  const EventSpectrumArgs& r;
  const MomentEntry* t;
  int64_t first, e;
  int k;
  double sln;
  __device__ double operator()(int64_t j) const {
    const int64_t i = first + j;
    return set_power(a, r, k, i, e, t[j].power, r.kind == REP_KIND_COUPLING ? event_tau(a, i) : 0.0, sln);
  }
};

// Pass B, one lane per event: per set X_{e,s} of both species over the tree's entries (small cached reads), kept in
// r.X for the list kernel, its bin, and one add each to count, sum and sum_sq in HBM -- a chunk's events hit a few
// hundred of the bins, so there is no table in LDS. The totals are summed per wave and added once per wave.
__global__ __launch_bounds__(256) void event_spectrum_tables_kernel(const EventRowsArgs a, const EventSpectrumArgs r) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = e < a.n_events;
  const MomentEntry* t = r.entries;
  int64_t c = 0, first = 0;
  double sln = 0.0;
  if (live && r.node_start) {
    c = tree_range(r.node_start, a.n_nodes, e, &first);
    t = r.entries + first;
    if (r.kind == REP_KIND_COUPLING) sln = a.weight5[2 * a.n_events + e];
  }
  const int64_t NB = spectrum_bins(r.sub_bits);
  for (int k = 0; k < r.n_k; ++k) {
    double X[2] = {0.0, 0.0};
    if (live) spectrum_event_power(t, c, SpectrumPower{a, r, t, first, e, k, sln}, X);
    for (int s = 0; s < 2; ++s) {
      const int64_t ks = 2 * k + s;
      double v[SP_TOT_MISPLACED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (live) {
        const double x = X[s];
        r.X[ks * a.n_events + e] = x;
        v[SP_TOT_EVENTS] = 1.0;
        const int b = spectrum_bin(x, r.sub_bits);
        if (b >= 0) {
          const double x2 = x * x;
          v[SP_TOT_POSITIVE] = 1.0, v[SP_TOT_SUM] = x, v[SP_TOT_SUM_SQ] = x2;
          unsafeAtomicAdd(&r.count[ks * NB + b], 1.0);
          unsafeAtomicAdd(&r.sum[ks * NB + b], x);
          unsafeAtomicAdd(&r.sum_sq[ks * NB + b], x2);
        } else if (x == 0.0) {
          v[SP_TOT_ZEROS] = 1.0;
        } else {
          v[SP_TOT_BAD] = 1.0;
        }
      }
      for (int q = 0; q < SP_TOT_MISPLACED; ++q) wave_add(&r.totals[ks * SP_TOT_COUNT + q], v[q]);
    }
  }
}

// The list kernel, one workgroup per (set, species). The candidates are the carried list's entries with id >= 0 and
// the chunk's X (finite, > 0) with id = event_offset + e. Once the running best T is full a candidate that does not
// come before its last entry is dropped; the others are appended to a tile in LDS (an LDS counter: the order in the
// tile is arbitrary, the sort makes the result a function of the set). A tile that may not take another round is
// sorted (bitonic, by spectrum_before: ties break by id) and its first T are merged into the best T by place
// (spectrum_place, one entry per lane). Padding entries (0, -1) sort last and merge like any other.
constexpr int SPECTRUM_BLOCK = 1024, SPECTRUM_TILE = 2048;

__global__ __launch_bounds__(SPECTRUM_BLOCK) void event_spectrum_top_kernel(const int64_t n, const int64_t event_offset,
                                                                           const EventSpectrumArgs r) {
  __shared__ uint64_t tile_b[SPECTRUM_TILE];
  __shared__ int64_t tile_i[SPECTRUM_TILE];
  __shared__ uint64_t best_b[2][SPECTRUM_MAX_TOP];
  __shared__ int64_t best_i[2][SPECTRUM_MAX_TOP];
  __shared__ int fill;
  const int T = r.top, tid = threadIdx.x;
  const int64_t ks = blockIdx.x;
  const double* X = r.X + ks * n;
  double* out_p = r.top_power + ks * T;
  int64_t* out_e = r.top_event + ks * T;
  int cur = 0;
  if (tid < SPECTRUM_MAX_TOP) best_b[0][tid] = 0, best_i[0][tid] = -1;
  if (tid == 0) fill = 0;
  __syncthreads();
  if (tid < T) {  // the carried list: candidates like the others (it need not arrive sorted)
    const int64_t id = out_e[tid];
    const uint64_t b = spectrum_bits(out_p[tid]);
    if (id >= 0 && spectrum_positive(b)) {
      const int at = atomicAdd(&fill, 1);
      tile_b[at] = b, tile_i[at] = id;
    }
  }
  __syncthreads();
  for (int64_t base = 0;; base += SPECTRUM_BLOCK) {
    const bool last = base >= n;
    const int64_t e = base + tid;
    if (e < n) {
      const uint64_t b = spectrum_bits(X[e]);
      const int64_t id = event_offset + e;
      const bool full = best_i[cur][T - 1] >= 0;
      if (spectrum_positive(b) && (!full || spectrum_before(b, id, best_b[cur][T - 1], best_i[cur][T - 1]))) {
        const int at = atomicAdd(&fill, 1);  // (at most TILE - BLOCK before the round: at < TILE)
        tile_b[at] = b, tile_i[at] = id;
      }
    }
    __syncthreads();
    const int have = fill;
    __syncthreads();
    if (have > SPECTRUM_TILE - SPECTRUM_BLOCK || (last && have > 0)) {
      int P = 64;
      while (P < have) P <<= 1;
      for (int q = have + tid; q < P; q += SPECTRUM_BLOCK) tile_b[q] = 0, tile_i[q] = -1;
      if (tid == 0) fill = 0;
      __syncthreads();
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int q = tid; q < P; q += SPECTRUM_BLOCK) {
            const int p = q ^ j;
            if (p > q) {
              const uint64_t bq = tile_b[q], bp = tile_b[p];
              const int64_t iq = tile_i[q], ip = tile_i[p];
              const bool swap = (q & k) == 0 ? spectrum_before(bp, ip, bq, iq) : spectrum_before(bq, iq, bp, ip);
              if (swap) {
                tile_b[q] = bp, tile_i[q] = ip;
                tile_b[p] = bq, tile_i[p] = iq;
              }
            }
          }
          __syncthreads();
        }
      const int L = P < T ? P : T;
      if (tid < T) {
        const int q = spectrum_place(best_b[cur], best_i[cur], T, tile_b, tile_i, L, tid, true);
        if (q < T) best_b[cur ^ 1][q] = best_b[cur][tid], best_i[cur ^ 1][q] = best_i[cur][tid];
      } else if (tid >= SPECTRUM_MAX_TOP && tid - SPECTRUM_MAX_TOP < L) {
        const int i = tid - SPECTRUM_MAX_TOP;
        const int q = spectrum_place(best_b[cur], best_i[cur], T, tile_b, tile_i, L, i, false);
        if (q < T) best_b[cur ^ 1][q] = tile_b[i], best_i[cur ^ 1][q] = tile_i[i];
      }
      cur ^= 1;
      __syncthreads();
    }
    if (last) break;
  }
  if (tid < T) {
    out_p[tid] = spectrum_value(best_b[cur][tid]);
    out_e[tid] = best_i[cur][tid];
  }
}

hipError_t launch_event_spectrum(const EventRowsArgs& a, const EventSpectrumArgs& r, hipStream_t s) {
  if (a.n_events <= 0) return hipSuccess;
  hipError_t e = launch_event_entries<false>(a, r.node_start, r.entries, 0, false, &r.totals[SP_TOT_MISPLACED], SkyAxes{}, 0, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(event_spectrum_tables_kernel, dim3((unsigned)((a.n_events + 255) / 256)), dim3(256), 0, s, a, r);
  e = hipGetLastError();
  if (e != hipSuccess || r.top <= 0) return e;
  hipLaunchKernelGGL(event_spectrum_top_kernel, dim3((unsigned)(2 * r.n_k)), dim3(SPECTRUM_BLOCK), 0, s, a.n_events,
                     a.event_offset, r);
  return hipGetLastError();
}

}  // namespace art
#endif  // ART_EVENT_KERNELS
