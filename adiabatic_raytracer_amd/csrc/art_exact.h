// art_exact.h -- exact sums of doubles: the fixed-point superaccumulator behind the exact event tables
// (art_exact_histogram_device, art_exact_finish_device, art_event_exact_device; DESIGN.md §3, "Exact tables").
//
// A finite double is ± m 2^q 2^-1074 with an integer m < 2^53 and q = max(e, 1) - 1 in 0 .. 2045, e the biased
// exponent (a subnormal has e = 0, takes q = 0 and has no implicit bit). A bin is EXACT_LIMBS int64 limbs, limb j
// carrying the bits [32 j, 32 j + 32) above 2^-1074: m << (q & 31) is at most 84 bits, cut into three 32-bit pieces
// that go to the limbs q >> 5, + 1 and + 2 (at most 63 + 2 = 65, the top one), negated for a negative value. So
// adding a value is at most three integer adds, and integer adds are associative: the limbs after any number of adds,
// once normalised, are a function of the multiset of the values alone.
//
// NORMALISED: every limb but the top one lies in [0, 2^32); the top one is signed and carries the sign and the
// headroom. exact_normalize carry-propagates to that form; it changes the representation and never the value.
// THE HEADROOM RULE (include/art.h states it for the callers): every entry point leaves the accumulators it added to
// normalised, and adds at most 2^30 values to a bin between two normalisations. A limb takes at most one piece,
// below 2^32 in size, per value, so between two normalisations it stays within 2^32 + 2^30 2^32 < 2^63 (the fewer
// than 2^31 records of one event call stay within 2^63 too). The top limb has no limb to carry into: it wraps when
// a running sum reaches 2^1069 in size, 2^45 times the largest double.
//
// exact_round gives the correctly rounded double of a bin: round-to-nearest-even of the infinitely precise sum.
// It reads the limbs and leaves them as they are.
//
// __host__ __device__: the kernels of this header (ART_EVENT_KERNELS, art_kernels.hip) and the host twins that
// art_post.cpp exports (art_exact_add_host, art_exact_normalize_host, art_exact_round_host) run the same functions.
#pragma once
#include "art_core.h"

namespace art {

constexpr int EXACT_LIMBS = ART_EXACT_LIMBS;
constexpr int64_t EXACT_MAX_ADDS = (int64_t)1 << 30;  // values per bin between two normalisations
constexpr int EXACT_LDS_BINS = 65536 / (EXACT_LIMBS * 8);  // 124 bins of 528 bytes fit the 64 KiB a block may take
constexpr int EXACT_LDS_FLUX_BINS = 56;  // the flux bins per species that art_event_exact_device keeps in LDS beside the totals

__host__ __device__ inline uint64_t exact_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  return b;
}

// The pieces of a double. False for a NaN or an infinity (nothing is to be added); else limb = q >> 5 and
// piece[0 .. 3) the signed pieces for the limbs limb, limb + 1, limb + 2 (zero pieces need no add).
struct ExactPieces {
  int limb;
  int64_t piece[3];
};
__host__ __device__ inline bool exact_encode(double v, ExactPieces* P) {
  const uint64_t b = exact_bits(v);
  const int e = (int)((b >> 52) & 0x7ff);
  if (e == 0x7ff) return false;
  const uint64_t frac = b & 0xfffffffffffffull;
  const uint64_t m = e ? frac | (1ull << 52) : frac;
  const int q = e ? e - 1 : 0, sh = q & 31;
  const uint64_t lo = m << sh;  // the low 64 bits of m << sh
  int64_t p0 = (int64_t)(lo & 0xffffffffull), p1 = (int64_t)(lo >> 32), p2 = sh ? (int64_t)(m >> (64 - sh)) : 0;
  if (b >> 63) {
    p0 = -p0;
    p1 = -p1;
    p2 = -p2;
  }
  P->limb = q >> 5;
  P->piece[0] = p0;
  P->piece[1] = p1;
  P->piece[2] = p2;
  return true;
}

// adds v to the bin at `acc` with plain adds (one adder); false, and nothing added, for a NaN or an infinity
__host__ __device__ inline bool exact_add(int64_t* acc, double v) {
  ExactPieces P;
  if (!exact_encode(v, &P)) return false;
  for (int c = 0; c < 3; ++c)
    if (P.piece[c] != 0) acc[P.limb + c] = (int64_t)((uint64_t)acc[P.limb + c] + (uint64_t)P.piece[c]);
  return true;
}

// carry-propagates the bin at `acc`: every limb but the top one into [0, 2^32), the carries into the next
__host__ __device__ inline void exact_normalize(int64_t* acc) {
  int64_t carry = 0;
  for (int j = 0; j < EXACT_LIMBS - 1; ++j) {
    const int64_t v = acc[j] + carry;  // (|acc[j]| < 2^63 - 2^31 by the headroom rule, |carry| <= 2^31)
    acc[j] = v & 0xffffffffll;
    carry = v >> 32;  // (arithmetic: the floor)
  }
  acc[EXACT_LIMBS - 1] = (int64_t)((uint64_t)acc[EXACT_LIMBS - 1] + (uint64_t)carry);
}

__host__ __device__ inline int exact_clz32(uint32_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __clz((int)x);
#else
  return __builtin_clz(x);
#endif
}

// The correctly rounded double of the bin at `acc`, which need not be normalised and is not changed. Two passes from
// the low limb up, so no copy of the bin is kept: the first carry-propagates for the sign alone, the second forms the
// 32-bit limbs of the magnitude (of the 67 there are: the top limb gives two) and keeps the highest non-zero one with
// the two below it and whether anything lower is non-zero. A sum below 2^-1022 + 2^-1074 2^52 is its own bit pattern
// (every multiple of 2^-1074 up to 2^53 of them is representable); above, 53 bits from the leading one, the guard bit
// and the sticky rest round to nearest even, and a carry out of the 53 bits moves the exponent up, to ±inf from 2047.
__host__ __device__ inline double exact_round(const int64_t* acc) {
  int64_t carry = 0;
  for (int j = 0; j < EXACT_LIMBS - 1; ++j) carry = (acc[j] + carry) >> 32;
  const bool neg = (int64_t)((uint64_t)acc[EXACT_LIMBS - 1] + (uint64_t)carry) < 0;
  uint32_t w2 = 0, w1 = 0, w0 = 0, prev1 = 0, prev2 = 0;
  bool older = false, sticky = false;
  int top = -1;
  carry = 0;
  uint64_t inc = 1;  // the + 1 of the two's complement, carried up while the limbs below are zero
  for (int j = 0; j <= EXACT_LIMBS; ++j) {
    uint32_t m;
    if (j < EXACT_LIMBS - 1) {
      const int64_t v = acc[j] + carry;
      carry = v >> 32;
      m = (uint32_t)(v & 0xffffffffll);
      if (neg) {
        const uint64_t x = (uint64_t)(uint32_t)~m + inc;
        m = (uint32_t)x;
        inc = x >> 32;
      }
    } else {  // the top limb: the low and the high half of its magnitude
      uint64_t t = (uint64_t)acc[EXACT_LIMBS - 1] + (uint64_t)carry;
      if (neg) t = ~t + inc;
      m = j == EXACT_LIMBS - 1 ? (uint32_t)t : (uint32_t)(t >> 32);
    }
    if (m != 0) {
      top = j;
      w2 = m;
      w1 = prev1;
      w0 = prev2;
      sticky = older;
    }
    older = older || prev2 != 0;
    prev2 = prev1;
    prev1 = m;
  }
  uint64_t bits = 0;
  if (top >= 0) {
    const int z = exact_clz32(w2);
    const int L = 32 * top + 31 - z;  // the leading bit of the magnitude, in units of 2^-1074
    if (L <= 52) {
      bits = top == 0 ? (uint64_t)w2 : ((uint64_t)w2 << 32) | w1;
    } else {
      const uint64_t hi = ((uint64_t)w2 << 32) | w1;
      const uint64_t t64 = z ? (hi << z) | ((uint64_t)w0 >> (32 - z)) : hi;  // the leading bit at bit 63
      const uint32_t rest = z ? w0 & ((1u << (32 - z)) - 1u) : w0;
      const uint64_t mant = t64 >> 11;
      const bool guard = (t64 >> 10) & 1, low = (t64 & 0x3ff) != 0 || rest != 0 || sticky;
      const uint64_t e = (uint64_t)(L - 51);  // the biased exponent: L = 52 is e = 1
      bits = ((e - 1) << 52) + mant + ((guard && (low || (mant & 1))) ? 1 : 0);  // (a carry moves into the exponent)
      if ((bits >> 52) >= 0x7ff) bits = 0x7ffull << 52;
    }
  }
  if (neg) bits |= 1ull << 63;
  double out;
  __builtin_memcpy(&out, &bits, sizeof out);
  return out;
}

}  // namespace art

#ifdef ART_EVENT_KERNELS
#include "art_event_replicates.h"

namespace art {

// one piece into one limb: a 64-bit integer add, in HBM or in LDS
__device__ inline void exact_atomic(int64_t* limb, int64_t piece) {
  atomicAdd((unsigned long long*)limb, (unsigned long long)piece);
}
// v into the bin at `acc` (HBM or LDS) with atomic adds; false, and nothing added, for a NaN or an infinity
__device__ inline bool exact_atomic_add(int64_t* acc, double v) {
  ExactPieces P;
  if (!exact_encode(v, &P)) return false;
  for (int c = 0; c < 3; ++c)
    if (P.piece[c] != 0) exact_atomic(acc + P.limb + c, P.piece[c]);
  return true;
}
// the lanes of the wave with `bad` set, added once per wave to *dst as a float64 count
__device__ inline void exact_count(double* dst, bool bad) {
  const unsigned long long b = __ballot(bad);
  if (b != 0 && (threadIdx.x & (warpSize - 1)) == 0) unsafeAtomicAdd(dst, (double)__popcll(b));
}
// a block-private table of `limbs` limbs: zeroed before, flushed after, only its non-zero limbs, one add each
__device__ inline void exact_lds_zero(int64_t* sh, int limbs) {
  for (int q = threadIdx.x; q < limbs; q += blockDim.x) sh[q] = 0;
}
__device__ inline void exact_lds_flush(const int64_t* sh, int limbs, int64_t* dst) {
  for (int q = threadIdx.x; q < limbs; q += blockDim.x)
    if (sh[q] != 0) exact_atomic(dst + q, sh[q]);
}

// values[i] into bin bins[i] of n_bins (a bin < 0 or >= n_bins is skipped). Grid-stride, so a block of the LDS build
// amortises the zeroing and the flush of its table over many items.
template <bool LDS>
__global__ __launch_bounds__(256) void exact_histogram_kernel(const int64_t n, const int32_t* __restrict__ bins,
                                                              const double* __restrict__ values, const int n_bins,
                                                              int64_t* __restrict__ acc, double* __restrict__ nonfinite) {
  extern __shared__ __attribute__((aligned(16))) int64_t sh_acc[];
  if (LDS) {
    exact_lds_zero(sh_acc, n_bins * EXACT_LIMBS);
    __syncthreads();
  }
  int64_t* const table = LDS ? sh_acc : acc;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // (every lane of a wave makes the same number of rounds, so the ballot of exact_count sees whole waves)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {
    const int64_t i = base + threadIdx.x;
    bool bad = false;
    if (i < n) {
      const int b = bins[i];
      if (b >= 0 && b < n_bins) bad = !exact_atomic_add(table + (int64_t)b * EXACT_LIMBS, values[i]);
    }
    exact_count(nonfinite, bad);
  }
  if (LDS) {
    __syncthreads();
    exact_lds_flush(sh_acc, n_bins * EXACT_LIMBS, acc);
  }
}

// one lane per bin
__global__ __launch_bounds__(256) void exact_normalize_kernel(const int64_t n_bins, int64_t* __restrict__ acc) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_bins) exact_normalize(acc + b * EXACT_LIMBS);
}
__global__ __launch_bounds__(256) void exact_finish_kernel(const int64_t n_bins, const int64_t* __restrict__ acc,
                                                           double* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_bins) out[b] = exact_round(acc + b * EXACT_LIMBS);
}

// the blocks of a grid-stride launch over n items: at most 4 per CU of the largest part, so a block's LDS table
// serves hundreds of items on a large call
static inline unsigned exact_grid(int64_t n) {
  const int64_t blocks = (n + 255) / 256;
  return (unsigned)(blocks < 1024 ? (blocks < 1 ? 1 : blocks) : 1024);
}

hipError_t launch_exact_histogram(int64_t n, const int32_t* bins, const double* values, int n_bins, int64_t* acc,
                                  double* nonfinite, bool lds, hipStream_t s) {
  for (int64_t at = 0; at < n; at += EXACT_MAX_ADDS) {  // (the headroom rule: normalised every 2^30 values)
    const int64_t m = n - at < EXACT_MAX_ADDS ? n - at : EXACT_MAX_ADDS;
    if (lds)
      hipLaunchKernelGGL(exact_histogram_kernel<true>, dim3(exact_grid(m)), dim3(256),
                         (size_t)n_bins * EXACT_LIMBS * sizeof(int64_t), s, m, bins + at, values + at, n_bins, acc, nonfinite);
    else
      hipLaunchKernelGGL(exact_histogram_kernel<false>, dim3(exact_grid(m)), dim3(256), 0, s, m, bins + at, values + at,
                         n_bins, acc, nonfinite);
    hipLaunchKernelGGL(exact_normalize_kernel, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, s, (int64_t)n_bins, acc);
  }
  return hipGetLastError();
}

hipError_t launch_exact_finish(int64_t n_bins, const int64_t* acc, double* out, hipStream_t s) {
  if (n_bins <= 0) return hipSuccess;
  hipLaunchKernelGGL(exact_finish_kernel, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, s, n_bins, acc, out);
  return hipGetLastError();
}

// The exact tables of set k of a chunk. One lane per node record, grid-stride; the record, its bins and its power as
// event_replicates_kernel takes them (event_record, set_power), so a row falls into the same bins with the same
// power as in the float tables. PATH 2: the totals and the flux table of the set are block-private in LDS
// ([totals, 2 bins | flux, 2 nbins bins], (2 + 2 nbins) 528 bytes), flushed once per block; 1: the totals alone;
// 0: every add goes to HBM. The sky map always does. Misplaced records are counted by set 0's launch.
template <int PATH>
__global__ __launch_bounds__(256) void event_exact_kernel(const EventRowsArgs a, const EventExactArgs r, const int k,
                                                          const SkyAxes A, const int cos_axis) {
  extern __shared__ __attribute__((aligned(16))) int64_t sh_acc[];
  const int sh_limbs = PATH == 2 ? (2 + 2 * r.nbins) * EXACT_LIMBS : PATH == 1 ? 2 * EXACT_LIMBS : 0;
  if (PATH) {
    exact_lds_zero(sh_acc, sh_limbs);
    __syncthreads();
  }
  int64_t* const g_tot = r.totals + (int64_t)k * 2 * EXACT_LIMBS;
  int64_t* const g_flux = r.flux + (int64_t)k * 2 * r.nbins * EXACT_LIMBS;
  int64_t* const tot = PATH ? sh_acc : g_tot;
  int64_t* const flux = PATH == 2 ? sh_acc + 2 * EXACT_LIMBS : g_flux;
  // EventReplicatesArgs' factor fields, for set_power
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < a.n_nodes; base += stride) {
    const int64_t i = base + threadIdx.x;
    const EventRecord rec = event_record(a, r.node_start, i, r.nbins, r.sky != nullptr, A, cos_axis);
    bool bad = false;
    if (rec.state == RECORD_FINAL) {
      const double pw = set_power(a, r, k, i, rec.e, rec.power, rec.tau, rec.sln);
      bad = !exact_atomic_add(tot + rec.species * EXACT_LIMBS, pw);
      if (!bad) {
        if (rec.fb >= 0) exact_atomic_add(flux + (int64_t)(rec.species * r.nbins + rec.fb) * EXACT_LIMBS, pw);
        if (rec.sb >= 0) exact_atomic_add(r.sky + ((int64_t)k * r.sky_size + rec.sb) * EXACT_LIMBS, pw);
      }
    }
    exact_count(r.nonfinite + k, bad);
    if (k == 0) exact_count(r.misplaced, rec.state == RECORD_MISPLACED);
  }
  if (PATH) {
    __syncthreads();
    exact_lds_flush(sh_acc, 2 * EXACT_LIMBS, g_tot);
    if (PATH == 2) exact_lds_flush(sh_acc + 2 * EXACT_LIMBS, 2 * r.nbins * EXACT_LIMBS, g_flux);
  }
}

// path: 2, 1 or 0 as event_exact_kernel's. One launch per set, then one normalisation of every table.
hipError_t launch_event_exact(const EventRowsArgs& a, const EventExactArgs& r, const SkyAxes& A, int cos_axis, int path,
                              hipStream_t s) {
  if (a.n_nodes > 0) {
    const dim3 grid(exact_grid(a.n_nodes)), block(256);
    for (int k = 0; k < r.n_k; ++k) {
      if (path == 2)
        hipLaunchKernelGGL(event_exact_kernel<2>, grid, block, (size_t)(2 + 2 * r.nbins) * EXACT_LIMBS * sizeof(int64_t), s,
                           a, r, k, A, cos_axis);
      else if (path == 1)
        hipLaunchKernelGGL(event_exact_kernel<1>, grid, block, (size_t)2 * EXACT_LIMBS * sizeof(int64_t), s, a, r, k, A,
                           cos_axis);
      else
        hipLaunchKernelGGL(event_exact_kernel<0>, grid, block, 0, s, a, r, k, A, cos_axis);
    }
  }
  const int64_t sets[3] = {(int64_t)r.n_k * 2, (int64_t)r.n_k * 2 * r.nbins, r.sky ? (int64_t)r.n_k * r.sky_size : 0};
  int64_t* const tables[3] = {r.totals, r.flux, r.sky};
  for (int t = 0; t < 3; ++t)
    if (sets[t] > 0)
      hipLaunchKernelGGL(exact_normalize_kernel, dim3((unsigned)((sets[t] + 255) / 256)), dim3(256), 0, s, sets[t], tables[t]);
  return hipGetLastError();
}

}  // namespace art
#endif  // ART_EVENT_KERNELS
