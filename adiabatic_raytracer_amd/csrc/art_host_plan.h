// art_host_plan.h -- the host paths' arithmetic that needs no HIP: the streamed call's upload units,
// block counts and the words of its scratch head and of its host signals; the row segments that
// scatter an output blob into the caller's arrays and gather the caller's inputs; the view of a blob
// as the C boundary's structs. Plain C++ like art_pieces.h (whose blob layout it uses):
// tools/hostplancheck.cpp compiles it with the host compiler (tests/test_host_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/art.h"
#include "art_pieces.h"

namespace art {
namespace host {

// ---- the streamed call's device scratch: the words of its head (STREAM_HEAD_BYTES, zeroed at the
// call's start), each an unsigned long long; the chunk flags and the records follow the head ----
enum HeadWord {
  HW_QUEUE = 0,           // the work queue's next chunk
  HW_STATS = 1,           // N_STATS_DEV words of statistics
  HW_INIT_NEXT = 16,      // the helpers' next tile to initialise
  HW_FIN_NEXT = 17,       // ... and to finalize
  HW_MISSES = 18,         // chunk claims that found their flag not yet raised
  HW_EXIT = 19,           // helper blocks that have left (SegOut::exit_count)
  HW_WAVES_DONE = 20,     // integrator waves that have counted themselves out
  HW_WAVES_STARTED = 21,  // ... and in
  HW_PIECE_CNT = 32,      // finished rays per piece (PIECES_MAX words)
  HW_PIECE_FIN = 96,      // finalized tiles per piece (PIECES_MAX words)
  HW_TRACE_WORDS = 160    // what ART_HOST_TRACE reads back: everything above
};
constexpr size_t STREAM_HEAD_BYTES = 2048;
static_assert(HW_PIECE_CNT + PIECES_MAX <= HW_PIECE_FIN && HW_PIECE_FIN + PIECES_MAX <= HW_TRACE_WORDS &&
                  HW_TRACE_WORDS * sizeof(unsigned long long) <= STREAM_HEAD_BYTES,
              "the per-piece words lie inside the head");

// The HostLane words the GPU reads and writes over PCIe (HostLane::hsig): the ready counter | the
// piece flags | helper blocks started | the last integrator fully resident on the GPU (ticket + 1;
// never reset) | from HSIG_DONE SegOut::done_host (the flag, the statistics, the flux)
constexpr int HSIG_NFLAG = 64;
enum HostSignal { HSIG_READY = 0, HSIG_FLAGS = 8, HSIG_STARTED = HSIG_FLAGS + HSIG_NFLAG, HSIG_RESIDENT = 76, HSIG_DONE = 80 };
static_assert(PIECES_MAX == HSIG_NFLAG, "one flag and one counter per piece");

// ---- the streamed call's plan ----

// coarse output pieces of 2^shift rays: 32..64 of them, none below 2^16 rays
inline int default_piece_shift(int64_t n) {
  int shift = 16;
  while (((int64_t)1 << (shift + 1)) * 32 <= n) ++shift;
  return shift;
}

// The bounds of the upload units of n rays: units of `first` rays until `lanes` rays are on their
// way, then doubling up to `step`; without ramp one first unit, then `step` at once.
inline std::vector<int64_t> upload_units(int64_t n, int64_t first, int64_t step, bool ramp, int64_t lanes) {
  std::vector<int64_t> ulo{0};
  if (!ramp) lanes = 0;
  for (int64_t lo = 0, sz = first; lo < n;) {
    lo = std::min(n, lo + sz);
    ulo.push_back(lo);
    if (lo >= lanes) sz = (ramp && sz < step) ? std::min(step, 2 * sz) : step;
  }
  return ulo;
}

// Helper blocks beside the integrator and the integrator's own, of `slots` block slots: a helper
// block of 2 waves per SIMD (hw = 2) shares a CU with one integrator block and costs one slot, a
// 1-wave/SIMD one holds a whole CU, two slots. serial: no persistent helpers, every slot integrates.
struct StreamBlocks {
  int helpers, iblocks;
};
inline StreamBlocks stream_blocks(int slots, int hw, int helpers_wanted, bool serial) {
  StreamBlocks b;
  b.helpers = std::min(slots - 1, std::max(1, helpers_wanted));
  b.iblocks = serial ? slots : slots - (hw == 2 ? b.helpers : 2 * b.helpers);
  return b;
}

// ---- blobs and the caller's arrays ----

// one row segment of a host-side copy (CopyPool::run)
struct Seg {
  void* dst;
  const void* src;
  size_t bytes;
};

// an input blob of m rays: [x0 (3m) k0 (3m) erg dw ln_t0 | species (int8 m)], the species from a
// 256-byte boundary
inline size_t in_blob_species_off(int64_t m) { return blob_up((size_t)m * 9 * sizeof(double)); }
inline size_t in_blob_bytes(int64_t m) { return in_blob_species_off(m) + blob_up((size_t)m); }

// The output blob of m rays (art_pieces.h: blob_cnt_off, blob_xd_off) seen as the C boundary's
// structs; xc.capacity = 0 and null rows without crossings.
struct BlobView {
  art_segment_out out;
  art_crossing_buf xc;
  art_crossing_buf* xcp() { return xc.capacity ? &xc : nullptr; }
};
inline BlobView blob_view(void* blob, int64_t m, int cap) {
  double* d = (double*)blob;
  int32_t* i32 = (int32_t*)(d + 8 * m);
  BlobView v{{d, d + 3 * m, d + 6 * m, d + 7 * m, i32, i32 + m, i32 + 2 * m}, {}};
  if (cap) {
    double* x = (double*)((char*)blob + blob_xd_off(m));
    const int64_t cm = (int64_t)cap * m;
    v.xc = art_crossing_buf{cap, (int32_t*)((char*)blob + blob_cnt_off(m)), x, x + 3 * cm, x + 6 * cm, x + 7 * cm, x + 8 * cm};
  }
  return v;
}

// Scatter: the output blob of the m rays [lo, lo + m) -> the caller's arrays of n rays (xc: only
// with cap). Crossing rows are [(comp * cap + j) * n + ray]: 3 cap rows of pos, of k, cap rows of t, dw, P.
inline std::vector<Seg> scatter_segs(const void* blob, int64_t m, int cap, int64_t lo, int64_t n, const art_segment_out& out,
                                     const art_crossing_buf* xc) {
  const BlobView b = blob_view(const_cast<void*>(blob), m, cap);
  const size_t row = (size_t)m * sizeof(double), irow = (size_t)m * sizeof(int32_t);
  std::vector<Seg> g;
  for (int q = 0; q < 3; ++q) {
    g.push_back({out.x_end + q * n + lo, b.out.x_end + q * m, row});
    g.push_back({out.k_end + q * n + lo, b.out.k_end + q * m, row});
  }
  g.push_back({out.u7_end + lo, b.out.u7_end, row});
  g.push_back({out.tau_end + lo, b.out.tau_end, row});
  g.push_back({out.status + lo, b.out.status, irow});
  g.push_back({out.n_accept + lo, b.out.n_accept, irow});
  g.push_back({out.n_reject + lo, b.out.n_reject, irow});
  if (cap) {
    g.push_back({xc->count + lo, b.xc.count, irow});
    for (int r = 0; r < 3 * cap; ++r) {
      g.push_back({xc->pos + r * n + lo, b.xc.pos + r * m, row});
      g.push_back({xc->k + r * n + lo, b.xc.k + r * m, row});
    }
    for (int r = 0; r < cap; ++r) {
      g.push_back({xc->t + r * n + lo, b.xc.t + r * m, row});
      g.push_back({xc->dw + r * n + lo, b.xc.dw + r * m, row});
      g.push_back({xc->p_nonad + r * n + lo, b.xc.p_nonad + r * m, row});
    }
  }
  return g;
}

// Gather: the caller's nine input rows and species of the rays [lo, lo + m), of n -> staging whose
// row r starts at rows + r * stride (an input blob of m rays: stride = m; staging laid out as the
// whole batch: rows = its base + lo, stride = n), the species at `sp`.
inline std::vector<Seg> gather_segs(double* rows, int64_t stride, int8_t* sp, int64_t m, int64_t lo, int64_t n, const double* x0,
                                    const double* k0, const double* erg, const double* dw, const double* ln_t0,
                                    const int8_t* species) {
  const double* src[9] = {x0, x0 + n, x0 + 2 * n, k0, k0 + n, k0 + 2 * n, erg, dw, ln_t0};
  std::vector<Seg> g;
  for (int r = 0; r < 9; ++r) g.push_back({rows + r * stride, src[r] + lo, (size_t)m * sizeof(double)});
  g.push_back({sp, species + lo, (size_t)m});
  return g;
}

}  // namespace host
}  // namespace art
