// art_pieces.h -- the streamed host pipeline's partition of a batch into output pieces, for the host
// (art_host_stream.cpp), the helpers (art_helper.h, art_ray_io.h) and the integrator (art_propagate.h):
// one definition, so the ray -> piece map, the pieces' bounds and their blobs' offsets cannot
// disagree between them. Plain C++ (no HIP): tools/piececheck.cpp compiles it with the host compiler.
//
// Rays [0, split) lie in coarse pieces of 2^shift rays, rays [split, n) in fine pieces of
// 2^fine_shift: a piece completes only with its slowest ray, and what is still on the GPU when the
// integrator ends is the call's tail (finalize, D2H, scatter), so the last rays of the batch -- the
// ones claimed just before the queue ran dry, where the last stragglers are -- go in small pieces,
// and the bulk in large ones, whose per-piece costs (a copy submission, a scatter) stay few.
// split is a multiple of 2^shift; every piece but the last holds a multiple of 1024 rays
// (HELPER_TILE: a helper's tile never spans two pieces) because both shifts are >= 10.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ART_PIECES_HD __host__ __device__ inline
#else
#define ART_PIECES_HD inline
#endif

namespace art {

constexpr int PIECES_MAX = 64;       // piece counters, flags and the lanes of a wave's histogram
constexpr int PIECE_MIN_SHIFT = 10;  // 2^10 = HELPER_TILE

struct Pieces {
  int64_t n;           // rays
  int64_t split;       // first ray of the fine pieces, a multiple of 2^shift (n: there are none)
  int32_t shift;       // coarse pieces: 2^shift rays
  int32_t fine_shift;  // fine pieces: 2^fine_shift rays (= shift when there are none)
  int32_t ncoarse;     // coarse pieces: ceil(min(split, n) / 2^shift)
  int32_t count;       // all pieces (<= PIECES_MAX)
};

// The partition of n rays: coarse pieces of 2^shift, and the last `region` rays -- rounded so that
// split is the next multiple of the coarse size at or above n - region, so at most `region` of
// them -- in fine pieces of 2^fine_shift. fine_shift <= 0 or >= shift, or region <= 0: one level.
// Both shifts grow until the pieces number at most PIECES_MAX.
ART_PIECES_HD Pieces make_pieces(int64_t n, int shift, int fine_shift, int64_t region) {
  Pieces q{};
  q.n = n;
  if (shift < PIECE_MIN_SHIFT) shift = PIECE_MIN_SHIFT;
  if (shift > 40) shift = 40;
  while (((n + ((int64_t)1 << shift) - 1) >> shift) > PIECES_MAX) ++shift;  // (one level fits from here on)
  const bool two = fine_shift > 0 && fine_shift < shift && region > 0;
  if (two && fine_shift < PIECE_MIN_SHIFT) fine_shift = PIECE_MIN_SHIFT;
  for (int fs = two ? fine_shift : shift;; ++fs) {
    const int64_t full = (int64_t)1 << shift;
    const int64_t all = ((n + full - 1) >> shift) << shift;  // n rounded up: no fine piece
    int64_t split = all;
    if (fs < shift) {
      const int64_t keep = n > region ? n - region : 0;
      split = ((keep + full - 1) >> shift) << shift;
    }
    const int64_t coarse = (split < n ? split : all) >> shift;
    const int64_t fine = split < n ? (n - split + ((int64_t)1 << fs) - 1) >> fs : 0;
    if (coarse + fine <= PIECES_MAX || fs >= shift) {
      q.split = fine ? split : n;  // (none: n itself, which a 32-bit ray index can hold)
      q.shift = shift;
      q.fine_shift = fine ? fs : shift;
      q.ncoarse = (int32_t)coarse;
      q.count = (int32_t)(coarse + fine);
      return q;
    }
  }
}

// the piece of a ray: a compare, a subtract and two shifts (I: the caller's index type -- the
// integrator's 32-bit ray index stays 32-bit)
template <class I>
ART_PIECES_HD int piece_of(const Pieces& q, I ray) {
  const I s = (I)q.split;
  return ray < s ? (int)(ray >> q.shift) : q.ncoarse + (int)((ray - s) >> q.fine_shift);
}

// the first ray of piece p (p = count: n)
ART_PIECES_HD int64_t piece_lo(const Pieces& q, int p) {
  const int64_t lo = p < q.ncoarse ? (int64_t)p << q.shift : q.split + ((int64_t)(p - q.ncoarse) << q.fine_shift);
  return lo < q.n ? lo : q.n;
}

ART_PIECES_HD int64_t piece_rays(const Pieces& q, int p) { return piece_lo(q, p + 1) - piece_lo(q, p); }

// ---- a piece's SoA output blob: [x (3m) k (3m) u7 tau | status n_acc n_rej (int32)] and, with
// crossings, [count (int32 m)] [pos (3 cap m) k (3 cap m) t dw p (cap m each)], each part from a
// 256-byte boundary ----
ART_PIECES_HD size_t blob_up(size_t b) { return (b + 255) & ~(size_t)255; }
ART_PIECES_HD size_t blob_cnt_off(int64_t m) { return blob_up((size_t)m * 8 * sizeof(double) + (size_t)m * 3 * sizeof(int32_t)); }
ART_PIECES_HD size_t blob_xd_off(int64_t m) { return blob_cnt_off(m) + blob_up((size_t)m * sizeof(int32_t)); }
ART_PIECES_HD size_t blob_bytes(int64_t m, int cap) {
  return cap ? blob_xd_off(m) + (size_t)cap * (size_t)m * 9 * sizeof(double) : blob_cnt_off(m);
}
// the blobs lie one after the other: the coarse ones a full coarse blob apart, then the fine ones
// a full fine blob apart; piece_blob_off(q, count, cap) is the size of them all
ART_PIECES_HD size_t piece_blob_off(const Pieces& q, int p, int cap) {
  const size_t sc = blob_up(blob_bytes((int64_t)1 << q.shift, cap)), sf = blob_up(blob_bytes((int64_t)1 << q.fine_shift, cap));
  return p < q.ncoarse ? sc * (size_t)p : sc * (size_t)q.ncoarse + sf * (size_t)(p - q.ncoarse);
}

}  // namespace art
