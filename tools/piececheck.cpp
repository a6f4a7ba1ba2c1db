// TEST TOOL ONLY: a host compile of the streamed pipeline's partition header (art_pieces.h), checked
// for one batch size and setting per run (tools/piececheck.py, tests/test_pieces.py):
//     piececheck N SHIFT FINE_SHIFT REGION
// The pieces must tile [0, N) without gap or overlap, number at most PIECES_MAX, agree with
// piece_of at both ends of every piece, hold a multiple of 1024 rays each (but the last), start the
// fine ones at a multiple of the coarse size, and have blobs that do not overlap.
// Prints "ok count ncoarse shift fine_shift split" or the first failure (exit status 1).
#include <cstdio>
#include <cstdlib>

#include "../adiabatic_raytracer_amd/csrc/art_pieces.h"

#define CHECK(c, ...)                  \
  if (!(c)) {                          \
    std::printf("FAIL " __VA_ARGS__);  \
    std::printf("\n");                 \
    return 1;                          \
  }

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int64_t n = std::atoll(argv[1]), region = std::atoll(argv[4]);
  const int shift = std::atoi(argv[2]), fine = std::atoi(argv[3]);
  const art::Pieces q = art::make_pieces(n, shift, fine, region);
  CHECK(q.count >= 1 && q.count <= art::PIECES_MAX, "count %d", q.count);
  CHECK(q.ncoarse >= 0 && q.ncoarse <= q.count, "ncoarse %d of %d", q.ncoarse, q.count);
  CHECK(q.shift >= art::PIECE_MIN_SHIFT && q.fine_shift >= art::PIECE_MIN_SHIFT && q.fine_shift <= q.shift,
        "shifts %d %d", q.shift, q.fine_shift);
  CHECK(q.n == n && q.split >= 0 && q.split <= n, "split %lld", (long long)q.split);
  if (q.ncoarse < q.count) {  // there are fine pieces
    CHECK((q.split & (((int64_t)1 << q.shift) - 1)) == 0, "split %lld is no multiple of 2^%d", (long long)q.split, q.shift);
    CHECK(q.split == (int64_t)q.ncoarse << q.shift, "split %lld after %d coarse pieces", (long long)q.split, q.ncoarse);
    CHECK(n - q.split <= (region > 0 ? region : 0) || q.split == 0, "fine region %lld above %lld", (long long)(n - q.split),
          (long long)region);
  }
  CHECK(art::piece_lo(q, 0) == 0, "first piece at %lld", (long long)art::piece_lo(q, 0));
  CHECK(art::piece_lo(q, q.count) == n, "pieces end at %lld", (long long)art::piece_lo(q, q.count));
  int64_t sum = 0;
  for (int p = 0; p < q.count; ++p) {
    const int64_t lo = art::piece_lo(q, p), hi = art::piece_lo(q, p + 1), m = art::piece_rays(q, p);
    CHECK(hi > lo && m == hi - lo, "piece %d [%lld, %lld) rays %lld", p, (long long)lo, (long long)hi, (long long)m);
    CHECK(m <= ((int64_t)1 << (p < q.ncoarse ? q.shift : q.fine_shift)), "piece %d has %lld rays", p, (long long)m);
    CHECK(p == q.count - 1 || m % 1024 == 0, "piece %d: %lld rays is no multiple of a tile", p, (long long)m);
    CHECK(lo % 1024 == 0, "piece %d starts inside a tile (%lld)", p, (long long)lo);
    CHECK(art::piece_of(q, lo) == p && art::piece_of(q, hi - 1) == p, "piece_of at the ends of piece %d: %d %d", p,
          art::piece_of(q, lo), art::piece_of(q, hi - 1));
    // the integrator's 32-bit ray index gives the same piece
    CHECK(art::piece_of(q, (int)lo) == p && art::piece_of(q, (int)(hi - 1)) == p, "32-bit piece_of, piece %d", p);
    sum += m;
    for (int cap = 0; cap <= 3; ++cap) {
      const size_t off = art::piece_blob_off(q, p, cap), next = art::piece_blob_off(q, p + 1, cap);
      CHECK(off % 256 == 0 && off + art::blob_bytes(m, cap) <= next, "blob of piece %d (capacity %d) overlaps the next", p, cap);
      CHECK(art::blob_cnt_off(m) >= (size_t)m * 76 && art::blob_xd_off(m) >= art::blob_cnt_off(m) + (size_t)m * 4,
            "blob parts of piece %d overlap", p);
    }
  }
  CHECK(sum == n, "the pieces hold %lld rays of %lld", (long long)sum, (long long)n);
  std::printf("ok %d %d %d %d %lld\n", q.count, q.ncoarse, q.shift, q.fine_shift, (long long)q.split);
  return 0;
}
