// TEST TOOL ONLY: a host compile of the host paths' plain-C++ plan header (art_host_plan.h), checked
// for one case per run (tools/hostplancheck.py, tests/test_host_plan.py):
//     hostplancheck units N FIRST STEP RAMP LANES   the upload units' bounds, which must tile [0, N)
//     hostplancheck blocks SLOTS HW HELPERS SERIAL  "helpers iblocks"
//     hostplancheck scatter N LO M CAP              a blob of the M rays from LO, laid out by art::blob_*, is
//                                                   scattered into arrays of N rays, and the inputs of those
//                                                   rays gathered into an input blob, by memcpy over the
//                                                   segment lists: every element of the piece must arrive,
//                                                   and nothing else may be written
// Prints the result, or "FAIL ..." with exit status 1. Without arguments: a fixed set of such
// cases (the sanitizer build of tools/asan runs that), then "hostplan OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../adiabatic_raytracer_amd/csrc/art_host_plan.h"

using namespace art::host;

#define CHECK(c, ...)                  \
  if (!(c)) {                          \
    std::printf("FAIL " __VA_ARGS__);  \
    std::printf("\n");                 \
    return 1;                          \
  }

static int units(int64_t n, int64_t first, int64_t step, bool ramp, int64_t lanes, bool print) {
  const std::vector<int64_t> u = upload_units(n, first, step, ramp, lanes);
  CHECK(u.size() >= 2 && u.front() == 0 && u.back() == n, "the units do not span [0, %lld)", (long long)n);
  for (size_t i = 1; i < u.size(); ++i) CHECK(u[i] > u[i - 1], "unit %zu is empty", i - 1);
  if (print) {
    for (size_t i = 0; i < u.size(); ++i) std::printf("%s%lld", i ? " " : "", (long long)u[i]);
    std::printf("\n");
  }
  return 0;
}

// the value of element `ray` of row `row` of array `arr` (all exactly representable)
static double code(int arr, int row, int64_t ray) { return (double)((arr * 64 + row) * 100000000LL + ray); }
constexpr double SENTINEL = -1.0;

static void run(const std::vector<Seg>& g, size_t* bytes) {
  for (const Seg& s : g) {
    std::memcpy(s.dst, s.src, s.bytes);
    *bytes += s.bytes;
  }
}

// rows of an array of n rays hold code(arr, row, ray) on [lo, lo + m) and the sentinel elsewhere
template <class T>
static bool holds(const std::vector<T>& a, int arr, int rows, int64_t n, int64_t lo, int64_t m) {
  for (int r = 0; r < rows; ++r)
    for (int64_t i = 0; i < n; ++i)
      if (a[r * n + i] != (T)((i >= lo && i < lo + m) ? code(arr, r, i) : SENTINEL)) return false;
  return true;
}

static int scatter(int64_t n, int64_t lo, int64_t m, int cap, bool print) {
  CHECK(n > 0 && m > 0 && lo >= 0 && lo + m <= n && cap >= 0, "bad piece");
  // ---- scatter: arrays 0..6 the segment outputs, 7 the crossing counts, 8..12 the crossing rows ----
  std::vector<char> blob(art::blob_bytes(m, cap) + 64, 0);
  BlobView b = blob_view(blob.data(), m, cap);
  double* drow[4] = {b.out.x_end, b.out.k_end, b.out.u7_end, b.out.tau_end};
  int32_t* irow[3] = {b.out.status, b.out.n_accept, b.out.n_reject};
  const int drows[4] = {3, 3, 1, 1};
  for (int a = 0; a < 4; ++a)
    for (int r = 0; r < drows[a]; ++r)
      for (int64_t i = 0; i < m; ++i) drow[a][r * m + i] = code(a, r, lo + i);
  // (int32 rows hold the ray alone: the code of (array, row 0) does not fit)
  for (int a = 0; a < 3; ++a)
    for (int64_t i = 0; i < m; ++i) irow[a][i] = (int32_t)(a * 10000000 + lo + i);
  double* xrow[5] = {b.xc.pos, b.xc.k, b.xc.t, b.xc.dw, b.xc.p_nonad};
  const int xrows[5] = {3 * cap, 3 * cap, cap, cap, cap};
  if (cap) {
    for (int64_t i = 0; i < m; ++i) b.xc.count[i] = (int32_t)(70000000 + lo + i);
    for (int a = 0; a < 5; ++a)
      for (int r = 0; r < xrows[a]; ++r)
        for (int64_t i = 0; i < m; ++i) xrow[a][r * m + i] = code(8 + a, r, lo + i);
  }
  std::vector<double> x(3 * n, SENTINEL), k(3 * n, SENTINEL), u7(n, SENTINEL), tau(n, SENTINEL);
  std::vector<int32_t> st(n, -1), acc(n, -1), rej(n, -1), cnt(n, -1);
  std::vector<double> xp(3 * cap * n, SENTINEL), xk(3 * cap * n, SENTINEL), xt(cap * n, SENTINEL), xdw(cap * n, SENTINEL),
      xpn(cap * n, SENTINEL);
  art_segment_out out{x.data(), k.data(), u7.data(), tau.data(), st.data(), acc.data(), rej.data()};
  art_crossing_buf xc{cap, cnt.data(), xp.data(), xk.data(), xt.data(), xdw.data(), xpn.data()};
  size_t sbytes = 0;
  const std::vector<Seg> sg = scatter_segs(blob.data(), m, cap, lo, n, out, cap ? &xc : nullptr);
  run(sg, &sbytes);
  CHECK(holds(x, 0, 3, n, lo, m) && holds(k, 1, 3, n, lo, m) && holds(u7, 2, 1, n, lo, m) && holds(tau, 3, 1, n, lo, m),
        "scatter: a double row of the segment outputs");
  std::vector<int32_t>* iv[4] = {&st, &acc, &rej, &cnt};
  for (int a = 0; a < (cap ? 4 : 3); ++a)
    for (int64_t i = 0; i < n; ++i)
      CHECK((*iv[a])[i] == ((i >= lo && i < lo + m) ? (int32_t)((a == 3 ? 70000000 : a * 10000000) + i) : -1),
            "scatter: int32 row %d at ray %lld", a, (long long)i);
  if (cap)
    CHECK(holds(xp, 8, 3 * cap, n, lo, m) && holds(xk, 9, 3 * cap, n, lo, m) && holds(xt, 10, cap, n, lo, m) &&
              holds(xdw, 11, cap, n, lo, m) && holds(xpn, 12, cap, n, lo, m),
          "scatter: a crossing row");
  // the segments hold the blob without its alignment padding
  const size_t payload = (size_t)m * (8 * sizeof(double) + 3 * sizeof(int32_t)) +
                         (cap ? (size_t)m * sizeof(int32_t) + (size_t)cap * m * 9 * sizeof(double) : 0);
  const size_t pad = (art::blob_cnt_off(m) - (size_t)m * 76) + (cap ? art::blob_xd_off(m) - art::blob_cnt_off(m) - (size_t)m * 4 : 0);
  CHECK(sbytes == payload && sbytes == art::blob_bytes(m, cap) - pad, "scatter: %zu bytes in the segments, the blob holds %zu",
        sbytes, art::blob_bytes(m, cap) - pad);
  // ---- gather: the nine input rows and the species into an input blob of m rays ----
  std::vector<double> x0(3 * n), k0(3 * n), erg(n), dw(n), lt(n);
  std::vector<int8_t> sp(n);
  for (int64_t i = 0; i < n; ++i) {
    for (int r = 0; r < 3; ++r) {
      x0[r * n + i] = code(20, r, i);
      k0[r * n + i] = code(21, r, i);
    }
    erg[i] = code(22, 0, i);
    dw[i] = code(23, 0, i);
    lt[i] = code(24, 0, i);
    sp[i] = (int8_t)(i % 120);
  }
  std::vector<char> ib(in_blob_bytes(m) + 64, (char)0x7f);
  double* rows = (double*)ib.data();
  int8_t* isp = (int8_t*)(ib.data() + in_blob_species_off(m));
  size_t gbytes = 0;
  run(gather_segs(rows, m, isp, m, lo, n, x0.data(), k0.data(), erg.data(), dw.data(), lt.data(), sp.data()), &gbytes);
  for (int64_t i = 0; i < m; ++i) {
    for (int r = 0; r < 3; ++r)
      CHECK(rows[r * m + i] == code(20, r, lo + i) && rows[(3 + r) * m + i] == code(21, r, lo + i), "gather: x0 or k0 row %d", r);
    CHECK(rows[6 * m + i] == code(22, 0, lo + i) && rows[7 * m + i] == code(23, 0, lo + i) && rows[8 * m + i] == code(24, 0, lo + i),
          "gather: erg, dw or ln_t0 at ray %lld", (long long)i);
    CHECK(isp[i] == (int8_t)((lo + i) % 120), "gather: species at ray %lld", (long long)i);
  }
  CHECK(gbytes == (size_t)m * 73, "gather: %zu bytes in the segments", gbytes);
  for (size_t o = (size_t)m * 72; o < ib.size(); ++o)  // nothing but the species beyond the rows
    CHECK((o >= in_blob_species_off(m) && o < in_blob_species_off(m) + (size_t)m) || ib[o] == (char)0x7f, "gather wrote at byte %zu", o);
  // staging laid out as the whole batch (the streamed call): row r of the piece at base + r n + lo
  std::vector<double> whole(9 * n, SENTINEL);
  std::vector<int8_t> wsp(n, (int8_t)-1);
  run(gather_segs(whole.data() + lo, n, wsp.data() + lo, m, lo, n, x0.data(), k0.data(), erg.data(), dw.data(), lt.data(),
                  sp.data()), &gbytes);
  for (int r = 0; r < 9; ++r)
    for (int64_t i = 0; i < n; ++i) {
      const double want = r < 3 ? x0[r * n + i] : r < 6 ? k0[(r - 3) * n + i] : r == 6 ? erg[i] : r == 7 ? dw[i] : lt[i];
      CHECK(whole[r * n + i] == ((i >= lo && i < lo + m) ? want : SENTINEL), "gather (batch layout): row %d ray %lld", r, (long long)i);
    }
  for (int64_t i = 0; i < n; ++i)
    CHECK(wsp[i] == ((i >= lo && i < lo + m) ? sp[i] : (int8_t)-1), "gather (batch layout): species at ray %lld", (long long)i);
  if (print) std::printf("ok %zu %zu\n", sg.size(), sbytes);
  return 0;
}

static int self_test() {
  if (units(20011, 1024, 4096, true, 8192, false) || units(20011, 1024, 4096, false, 8192, false) ||
      units(777, 1024, 4096, true, 0, false) || units(10000000, 1 << 16, 1 << 18, true, 496 * 256, false))
    return 1;
  const StreamBlocks b = stream_blocks(512, 2, 16, false);
  CHECK(b.helpers == 16 && b.iblocks == 496, "blocks %d %d", b.helpers, b.iblocks);
  CHECK(default_piece_shift(10000000) == 18 && default_piece_shift(1250000) == 16, "piece shifts");
  for (int cap = 0; cap <= 3; cap += 3)
    if (scatter(5000, 3000, 1000, cap, false) || scatter(777, 0, 777, cap, false) || scatter(2049, 2048, 1, cap, false)) return 1;
  std::printf("hostplan OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_test();
  const std::string what = argv[1];
  if (what == "units" && argc == 7)
    return units(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoi(argv[5]) != 0, std::atoll(argv[6]), true);
  if (what == "blocks" && argc == 6) {
    const StreamBlocks b = stream_blocks(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]) != 0);
    std::printf("%d %d\n", b.helpers, b.iblocks);
    return 0;
  }
  if (what == "scatter" && argc == 6) return scatter(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoi(argv[5]), true);
  return 2;
}
