// TEST TOOL ONLY: a host compile of the exact accumulator (art_exact.h: exact_encode, exact_add, exact_normalize,
// exact_round, the functions the kernels and the host twins of libart run), on the vectors of tests/test_exact.py
// whose answers are known in closed form, and on pseudo-random ones against a plain big-integer reference written
// here. The sanitizer build of tools/asan runs it (build/exact_asan; tests/test_exact.py): any out-of-range limb
// index, signed overflow or bad shift is a report. Prints "exact OK", or "FAIL ..." with exit status 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../adiabatic_raytracer_amd/csrc/art_exact.h"

using art::EXACT_LIMBS;

#define CHECK(c, ...)                  \
  if (!(c)) {                          \
    std::printf("FAIL " __VA_ARGS__);  \
    std::printf("\n");                 \
    return 1;                          \
  }

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static double sum_of(const std::vector<double>& v, std::vector<int64_t>* limbs = nullptr) {
  std::vector<int64_t> acc(EXACT_LIMBS, 0);
  for (double x : v) art::exact_add(acc.data(), x);
  art::exact_normalize(acc.data());
  if (limbs) *limbs = acc;
  return art::exact_round(acc.data());
}

// The reference: the sum as sign and magnitude in 32-bit digits (68 of them), schoolbook; then the rounding by the
// definition -- the 53 bits from the leading one, round half to even on the exact remainder.
struct Big {
  std::vector<uint32_t> d = std::vector<uint32_t>(68, 0);
  bool neg = false;
};
static int cmp_mag(const Big& a, const Big& b) {
  for (int j = 67; j >= 0; --j)
    if (a.d[j] != b.d[j]) return a.d[j] < b.d[j] ? -1 : 1;
  return 0;
}
static Big big_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  const int e = (int)((b >> 52) & 0x7ff);
  const uint64_t frac = b & 0xfffffffffffffull, m = e ? frac | (1ull << 52) : frac;
  const int q = e ? e - 1 : 0;
  Big r;
  r.neg = (b >> 63) != 0;
  for (int bit = 0; bit < 53; ++bit)
    if ((m >> bit) & 1) r.d[(q + bit) / 32] |= 1u << ((q + bit) % 32);
  return r;
}
static Big big_add(const Big& a, const Big& b) {
  Big r;
  if (a.neg == b.neg) {
    uint64_t c = 0;
    for (int j = 0; j < 68; ++j) {
      c += (uint64_t)a.d[j] + b.d[j];
      r.d[j] = (uint32_t)c;
      c >>= 32;
    }
    r.neg = a.neg;
    return r;
  }
  const int s = cmp_mag(a, b);
  if (s == 0) return r;
  const Big &hi = s > 0 ? a : b, &lo = s > 0 ? b : a;
  int64_t borrow = 0;
  for (int j = 0; j < 68; ++j) {
    int64_t x = (int64_t)hi.d[j] - lo.d[j] - borrow;
    borrow = x < 0;
    r.d[j] = (uint32_t)(x + (borrow ? ((int64_t)1 << 32) : 0));
  }
  r.neg = hi.neg;
  return r;
}
static int big_bit(const Big& a, int i) { return i < 0 ? 0 : (a.d[i / 32] >> (i % 32)) & 1; }
static double big_round(const Big& a) {
  int L = -1;
  for (int i = 68 * 32 - 1; i >= 0 && L < 0; --i)
    if (big_bit(a, i)) L = i;
  if (L < 0) return 0.0;
  uint64_t mant = 0;
  const int low = L > 52 ? L - 52 : 0;
  for (int i = L; i >= low; --i) mant = (mant << 1) | (uint64_t)big_bit(a, i);
  bool guard = big_bit(a, low - 1), sticky = false;
  for (int i = low - 2; i >= 0; --i) sticky = sticky || big_bit(a, i);
  if (guard && (sticky || (mant & 1))) ++mant;
  const double r = std::ldexp((double)mant, low - 1074);  // (mant <= 2^53: exact; ldexp gives inf beyond the range)
  return a.neg ? -r : r;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), tiny = 5e-324, p53 = 9007199254740992.0;
  const double big = std::numeric_limits<double>::max();
  // cancellation, ties to even, subnormals, overflow, the signed zero-sum
  CHECK(same(sum_of({1e308, 1.0, -1e308}), 1.0), "cancellation");
  CHECK(same(sum_of({p53, 1.0, 1.0}), p53 + 2.0) && same(sum_of({1.0, p53, 1.0}), p53 + 2.0), "2^53 + 1 + 1");
  CHECK(same(sum_of({p53, 1.0}), p53) && same(sum_of({p53, 3.0}), p53 + 4.0), "ties to even");
  CHECK(same(sum_of({p53, 1.0, tiny}), p53 + 2.0), "a sticky bit far below the tie");
  CHECK(same(sum_of({tiny, tiny, tiny}), 1.5e-323), "three times the smallest subnormal");
  CHECK(same(sum_of({std::ldexp(1.0, -1022) - tiny, tiny}), std::ldexp(1.0, -1022)), "out of the subnormal range");
  CHECK(same(sum_of({1.7e308, 1.7e308}), inf) && same(sum_of({-1.7e308, -1.7e308}), -inf), "overflow");
  CHECK(same(sum_of({1.7e308, 1.7e308, -1.7e308}), 1.7e308), "overflow taken back");
  CHECK(same(sum_of({big, std::ldexp(1.0, 969)}), big) && same(sum_of({big, std::ldexp(1.0, 970)}), inf), "the last tie");
  CHECK(same(sum_of({1.5, -1.5}), 0.0) && same(sum_of({-0.0, -0.0}), 0.0) && same(sum_of({}), 0.0), "zero sums are +0");
  {
    int64_t acc[EXACT_LIMBS] = {0};
    CHECK(!art::exact_add(acc, inf) && !art::exact_add(acc, -inf) && !art::exact_add(acc, std::nan("")), "non-finite");
    for (int j = 0; j < EXACT_LIMBS; ++j) CHECK(acc[j] == 0, "a non-finite value was added");
    CHECK(art::exact_add(acc, big) && art::exact_add(acc, -big) && art::exact_add(acc, tiny), "the extreme exponents");
  }
  // pseudo-random sums over the whole exponent range against the reference, and the limbs' order-independence
  uint64_t state = 1769;
  auto next = [&state]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 11;
  };
  for (int round = 0; round < 400; ++round) {
    const int n = 1 + (int)(next() % 40);
    std::vector<double> v;
    Big ref;
    for (int i = 0; i < n; ++i) {
      uint64_t bits = (next() << 11) ^ next();
      if (round % 3 == 0) bits &= ~(0x7c0ull << 52);  // small exponents: subnormal and near-subnormal sums
      if (((bits >> 52) & 0x7ff) == 0x7ff) bits ^= 1ull << 62;
      double x;
      std::memcpy(&x, &bits, 8);
      if (round % 5 == 0 && i % 2) x = -v.back() * (1.0 + (double)(next() % 3) * 0x1p-52);  // near cancellation
      if (!std::isfinite(x)) x = 0.0;
      v.push_back(x);
      ref = big_add(ref, big_of(x));
    }
    std::vector<int64_t> a, b;
    const double got = sum_of(v, &a), want = big_round(ref);
    CHECK(same(got, want), "round %d: %a, the reference gives %a", round, got, want);
    std::vector<double> w(v.rbegin(), v.rend());
    CHECK(same(sum_of(w, &b), got) && a == b, "round %d: the limbs depend on the order", round);
    for (int j = 0; j < EXACT_LIMBS - 1; ++j) CHECK(a[j] >= 0 && a[j] <= 0xffffffffll, "round %d: limb %d is not normalised", round, j);
  }
  // the headroom rule's extreme states: normalising keeps the value, rounding does not need the normalised form
  const int64_t hi = 0xffffffffll + ((int64_t)1 << 30) * 0xffffffffll, lo = -(((int64_t)1 << 30) * 0xffffffffll);
  for (int pattern = 0; pattern < 4; ++pattern) {
    int64_t acc[EXACT_LIMBS], norm[EXACT_LIMBS];
    for (int j = 0; j < EXACT_LIMBS; ++j) acc[j] = pattern == 0 ? hi : pattern == 1 ? lo : ((j + pattern) & 1) ? hi : lo;
    acc[EXACT_LIMBS - 1] = pattern - 2;
    std::memcpy(norm, acc, sizeof acc);
    art::exact_normalize(norm);
    for (int j = 0; j < EXACT_LIMBS - 1; ++j) CHECK(norm[j] >= 0 && norm[j] <= 0xffffffffll, "pattern %d limb %d", pattern, j);
    CHECK(same(art::exact_round(acc), art::exact_round(norm)), "pattern %d: normalising changed the value", pattern);
    int64_t again[EXACT_LIMBS];
    std::memcpy(again, norm, sizeof norm);
    art::exact_normalize(again);
    CHECK(std::memcmp(again, norm, sizeof norm) == 0, "pattern %d: normalising twice", pattern);
  }
  // 2^20 copies of the largest double below 2
  {
    int64_t acc[EXACT_LIMBS] = {0};
    const double x = 0x1.fffffffffffffp+0;
    for (int i = 0; i < (1 << 20); ++i) art::exact_add(acc, x);
    CHECK(same(art::exact_round(acc), std::ldexp(x, 20)), "2^20 copies");
  }
  std::printf("exact OK\n");
  return 0;
}
