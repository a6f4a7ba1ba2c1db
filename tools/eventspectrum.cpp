// TEST TOOL ONLY: host build of the product's event power spectrum functions (art_event_spectrum.h) -- the bin
// rule, the order and merge of the top lists and the per-tree X -- so the CPU tests can hold them against numpy
// without a GPU. Never loaded by the product (adiabatic_raytracer_amd).
#include "../adiabatic_raytracer_amd/csrc/art_event_spectrum.h"

using namespace art;

extern "C" {

// spectrum_bin of n values
void es_bins(int64_t n, const double* x, int32_t m, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = spectrum_bin(x[i], m);
}

// The best T of two lists sorted by (X descending, id ascending), as (power, id) pairs padded with (0.0, -1)
void es_merge(int32_t na, const double* ap, const int64_t* ai, int32_t nb, const double* bp, const int64_t* bi, int32_t T,
              double* op, int64_t* oi) {
  uint64_t* a = new uint64_t[na + nb + T + 1];
  uint64_t* b = a + na;
  uint64_t* o = b + nb;
  for (int i = 0; i < na; ++i) a[i] = spectrum_bits(ap[i]);
  for (int i = 0; i < nb; ++i) b[i] = spectrum_bits(bp[i]);
  spectrum_merge(a, ai, na, b, bi, nb, T, o, oi);
  for (int i = 0; i < T; ++i) op[i] = spectrum_value(o[i]);
  delete[] a;
}

// X_{e,s} of a forest of n_trees trees whose records lie in node order: tree e owns start[e] .. start[e + 1] of
// species (-1: not a final record, 0 axion, 1 photon) and power. X: (2, n_trees). With check != 0 every X is also
// held against moment_group(..., MOMENT_KEY_SPECIES) of the same entries: returns the number of X whose bits differ.
int64_t es_forest(int64_t n_trees, const int64_t* start, const int32_t* species, const double* power, double* X,
                  int32_t check) {
  int64_t differ = 0;
  for (int64_t e = 0; e < n_trees; ++e) {
    const int64_t c = start[e + 1] - start[e];
    MomentEntry* t = new MomentEntry[c > 0 ? c : 1];
    for (int64_t j = 0; j < c; ++j) {
      const int32_t s = species[start[e] + j];
      t[j] = MomentEntry{s < 0 ? MOMENT_NONE : (s ? MOMENT_PHOTON : MOMENT_AXION), -1, power[start[e] + j]};
    }
    double x[2];
    spectrum_event_power(t, c, [&](int64_t j) { return t[j].power; }, x);
    X[e] = x[0], X[n_trees + e] = x[1];
    for (int64_t j = 0; check && j < c; ++j) {
      double g;
      const int key = moment_group(t, c, j, MOMENT_KEY_SPECIES, 0, &g);
      if (key >= 0 && spectrum_bits(g) != spectrum_bits(x[key])) ++differ;
    }
    delete[] t;
  }
  return differ;
}

}  // extern "C"
