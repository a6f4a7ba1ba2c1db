// TEST TOOL ONLY: host build of the product's per-tree group-by (art_event_moments.h), so the CPU tests
// can hold it against trees.event_moments without a GPU. Never loaded by the product
// (adiabatic_raytracer_amd).
#include "../adiabatic_raytracer_amd/csrc/art_event_moments.h"

using namespace art;

extern "C" {

// The tables of a forest of n_trees trees whose entries lie in node order: tree e owns
// start[e] .. start[e + 1] of flux / sky / power (the three fields of a MomentEntry; flux as pass A
// encodes it). a[e]: the event's a_e without its photon rows (attempts - 1). Adds, as the kernel
// does, X² and X a_e per (tree, key) group to flux_sq, flux_xa (2 nbins), sky_sq, sky_xa (sky_size)
// and to totals (8). Returns 0, or -1 for a key outside its table.
int em_forest(int64_t n_trees, const int64_t* start, const int32_t* flux, const int32_t* sky, const double* power,
              const int64_t* a, int32_t nbins, int64_t sky_size, double* flux_sq, double* flux_xa, double* sky_sq,
              double* sky_xa, double* totals) {
  for (int64_t e = 0; e < n_trees; ++e) {
    const int64_t c = start[e + 1] - start[e];
    MomentEntry* t = new MomentEntry[c > 0 ? c : 1];
    for (int64_t j = 0; j < c; ++j) t[j] = MomentEntry{flux[start[e] + j], sky[start[e] + j], power[start[e] + j]};
    const double ae = (double)(a[e] + moment_photon_rows(t, c, nbins));
    totals[EM_TOT_EVENTS] += 1.0;
    totals[EM_TOT_A1] += ae;
    totals[EM_TOT_A2] += ae * ae;
    for (int64_t j = 0; j < c; ++j)
      for (int which = MOMENT_KEY_FLUX; which <= MOMENT_KEY_SPECIES; ++which) {
        double X;
        const int key = moment_group(t, c, j, which, nbins, &X);
        if (key < 0) continue;
        if (key >= (which == MOMENT_KEY_FLUX ? 2 * (int64_t)nbins : which == MOMENT_KEY_SKY ? sky_size : 2)) {
          delete[] t;
          return -1;
        }
        if (which == MOMENT_KEY_FLUX) {
          flux_sq[key] += X * X;
          flux_xa[key] += X * ae;
        } else if (which == MOMENT_KEY_SKY) {
          sky_sq[key] += X * X;
          sky_xa[key] += X * ae;
        } else {
          totals[EM_TOT_Q_AXION + key] += X * X;
          totals[EM_TOT_C_AXION + key] += X * ae;
        }
      }
    delete[] t;
  }
  return 0;
}

int em_entry_bytes() { return (int)sizeof(MomentEntry); }

}  // extern "C"
