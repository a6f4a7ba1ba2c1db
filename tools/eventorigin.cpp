// TEST TOOL ONLY: host build of the product's origin binning (art_event_origin.h), so the CPU tests can hold
// origin_bin_of against trees.origin_bins without a GPU. Never loaded by the product (adiabatic_raytracer_amd).
#include <cmath>

#include "../adiabatic_raytracer_amd/csrc/art_event_origin.h"

using namespace art;

extern "C" {

// out[i] = origin_bin_of of the point (xyz[i], xyz[n + i], xyz[2 n + i]) (SoA, as the sampler's x) for the axes n_r,
// n_theta, n_phi; r_all != 0: one r bin holding every finite r
void eo_bins(int64_t n, const double* xyz, int32_t n_r, int32_t n_theta, int32_t n_phi, int32_t theta_axis, int32_t r_all,
             double r_lo, double r_hi, double cm, double sm, int32_t* out) {
  const OriginAxes O{{n_r, n_theta, n_phi}, r_all, theta_axis, r_lo, r_hi, cm, sm};
  for (int64_t i = 0; i < n; ++i) out[i] = origin_bin_of(O, xyz[i], xyz[n + i], xyz[2 * n + i]);
}

}  // extern "C"
