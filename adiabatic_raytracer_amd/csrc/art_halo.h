// art_halo.h -- the halo velocity model (beyond the reference, whose sampler draws every axion at
// 220/√3 per component and whose Maxwellian draw with v_NS is a commented-out line,
// RayTracer.jl:1531-1533): f∞(u) ∝ exp(-|u + v_NS|²/v0²) in the star's frame, u the axion's velocity
// at infinity, v0 the most probable speed, v_NS the star's velocity in the halo frame. The three
// formulas live here and nowhere else: the proposal speed, the incoming asymptote of the Kepler
// hyperbola through the sampled point, and the importance ratio that multiplies sln_prob. All
// speeds in km/s, GM in km³/s². Plain C++ (<cmath> only): the kernels include it, and so does
// tools/halocheck.cpp with the host compiler (tests/test_halo_host.py).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ART_HALO_HD __host__ __device__
#else
#define ART_HALO_HD
#endif

namespace art {

// What the kernels need of an art_halo (include/art.h), v_prop resolved: vp = sqrt(v0² + |v_NS|²)
// when none is given.
struct HaloK {
  double v0, v_ns[3], vp;
};

// The proposal speed at infinity from one uniform U in [0, 1): density ∝ s exp(-s²/vp²), the
// speed of a 2-d Gaussian -- one closed-form inversion, and its ratio to the 3-d Maxwellian's
// s² exp(-s²/v0²) stays bounded for vp >= v0.
ART_HALO_HD inline double halo_speed(double U, double vp) { return vp * sqrt(-log(1.0 - U)); }

// The velocity at infinity u of the Newtonian orbit that passes x [km] in the direction d (unit)
// with the speed s at infinity: v = sqrt(s² + 2GM/r) d, and the incoming asymptote of its hyperbola
//   u = s [(s - v_r) v + (GM/r) r̂] / (s² + GM/r - s v_r),   v_r = v·r̂,
// the solution of the eccentricity-vector identity v×L - GM r̂ = u×L + GM û (L = x×v) with |u| = s
// (the outgoing asymptote has -GM û there). The denominator is positive for every direction:
// (s² + GM/r)² > s² (s² + 2GM/r) >= (s v_r)².
ART_HALO_HD inline void halo_asymptote(const double x[3], const double d[3], double s, double GM, double u[3]) {
  const double r = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double ir = 1.0 / r;
  const double gmr = GM * ir;
  const double vloc = sqrt(s * s + 2.0 * gmr);
  const double rh[3] = {x[0] * ir, x[1] * ir, x[2] * ir};
  const double vr = vloc * (d[0] * rh[0] + d[1] * rh[1] + d[2] * rh[2]);
  const double f = s / (s * s + gmr - s * vr);
  const double a = (s - vr) * vloc;
  for (int i = 0; i < 3; ++i) u[i] = f * (a * d[i] + gmr * rh[i]);
}

// F = (220/v0) (vp/v0)² exp(s²/vp² - |u + v_NS|²/v0²): the importance ratio 4π v s f∞(u) / p(s) of
// isotropic local directions and halo_speed's proposal, written against the reference's
// dense_extra = 2/√π · c/220 · v_esc/c (MainRunner.jl:552), which is that ratio's Maxwellian at
// v0 = 220 and v_NS = 0 integrated over speeds. Exactly 1 for v_NS = 0, vp = v0 = 220.
ART_HALO_HD inline double halo_factor(const double u[3], double s, double v0, const double v_ns[3], double vp) {
  const double w[3] = {u[0] + v_ns[0], u[1] + v_ns[1], u[2] + v_ns[2]};
  const double e = (s * s) / (vp * vp) - (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) / (v0 * v0);
  return (220.0 / v0) * ((vp / v0) * (vp / v0)) * exp(e);
}

}  // namespace art
