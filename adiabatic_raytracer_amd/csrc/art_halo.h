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

// q = |u + v_NS|²/v0², the model's exponent, summed and rounded in one fixed order
ART_HALO_HD inline double halo_q(const double u[3], const HaloK& h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double w0 = u[0] + h.v_ns[0], w1 = u[1] + h.v_ns[1], w2 = u[2] + h.v_ns[2];
  return ((w0 * w0 + w1 * w1) + w2 * w2) / (h.v0 * h.v0);
}

// R = F_target / F_base = (v0_b/v0_h)³ exp(q_b - q_h): what an event drawn and weighted under `base`
// is worth under `target` (the halo scan, art_event_haloscan.h). The s²/vp² term of halo_factor
// cancels, so neither model's vp enters. Every operation is rounded on its own and the exponent is
// the difference of the two q, so target == base gives exp(0) * 1 = 1.0 exactly. On the device the
// exponential is art_core.h's fexp (a hipcc unit includes art_core.h before this header).
ART_HALO_HD inline double halo_ratio(const double u[3], const HaloK& base, const HaloK& target) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = halo_q(u, base) - halo_q(u, target);
#if defined(__HIP_DEVICE_COMPILE__)
  const double e = fexp(x);
#else
  const double e = exp(x);
#endif
  const double r = base.v0 / target.v0;
  return ((r * r) * r) * e;
}

}  // namespace art
