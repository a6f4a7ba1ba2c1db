// art_step.h -- what one integrator step is made of: the statistics slots, the dense-output and
// scan-point arithmetic, the initial step size, affect!, the stage tables and the tuning constants.
// Included by both translation units (art_kernels.hip, art_kernels_nolicm.hip) ahead of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "art_core.h"
#include "art_internal.h"

namespace art {

// stats[]: totals over the launch, for the roofline accounting (tools/count_flops.cpp)
enum { ST_ATTEMPTS = 0, ST_ACCEPTED, ST_ROOT_STEPS, ST_SCAN_EVALS, ST_INTERP_EVALS, ST_RAYS, ST_INIT_RHS, ST_CERT,
       ST_NSTATS = 8 };

// cubic Hermite dense output between (u0, f0) and (u1, f1) over h at fraction th
template <class T>
__host__ __device__ inline void hermite7(const T* u0, const T* f0, const T* u1, const T* f1, const T& h,
                                         const T& th, T* out) {
  const T a = 1.0 - th;
  const T b = th * (th - 1.0);
  const T c1 = 1.0 - 2.0 * th;
  const T c2 = (th - 1.0) * h;
  const T c3 = th * h;
#pragma unroll
  for (int i = 0; i < 7; ++i) out[i] = a * u0[i] + th * u1[i] + b * (c1 * (u1[i] - u0[i]) + c2 * f0[i] + c3 * f1[i]);
}

// one component of hermite7
__device__ inline double hermite1(double u0, double f0, double u1, double f1, double h, double th) {
  return (1.0 - th) * u0 + th * u1 + th * (th - 1.0) * ((1.0 - 2.0 * th) * (u1 - u0) + (th - 1.0) * h * f0 + th * h * f1);
}

__device__ inline int sgn(double x) { return (x > 0.0) - (x < 0.0); }

// One point of the resonance scan: the condition on the cubic Hermite interpolant of the
// step (u0, f0) -> (u1, f1) over h, at fraction th and t = e^(τ + th h), the interpolant parked
// in LDS: S = the lane's base in the [slot][component][lane] layout, slots 0-3 = u0, f0, u1, f1,
// slot 4 = (h, τ). The cooperative grid pass and the per-lane bracket evaluations both go
// through here, so a recomputed grid value is bit-identical to the one whose sign the grid pass
// recorded.
__device__ inline void scan_nd_lds(const KParams& P, const double* S, int stride, double th, double& N, double& D) {
  double u0[7], f0[7], u1[7], f1[7], ui[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    u0[i] = S[(0 * 7 + i) * stride];
    f0[i] = S[(1 * 7 + i) * stride];
    u1[i] = S[(2 * 7 + i) * stride];
    f1[i] = S[(3 * 7 + i) * stride];
  }
  const double h = S[(4 * 7 + 0) * stride], tau = S[(4 * 7 + 1) * stride];
  hermite7(u0, f0, u1, f1, h, th, ui);
#pragma unroll
  for (int i = 0; i < 7; ++i) ui[i] = (th == 1.0) ? u1[i] : ui[i];  // the step's end point exactly
  condition_nd(P, ui, fexp(tau + th * h), N, D);
}

__device__ inline double scan_point_lds(const KParams& P, const double* S, int stride, double th) {
  double N, D;
  scan_nd_lds(P, S, stride, th, N, D);
  return 0.5 * N / D;  // = condition_t, bit for bit
}

// The integrator's span from in-kernel clock stamps (stats[ST_T0], stats[ST_T1]: the earliest
// wave start as the max of ~t, the latest wave end): s_memrealtime is the device's one 100 MHz
// constant clock, so the figure is the launch's own duration without a profiler's completion
// signals (art_recent_kernel_span_ms). Two atomics per wave.
__device__ inline void span_stamp(unsigned long long* stats, bool end) {
  if ((threadIdx.x & 63) == 0) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    atomicMax(stats + (end ? ST_T1 : ST_T0), end ? t : ~t);
  }
}

// Completes this wave's LDS traffic before other lanes of the same wave read it.
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 2-bit sign code of a scan value: 0 zero, 1 positive, 2 negative, 3 NaN
__device__ inline unsigned sign_code(double c) { return isnan(c) ? 3u : (c > 0.0 ? 1u : (c < 0.0 ? 2u : 0u)); }

// sign_code(½ N / D) without the division where its sign is certain: D > 0 and finite, N a
// normal number and the quotient far from underflow. Otherwise the division decides.
__device__ inline unsigned sign_code_nd(double N, double D) {
  const double aN = fabs(N);
  if (D > 0.0 && D < INFINITY && aN >= 1e-290 && !(aN < 1e-290 * D)) return N > 0.0 ? 1u : 2u;
  return sign_code(0.5 * N / D);
}

// ode_determine_initdt (DiffEqBase) for an order-6 method, in two halves around its one extra RHS
// evaluation (init_one evaluates both RHS at ONE inlined site). initdt_begin returns the step when
// no probe is needed, else NaN with the probe point u1 = u0 + dt0 f0 at tau0 + dt0.
struct InitDt {
  double sk[7], d1, dt0;
};
__device__ inline double initdt_begin(const KParams& P, const double* u0, const double* f0, double tau0, double dtmax,
                                      InitDt& s, double* u1) {
  double d0 = 0.0, d1 = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    s.sk[i] = P.abstol + fabs(u0[i]) * P.reltol;
    d0 += (u0[i] / s.sk[i]) * (u0[i] / s.sk[i]);
    d1 += (f0[i] / s.sk[i]) * (f0[i] / s.sk[i]);
  }
  d0 = sqrt(d0 / 7.0);
  d1 = sqrt(d1 / 7.0);
  double dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * (d0 / d1);
  dt0 = fmin(dt0, dtmax);
  const double at = fabs(tau0);
  const double eps_t = nextafter(at, INFINITY) - at;
  if (dt0 < 10.0 * eps_t) return fmax(1e-6, P.dtmin);
#pragma unroll
  for (int i = 0; i < 7; ++i) u1[i] = u0[i] + dt0 * f0[i];
  s.d1 = d1;
  s.dt0 = dt0;
  return NAN;
}
__device__ inline double initdt_end(const KParams& P, const double* f0, const double* f1, double dtmax, const InitDt& s) {
  bool same = true;
  double d2 = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    same = same && (f0[i] == f1[i]);
    const double q = (f1[i] - f0[i]) / s.sk[i];
    d2 += q * q;
  }
  if (same) return fmax(P.dtmin, 100.0 * s.dt0);
  d2 = sqrt(d2 / 7.0) / s.dt0;
  const double mx = fmax(s.d1, d2);
  const double dt1 = (mx <= 1e-15) ? fmax(1e-6, s.dt0 * 1e-3) : pow(10.0, -(2.0 + log10(mx)) / 6.0);
  return fmax(P.dtmin, fmin(fmin(100.0 * s.dt0, dt1), dtmax));
}

// ---------------------------------------------------------------------------
// affect! (RayTracer.jl:301-350). Returns 0 = skipped, 1 = recorded, 2 = recorded + terminate.
__device__ inline int affect(const KParams& P, const SegIn& in, const SegOut& out, int64_t n, int64_t ray,
                             const double* u, double tau, double erg, int& ncross, int max_crossings) {
  double st, ct, sp, cp;
  msincos(u[1], st, ct);
  msincos(u[2], sp, cp);
  if (ncross == 0) {  // a "crossing" at the start point is not new (:303-314)
    const double s = 1.0001;
    const double pos[3] = {st * cp * u[0], st * sp * u[0], ct * u[0]};
    bool all_lt = true, all_gt = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double x0i = fabs(in.x0[i * n + ray]);
      all_lt = all_lt && (fabs(pos[i]) < x0i * s);
      all_gt = all_gt && (fabs(pos[i]) > x0i / s);
    }
    if (all_lt && all_gt) return 0;
  }
  double x[3], k[3];
  sph_to_cart(u, erg, P.rs_eff, x, k);
  if (sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) < P.rNS101) return 0;  // :322-324
  const int j = ncross;
  if (out.xcount && j < out.cap) {
    const double dwc = u[6] / erg;  // P_nonAD: finalize_kernel
    double2* rq = reinterpret_cast<double2*>(out.xrec + ((int64_t)ray * out.cap + j) * X_REC);
    rq[0] = make_double2(x[0], x[1]);
    rq[1] = make_double2(x[2], k[0]);
    rq[2] = make_double2(k[1], k[2]);
    rq[3] = make_double2(exp(tau), dwc);
  }
  ncross = j + 1;
  const int maxc = max_crossings <= 0 ? -1 : max_crossings;
  return (ncross >= maxc) ? 2 : 1;
}

// ---------------------------------------------------------------------------
// Stage glue, table-driven. Slot s (0-based) of an attempt evaluates the next stage at
//   y = u + h (cf[s] f + cA[s] kA + Σ_q cL[s][q] L_q),   t = τ + ct[s] h,
// where kA is ONE register-resident stage vector (k2, later k8 -- their lifetimes do not
// overlap) and L_0..L_4 are stage vectors parked in LDS (k3..k7 for Vern6; k3, k4 for RK4).
// Coefficients are wave-uniform scalar loads; the RHS is inlined once.
constexpr int LDS_SLOTS = 5;
// The wave-uniform scalars of one slot in one 48-byte row, and its five LDS coefficients in one
// 40-byte row of cL: both loaded at the slot's start and waited for once, ahead of the cf*f
// products, so that no scalar load stands among the slot's LDS reads (scalar loads return out
// of order: a wait for one would drain the LDS reads with it). (The five folded into SlotRow, for
// the flat builds' prefetch to carry them, did not reproduce the results bit for bit: DESIGN §6.)
struct alignas(16) SlotRow {
  double cf, cA, ct;
  int lmask;   // bit q: cL[s][q] != 0 -- the LDS slots stage s reads (bit q guards block q of the glue)
  int storeA;  // after the slot: kk -> kA?
  int storeL;  // after the slot: kk -> L[storeL] (-1: no)
  int pad;
};
struct StageTable {
  SlotRow row[8];
  double cL[8][LDS_SLOTS];
  double e_f, e_A, e_L[LDS_SLOTS], e_k;  // error weights (Vern6): btilde of f, kA(=k8), L, k9
};

// (static: both translation units, art_kernels.hip and art_kernels_nolicm.hip, hold their own copy)
static __constant__ StageTable c_vern6 = {
    // {cf = a_{s+2,1}, cA (k2 for slots 0..6, k8 for slot 7), ct, lmask, storeA, storeL}
    {{Vern6::a21, 0.0, Vern6::c2, 0x0, 1, -1, 0},
     {Vern6::a31, Vern6::a32, Vern6::c3, 0x0, 0, 0, 0},
     {Vern6::a41, 0.0, Vern6::c4, 0x1, 0, 1, 0},
     {Vern6::a51, 0.0, Vern6::c5, 0x3, 0, 2, 0},
     {Vern6::a61, 0.0, Vern6::c6, 0x7, 0, 3, 0},
     {Vern6::a71, 0.0, Vern6::c7, 0xf, 0, 4, 0},
     {Vern6::a81, 0.0, 1.0, 0x1f, 1, -1, 0},
     {Vern6::a91, Vern6::a98, 1.0, 0x1e, 0, -1, 0}},
    // cL: coefficients of k3..k7
    {{0, 0, 0, 0, 0},
     {0, 0, 0, 0, 0},
     {Vern6::a43, 0, 0, 0, 0},
     {Vern6::a53, Vern6::a54, 0, 0, 0},
     {Vern6::a63, Vern6::a64, Vern6::a65, 0, 0},
     {Vern6::a73, Vern6::a74, Vern6::a75, Vern6::a76, 0},
     {Vern6::a83, Vern6::a84, Vern6::a85, Vern6::a86, Vern6::a87},
     {0, Vern6::a94, Vern6::a95, Vern6::a96, Vern6::a97}},
    Vern6::e1, Vern6::e8, {0.0, Vern6::e4, Vern6::e5, Vern6::e6, Vern6::e7}, Vern6::e9};

static __constant__ StageTable c_rk4 = {
    {{0.5, 0.0, 0.5, 0x0, 1, -1, 0},
     {0.0, 0.5, 0.5, 0x0, 0, 0, 0},
     {0.0, 0.0, 1.0, 0x1, 0, 1, 0},
     {1.0 / 6.0, 2.0 / 6.0, 1.0, 0x3, 0, -1, 0},
     {0, 0, 0, 0, 0, -1, 0}, {0, 0, 0, 0, 0, -1, 0}, {0, 0, 0, 0, 0, -1, 0}, {0, 0, 0, 0, 0, -1, 0}},
    {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {1.0, 0, 0, 0, 0}, {2.0 / 6.0, 1.0 / 6.0, 0, 0, 0},
     {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}},
    0.0, 0.0, {0, 0, 0, 0, 0}, 0.0};

enum LaneMode { M_IDLE = 0, M_STEP = 2, M_ROOT = 3 };

// Lanes per block of the persistent integrator. A block retires only when all its waves are
// done, so smaller blocks free their CU slots sooner while a launch drains (the next launch,
// on another stream, fills them).
constexpr int BLOCK = 256;
constexpr int SCAN_WORDS = 4;  // 2-bit codes for up to 64 grid points (interp_points <= 65)
constexpr int SUNROLL_FLAT = 1;  // the stage slot loop: one RHS site
constexpr int SUNROLL_GR = 2;  // GR: two RHS sites (A/B: lone GR tail ray -6%; flat: bulk +-0, lone +1%)
constexpr int PRIO_ITERS = 1024;  // attempts from which a ray counts as an outlier (propagate_kernel, s_setprio)
// Waves per SIMD the integrator is register-budgeted for (1: 512 VGPR+AGPR, 2: 256).
#ifndef ART_WAVES_PER_SIMD
#define ART_WAVES_PER_SIMD 2
#endif
// (DON = 3) a wave's finished-ray counts go out every 128 iterations (~2.5 ms of a flat ray's
// steps; every 8: -3%, every 32: -1%, profiles/r03sg_flush.jsonl)
constexpr int STREAM_FLUSH = 127;
constexpr int DRAIN_FLUSH_MASK = 7;  // (once the queue is drained: every 8th iteration, so the drain pays few write-backs)

// ---------------------------------------------------------------------------
// One loop iteration = one step attempt for every live lane: a runtime loop over the
// stage slots with the RHS inlined once. A lane that takes a new ray loads its fresh state
// (init_kernel) and steps in the same iteration; lanes polishing a crossing (M_ROOT)
// re-step from the step start. After the slots, the wave-cooperative scan and one per-lane
// condition call site (brackets, Illinois, root polish) serve the ContinuousCallback.
// GEOM_FLAT: flat space, no boundary layer, anisotropic plasma (the headline workload). The
// kernel then works on a copy of the parameters whose rs_eff, bndry_lyr and isotropic are
// compile-time constants, so the Schwarzschild, boundary-layer and isotropic branches of
// the physics fold away instead of holding registers. GEOM_ANY reads them at run time.
// GEOM_GR: Schwarzschild (rs > 0), no boundary layer, anisotropic (configs[3]): only the
// boundary-layer and isotropic branches fold away, and rs != 0 is assumed.
enum { GEOM_ANY = 0, GEOM_FLAT = 1, GEOM_GR = 2 };

}  // namespace art
