// art_ray_io.h -- a ray's records around the integrator: its fresh state (init_one), its end state and
// crossings (finalize_one), the donation record, the streamed pipeline's piece counts and chunk flags, the
// hot rule and the cyclotron crossing.
#pragma once
#include "art_step.h"

namespace art {

// propagate_kernel's arguments as the kernel-argument segment holds them: its parameter list in order,
// each at its natural alignment. The headline build's cold blocks (a crossing's record, a finishing lane's
// stores, the piece counts, the wave's end) read what they need from there when they run (cold_args)
// instead of holding the pointers, counts and caps live across the stage slots, where the register
// allocator parks them in lanes of a VGPR and brings them back tuple by tuple (DESIGN §3 "Register budget").
struct PropArgs {
  KParams P;
  int64_t n;
  SegIn in;
  SegOut out;
  int32_t max_crossings;
  unsigned long long* queue;
  unsigned long long* stats;
};
static_assert(offsetof(PropArgs, n) == sizeof(KParams) && offsetof(PropArgs, in) == sizeof(KParams) + 8 &&
                  offsetof(PropArgs, out) == offsetof(PropArgs, in) + sizeof(SegIn) &&
                  offsetof(PropArgs, max_crossings) == offsetof(PropArgs, out) + sizeof(SegOut) &&
                  offsetof(PropArgs, queue) == offsetof(PropArgs, max_crossings) + 8,
              "PropArgs mirrors propagate_kernel's parameter list without padding of its own");
// The arguments, for one cold block: called at the block's head. The empty volatile asm hands the segment's
// address back as a value the optimiser knows nothing about, so the block's scalar loads can be neither
// hoisted out of it nor merged with another block's; they stay loads from the constant address space.
__device__ __forceinline__ const PropArgs& cold_args() {
  auto p = (const __attribute__((address_space(4))) PropArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const PropArgs*)p;
}
template <bool COLD>
__device__ __forceinline__ const PropArgs* cold_args_if() {
  if constexpr (COLD) return &cold_args();
  else return nullptr;
}
// One wave-uniform double as a scalar pair of its own: arguments that arrive in one wide scalar load form
// one register tuple, and a tuple is spilled and restored whole (8 lane reads for one double).
__device__ __forceinline__ double own_pair(double x) {
  double r;
  asm("s_mov_b64 %0, %1" : "=s"(r) : "s"(x));
  return r;
}

// (DON = 3) a wave's LDS histogram of finished rays per piece (lane l: piece l) into the
// pieces' global counts: the wave's end-record stores released once (agent scope), then one
// atomic add per piece with a count (the helpers poll piece_cnt)
__device__ inline void stream_flush(const SegOut& out, unsigned* hist, int lane) {
  const unsigned c = hist[lane];
  if (__ballot(c != 0u) == 0ull) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the write-back done before the counts, always)
  if (c != 0u) {
    hist[lane] = 0u;
    __hip_atomic_fetch_add(out.piece_cnt + lane, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One ray's complete integrator state as a CONT_REC record (tail donation, graduation):
// [u (7) | f (7) | τ, dt, qpow, cprev, bstart, erg | int4 {ray, n_acc, n_rej, ncross} |
//  int4 {iter, sprev, flags, save_k}]
__device__ inline void write_cont_rec(double* rec, const double* u, const double* f, double tau, double dt, double qpow,
                                      double cprev, double bstart, double erg, int ray, int n_acc, int n_rej,
                                      int ncross, int iter, int sprev, bool photon, bool cprev_ok, bool just_evented,
                                      int save_k) {
  double2* rq = reinterpret_cast<double2*>(rec);
  const double v[20] = {u[0], u[1], u[2], u[3], u[4], u[5], u[6], f[0], f[1], f[2],
                        f[3], f[4], f[5], f[6], tau, dt, qpow, cprev, bstart, erg};
#pragma unroll
  for (int i = 0; i < 10; ++i) rq[i] = make_double2(v[2 * i], v[2 * i + 1]);
  int4* ri = reinterpret_cast<int4*>(rq + 10);
  ri[0] = make_int4(ray, n_acc, n_rej, ncross);
  ri[1] = make_int4(iter, sprev, (photon ? 1 : 0) | (cprev_ok ? 2 : 0) | (just_evented ? 4 : 0), save_k);
}

template <int GEOM>
__device__ inline KParams specialize(const KParams& P) {
  KParams Q = P;
  if (GEOM == GEOM_FLAT) {
    Q.rs_eff = 0.0;
    Q.bndry_lyr = -1.0;
    Q.isotropic = 0;
    Q.cert_rmin = 0.0;
  } else if (GEOM == GEOM_GR) {
    __builtin_assume(Q.rs_eff > 0.0);
    Q.bndry_lyr = -1.0;
    Q.isotropic = 0;
  }
  return Q;
}

// Fresh state of ray i (init_kernel; the maskless streamed integrator, DON = 3, runs it for
// each chunk it claims): u0 (RayTracer.jl:179-216: k_norm_Cart onto the axion shell, Cartesian
// -> (r, θ, φ), covariant celerity), f(u0) with the hamiltonian's in-place clamp (:531), the
// initial dt (ode_determine_initdt, order 6, with its probe RHS; RK4: the fixed step) and the
// condition value that seeds the callback's sign memory, into the ray's fresh-state record
// (U0_REC doubles at in.u0 + i U0_REC: [u0 (7) | f0 (7) | dt | c0 | erg | ln t0 | species | 0]),
// ten 16-byte stores. Returns the RHS evaluations it took.
__device__ inline unsigned init_one(const KParams& P, int64_t n, int64_t i, const SegIn& in) {
  const double xs[3] = {in.x0[i], in.x0[n + i], in.x0[2 * n + i]};
  const double ks[3] = {in.k0[i], in.k0[n + i], in.k0[2 * n + i]};
  const double erg = in.erg[i], tau = in.lnt0[i];
  const bool photon = in.species[i] != ART_AXION;
  double u[7], f[7], y[7];
  initial_state(P, xs, ks, erg, in.dw[i], u);
  // pass 0: f(u0); pass 1 (Vern6, when initdt asks for it): its probe f(u1). One inlined RHS site:
  // with two, the helper kernel needed more than the 256 VGPRs of 2 waves per SIMD and spilled
  double dt = P.integrator == ART_RK4 ? (P.ln_t_end - tau) / P.n_fixed : NAN;
  InitDt ids;
  unsigned nrhs = 0;
#pragma unroll
  for (int c = 0; c < 7; ++c) y[c] = u[c];
  double ty = tau;
  for (int pass = 0; pass < 2; ++pass) {
    double r[7];
    rhs(P, photon, y, ty, erg, r);
    ++nrhs;
    if (pass == 0) {
#pragma unroll
      for (int c = 0; c < 7; ++c) f[c] = r[c];
      if (photon && u[0] < P.rNS) u[0] = P.rNS;  // hamiltonian's in-place clamp (:531)
      if (P.integrator == ART_RK4) break;
      dt = initdt_begin(P, u, f, tau, P.ln_t_end - tau, ids, y);
      if (!isnan(dt)) break;
      ty = tau + ids.dt0;
    } else {
      dt = initdt_end(P, f, r, P.ln_t_end - tau, ids);
    }
  }
  const double c0 = condition_t(P, u, fexp(tau));
  const double v[U0_REC] = {u[0], u[1], u[2], u[3], u[4], u[5], u[6], f[0], f[1], f[2],
                            f[3], f[4], f[5], f[6], dt,   c0,   erg,  tau,  photon ? 1.0 : 0.0, 0.0};
  double2* rq = reinterpret_cast<double2*>(in.u0 + i * U0_REC);
#pragma unroll
  for (int c = 0; c < U0_REC / 2; ++c) rq[c] = make_double2(v[2 * c], v[2 * c + 1]);
  return nrhs;
}

// np.histogram's bin of x for `nbins` equal bins over [-π, π] (numpy 2.x histogram: the
// index from (x - lo) / (hi - lo) * nbins, then corrected against the edges of
// linspace(lo, hi, nbins + 1) = i * ((hi - lo) / nbins) + lo, the right edge in the last bin),
// with the same roundings: no contraction into FMAs. -1 outside [lo, hi] (and for NaN).
// The range defaults to flux_kernel's fixed [-π, π]; flux_phi_kernel also takes a data-dependent
// one (np.histogram(a, bins) without `range` bins over [a.min(), a.max()], plot/flux.py:43-47).
__host__ __device__ inline int np_hist_bin(double x, int nbins, double lo = -PI, double hi = PI) {
#pragma clang fp contract(off)  // numpy rounds every product and sum (HIP's __dmul_rn would still fuse)
  if (!(x >= lo && x <= hi)) return -1;
  const double span = hi - lo;
  int i = (int)(((x - lo) / span) * (double)nbins);
  if (i == nbins) i -= 1;
  const double step = span / (double)nbins;
  const double e0 = (double)i * step + lo;
  if (x < e0) i -= 1;
  const double e1 = (i + 1 == nbins) ? hi : (double)(i + 1) * step + lo;
  if (x >= e1 && i != nbins - 1) i += 1;
  return i;
}

// The radiated-flux bin of one segment's end state (plot/flux.py:38-48 over a batch's escaping
// segments): is_final -- no crossing and escaped beyond 1.1 rNS (MainRunner.jl:203-209) -- and
// the azimuth of its momentum binned as np.histogram(range = (-π, π)); -1 = not counted.
// flux_kernel and the streamed pipeline's helpers (finalize_one) both bin through here.
__device__ inline bool end_is_final(const KParams& P, const double* x, int status) {
  const double xr = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  return !(status == ART_STATUS_CROSSING || !(xr > 1.1 * P.rNS));
}
__device__ inline int flux_bin_of(const KParams& P, const double* x, const double* k, int status, int nbins) {
  if (!end_is_final(P, x, status)) return -1;
  return np_hist_bin(atan2(k[1], k[0]), nbins);
}

// End state of ray i in Cartesian form (back-transform, RayTracer.jl:393-416) from the raw end
// record the integrator left in out.rec, spread into the SoA outputs at o (row stride m), and
// the conversion probability of every recorded crossing (get_Prob_nonAD with Nc = 1,
// MainRunner.jl:265). finalize_kernel runs it one thread per ray; the maskless streamed
// integrator (DON = 3) for each chunk whose rays have all finished.
__device__ inline void finalize_one(const KParams& P, int64_t n, int64_t i, int64_t o, int64_t m, const SegIn& in,
                                    const SegOut& out, double* fl = nullptr, int fl_nbins = 0) {
  const double erg = in.erg[i];
  int ncross = 0;
  {
    const double2* rq = reinterpret_cast<const double2*>(out.rec + i * END_REC);
    double u[7], xe[3], ke[3];
    const double2 q0 = rq[0], q1 = rq[1], q2 = rq[2], q3 = rq[3];
    const int4 ri = reinterpret_cast<const int4*>(rq + 4)[0];
    u[0] = q0.x; u[1] = q0.y; u[2] = q1.x; u[3] = q1.y; u[4] = q2.x; u[5] = q2.y; u[6] = q3.x;
    back_transform(P, u, erg, xe, ke);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out.x_end[c * m + o] = xe[c];
      out.k_end[c * m + o] = ke[c];
    }
    out.u7_end[o] = u[6];
    out.tau_end[o] = q3.y;
    out.status[o] = ri.x;
    out.n_acc[o] = ri.y;
    out.n_rej[o] = ri.z;
    ncross = ri.w;
    if (out.xcount) out.xcount[o] = ncross;
    if (out.ntimes >= 2) out.traj_n[o] = reinterpret_cast<const int4*>(rq + 4)[1].x;
    if (fl) {  // (the streamed pipeline's helpers: the ray's radiated-flux bin, an exact count)
      const int bin = flux_bin_of(P, xe, ke, ri.x, fl_nbins);
      if (bin >= 0) atomicAdd(&fl[(in.species[i] == ART_AXION ? 0 : 1) * fl_nbins + bin], 1.0);
    }
  }
  if (out.ntimes >= 2) {  // saveat: start (u0 back-transformed), interior to Cartesian, end
    double u0[7], xs[3], ks[3];
#pragma unroll
    for (int c = 0; c < 7; ++c) u0[c] = in.u0[i * U0_REC + c];
    back_transform(P, u0, erg, xs, ks);
    const int mt = out.traj_n[o];
    for (int k = 0; k < mt; ++k) {
      double x[3];
      if (k == 0) {
        x[0] = xs[0]; x[1] = xs[1]; x[2] = xs[2];
        out.traj_t[o] = in.lnt0[i];
      } else if (k == mt - 1) {
        x[0] = out.x_end[o]; x[1] = out.x_end[m + o]; x[2] = out.x_end[2 * m + o];
        out.traj_t[int64_t(k) * m + o] = out.tau_end[o];
      } else {
        const double r = out.traj[(int64_t(0) * out.ntimes + k) * m + o];
        double st, ct, sp, cp;
        msincos(out.traj[(int64_t(1) * out.ntimes + k) * m + o], st, ct);
        msincos(out.traj[(int64_t(2) * out.ntimes + k) * m + o], sp, cp);
        x[0] = r * st * cp; x[1] = r * st * sp; x[2] = r * ct;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) out.traj[(int64_t(c) * out.ntimes + k) * m + o] = x[c];
    }
  }
  if (!out.xcount) return;
  const int mc = ncross < out.cap ? ncross : out.cap;
  for (int j = 0; j < mc; ++j) {
    const double2* rq = reinterpret_cast<const double2*>(out.xrec + (i * out.cap + j) * X_REC);
    const double2 q0 = rq[0], q1 = rq[1], q2 = rq[2], q3 = rq[3];
    const double x[3] = {q0.x, q0.y, q1.x}, k[3] = {q1.y, q2.x, q2.y};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out.xpos[(int64_t(c) * out.cap + j) * m + o] = x[c];
      out.xk[(int64_t(c) * out.cap + j) * m + o] = k[c];
    }
    out.xt[int64_t(j) * m + o] = q3.x;
    const double dwc = q3.y;
    out.xdw[int64_t(j) * m + o] = dwc;
    out.xp[int64_t(j) * m + o] = prob_nonad_single(P, x, k, erg * fabs(dwc));  // erg_inf_ini .* abs.(Δωc)
  }
  if (out.nan_fill) {
    for (int j = mc; j < out.cap; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        out.xpos[(int64_t(c) * out.cap + j) * m + o] = NAN;
        out.xk[(int64_t(c) * out.cap + j) * m + o] = NAN;
      }
      out.xt[int64_t(j) * m + o] = NAN;
      out.xdw[int64_t(j) * m + o] = NAN;
      out.xp[int64_t(j) * m + o] = NAN;
    }
  }
}

// (DON = 3) the SoA output blob of piece p (art_host_stream.cpp, StreamCall: the same
// layout and 256-byte alignments), its rows m long
__device__ inline SegOut piece_blob(const SegOut& out, int64_t n, int p, int64_t& m) {
  m = piece_rays(out.pieces, p);
  char* db = out.blob + piece_blob_off(out.pieces, p, out.cap);
  double* dd = (double*)db;
  int32_t* di32 = (int32_t*)(dd + 8 * m);
  SegOut ol{};
  ol.x_end = dd; ol.k_end = dd + 3 * m; ol.u7_end = dd + 6 * m; ol.tau_end = dd + 7 * m;
  ol.status = di32; ol.n_acc = di32 + m; ol.n_rej = di32 + 2 * m;
  ol.rec = out.rec;
  if (out.cap) {
    double* x = (double*)(db + blob_xd_off(m));
    ol.cap = out.cap;
    ol.xcount = (int32_t*)(db + blob_cnt_off(m));
    ol.xpos = x; ol.xk = x + 3 * out.cap * m; ol.xt = x + 6 * out.cap * m; ol.xdw = x + 7 * out.cap * m;
    ol.xp = x + 8 * out.cap * m;
    ol.xrec = out.xrec;
    ol.nan_fill = 1;
  }
  return ol;
}

// ---- the maskless streamed pipeline's helper duty (DON = 3, SegOut::helpers) ----
constexpr int S3_TILE = HELPER_TILE;  // (4 rays per thread: the claim, the barriers and the L2 write-back of
                                     // the hand-off amortised over 4 rays)
constexpr unsigned long long S3_WAIT_TICKS = 2000000000ull;  // 20 s of s_memrealtime without progress: give up

__device__ inline unsigned long long ld_sys(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ inline unsigned long long ld_agent(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline bool ld_abort(const SegOut& out) {
  return __hip_atomic_load(out.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
}

// (DON = 3) the claimed chunk's fresh state: its flag as the leader lane reads it now, or after
// a bounded wait (false: the wait timed out or another wave gave up; the wave stops taking rays)
__device__ inline bool chunk_flag(const SegOut& out, int wnext, int leader) {
  unsigned v = 0;
  if ((int)(threadIdx.x & 63) == leader)
    v = __hip_atomic_load(out.chunk_ready + wnext / CHUNK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_amdgcn_readlane((int)v, leader) != 0;
}
__device__ inline bool chunk_wait(const SegOut& out, int wnext, int leader) {
  int ok = 1;
  if ((int)(threadIdx.x & 63) == leader) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(out.chunk_ready + wnext / CHUNK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      if (__hip_atomic_load(out.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u ||
          __builtin_amdgcn_s_memrealtime() - t0 > out.wait_ticks) {
        __hip_atomic_store(out.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(32);
    }
  }
  return __shfl(ok, leader) != 0;
}

// The hot rule (SegOut::hot): a ray that has advanced less than hot_dtau + hot_slope
// log2(attempts / 256) in ln t since its start
__device__ inline bool hot_lags(const SegOut& out, double dtau, double log2_att_256) {
  return dtau < out.hot_dtau + out.hot_slope * log2_att_256;
}

// One crossing of the cyclotron resonance inside the completed step parked in the lane's LDS slots
// (0-3: u, f, y, kk; 4: h, τ), g0 and g1 being cyclotron_g at its two ends: the root of g on the
// step's cubic Hermite interpolant of (r, θ, φ) at time τ + θh by Illinois in θ ∈ [0, 1] (bounded;
// per lane: it runs about once per ray), the full state there back-transformed to Cartesian as
// affect does for the plasma crossings, and cyclotron_tau added to the ray's optical depth. The
// sums live in the ray's own output slots: a ray has one owner at a time, so the donation record
// carries nothing of this.
__device__ inline void cyclotron_crossing(const KParams& P, const double* L, double erg, double g0, double g1,
                                          const SegOut& out, int64_t n, int64_t ray) {
  const double h = L[(4 * 7 + 0) * BLOCK], tau0 = L[(4 * 7 + 1) * BLOCK];
  auto at = [&](int c, double th) {
    return hermite1(L[(0 * 7 + c) * BLOCK], L[(1 * 7 + c) * BLOCK], L[(2 * 7 + c) * BLOCK], L[(3 * 7 + c) * BLOCK], h, th);
  };
  double a = 0.0, ga = g0, b = 1.0, gb = g1, th = 0.5;
  int side = 0;
#pragma unroll 1
  for (int it = 0; it < 40; ++it) {
    th = a - ga * (b - a) / (gb - ga);
    if (!(th > a && th < b)) th = 0.5 * (a + b);
    const double ui[3] = {at(0, th), at(1, th), at(2, th)};
    const double g = cyclotron_g(P, ui, tau0 + th * h, erg);
    if (!(fabs(g) > 1e-15)) break;  // (a NaN ends the search too)
    if ((g < 0.0) == (ga < 0.0)) { a = th; ga = g; if (side == -1) gb *= 0.5; side = -1; }
    else { b = th; gb = g; if (side == 1) ga *= 0.5; side = 1; }
    if (b - a < 1e-14) break;
  }
  double ui[7], x[3], k[3];
#pragma unroll
  for (int c = 0; c < 7; ++c) ui[c] = at(c, th);
  back_transform(P, ui, erg, x, k);
  const double lnt = tau0 + th * h;
  const double tc = cyclotron_tau(P, x, k, fexp(lnt));
  const int cnt = out.cyc_count[ray];
  out.cyc_tau[ray] += tc;
  out.cyc_count[ray] = cnt + 1;
  if (cnt == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out.cyc_pos[c * n + ray] = x[c];
    out.cyc_lnt[ray] = lnt;
  }
}

}  // namespace art
