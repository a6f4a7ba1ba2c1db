// art_sample.h -- sample_kernel: the sampler of the conversion surface (find_samples_new).
#pragma once
#include <hip/hip_runtime.h>

#include "art_core.h"
#include "art_event.h"
#include "art_halo.h"
#include "art_internal.h"

namespace art {

// ---------------------------------------------------------------------------
// find_samples_new (RayTracer.jl:1480-1653) + main_runner's erg and k_init
// (MainRunner.jl:511-529): persistent lanes, one ray per lane, one attempt per lane per outer
// iteration; all lanes of a wave walk their lines' 0.5 km Euler steps in lockstep.
//
// Per step, the ContinuousCallback(interp_points = 20) scan (:1603-1613) is WAVE-COOPERATIVE:
//   * a step whose every point is provably below the resonance (certified negative, below)
//     needs only its last point -- the value the next step's first bracket starts from;
//   * every other step needs its 19 points.
// Those items (source lane, point) of the whole wave are evaluated 64 at a time by all lanes
// on the source lines (kept in LDS), so one lane's uncertified step no longer makes the whole
// wave evaluate 19 points. Each item leaves the signbit and nonzero-ness of its value in its
// source lane's bit masks; a lane then finds its sign changes (the reference's brackets:
// signbit differs, both values nonzero) with bit operations. Brackets are queued (in each
// lane's order of discovery) and resolved 64 at a time -- Illinois on the exact line and the
// affect! test (rr > rNS, E_loc > ωp, :1585-1597) -- and each lane then counts its valid
// crossings in order and keeps the randInx-th (:1623-1636). Every value is computed by the same
// expression on the same operands as a per-lane scan would, so the samples do not change.
constexpr int SQCAP = 128;  // bracket queue entries per wave

// closest approach of the line x0 + va s to the centre within [s0, s1], squared
__device__ inline double line_rmin2(const double* x0, const double* va, double s0, double s1) {
  const double sd = -(x0[0] * va[0] + x0[1] * va[1] + x0[2] * va[2]);
  const double sm = fmin(fmax(sd, s0), s1);
  double xm[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) xm[i] = x0[i] + va[i] * sm;
  return xm[0] * xm[0] + xm[1] * xm[1] + xm[2] * xm[2];
}

// The sampler's certificates on the segment [s0, s1] of a line (x0 + va s, energy E): 1 when every
// point of it provably has a negative condition, 2 when every point provably has a positive one,
// 0 otherwise. The bounds are derived at sample_kernel's step loop; both hold for a segment of any
// length (a block of steps as well as one step) and whatever the sign of the point before it.
__device__ inline int seg_cert(const KParams& P, const double* X0, const double* VA, double E, double s0, double s1,
                               double cert_lhs, double cert_rhs) {
  // The radii's square root and the three reciprocals in single precision (v_sqrt_f32, v_rcp_f32 of
  // the rounded operand: relative error < 3e-7 each): every bound below is widened by 2e-6 (db, the
  // negative test) or 1e-6 (g^rr, bmin, rmin > 10) to stay conservative, and the negative test's
  // own 1e-6 margin on m_a² is kept whole; a certified segment is still provably one-signed.
  const double rm2 = line_rmin2(X0, VA, s0, s1);
  const double rmin = (double)__builtin_amdgcn_sqrtf((float)rm2);
  double xa[3], xb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { xa[i] = X0[i] + VA[i] * s0; xb[i] = X0[i] + VA[i] * s1; }
  const double ra2 = xa[0] * xa[0] + xa[1] * xa[1] + xa[2] * xa[2];
  const double rb2 = xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2];
  const double ba = (P.cm * (3.0 * xa[2] * xa[2] - ra2) + 3.0 * P.sm * xa[0] * xa[2]) * (double)__builtin_amdgcn_rcpf((float)ra2);
  const double bb = (P.cm * (3.0 * xb[2] * xb[2] - rb2) + 3.0 * P.sm * xb[0] * xb[2]) * (double)__builtin_amdgcn_rcpf((float)rb2);
  const double irmin = (double)__builtin_amdgcn_rcpf((float)rmin);
  const double al = (s1 - s0) * irmin;
  const double db = 0.75 * al * al * (1.0 + 2e-6) + 1e-12;
  const double bmax = fmin(2.0, fmax(fabs(ba), fabs(bb)) * (1.0 + 1e-6) + db);
  if (cert_lhs * 0.5 * bmax < cert_rhs * (rm2 * rmin) * (1.0 - 2e-6)) return 1;
  if (rmin > 10.0 * (1.0 + 1e-6)) {
    const double bmin = (ba * bb > 0.0) ? fmin(fabs(ba), fabs(bb)) * (1.0 - 1e-6) - db : -1.0;
    const double rmax2 = fmax(ra2, rb2);
    const double grr = 1.0 - P.rs_gr * irmin * (1.0 + 1e-6);  // (rounded down: a smaller g^rr)
    if (bmin > 0.0 && P.wp2n * bmin * grr > E * E * (1.0 + 1e-6) * (rmax2 * sqrt(rmax2))) return 2;
  }
  return 0;
}

// Two builds, by waves per SIMD (the LDS allows 3): at 3 the kernel spills a few
// loop-invariant values, reloaded once per scan step -- a good trade where a line has ~111
// steps with uncertified ones among them, not where it has ~650 mostly skipped ones
// (launch_sample picks by the line length).
//
// HALO (art_halo.h): the speed at infinity s is drawn per attempt from the proposal of scale vp
// (halo_speed of U[6]; U[7] and U[8] are drawn and unused, so the stream does not move) and
// vifty is the incoming asymptote of the Kepler orbit through the accepted point
// (halo_asymptote). The proposal scale is the kernel's one more argument, `vp`: a parameter pack
// that is empty without HALO, so those instantiations keep their argument list and their code.
__device__ inline double halo_vp() { return 0.0; }
__device__ inline double halo_vp(double vp) { return vp; }

template <int WPS, bool BLOCKS, bool HALO = false, class... VP>
__global__ __launch_bounds__(256, WPS) void sample_kernel(const KParams P, const double maxR, const uint64_t seed,
                                                     const int64_t ray_offset, const int64_t n, double* __restrict__ xo,
                                                     double* __restrict__ ko, double* __restrict__ ergo,
                                                     double* __restrict__ vifo, int32_t* __restrict__ wo,
                                                     int32_t* __restrict__ ao, unsigned long long* __restrict__ queue,
                                                     const VP... vp) {
  static_assert(sizeof...(VP) == (HALO ? 1 : 0), "the HALO builds take the proposal scale, the others nothing");
  // line data of every lane [component][lane]: x0 (3), va (3), vl (3), E, 1/E², vIfty (3; HALO: s
  // in row 11, rows 12 and 13 unused).
  // A lane reads its own line from here too (its registers hold none of it across the step
  // loop: the kernel fits 2 waves/SIMD without spills)
  __shared__ double sline[14 * 256];
  __shared__ double slast[256];           // value at the step's last point
  __shared__ unsigned char ssrc[2 * 256];  // compact lists: uncertified lanes, certified lanes
  __shared__ double sqa[4 * SQCAP], sqb[4 * SQCAP];  // bracket queue: ends -> root
  __shared__ unsigned char sqsrc[4 * SQCAP], sqok[4 * SQCAP];
  __shared__ double sgrid[32];  // (0.5 j)/19: a full step's grid offsets, the same rounding as the division
  __shared__ unsigned char spair[4 * 64 * 3];  // a wave's (lane, step of the block) pairs to scan: lane << 2 | step
  __shared__ unsigned sbm[256];  // (step-by-step scan) a lane's sign changes of the step not queued yet
  const int lane = threadIdx.x & 63;
  const int wb = threadIdx.x & ~63;
  const int wq = (threadIdx.x >> 6) * SQCAP;
  double* const Lx = sline + threadIdx.x;
  int64_t ray = -1;
  uint32_t attempt = 0;
  int64_t wnext = 0, wend = 0;
  bool exhausted = false;
  const double send = 2.2 * maxR;
  const int nsteps = (int)ceil(send / 0.5);
  const int np = 20;  // ContinuousCallback(interp_points=20) (:1603)
  const int nper = np - 1;
  // certified-negative scan steps: GJ plasma without a boundary layer only (ART_SCAN_CERT=0: off)
  const bool cert_ok = !(P.bndry_lyr > 0.0) && P.mass_a > 0.0 && P.cert_fac < 1e300;
  const double cert_lhs = 2.0 * P.wp2n, cert_rhs = P.mass_a2 * (1.0 - 1e-6);
  // r_win³ = 2 wp2n / (m_a² (1 - 1e-6)) with a margin: ωp² < m_a² (1 - 1e-6) beyond it
  const double r_win2 = cert_ok ? pow(cert_lhs / cert_rhs, 2.0 / 3.0) * (1.0 + 3e-6) : 0.0;
  // sampler_sign_fast's domain (the condition's exterior branch: r > 10 km, r >= rNS) with a margin,
  // and the radius below which both ends of a step put all of it inside the star
  const double r_lim = fmax(10.0, P.rNS) * (1.0 + 1e-9), r_lim2 = r_lim * r_lim;
  const double r_in2 = (P.rNS * (1.0 - 1e-9)) * (P.rNS * (1.0 - 1e-9));
  const unsigned long long lt = (1ull << lane) - 1ull;
  if (threadIdx.x < np) sgrid[threadIdx.x] = 0.5 * double(threadIdx.x) / double(np - 1);
  __syncthreads();
#ifdef ART_SAMPLER_SECTIONS
  // dev build: s_memtime cycles per section, summed over the wave's iterations, into queue[8..15]
  // [refill + line set-up, step loop control + window, certificate, grid pass, brackets + flush,
  //  sample out]; queue[14] wave-steps with a grid pass, queue[15] wave-steps run
  unsigned long long q_sec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long q_last = __builtin_amdgcn_s_memtime();
#define ART_QMARK(k)                                                \
  {                                                                 \
    const unsigned long long q_now_ = __builtin_amdgcn_s_memtime(); \
    q_sec[k] += q_now_ - q_last;                                    \
    q_last = q_now_;                                                \
  }
#else
#define ART_QMARK(k)
#endif
  while (true) {
    if (!exhausted) {
      unsigned long long need = __ballot(ray < 0);
      while (need != 0ull && !exhausted) {
        if (wnext >= wend) {
          unsigned long long base = 0;
          const int leader = __ffsll((long long)need) - 1;
          if (lane == leader) base = atomicAdd(queue, (unsigned long long)CHUNK);
          base = __shfl(base, leader);
          if ((int64_t)base >= n) { exhausted = true; break; }
          wnext = (int64_t)base;
          wend = (wnext + CHUNK < n) ? wnext + CHUNK : n;
        }
        const int rank = __popcll(need & lt);
        const int64_t avail = wend - wnext;
        const int take = (int)(avail < (int64_t)__popcll(need) ? avail : (int64_t)__popcll(need));
        if (ray < 0 && rank < take) { ray = wnext + rank; attempt = 0; }
        wnext += take;
        need = __ballot(ray < 0);
      }
    }
    if (__ballot(ray >= 0) == 0ull) break;
    const bool active = ray >= 0;

    // ---- one attempt of every active lane: its line (:1486-1531) ----
    double U[10];
    attempt_uniforms(seed, uint64_t(ray_offset + (active ? ray : 0)), attempt, U);
    // sin(acos c) as √((1 - c)(1 + c)) and the FMA sincos of the integrator (arguments in
    // [0, 2π)): equal to the reference's values to an ulp, without ocml's acos and its
    // large-argument sincos path, whose registers set the kernel's occupancy
    double sti, cti, spi, cpi, stl, ctl, spl, cpl, sR, cR;
    cti = 1.0 - 2.0 * U[0];
    sti = sqrt((1.0 - cti) * (1.0 + cti));
    msincos(U[1] * 2.0 * PI, spi, cpi);
    ctl = 1.0 - 2.0 * U[2];
    stl = sqrt((1.0 - ctl) * (1.0 + ctl));
    msincos(U[3] * 2.0 * PI, spl, cpl);
    msincos(U[4] * 2.0 * PI, sR, cR);
    const double rR = sqrt(U[5]) * maxR;
    const double va[3] = {sti * cpi, sti * spi, cti};
    const double vl[3] = {stl * cpl, stl * spl, ctl};
    const double x1 = rR * cR, x2 = rR * sR;
    // rotate (x1, x2, 0) by Inv[EulerMatrix(ϕi, θi, 0)] (:1523-1524); cos(-a) = cos a, sin(-a) = -sin a
    double x0[3] = {x1 * cpi * cti - x2 * spi, x2 * cpi + x1 * spi * cti, -x1 * sti};
    double vI[3], vmag;
    if constexpr (HALO) {
      vmag = halo_speed(U[6], halo_vp(vp...));
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) vI[i] = (220.0 + U[6 + i] * 1.0e-5) / sqrt(3.0);
      vmag = sqrt(vI[0] * vI[0] + vI[1] * vI[1] + vI[2] * vI[2]);
    }
    const double gammaA = 1.0 / sqrt(1.0 - (vmag / C_KM) * (vmag / C_KM));
    const double E = P.mass_a * sqrt(1.0 + (vmag / C_KM * gammaA) * (vmag / C_KM * gammaA));
    const double iE2 = 1.0 / (E * E);
#pragma unroll
    for (int i = 0; i < 3; ++i) x0[i] += va[i] * (-maxR * 1.1);
    int randInx = 1 + (int)(U[9] * 6.0);
    if (randInx > 6) randInx = 6;
    int count = 0;
    double xsel[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Lx[i * 256] = x0[i];
      Lx[(3 + i) * 256] = va[i];
      Lx[(6 + i) * 256] = vl[i];
    }
    Lx[9 * 256] = E;
    Lx[10 * 256] = iE2;
    if constexpr (HALO) {
      Lx[11 * 256] = vmag;
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) Lx[(11 + i) * 256] = vI[i];
    }
    double c_prev = sampler_condition_e(P, x0, vl, E, iE2);
    int qn = 0;  // queued brackets (wave-uniform)
    // This line's window: its chord through the sphere r <= r_win, outside which
    // ωp² <= 2 wp2n / r³ < m_a² (1 - 1e-6) on every point (|b| <= 2), so every step there is
    // certified negative once the point before is negative -- the certificate below would say
    // so too, step by step; here it costs one comparison, and a wave whose lanes are all
    // outside their windows jumps to the next window (the big-maxR scan points walk ~650
    // steps per line, ~99% of them certified).
    double w_in = 1e300, w_out = -1e300;
    if (active && cert_ok) {
      const double sc = -(x0[0] * va[0] + x0[1] * va[1] + x0[2] * va[2]);
      const double h2 = r_win2 - ((x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]) - sc * sc);
      if (h2 > 0.0) {
        const double h = sqrt(h2);
        w_in = sc - h - 1e-6;
        w_out = sc + h + 1e-6;
      }
    }

    // resolve the queued brackets: Illinois on the exact line (the lane that found one owns
    // it), then each owner counts its valid crossings in queue order and keeps the randInx-th
    auto flush = [&]() {
      wave_lds_sync();
      #pragma unroll 1
      for (int t = lane; t < qn; t += 64) {
        const int src = sqsrc[wq + t];
        const double* S = sline + wb + src;
        const double X0[3] = {S[0], S[256], S[2 * 256]}, VA[3] = {S[3 * 256], S[4 * 256], S[5 * 256]};
        const double VL[3] = {S[6 * 256], S[7 * 256], S[8 * 256]};
        const double Es = S[9 * 256], iEs = S[10 * 256];
        double a = sqa[wq + t], b = sqb[wq + t], root = b;
        double xr[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) xr[i] = X0[i] + VA[i] * a;
        double fa = sampler_condition_e(P, xr, VL, Es, iEs);
#pragma unroll
        for (int i = 0; i < 3; ++i) xr[i] = X0[i] + VA[i] * b;
        double fb = sampler_condition_e(P, xr, VL, Es, iEs);
        int side = 0;
        #pragma unroll 1
        for (int it = 0; it < 100; ++it) {  // Illinois on the exact line
          root = a - fa * (b - a) / (fb - fa);
#pragma unroll
          for (int i = 0; i < 3; ++i) xr[i] = X0[i] + VA[i] * root;
          const double fr = sampler_condition_e(P, xr, VL, Es, iEs);
          if (fr == 0.0 || (b - a) < 1e-13 * fmax(1.0, fabs(root))) break;
          if (signbit(fr) == signbit(fa)) { a = root; fa = fr; if (side == -1) fb *= 0.5; side = -1; }
          else { b = root; fb = fr; if (side == 1) fa *= 0.5; side = 1; }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) xr[i] = X0[i] + VA[i] * root;
        // affect! (:1585-1597): keep crossings outside the star with E_loc > ωp
        const double rr = sqrt(xr[0] * xr[0] + xr[1] * xr[1] + xr[2] * xr[2]);
        double gtt, grr;
        metric_tr(rr, P.rs_gr, gtt, grr);
        sqa[wq + t] = root;
        sqok[wq + t] = (rr > P.rNS && Es / sqrt(grr) > wp_cart(P, xr)) ? 1 : 0;
      }
      wave_lds_sync();
      for (int t = 0; t < qn; ++t) {
        if (sqsrc[wq + t] == lane && sqok[wq + t] && active) {
          ++count;
          if (count == randInx) {
            const double r = sqa[wq + t];
#pragma unroll
            for (int i = 0; i < 3; ++i) xsel[i] = Lx[i * 256] + Lx[(3 + i) * 256] * r;
          }
        }
      }
      qn = 0;
      wave_lds_sync();
    };

    ART_QMARK(0)
    if constexpr (BLOCKS) {
    // Blocks of KB = 3 steps (1.5 km). Per block: ONE certificate of the whole block per lane (most
    // blocks away from the conversion surface pass it); the steps of the lanes whose block failed
    // are certified one by one as wave-cooperative items (lane, step); the grid points of every
    // uncertified (lane, step) pair of the block are evaluated together, 64 items a pass, so a pass
    // is rarely left part-empty. A certificate holds whatever the point before it (the sign logic
    // below sees a certified point as the value it provably has: nonzero, of the certified sign),
    // so a block or step is certified whatever c_prev is, and a sign change at its first point is
    // found by the same bit logic as an evaluated one. The evaluated points and their arithmetic
    // are those of the step-by-step scan (ART_SAMPLER_STEPWISE), so the samples do not change.
    // (the step masks of a block share 64-bit words: at most 3 steps; blocks of 2 measured slower,
    // 128 vs 119 ms per 1e7 flat samples, profiles/r05h_ab_sampler.txt)
    constexpr int KB = 3;
    const int wp = (threadIdx.x >> 6) * 64 * KB;  // this wave's pair list in spair
    for (int st0 = 0; st0 < nsteps; st0 += KB) {
#ifdef ART_SAMPLER_SECTIONS
      q_sec[7] += 1;
#endif
      const int kmax = min(KB, nsteps - st0);
      const double S0 = st0 * 0.5;
      const double S1 = fmin((st0 + kmax - 1) * 0.5 + 0.5, send);
      const bool quiet = !active || (cert_ok && c_prev < 0.0 && (S1 < w_in || S0 > w_out));
      if (__ballot(!quiet) == 0ull) {
        // every lane outside its window: jump to one step before the earliest next window start
        int nxt = (active && S1 < w_in && w_in < send) ? (int)floor(w_in * 2.0) - 1 : nsteps;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) nxt = min(nxt, __shfl_xor(nxt, o));
        nxt = __builtin_amdgcn_readfirstlane(nxt);  // (wave-uniform: keeps the step counter and kmax scalar)
        if (nxt > st0 + KB) st0 = nxt - KB;
        continue;
      }
      ART_QMARK(1)
      int bc = 0;  // the whole block certified: 1 negative, 2 positive
      if (active && quiet) {
        bc = 1;  // outside its window after a negative point
      } else if (active && cert_ok) {
        const double X0[3] = {Lx[0], Lx[256], Lx[2 * 256]}, VA[3] = {Lx[3 * 256], Lx[4 * 256], Lx[5 * 256]};
        bc = seg_cert(P, X0, VA, E, S0, S1, cert_lhs, cert_rhs);
      }
      const unsigned kmask = (1u << kmax) - 1u;
      unsigned cneg = bc == 1 ? kmask : 0u, cpos = bc == 2 ? kmask : 0u;  // certified steps, bit k
      // the steps of the lanes whose block failed, certified as items (lane u, step k), t = u kmax + k
      const bool fail = active && cert_ok && bc == 0 && kmax > 1;
      const unsigned long long mF = __ballot(fail);
      if (mF != 0ull) {
        const int nF = __popcll(mF);
        const int fix = __popcll(mF & lt);
        if (fail) ssrc[wb + fix] = (unsigned char)lane;
        wave_lds_sync();
        const int totc = nF * kmax;
        #pragma unroll 1
        for (int w0 = 0; w0 < totc; w0 += 64) {
          const int t = w0 + lane;
          int r = 0;
          if (t < totc) {
            const int u = t / kmax;
            const int k = t - u * kmax;
            const double* S = sline + wb + ssrc[wb + u];
            const double X0[3] = {S[0], S[256], S[2 * 256]}, VA[3] = {S[3 * 256], S[4 * 256], S[5 * 256]};
            const double s0 = (st0 + k) * 0.5;
            r = seg_cert(P, X0, VA, S[9 * 256], s0, fmin(s0 + 0.5, send), cert_lhs, cert_rhs);
          }
          const unsigned long long mn = __ballot(r == 1), mp = __ballot(r == 2);
          if (fail) {
            const int a = fix * kmax;
            const int lo = max(a, w0), hi = min(a + kmax, w0 + 64);
            if (lo < hi) {
              const unsigned long long run = (1ull << (hi - lo)) - 1ull;
              cneg |= (unsigned)((mn >> (lo - w0)) & run) << (lo - a);
              cpos |= (unsigned)((mp >> (lo - w0)) & run) << (lo - a);
            }
          }
        }
        wave_lds_sync();
      }
      ART_QMARK(2)
      // the uncertified (lane, step) pairs, lane-major, each lane's in step order: their grid points
      // are the items t = pair nper + j - 1, and each owner takes its pairs' runs of the ballots
      const unsigned unc = active ? (kmask & ~(cneg | cpos)) : 0u;
      const int m = __popc(unc);
      const unsigned long long b0 = __ballot(m & 1), b1 = __ballot(m & 2);
      const int off = __popcll(b0 & lt) + 2 * __popcll(b1 & lt);
      const int npairs = __popcll(b0) + 2 * __popcll(b1);
      // bits [20 k, 20 k + 20): signbit / nonzero-ness of step k's point j (bit 0: the point before it)
      unsigned long long sb = 0ull, nz = 0ull;
      if (npairs > 0) {
#ifdef ART_SAMPLER_SECTIONS
        q_sec[6] += 1;
#endif
        {
          unsigned rem = unc;
          for (int i = 0; rem != 0u; ++i) {
            spair[wp + off + i] = (unsigned char)(lane << 2 | __builtin_ctz(rem));
            rem &= rem - 1u;
          }
        }
        wave_lds_sync();
        const int tot = npairs * nper;
        __builtin_amdgcn_s_setprio(0);
        #pragma unroll 1
        for (int w0 = 0; w0 < tot; w0 += 64) {
          const int t = w0 + lane;
          bool neg = false, nonz = false;
          if (t < tot) {
            const int pr = t / nper;
            const int j = t - pr * nper + 1;
            const int e = spair[wp + pr];
            const int src = e >> 2, k = e & 3;
            const double* S = sline + wb + src;
            const double s0 = (st0 + k) * 0.5;
            const double s1 = fmin(s0 + 0.5, send);
            // (s1 - s0) j / 19: from the table for a full 0.5 km step, else divided
            const double sc = s0 + (s1 - s0 == 0.5 ? sgrid[j] : (s1 - s0) * double(j) / double(np - 1));
            double xl[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) xl[i] = S[i * 256] + S[(3 + i) * 256] * sc;
            const double VL[3] = {S[6 * 256], S[7 * 256], S[8 * 256]};
            const int fs = cert_ok ? sampler_sign_fast(P, xl, VL, P.mass_a2 * S[10 * 256], r_lim2) : 0;
            double v = fs == 1 ? -1.0 : 1.0;  // (a decided point: only its sign and nonzero-ness are read)
            if (fs == 0) v = sampler_condition_e(P, xl, VL, S[9 * 256], S[10 * 256]);
            if (j == nper && k == kmax - 1) slast[wb + src] = v;
            neg = signbit(v);
            nonz = v != 0.0;
          }
          const unsigned long long mneg = __ballot(neg), mnz = __ballot(nonz);
          unsigned rem = unc;
          for (int i = 0; rem != 0u; ++i) {
            const int k = __builtin_ctz(rem);
            rem &= rem - 1u;
            const int a = (off + i) * nper;
            const int lo = max(a, w0), hi = min(a + nper, w0 + 64);
            if (lo < hi) {
              const unsigned long long run = (1ull << (hi - lo)) - 1ull;
              const int at = 20 * k + (lo - a) + 1;
              sb |= ((mneg >> (lo - w0)) & run) << at;
              nz |= ((mnz >> (lo - w0)) & run) << at;
            }
          }
        }
        __builtin_amdgcn_s_setprio(1);
        wave_lds_sync();
      }
      ART_QMARK(3)
      if (active) {
        // certified steps: points 1..19 nonzero and of the certified sign
        const unsigned long long p19 = 0xFFFFEull;
        for (int k = 0; k < kmax; ++k) {
          if ((cneg >> k) & 1u) { sb |= p19 << (20 * k); nz |= p19 << (20 * k); }
          else if ((cpos >> k) & 1u) nz |= p19 << (20 * k);
        }
        // bit 0 of each step: the point before it (c_prev, then the previous step's point 19)
        sb |= signbit(c_prev) ? 1ull : 0ull;
        nz |= (c_prev != 0.0) ? 1ull : 0ull;
        for (int k = 1; k < kmax; ++k) {
          sb |= ((sb >> (20 * k - 1)) & 1ull) << (20 * k);
          nz |= ((nz >> (20 * k - 1)) & 1ull) << (20 * k);
        }
        const int kl = kmax - 1;  // the value the next block's first bracket starts from (read for its sign)
        if ((unc >> kl) & 1u) c_prev = slast[threadIdx.x];
        else if ((cneg >> kl) & 1u) c_prev = -1.0;
        else if ((cpos >> kl) & 1u) c_prev = 1.0;
      }
      // queue the sign changes in (point j-1, point j] of each step (signbits differ, both nonzero),
      // step by step, so each lane's brackets stay in their order along the line
      for (int k = 0; k < kmax; ++k) {
        const int st = st0 + k;
        const double s0 = st * 0.5;
        const double s1 = fmin(s0 + 0.5, send);
        const unsigned sbk = (unsigned)(sb >> (20 * k)) & 0xFFFFFu, nzk = (unsigned)(nz >> (20 * k)) & 0xFFFFFu;
        unsigned br = active ? (sbk ^ (sbk << 1)) & nzk & (nzk << 1) & (((1u << np) - 1u) & ~1u) : 0u;
        unsigned long long bm = __ballot(br != 0u);
        if (bm == 0ull) continue;
        // the previous step's last grid point, where a bracket at point 1 opens
        const double ps0 = (st - 1) * 0.5;
        const double pds = fmin(ps0 + 0.5, send) - ps0;
        const double s_start = st == 0 ? 0.0 : ps0 + (pds == 0.5 ? sgrid[nper] : pds * double(nper) / double(np - 1));
        while (bm != 0ull) {
          if (qn + 64 > SQCAP) flush();
          if (br != 0u) {
            const int ip = __builtin_ctz(br);
            const int slot = qn + __popcll(bm & lt);
            sqa[wq + slot] = (ip == 1) ? s_start : s0 + (s1 - s0) * double(ip - 1) / double(np - 1);
            sqb[wq + slot] = s0 + (s1 - s0) * double(ip) / double(np - 1);
            sqsrc[wq + slot] = (unsigned char)lane;
            br &= br - 1u;
          }
          qn = __builtin_amdgcn_readfirstlane(qn + __popcll(bm));  // (wave-uniform)
          bm = __ballot(br != 0u);
        }
      }
      ART_QMARK(4)
    }
    } else {  // step by step (round 4)
    // The bracket queue is resolved (flush: Illinois with its three inlined conditions) at the top
    // of this loop and after it, not inside the insertion below: a queue that fills up there ends
    // the pass, the rest wait in sbm, and the loop comes back to the same step after resolving it.
    // Inside the insertion the flush's registers stacked on the step's live state: 71 spilled VGPRs
    // in the 3-wave build, 51 now; 10^7 flat samples 118 -> 115 ms, bit-identical
    // (profiles/r05q_ab_sampler_flush.txt). (The block scan, 2 waves/SIMD, does not spill.)
    bool sres = false;  // (wave-uniform) this step's brackets wait behind a full queue
    for (int st = 0; st < nsteps;) {
      const double s0 = st * 0.5;
      const double s1 = fmin(s0 + 0.5, send);
      if (sres) {
        flush();
      } else {
#ifdef ART_SAMPLER_SECTIONS
      q_sec[7] += 1;
#endif
      const bool quiet = !active || (cert_ok && c_prev < 0.0 && (s1 < w_in || s0 > w_out));
      if (__ballot(!quiet) == 0ull) {
        // every lane is certified outside its window: jump to one step before the earliest
        // next window start (certified steps change nothing but the step counter)
        int nxt = (active && s1 < w_in && w_in < send) ? (int)floor(w_in * 2.0) - 1 : nsteps;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) nxt = min(nxt, __shfl_xor(nxt, o));
        nxt = __builtin_amdgcn_readfirstlane(nxt);  // (wave-uniform: keeps the step counter scalar)
        st = nxt > st + 1 ? nxt : st + 1;
        continue;
      }
      // Certified-negative step: with the axion shell imposed (w normalised), the condition
      // is ½(-m_a² + ωp² (1 - g^rr k∥²/E²))/E² with 0 <= g^rr k∥² <= E² (Cauchy-Schwarz, the
      // factor is at most 1), and ωp² = wp2n |b| / r³ <= 2 wp2n / r³ (|b| <= √(4a1² + a2²)
      // <= 2). Where 2 wp2n / r_min³ stays below m_a² on the whole segment (r_min: the line's
      // closest approach to the centre within [s0, s1]), all its points are negative. If the
      // point before is negative too, no sign change can occur: only the last point is
      // evaluated, for the value a bracket opening at the next step's first point starts from.
      //
      // Both bounds use b = Bz/B_n at the step's two end points, b = cosθm (3z² - r²)/r² +
      // 3 sinθm x z / r² (ψ = φ at t = 0): a quadratic form n̂ᵀ M n̂ of the direction n̂, M with
      // eigenvalues -cosθm and (cosθm ± 3)/2, so λmax - λmin = 3. The step projects onto a
      // great-circle arc of angle α <= L/r_min (the radial projection shrinks lengths by 1/|x|),
      // along which b(φ) = C + A cos 2φ + B sin 2φ with √(A² + B²) <= (λmax - λmin)/2, so
      // |b''| <= 6 and b stays within 6 α²/8 of the chord between its end values:
      // |b| <= min(2, max(|b_a|, |b_b|) + 0.75 α²), and where b_a, b_b share a sign,
      // |b| >= min(|b_a|, |b_b|) - 0.75 α². (Until round 3 the bound was the first-order
      // |b_a| ± (3 + 3|sinθm|) α, about 100x wider at 0.5 km steps: the uncertified steps
      // drop by a third)
      //  * negative: ωp² <= wp2n |b|max / r_min³ < m_a² (see above);
      //  * positive (the point before positive too): outside g_schwartz's interior patch
      //    (r > 10 km), g^rr g^tt = -1, so Cauchy-Schwarz on k∥ with w on the axion shell gives
      //    1 - g^rr k∥²/E² >= g^rr m_a²/E² and the condition >= ½ m_a² (ωp² g^rr/E² - 1)/E² > 0
      //    when wp2n |b|min g^rr(r_min) > E² r_max³ (r_max: at an end of the step).
      ART_QMARK(1)
      bool cert = active && quiet;
      if (active && !quiet && cert_ok && c_prev != 0.0 && !isnan(c_prev)) {
        const double X0[3] = {Lx[0], Lx[256], Lx[2 * 256]}, VA[3] = {Lx[3 * 256], Lx[4 * 256], Lx[5 * 256]};
        const double rm2 = line_rmin2(X0, VA, s0, s1);
        const double rmin = (double)__builtin_amdgcn_sqrtf((float)rm2);
        double xa[3], xb[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { xa[i] = X0[i] + VA[i] * s0; xb[i] = X0[i] + VA[i] * s1; }
        const double ra2 = xa[0] * xa[0] + xa[1] * xa[1] + xa[2] * xa[2];
        const double rb2 = xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2];
        // (the square root and reciprocals in single precision, < 3e-7 relative each, with the bounds
        // widened as in seg_cert; the 1e-6 margin on m_a² kept whole: a certified step is still
        // provably one-signed)
        const double ba = (P.cm * (3.0 * xa[2] * xa[2] - ra2) + 3.0 * P.sm * xa[0] * xa[2]) * (double)__builtin_amdgcn_rcpf((float)ra2);
        const double bb = (P.cm * (3.0 * xb[2] * xb[2] - rb2) + 3.0 * P.sm * xb[0] * xb[2]) * (double)__builtin_amdgcn_rcpf((float)rb2);
        const double irmin = (double)__builtin_amdgcn_rcpf((float)rmin);
        const double al = (s1 - s0) * irmin;
        const double db = 0.75 * al * al * (1.0 + 2e-6) + 1e-12;
        if (c_prev < 0.0) {
          const double bmax = fmin(2.0, fmax(fabs(ba), fabs(bb)) * (1.0 + 1e-6) + db);
          cert = cert_lhs * 0.5 * bmax < cert_rhs * (rm2 * rmin) * (1.0 - 2e-6);
        } else if (rmin > 10.0 * (1.0 + 1e-6)) {
          const double bmin = (ba * bb > 0.0) ? fmin(fabs(ba), fabs(bb)) * (1.0 - 1e-6) - db : -1.0;
          const double rmax2 = fmax(ra2, rb2);
          const double grr = 1.0 - P.rs_gr * irmin * (1.0 + 1e-6);  // (rounded down: a smaller g^rr)
          cert = bmin > 0.0 && P.wp2n * bmin * grr > E * E * (1.0 + 1e-6) * (rmax2 * sqrt(rmax2));
        }
      }
      const bool unc = active && !cert;
      // A step wholly inside the star (both ends below rNS, so the whole segment is) holds no
      // crossing affect! keeps (rr > rNS, :1585-1597): its brackets would all be resolved and
      // dropped, so none is queued, and only its last point is evaluated -- the value the next
      // step's first bracket starts from. (~40% of the flat workload's uncertified steps.)
      bool inner = false;
      if (unc && cert_ok) {
        const double X0[3] = {Lx[0], Lx[256], Lx[2 * 256]}, VA[3] = {Lx[3 * 256], Lx[4 * 256], Lx[5 * 256]};
        double xa[3], xb[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { xa[i] = X0[i] + VA[i] * s0; xb[i] = X0[i] + VA[i] * s1; }
        inner = fmax(xa[0] * xa[0] + xa[1] * xa[1] + xa[2] * xa[2], xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2]) < r_in2;
      }
      const unsigned long long mU = __ballot(unc && !inner), mI = __ballot(inner);
      const int nU = __popcll(mU), nI = __popcll(mI);
      ART_QMARK(2)
      if (nU + nI == 0) {  // all certified: no point, no bracket, c_prev unchanged
        ++st;
        continue;
      }
#ifdef ART_SAMPLER_SECTIONS
      q_sec[6] += 1;
#endif
      // this lane's rank among the uncertified ones (the inner steps' lanes after the others)
      const int uix = inner ? nU + __popcll(mI & lt) : __popcll(mU & lt);
      if (unc) ssrc[wb + uix] = (unsigned char)lane;
      // bit j: signbit / nonzero-ness of point j (bit 0: the step start)
      unsigned sb = signbit(c_prev) ? 1u : 0u, nz = (c_prev != 0.0) ? 1u : 0u;
      wave_lds_sync();
      // items: (uncertified lane u, point j = 1..nper) lane-major, t = u nper + j - 1. A certified
      // step needs no point at all: its last point -- the next step's bracket start -- has the
      // certified sign, and c_prev is only ever read for its sign (the next certificate, the
      // bit-0 sign and nonzero-ness of the next scan), so it keeps the value it had. Each pass's
      // signs come back as two ballots, from which every owner takes the run of its own items'
      // bits (round 4: until then point-major items ORed their bits into LDS words with two LDS
      // atomics each, ~13 lanes deep on one word, and divided by the variable nU: 3.3 LDS
      // bank-conflict cycles per LDS instruction. Samples bit-identical, time unchanged: the
      // kernel is VALU-bound, profiles/r04aq_sampler_pmc.txt).
      // items: the other lanes' 19 points each, then the inner lanes' last points
      const int totN = nU * nper, tot = totN + nI;
      __builtin_amdgcn_s_setprio(0);  // brackets: short dependent chains) at the high one: 118.5 -> 117.1 ms
      #pragma unroll 1
      for (int w0 = 0; w0 < tot; w0 += 64) {
        const int t = w0 + lane;
        bool neg = false, nonz = false;
        if (t < tot) {
          int src, j;
          if (t < totN) {
            const int u = t / nper;
            j = t - u * nper + 1;
            src = ssrc[wb + u];
          } else {
            j = nper;
            src = ssrc[wb + nU + (t - totN)];
          }
          const double* S = sline + wb + src;
          // (s1 - s0) j / 19: from the table for a full 0.5 km step (wave-uniform), else divided
          const double sc = s0 + (s1 - s0 == 0.5 ? sgrid[j] : (s1 - s0) * double(j) / double(np - 1));
          double xl[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) xl[i] = S[i * 256] + S[(3 + i) * 256] * sc;
          const double VL[3] = {S[6 * 256], S[7 * 256], S[8 * 256]};
          // the point's sign without the condition where it is decided (sampler_sign_fast), else the
          // condition itself; a decided point carries ±1 (only its sign and nonzero-ness are read)
          const int fs = cert_ok ? sampler_sign_fast(P, xl, VL, P.mass_a2 * S[10 * 256], r_lim2) : 0;
          double v = fs == 1 ? -1.0 : 1.0;
          if (fs == 0) v = sampler_condition_e(P, xl, VL, S[9 * 256], S[10 * 256]);
          if (j == nper) slast[wb + src] = v;
          neg = signbit(v);
          nonz = v != 0.0;
        }
        const unsigned long long mneg = __ballot(neg), mnz = __ballot(nonz);
        if (unc && !inner) {
          const int a = uix * nper;
          const int lo = max(a, w0), hi = min(a + nper, w0 + 64);
          if (lo < hi) {
            const unsigned long long run = (1ull << (hi - lo)) - 1ull;
            const int at = lo - a + 1;
            sb |= (unsigned)((mneg >> (lo - w0)) & run) << at;
            nz |= (unsigned)((mnz >> (lo - w0)) & run) << at;
          }
        }
      }
      __builtin_amdgcn_s_setprio(1);
      wave_lds_sync();
      // this lane's sign changes in (point j-1, point j]: signbits differ, both values nonzero
      unsigned br = 0u;
      if (unc) {
        if (!inner) br = (sb ^ (sb << 1)) & nz & (nz << 1) & (((1u << np) - 1u) & ~1u);
        c_prev = slast[threadIdx.x];
      }
      ART_QMARK(3)
      if (__ballot(br != 0u) == 0ull) {
        ++st;
        continue;
      }
      sbm[threadIdx.x] = br;
      }
      // the previous step's last grid point, where a bracket at point 1 opens
      const double ps0 = (st - 1) * 0.5;
      const double pds = fmin(ps0 + 0.5, send) - ps0;
      const double s_start = st == 0 ? 0.0 : ps0 + (pds == 0.5 ? sgrid[nper] : pds * double(nper) / double(np - 1));
      // queue the brackets, each lane's in its order along the line
      unsigned br = sbm[threadIdx.x];
      unsigned long long bm = __ballot(br != 0u);
      sres = false;
      while (bm != 0ull) {
        if (qn + 64 > SQCAP) {  // (the rest wait in sbm; the loop's top resolves the queue)
          sres = true;
          sbm[threadIdx.x] = br;
          break;
        }
        if (br != 0u) {
          const int ip = __builtin_ctz(br);
          const int slot = qn + __popcll(bm & lt);
          sqa[wq + slot] = (ip == 1) ? s_start : s0 + (s1 - s0) * double(ip - 1) / double(np - 1);
          sqb[wq + slot] = s0 + (s1 - s0) * double(ip) / double(np - 1);
          sqsrc[wq + slot] = (unsigned char)lane;
          br &= br - 1u;
        }
        qn = __builtin_amdgcn_readfirstlane(qn + __popcll(bm));  // (wave-uniform)
        bm = __ballot(br != 0u);
      }
      ART_QMARK(4)
      if (!sres) ++st;
    }
    }
    if (qn > 0) flush();
    ART_QMARK(4)

    if (active) {
      const bool give_up = attempt + 1 >= 1000000u;  // bounded: no conversion surface reachable
      if (count >= randInx || give_up) {
        if (count < randInx) { xsel[0] = xsel[1] = xsel[2] = NAN; count = 0; }
        const double rmag = sqrt(xsel[0] * xsel[0] + xsel[1] * xsel[1] + xsel[2] * xsel[2]);
        double vIl[3], vmagl;
        if constexpr (HALO) {
          // the asymptote of the Newtonian orbit through (xsel, vl) with the attempt's speed
          vmagl = Lx[11 * 256];
          const double dl[3] = {Lx[6 * 256], Lx[7 * 256], Lx[8 * 256]};
          halo_asymptote(xsel, dl, vmagl, P.GM_c2 * C_KM * C_KM, vIl);
        } else {
          vIl[0] = Lx[11 * 256]; vIl[1] = Lx[12 * 256]; vIl[2] = Lx[13 * 256];
          vmagl = sqrt(vIl[0] * vIl[0] + vIl[1] * vIl[1] + vIl[2] * vIl[2]);  // = vmag
        }
        const double vml = sqrt(vmagl * vmagl + 2.0 * P.GM_c2 * C_KM * C_KM / rmag) / C_KM;  // :1644
        double vel[3], vc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { vel[i] = Lx[(6 + i) * 256] * vml; vc[i] = vIl[i] / C_KM; }
        // MainRunner.jl:514-529: erg_inf_ini from vIfty/c, k_init = k_norm_Cart(ax_fix = true)
        const double vm = sqrt(vc[0] * vc[0] + vc[1] * vc[1] + vc[2] * vc[2]);
        const double gA = 1.0 / sqrt(1.0 - vm * vm);
        const double Ei = P.mass_a * sqrt(1.0 + (vm * gA) * (vm * gA));
        double kn[3];
        k_norm_axion_shell(P, xsel, vel, Ei, kn);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          xo[c * n + ray] = xsel[c];
          ko[c * n + ray] = kn[c];
          vifo[c * n + ray] = vc[c];
        }
        ergo[ray] = Ei;
        wo[ray] = count;
        ao[ray] = (int32_t)(attempt + 1);
        ray = -1;
      } else {
        ++attempt;
      }
    }
    ART_QMARK(5)
  }
#ifdef ART_SAMPLER_SECTIONS
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 8; ++k) atomicAdd(queue + 8 + k, q_sec[k]);
#endif
}

}  // namespace art
