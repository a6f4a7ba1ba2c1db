// art_propagate.h -- propagate_kernel, the persistent integrator.
//
// propagate_kernel: RT.propagate (RayTracer.jl:171-452) for a batch of segments.
//   * one wavefront lane per ray; the 7-D state u = [r θ φ | w | u7] and its FSAL
//     derivative live in VGPRs; NS parameters are kernel arguments (SGPRs);
//   * persistent lanes with a wave-aggregated work queue: a lane whose segment ends pulls
//     the next ray id from a 64-ray chunk the wave claimed with ONE global atomicAdd, so
//     short and long segments (12 vs 5000 steps) never idle a wave;
//   * every loop iteration is ONE integrator step attempt for every live lane: ordinary
//     adaptive steps, and the re-steps that polish a resonance root on the true
//     trajectory (mode ROOT), run the same unrolled stage code in lockstep;
//   * HBM is touched only to load a segment's initial conditions and to store its end
//     state and its crossings (Σ ≈ 220 B per segment).
#pragma once
#include "art_ray_io.h"

namespace art {

// DON: the tail-donation instantiations (SegOut::donate / cont_mode honoured); the others
// carry none of that code, so a lone pass pays nothing for it
// WPS: waves per SIMD the registers are budgeted for (the default 2; the GR continuation
// launch, below, uses 1)
// CYC: the cyclotron-resonance observation (SegOut::cyc_tau ...; Vern6 without saveat, DON 0/1);
// the other instantiations carry none of its code
template <int INTEG, int GEOM, bool SAVE, int DON, int WPS = ART_WAVES_PER_SIMD, bool CYC = false>
__global__ __launch_bounds__(BLOCK, WPS) void propagate_kernel(const KParams P_in, const int64_t n,
                                                                              const SegIn in, const SegOut out,
                                                                              const int32_t max_crossings,
                                                                              unsigned long long* __restrict__ queue,
                                                                              unsigned long long* __restrict__ stats) {
  const KParams P = specialize<GEOM>(P_in);
  // HEAD: the headline build (the streamed host call's flat Vern6 integrator) keeps fewer wave-uniform
  // scalars live across the stage slots, where the allocator parks them in lanes of v254/v255 and reads
  // them back tuple by tuple (DESIGN §3 "Register budget", §6 "Spilled scalars"):
  //  * its cold blocks (a crossing's record, a finishing lane's stores, the piece counts, the wave's end)
  //    read `in`, `out`, n and the statistics' address from the kernel-argument segment when they run
  //    (cold_args, art_ray_io.h);
  //  * ln_t_end and dtmin are scalar pairs of their own (own_pair) and the step size is one basic block:
  //    4 lane reads on every path, not 16-24;
  //  * the sign-code fast paths rebuild their masks from one scalar instead of restoring eight.
  // 127 -> 85 spill slots, 233 -> 118 lane reads in the main loop outside the slot loop; the host call
  // 87.1-87.7 -> 85.7-86.2 ms. Every other instantiation compiles to the code it had before: applied to
  // all builds, the same changes cost the device launch 0.5-0.9 ms and the GR batch 1%. The refill keeps
  // its arguments in registers: written through references, it changed every build's code.
  constexpr bool HEAD = DON == 3 && GEOM == GEOM_FLAT && !SAVE && !CYC && INTEG != ART_RK4;
  constexpr bool COLD = HEAD, OWN = HEAD, FASTN = HEAD;
  const SegIn& in_k = in;
  const SegOut& out_k = out;
  constexpr bool RK4 = (INTEG == ART_RK4);
  // the work queue: fresh rays [0, n), or in a continuation launch the donated records
  const bool cont = DON == 1 && out.cont_mode;
  const int64_t nq = cont ? (int64_t)*out.cont_src_count : n;
  unsigned long long* const rqueue = cont ? out.cont_queue : queue;
  // the callbacks (RayTracer.jl:357-368) are installed only when make_tree (:361-377)
  const bool cbs = max_crossings != ART_NO_CALLBACKS;
  constexpr int NSLOT = RK4 ? 4 : 8;
  constexpr int SUNROLL = GEOM == GEOM_GR ? SUNROLL_GR : SUNROLL_FLAT;
  const StageTable& T = RK4 ? c_rk4 : c_vern6;
  __shared__ double lds[LDS_SLOTS * 7 * BLOCK];  // [slot][component][lane]: conflict-free ds_read_b64
  __shared__ unsigned codes[SCAN_WORDS * BLOCK];  // [word][lane]: 2-bit sign codes of the grid scan
  __shared__ double lastv[BLOCK];                 // value at the last grid point (before: b at the step's end)
  __shared__ double lastt[BLOCK];                 // t at the step's end (the scan certificate)
  __shared__ unsigned char srcl[BLOCK];           // compact list of the wave's scanning lanes
  __shared__ double thgrid[SCAN_WORDS * 16 + 1];  // Θs = j/(npts-1): range(0, 1, length = npts)
  __shared__ unsigned pend_lds[BLOCK / 64][64];  // (DON = 3) per wave: finished rays per piece, not yet counted
  double* const L = lds + threadIdx.x;
  const int wbase = threadIdx.x & ~63;
  const int lane = threadIdx.x & 63;
  const double tend = OWN ? own_pair(P.ln_t_end) : P.ln_t_end, dtmin = OWN ? own_pair(P.dtmin) : P.dtmin;
  const int npts = P.interp_points;
  for (int j = threadIdx.x; j < npts; j += BLOCK) thgrid[j] = double(j) / double(npts - 1);
  if constexpr (DON == 3) {
    pend_lds[threadIdx.x >> 6][threadIdx.x & 63] = 0u;
    if (out.waves_started && (threadIdx.x & 63) == 0) {
      const unsigned long long old =
          __hip_atomic_fetch_add(out.waves_started, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (out.resident_host && old + 1ull == (unsigned long long)out.waves_total)  // (a vector store to host memory)
        __hip_atomic_store(out.resident_host, out.resident_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  span_stamp(stats, false);
  __syncthreads();

  int mode = M_IDLE;
  int ray = -1;
  // Loop-carried per-lane flags: bool lets the compiler keep them as 64-bit lane masks in SGPR
  // pairs, which the integrator's SGPR pressure spills to VGPR lanes; int keeps them in VGPRs.
  // The per-iteration flags of the loop below are int too (A/B: 1e7 flat -0.7%).
  int photon = true;
  double erg = 0.0;
  // qpow = qold^(1/15) of the PI controller, updated only when qold changes (on accept)
  const double qpow_init = pow(1e-4, 1.0 / 15.0);
  double u[7], f[7], tau = 0.0, dt = 0.0, qpow = qpow_init;
  double cprev = 0.0;
  double bstart = NAN;  // Bz/B_n at u (the previous step's last RHS) for the scan certificate
  int cprev_ok = true;  // cprev holds the condition at the step start (false after a certified step)
  int sprev = 0;
  int just_evented = false;
  int n_acc = 0, n_rej = 0, ncross = 0, iter = 0;
  double hroot = 0.0, r_tha = 0.0, r_ca = 0.0, r_thb = 0.0, r_cb = 0.0, r_t = 0.0, r_slope = 1.0, post_c = 0.0;
  int post_s = 0, r_side = 0, r_it = 0;
  int wnext = 0, wend = 0;
  int tick = 0;                          // (DON = 3) iterations, for the flushes of the piece counts
  bool cready = false;                   // (DON = 3) the claimed chunk's fresh state is in
  int save_k = 1;  // SAVE: the next interior saveat index
  double gprev = 0.0;  // CYC: cyclotron_g at (u, tau), recomputed whenever the lane takes a ray
  bool exhausted = false;
  unsigned s_att = 0, s_acc = 0, s_root = 0, s_scan = 0, s_interp = 0, s_rays = 0, s_cert = 0;
#ifdef ART_SECTION_TIMING
  // dev build: s_memtime cycles per main-loop section, summed over the wave's iterations
  unsigned long long t_sec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_last = __builtin_amdgcn_s_memtime();
#define ART_TMARK(k)                                                  \
  {                                                                   \
    const unsigned long long t_now_ = __builtin_amdgcn_s_memtime();   \
    t_sec[k] += t_now_ - t_last;                                      \
    t_last = t_now_;                                                  \
  }
#else
#define ART_TMARK(k)
#endif
#pragma unroll
  for (int i = 0; i < 7; ++i) { u[i] = 0.0; f[i] = 0.0; }

  while (true) {
    // ---- refill idle lanes from the wave's chunk (one atomicAdd per 64 rays) ----
    if (!exhausted) {
      unsigned long long need = __ballot(mode == M_IDLE);
      while (need != 0ull) {
        if (wnext >= wend) {
          unsigned long long base = 0;
          const int leader = __ffsll((long long)need) - 1;
          if (lane == leader) base = atomicAdd(rqueue, (unsigned long long)CHUNK);
          base = __shfl(base, leader);
          if ((int64_t)base >= nq) { exhausted = true; break; }
          wnext = __builtin_amdgcn_readfirstlane((int)base);
          wend = __builtin_amdgcn_readfirstlane((int)((int64_t)base + CHUNK < nq ? (int64_t)base + CHUNK : nq));
          cready = false;
        }
        int lim = wend;
        if constexpr (DON == 3) {
          // the chunk's fresh state (the helpers' chunk flag); while it is not in, a wave with
          // other rays goes on integrating them, and an empty wave waits (bounded)
          if (!cready) {
            const int leader = __ffsll((long long)need) - 1;
            if (!chunk_flag(out, wnext, leader)) {
              if (lane == leader) atomicAdd(out.init_next + 2, 1ull);  // (the misses, for the host's trace)
              if (__ballot(mode != M_IDLE) != 0ull) break;
              if (!chunk_wait(out, wnext, leader)) { exhausted = true; break; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            cready = true;
          }
        }
        const int rank = __popcll(need & ((1ull << lane) - 1ull));
        const int cnt = __popcll(need);
        const int take = (lim - wnext) < cnt ? (lim - wnext) : cnt;
        const bool takes = mode == M_IDLE && rank < take;
        if (mode == M_IDLE && rank < take && cont) {
          // a donated ray: its complete state from the tail-donation record
          mode = M_STEP;
          const double2* rq = reinterpret_cast<const double2*>(out.cont_src + (int64_t)(wnext + rank) * CONT_REC);
          double v[20];
#pragma unroll
          for (int i = 0; i < 10; ++i) {
            const double2 q = rq[i];
            v[2 * i] = q.x;
            v[2 * i + 1] = q.y;
          }
#pragma unroll
          for (int i = 0; i < 7; ++i) {
            u[i] = v[i];
            f[i] = v[7 + i];
          }
          tau = v[14];
          dt = v[15];
          qpow = v[16];
          cprev = v[17];
          bstart = v[18];
          erg = v[19];
          const int4 i0 = reinterpret_cast<const int4*>(rq + 10)[0], i1 = reinterpret_cast<const int4*>(rq + 10)[1];
          ray = i0.x;
          n_acc = i0.y;
          n_rej = i0.z;
          ncross = i0.w;
          iter = i1.x;
          sprev = i1.y;
          save_k = i1.w;
          photon = i1.z & 1;
          cprev_ok = (i1.z >> 1) & 1;
          just_evented = (i1.z >> 2) & 1;
        } else if (mode == M_IDLE && rank < take) {
          ray = (DON == 1 && out.order) ? out.order[wnext + rank] : wnext + rank;
          mode = M_STEP;
          // fresh segment: u0, f(u0), the initial dt and the initial condition value, all
          // precomputed by the init pass, with erg, ln t0 and the species: one 160-byte record
          const double2* rq = reinterpret_cast<const double2*>(in.u0 + (int64_t)ray * U0_REC);
          double v[U0_REC - 2];
#pragma unroll
          for (int i = 0; i < U0_REC / 2 - 1; ++i) {
            const double2 q = rq[i];
            v[2 * i] = q.x;
            v[2 * i + 1] = q.y;
          }
          const double sp = rq[U0_REC / 2 - 1].x;
#pragma unroll
          for (int i = 0; i < 7; ++i) {
            u[i] = v[i];
            f[i] = v[7 + i];
          }
          dt = v[14];
          cprev = v[15];
          erg = v[16];
          tau = v[17];
          photon = sp != 0.0;
          cprev_ok = true;
          bstart = NAN;
          sprev = isnan(cprev) ? 0 : sgn(cprev);
          n_acc = n_rej = ncross = iter = 0;
          save_k = 1;
          just_evented = false;
          qpow = qpow_init;  // qoldinit = 1e-4
          s_rays += 1;
        }
        if constexpr (CYC) {
          // the start-of-step g is a pure function of the state a ray is taken with (fresh, refilled
          // or a donated one resumed): never the value the lane's previous ray left behind
          if (takes) gprev = photon ? cyclotron_g(P, u, tau, erg) : 0.0;
        }
        wnext += take;
        need = __ballot(mode == M_IDLE);
      }
    }
    if (__ballot(mode != M_IDLE) == 0ull) break;  // every lane idle and the queue drained
    // A wave holding an outlier ray (PRIO_ITERS attempts and more: ~20x the mean) asks the
    // SIMD's arbiter for issue priority. The one ray that sets a launch's (or a scan point's)
    // drain time then runs at close to its lone-wave speed while the bulk of the batch still
    // shares its SIMD; the other waves fill the issue slots it leaves.
    const bool outlier = __ballot(iter >= PRIO_ITERS) != 0ull;
    if (outlier) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(0);
    ART_TMARK(0)  // refill

    // ---- this iteration's step size ----
    int last = false, forced = false;
    double hs = 0.0;
    if (mode == M_ROOT) {
      hs = r_t * hroot;
    } else if (mode == M_STEP) {
      // (min(dt, dtmax) is implied: the span end clips every step.) OWN: one basic block, selects and no
      // branches, so each of tend and dtmin is restored from its spill lanes once, whichever case the lane is
      if constexpr (OWN) {
        last = tau + dt >= tend;
        forced = !RK4 && !last && dt < dtmin;
        hs = last ? tend - tau : (forced ? dtmin : dt);
      } else {
        hs = dt;
        if (tau + hs >= tend) { hs = tend - tau; last = true; }
        else if (!RK4 && hs < dtmin) { hs = dtmin; forced = true; }
      }
    }

    // ---- stage slots: one RHS per slot per lane ----
    double kA[7], y[7], kk[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) kA[i] = 0.0;  // read (times a zero coefficient) before its first store
    // flat builds: the next slot's row of scalars is loaded before this slot's RHS, so its
    // scalar-load latency hides behind the RHS instead of opening the next slot: 1e7 flat device
    // launch 84.0 -> 83.4 ms (3 interleaved pairs, profiles/r05c_ab_prefetch.jsonl); the GR build
    // (slot loop unrolled by two) lost 0.5% with it (profiles/r05d_ab_gr_prefetch.txt)
    constexpr bool PF = GEOM == GEOM_FLAT;
    SlotRow Rnext = T.row[0];
#pragma unroll SUNROLL
    for (int s = 0; s < NSLOT; ++s) {
      const SlotRow R = PF ? Rnext : T.row[s];
      const double cf = R.cf, cA = R.cA;
      double cq[LDS_SLOTS];  // the row of LDS coefficients, loaded with R: one scalar wait per slot
#pragma unroll
      for (int q = 0; q < LDS_SLOTS; ++q) cq[q] = T.cL[s][q];
      double acc[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) acc[i] = cf * f[i];
      if (cA != 0.0) {  // wave-uniform: only Vern6's a32 and a98 rows use the register stage
#pragma unroll
        for (int i = 0; i < 7; ++i) acc[i] = fma(cf, f[i], cA * kA[i]);  // (the rounding of the general form)
      }
      // one block per LDS slot, guarded by the slot's wave-uniform bit of lmask (compile-time bounds:
      // no trip count, no remainder loop). A block's seven reads land in temporaries of their own, so
      // all are in flight before its first FMA and nothing but LDS reads is waited for. The order of
      // the sum, ascending q, is the results' (art_tail.h folds the same sums).
      const int lm = R.lmask;
#pragma unroll
      for (int q = 0; q < LDS_SLOTS; ++q) {
        if ((lm >> q) & 1) {
          double t[7];
#pragma unroll
          for (int i = 0; i < 7; ++i) t[i] = L[(q * 7 + i) * BLOCK];
#pragma unroll
          for (int i = 0; i < 7; ++i) acc[i] += cq[q] * t[i];
        }
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) y[i] = u[i] + hs * acc[i];
      const double ty = tau + R.ct * hs;
      if constexpr (PF) Rnext = T.row[s + 1 < NSLOT ? s + 1 : s];
      // Every lane evaluates the photon RHS -- idle lanes (a draining wave) on stale state,
      // whose results nothing reads -- so the slot has no divergent control flow. Axion
      // segments (the tree driver's batches) take a wave-uniform detour and a select.
      double aux[2];
      if constexpr (GEOM != GEOM_ANY) rhs_photon_gj(P, y, ty, erg, kk, aux);
      else rhs_photon(P, y, ty, erg, kk, aux);
      if (s == NSLOT - 1) {  // the end point's b and t for the scan certificate (lastv and codes are free)
        lastv[threadIdx.x] = aux[0];
        lastt[threadIdx.x] = aux[1];
      }
      if (__ballot(!photon) != 0ull) {
        double ka[7];
        rhs_axion(P, y, ty, erg, ka);
#pragma unroll
        for (int i = 0; i < 7; ++i) kk[i] = photon ? kk[i] : ka[i];
      }
      if (R.storeA) {
#pragma unroll
        for (int i = 0; i < 7; ++i) kA[i] = kk[i];
      }
      const int sl = R.storeL;
      if (sl >= 0) {
#pragma unroll
        for (int i = 0; i < 7; ++i) L[(sl * 7 + i) * BLOCK] = kk[i];
      }
    }
    ART_TMARK(1)  // step size and stage slots
    // The rest of the iteration -- error norm, controller, certificate, scan, walk, refill --
    // is latency-bound (short dependent chains, LDS round trips, the loads of a refill), the
    // stage slots issue-bound. At a higher issue priority than the partner wave's stage slots,
    // its instructions issue as soon as they are ready and the slots fill the gaps, instead of
    // the older wave's slots taking every issue cycle while this wave's chain waits behind
    // them (the arbiter goes by priority, then age). The priority drops back to the slots' level
    // at the top of the next iteration. 1e7 flat rays: 84.34 -> 82.53 ms (profiles/r04b_ab.txt,
    // 3 interleaved runs each); the grid pass at the slots' priority instead: 81.69 against
    // 81.42 (profiles/r04c_ab_grid_prio.txt). ART_NO_PRIO_PHASE switches it off (A/B).
    if (outlier) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(1);
    // y = u_{n+1}, kk = f(u_{n+1}) for stepping lanes
    // EEst² = mean of the 7 squared scaled errors: the controller needs EEst only through
    // EEst <= 1 and its logarithm (ln EEst = ½ ln EEst²), so no square root is taken
    double EEst2 = 0.0;
    if (mode == M_STEP || mode == M_ROOT) {
      if (photon && y[0] < P.rNS) y[0] = P.rNS;  // clamp on the FSAL stage (:531)
      if (!RK4) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          // explicit FMAs: the contraction of a sum of three products is the compiler's choice
          // (it prefers the product with fewer uses), so written out it could round differently
          // in the tail kernel's straight-line code (tests/test_gpu_tail_donation.py)
          double e = fma(T.e_k, kk[i], fma(T.e_A, kA[i], T.e_f * f[i]));
#pragma unroll
          for (int q = 1; q < LDS_SLOTS; ++q) e = fma(T.e_L[q], L[(q * 7 + i) * BLOCK], e);
          e *= hs;
          const double q = e * frcp(P.abstol + fmax_abs(u[i], y[i]) * P.reltol);
          acc += q * q;
        }
        EEst2 = acc * (1.0 / 7.0);
      }
    }

    // ---- controller (STEP lanes) ----
    int finish = -1;
    int scan = false;  // accepted step to be scanned for sign changes
    double dtnext = dt;
    if (mode == M_STEP) {
      s_att += 1;
      ++iter;
      bool finite = !isnan(EEst2) && !isinf(EEst2);
#pragma unroll
      for (int i = 0; i < 7; ++i) finite = finite && !isnan(y[i]) && !isinf(y[i]);
      if (!finite) {
        finish = ART_STATUS_NONFINITE;
      } else {
        // PI controller (OrdinaryDiffEq: beta1 = 7/60, beta2 = 1/15, gamma = 0.9, qmin = 0.2, qmax = 10)
        // EEst^(7/60) and max(EEst, 1e-4)^(1/15) are the 7th and 4th powers of y = EEst^(1/60)
        // = (EEst²)^(1/120): one logarithm and one exponential (OrdinaryDiffEq itself uses
        // FastPower.fastpower, an exp2/log2 approximation)
        double q = 1.0, q11 = 1.0, y60 = 0.0;
        bool accept = true;
        if (!RK4) {
          if (EEst2 == 0.0) {
            q = 0.1;
          } else {
            y60 = fexp(flog(EEst2) * (1.0 / 120.0));
            const double y2 = y60 * y60;
            q11 = (y2 * y2) * (y2 * y60);
            q = q11 * frcp(qpow);
            q = fmax(0.1, fmin(5.0, q * (1.0 / 0.9)));
          }
          accept = (EEst2 <= 1.0) || forced;
        }
        if (!accept) {
          dt = hs * frcp(fmin(5.0, q11 * (1.0 / 0.9)));
          ++n_rej;
          if (iter >= P.maxiters) finish = ART_STATUS_MAXITERS;
        } else {
          ++n_acc;
          s_acc += 1;
          if (!RK4) {
            const double ym = fmax(y60, 0.8576958985908941);  // (1e-4)^(1/60)
            qpow = (ym * ym) * (ym * ym);
            dtnext = hs * frcp(q);
          }
          scan = true;
        }
      }
    }

    // ---- resonance scan of the accepted steps (ContinuousCallback, RayTracer.jl:357-358) ----
    // (a) Wave-cooperative grid pass: every lane of the wave evaluates (source lane, grid
    //     point) items of all the wave's accepted steps, so lanes whose attempt was rejected
    //     (and the idle lanes of a draining wave) share the 49-point scans instead of waiting.
    //     Each item leaves a 2-bit sign code in the source lane's LDS words.
    const int nper = npts - 1;
    // (0) certified steps (scan_certified_code, art_core.h): every grid point of the step
    //     provably has a positive (1), negative (2) or undefined (3, NaN) condition, so its codes are
    //     known without evaluating them; its end value is not needed unless the next step
    //     opens a bracket at its start (then it is recomputed there, bit-identically:
    //     cprev_ok = false).
    // without callbacks (make_tree = false: ART_NO_CALLBACKS) every step is "certified NaN":
    // no sign change can open a bracket, so nothing is scanned or recorded
    const double bend = lastv[threadIdx.x];
    const int ccode =
        !scan ? 0 : (cbs ? scan_certified_code(P, u, f, y, kk, hs, bend, lastt[threadIdx.x], bstart) : 3);
    const int cert = ccode != 0;
    s_cert += cert ? 1u : 0u;
    // every lane parks (u, f, y, kk, h, τ) in its LDS slots (free after the error estimate):
    // the scan reads the interpolants from there, and the registers stay free until the
    // state is reloaded after the scan
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      L[(0 * 7 + i) * BLOCK] = u[i];
      L[(1 * 7 + i) * BLOCK] = f[i];
      L[(2 * 7 + i) * BLOCK] = y[i];
      L[(3 * 7 + i) * BLOCK] = kk[i];
    }
    L[(4 * 7 + 0) * BLOCK] = hs;
    L[(4 * 7 + 1) * BLOCK] = tau;
    const int grid = scan && !cert;
    const unsigned long long smask = __ballot(grid);
    // lanes polishing a crossing need the condition at the end of their re-step (th = 1 of the
    // parked step): those items ride in the same pass, after the grid items
    const unsigned long long rmask = __ballot(mode == M_ROOT);
    const int ns_g = __popcll(smask), crank = __popcll(smask & ((1ull << lane) - 1ull));
    // N and D of the items this lane evaluates in the first two passes (see (c0) below)
    double gN0 = 0.0, gD0 = 1.0, gN1 = 0.0, gD1 = 1.0;
    ART_TMARK(2)  // error norm, controller, certificate and parking
    if ((smask | rmask) != 0ull) {
      const int ns = __popcll(smask), nr = __popcll(rmask);
      if (grid) {
        srcl[wbase + __popcll(smask & ((1ull << lane) - 1ull))] = lane;
#pragma unroll
        for (int w = 0; w < SCAN_WORDS; ++w) codes[w * BLOCK + threadIdx.x] = 0u;
      }
      if (mode == M_ROOT) srcl[wbase + ns + __popcll(rmask & ((1ull << lane) - 1ull))] = lane;
      wave_lds_sync();
      // grid item w = (j - 1) ns + c: point-major, advanced by 64 items per pass; then the
      // root items
      const int tg = ns * nper, total = tg + nr;
      const int dj = ns ? 64 / ns : 0, dc = ns ? 64 % ns : 0;
      int c = ns ? lane % ns : 0, j = ns ? lane / ns + 1 : 0;
#pragma unroll 1
      for (int w0 = 0; w0 < total; w0 += 64) {
        const int t = w0 + lane;
        if (t < total) {  // one evaluation site for both kinds of item (no divergent second copy)
          const bool gi = t < tg;
          const int src = srcl[wbase + (gi ? c : ns + (t - tg))];
          double N, D;
          scan_nd_lds(P, lds + wbase + src, BLOCK, gi ? thgrid[j] : 1.0, N, D);
          if (w0 == 0) {
            gN0 = N;
            gD0 = D;
          } else if (w0 == 64) {
            gN1 = N;
            gD1 = D;
          }
          if (!gi || j == nper) {  // a root item's value; the end value opens the next step's brackets
            const double cv = 0.5 * N / D;  // = scan_point_lds, bit for bit
            lastv[wbase + src] = cv;
          }
          if (gi) {
            const unsigned code = (j == nper) ? sign_code(lastv[wbase + src]) : sign_code_nd(N, D);
            atomicOr(&codes[((j - 1) >> 4) * BLOCK + wbase + src], code << (2 * ((j - 1) & 15)));
            s_scan += 1;
          }
        }
        c += dc;
        j += dj;
        if (c >= ns) {
          c -= ns;
          j += 1;
        }
      }
      wave_lds_sync();
    }

    ART_TMARK(3)  // grid pass
    // (b) Per lane: walk the sign codes exactly as the sequential scan would (NaN resets the
    //     sign memory; a sign change opens an Illinois search on the interpolant, ignored
    //     right after an event -- DiffEq repeat_nudge), plus the single evaluations of fresh
    //     lanes (initial sign) and of lanes polishing a crossing. Condition evaluations
    //     here only happen at brackets, Illinois points and root polish steps.
    //     ph: 0 done, 1 single point (INIT / ROOT), 2 walk codes, 3 Illinois, 5 value at the
    //     change point, 6 value at the bracket start, 7 value at the step's last nonzero point.
    int ph = scan ? 2 : 0;  // (polishing lanes: their value came with the grid pass, below)
    int ip = 1, last_j = 0;
    int last_s = sprev;
    double last_c = cprev;
    int lc_ok = cprev_ok;  // last_c is the value at grid point last_j (0: the step start)
    unsigned cw[SCAN_WORDS] = {0u, 0u, 0u, 0u};
    if (ph == 2) {
#pragma unroll
      for (int w = 0; w < SCAN_WORDS; ++w)
        cw[w] = cert ? 0x55555555u * (unsigned)ccode : codes[w * BLOCK + threadIdx.x];
      // fast path: every grid point has the previous sign (or the previous sign is unknown
      // and every point has one common nonzero sign)
      // (FASTN: nper through an empty asm, so the masks below are rebuilt from this one scalar here and not
      // hoisted out of the main loop, spilled and restored, two to four lane reads a block)
      int nper_f = nper;
      if constexpr (FASTN) asm volatile("" : "+s"(nper_f));
      const unsigned s0 = cw[0] & 3u;
      if (s0 == 1u || s0 == 2u) {
        bool same = (last_s == 0) || (last_s == (s0 == 1u ? 1 : -1));
#pragma unroll
        for (int w = 0; w < SCAN_WORDS; ++w) {
          const int nw = nper_f - 16 * w;
          if (nw <= 0) break;
          const unsigned m = nw >= 16 ? 0xffffffffu : ((1u << (2 * nw)) - 1u);
          same = same && ((cw[w] & m) == ((s0 * 0x55555555u) & m));
        }
        if (same) {
          last_s = (s0 == 1u) ? 1 : -1;
          last_j = nper;
          if (!cert) last_c = lastv[threadIdx.x];
          lc_ok = !cert;
          ph = 0;
        }
      } else if (s0 == 3u) {  // every point NaN: no resonance possible, the sign memory resets
        bool all = true;
#pragma unroll
        for (int w = 0; w < SCAN_WORDS; ++w) {
          const int nw = nper_f - 16 * w;
          if (nw <= 0) break;
          const unsigned m = nw >= 16 ? 0xffffffffu : ((1u << (2 * nw)) - 1u);
          all = all && ((cw[w] & m) == m);
        }
        if (all) {  // with no sign remembered, the bracket-start value is never read
          last_s = 0;
          lc_ok = false;
          ph = 0;
        }
      }
    }
    double i_tha = 0.0, i_ca = 0.0, i_thb = 0.0, i_cb = 0.0, i_tr = 0.0, i_cg = 0.0;
    int i_side = 0, i_it = 0;
    int hit = false, root_done = false;
    // a crossing in (θ_last, θ_ip]: polish it on the true trajectory (mode ROOT), from t_int
    auto open_root = [&](double t_int) {
      const double thg = thgrid[ip];
      const double last_th = thgrid[last_j];
      hit = true;
      hroot = hs;
      r_tha = last_th; r_ca = last_c; r_thb = thg; r_cb = i_cg;
      r_slope = (i_cg - last_c) / (thg - last_th);
      r_t = (t_int > last_th && t_int < thg) ? t_int : 0.5 * (last_th + thg);
      r_side = 0;
      r_it = 0;
      post_c = i_cg;
      post_s = sgn(i_cg);
      dt = dtnext;
    };
    // the values at the change point (i_cg) and at the bracket start (last_c) are known
    auto open_bracket = [&]() {
      lc_ok = true;
      i_tha = thgrid[last_j];
      i_ca = last_c;
      i_thb = thgrid[ip];
      i_cb = i_cg;
      i_tr = i_tha - i_ca * (i_thb - i_tha) / (i_cb - i_ca);
      i_side = 0;
      i_it = 0;
      // The interpolant's root only seeds the polish on the true trajectory -- except right
      // after an event, where DiffEq's repeat_nudge asks whether it lies below θ = 0.01. Only
      // then is it refined by Illinois on the interpolant (ph 3); otherwise Vern6 starts the
      // polish from the secant point, which saves the ~6.6 lone-lane Illinois iterations a
      // bracket would cost the whole wave. (The fixed-step RK4 path keeps the Illinois seed:
      // with its tiny steps the oracle's own 1-ulp sensitivity is ~1e-12, and a different seed
      // moves grazing crossings by more.)
      if (RK4 || (just_evented && i_tha < 0.01)) {
        ph = 3;
      } else {
        open_root(i_tr);
        ph = 0;
      }
    };
    // walk the codes from grid point ip (no evaluations): ph 5 at a sign change, 7 when the
    // value at the last nonzero point is still needed, else 0
    auto walk = [&]() {
      WalkState ws{ip, last_s, last_j, lc_ok != 0};
      bool found = false;
      if (!walk_codes_bits(cw, nper, ws, found)) walk_codes_loop(cw, nper, ws, found);
      ip = ws.ip;
      last_s = ws.last_s;
      last_j = ws.last_j;
      lc_ok = ws.lc_ok;
      if (found) {
        ph = 5;
      } else if (!lc_ok && last_j == nper) {
        if (!cert) {  // a certified step leaves it to the next step's start (th = 0)
          last_c = lastv[threadIdx.x];
          lc_ok = true;
        }
        ph = 0;
      } else if (!lc_ok && last_s != 0) {
        ph = 7;
      } else {  // (with no sign remembered the bracket-start value is never read)
        ph = 0;
      }
    };
    // bracketed polish on the true trajectory (Newton with the interpolant slope, then Illinois)
    auto polish = [&](double ci) {
      ++r_it;
      bool done = !(fabs(ci) > 1e-12);
      if (!done) {
        if (sgn(ci) == sgn(r_ca)) { r_tha = r_t; r_ca = ci; if (r_side == -1) r_cb *= 0.5; r_side = -1; }
        else { r_thb = r_t; r_cb = ci; if (r_side == 1) r_ca *= 0.5; r_side = 1; }
        done = (r_thb - r_tha) * hroot < 1e-13 || r_it >= 9;
        if (!done) {
          double tn = (r_it == 1) ? r_t - ci / r_slope : r_tha - r_ca * (r_thb - r_tha) / (r_cb - r_ca);
          if (!(tn > r_tha && tn < r_thb)) tn = 0.5 * (r_tha + r_thb);
          r_t = tn;
        }
      }
      root_done = done;
      ph = 0;
    };
    if (mode == M_ROOT) {  // the re-stepped end's value, from the grid pass
      s_root += 1;
      polish(lastv[threadIdx.x]);
    }
    ART_TMARK(4)  // sign-code fast paths
    if (ph == 2) walk();
    ART_TMARK(5)  // code walk
    // (c0) The values a bracket (ph 5: at the change point and, when unknown, at the last
    //      nonzero point before it) or the next step's bracket start (ph 7) needs are grid
    //      points of this step: item (j - 1) ns + c of the grid pass (c: this lane's rank among
    //      the sources), evaluated by lane w & 63 in pass w >> 6, whose N and D from the first
    //      two passes are still in that lane's registers. ½ N / D there is scan_point_lds's
    //      value bit for bit, so no second evaluation is needed. (The step's start point,
    //      last_j = 0, and later passes go to the cooperative pass.)
    {
      const bool want = grid && (ph == 5 || ph == 7);
      const int ja = (ph == 5) ? ip : last_j;
      const int wa = (want && ja >= 1) ? (ja - 1) * ns_g + crank : (want ? 1 << 20 : 0);
      const bool needb = want && ph == 5 && !lc_ok;
      const int wb = needb ? (last_j >= 1 ? (last_j - 1) * ns_g + crank : 1 << 20) : 0;
      if (__ballot(want) != 0ull) {
        const int la = wa & 63, lb = wb & 63;
        const double nA0 = __shfl(gN0, la), dA0 = __shfl(gD0, la), nA1 = __shfl(gN1, la), dA1 = __shfl(gD1, la);
        const double nB0 = __shfl(gN0, lb), dB0 = __shfl(gD0, lb), nB1 = __shfl(gN1, lb), dB1 = __shfl(gD1, lb);
        if (want && wa < 128 && wb < 128) {
          const double va = 0.5 * ((wa >> 6) ? nA1 : nA0) / ((wa >> 6) ? dA1 : dA0);
          if (ph == 7) {
            last_c = va;
            lc_ok = true;
            ph = 0;
          } else {
            i_cg = va;
            if (needb) last_c = 0.5 * ((wb >> 6) ? nB1 : nB0) / ((wb >> 6) ? dB1 : dB0);
            open_bracket();
          }
        }
      }
    }
    // (c) One cooperative pass evaluates the pending condition values of the whole wave at
    //     once: the re-stepped end of polishing lanes (ph 1, th = 1 of their parked step), the
    //     change point of a bracket (ph 5) and its start when unknown, and the step's last
    //     nonzero grid point (ph 7). Requests (source lane, th) go to LDS and any lane
    //     evaluates any request, so a lane with two values needs one pass, not two.
    {
      const int nq = (ph == 1 || ph == 7) ? 1 : (ph == 5 ? (lc_ok ? 1 : 2) : 0);
      const unsigned long long lt = (1ull << lane) - 1ull;
      const unsigned long long b1 = __ballot(nq >= 1), b2 = __ballot(nq == 2);
      const int total = __popcll(b1) + __popcll(b2);
      if (total > 0 && total <= 64) {
        const int off = __popcll(b1 & lt) + __popcll(b2 & lt);
        wave_lds_sync();  // the walk's lastv reads are done
        if (nq >= 1) {
          srcl[wbase + off] = lane;
          lastv[wbase + off] = (ph == 1) ? 1.0 : (ph == 7 ? thgrid[last_j] : thgrid[ip]);
        }
        if (nq == 2) {
          srcl[wbase + off + 1] = lane;
          lastv[wbase + off + 1] = thgrid[last_j];
        }
        wave_lds_sync();
        if (lane < total) {
          const int src = srcl[wbase + lane];
          lastt[wbase + lane] = scan_point_lds(P, lds + wbase + src, BLOCK, lastv[wbase + lane]);
        }
        wave_lds_sync();
        if (nq >= 1) {
          const double r1 = lastt[wbase + off];
          if (ph == 1) {
            s_root += 1;
            polish(r1);
          } else if (ph == 7) {  // value at the step's last nonzero grid point (next step's bracket start)
            s_interp += 1;
            last_c = r1;
            lc_ok = true;
            ph = 0;
          } else {  // ph 5
            s_interp += (unsigned)nq;
            i_cg = r1;
            if (nq == 2) last_c = lastt[wbase + off + 1];
            open_bracket();
          }
        }
      }
    }
    ART_TMARK(6)  // cooperative pass
    // (d) Per lane, for the rare rest: more than 64 pending values, Illinois on the interpolant
    //     (repeat_nudge), and walking on after an ignored crossing.
    //     ph: 0 done, 1 re-stepped end (ROOT), 2 walk codes, 3 Illinois, 5 value at the change
    //     point, 6 value at the bracket start, 7 value at the step's last nonzero point.
#pragma unroll 1
    while (ph != 0) {
      if (ph == 2) {
        walk();
        if (ph == 0) break;
      }
      double th = 1.0;  // ph 1: the re-stepped end y at τ + h is the parked step's th = 1
      if (ph == 3) th = i_tr;
      else if (ph == 5) th = thgrid[ip];
      else if (ph == 6 || ph == 7) th = thgrid[last_j];
      const double ci = scan_point_lds(P, L, BLOCK, th);
      if (ph == 1) {
        s_root += 1;
        polish(ci);
        continue;
      }
      s_interp += 1;
      if (ph == 7) {
        last_c = ci;
        lc_ok = true;
        ph = 0;
      } else if (ph == 5 || ph == 6) {
        if (ph == 5) i_cg = ci;
        else last_c = ci;
        if (ph == 5 && !lc_ok) ph = 6;
        else open_bracket();
      } else {  // ph == 3: Illinois on the interpolant inside (i_tha, i_thb]
        bool stop = ci == 0.0 || isnan(ci) || (i_thb - i_tha) < 1e-12;
        bool below = false;
        if (!stop) {
          if (sgn(ci) == sgn(i_ca)) { i_tha = i_tr; i_ca = ci; if (i_side == -1) i_cb *= 0.5; i_side = -1; }
          else { i_thb = i_tr; i_cb = ci; if (i_side == 1) i_ca *= 0.5; i_side = 1; }
          // Every later iterate stays in [i_tha, i_thb]: once that lies below θ = 0.01 right
          // after an event, the root is ignored (repeat_nudge) wherever Illinois would end,
          // so the search stops here with the same outcome
          below = just_evented && i_thb < 0.01;
          if (below) {
            stop = true;
          } else {
            const double tn = i_tha - i_ca * (i_thb - i_tha) / (i_cb - i_ca);
            if (tn == i_tr) stop = true;
            else i_tr = tn;
            if (++i_it >= 40) stop = true;
          }
        }
        if (stop) {
          const double t_int = i_tr;
          if (!below && !(just_evented && t_int < 0.01)) {  // DiffEq repeat_nudge after an event
            open_root(t_int);
            ph = 0;
          } else {  // ignored: continue the walk after the change point
            last_s = sgn(i_cg);
            last_c = i_cg;
            last_j = ip;
            lc_ok = true;
            ++ip;
            ph = 2;
          }
        }
      }
    }
    ART_TMARK(7)  // per-lane fallback loop
    if constexpr (SAVE) {
      // saveat (RayTracer.jl:176, 383): the interior save times ln t0 + kΔ that this completed
      // step passed -- an accepted step without a crossing, or the polish step that ends at a
      // root -- from the step's parked interpolant. finalize_kernel adds the start and the end.
      if (((scan && !hit) || root_done) && save_k < out.ntimes - 1) {
        const double t0 = in.lnt0[ray];
        const double D = (tend - t0) / double(out.ntimes - 1);
        const double tb = (last && !root_done) ? tend : tau + hs;
        while (save_k < out.ntimes - 1) {
          const double ts = t0 + double(save_k) * D;
          if (!(ts <= tb)) break;
          const double th = (ts - tau) / hs;
#pragma unroll
          for (int c = 0; c < 3; ++c)
            out.traj[(int64_t(c) * out.ntimes + save_k) * n + ray] =
                hermite1(L[(0 * 7 + c) * BLOCK], L[(1 * 7 + c) * BLOCK], L[(2 * 7 + c) * BLOCK],
                         L[(3 * 7 + c) * BLOCK], hs, th);
          out.traj_t[int64_t(save_k) * n + ray] = ts;
          ++save_k;
        }
      }
    }
    // reload the state each lane continues from: the step's end (y, kk: slots 2-3) after an
    // accepted step or a finished polish, else its start (u, f: slots 0-1)
    {
      const double* Ls = L + ((root_done || (scan && !hit)) ? 2 * 7 * BLOCK : 0);
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        u[i] = Ls[i * BLOCK];
        f[i] = Ls[(7 + i) * BLOCK];
      }
    }
    if (hit) mode = M_ROOT;
    if (root_done || (scan && !hit)) bstart = bend;
    if (root_done) {
      const double tau_r = tau + hs;
      const PropArgs* const A = cold_args_if<COLD>();  // (cold: a crossing is recorded)
      const int a = affect(P, COLD ? A->in : in_k, COLD ? A->out : out_k, COLD ? A->n : n, ray, u, tau_r, erg, ncross,
                           COLD ? A->max_crossings : max_crossings);
      tau = tau_r;
      cprev = post_c;  // the post-event side (DiffEq repeat_nudge): the root is not re-found
      cprev_ok = true;
      sprev = post_s;
      just_evented = true;
      mode = M_STEP;
      if (a == 2) finish = ART_STATUS_CROSSING;
      else if (photon && u[0] < P.rNS101) finish = ART_STATUS_HIT_NS;  // cb_r after the event
      else if (iter >= P.maxiters) finish = ART_STATUS_MAXITERS;
    }
    if (scan && !hit) {
      tau = last ? tend : tau + hs;
      cprev = last_c;
      cprev_ok = lc_ok;
      sprev = last_s;
      just_evented = false;
      dt = dtnext;
      if (cbs && photon && u[0] < P.rNS101) finish = ART_STATUS_HIT_NS;  // cb_r (:352-368)
      else if (last) finish = ART_STATUS_SUCCESS;
      else if (iter >= P.maxiters) finish = ART_STATUS_MAXITERS;
    }

    if constexpr (CYC) {
      // Cyclotron resonance (cyclotron_g, art_core.h): after every completed step of a photon --
      // saveat's condition -- the sign of g at the state the next step starts from against g at this
      // step's start. A passive observation: it reads the step's parked interpolant and writes only
      // the ray's own cyc_* slots; no step, step size, event or other output depends on it.
      if (((scan && !hit) || root_done) && photon) {
        const double g1 = cyclotron_g(P, u, tau, erg);
        if ((gprev < 0.0 && g1 >= 0.0) || (gprev >= 0.0 && g1 < 0.0)) cyclotron_crossing(P, L, erg, gprev, g1, out, n, ray);
        gprev = g1;
      }
    }
    int fin_piece = -1;  // (DON = 3) the piece of a ray finishing now
    if (finish >= 0) {  // the raw end record; finalize_kernel back-transforms it (RayTracer.jl:393-416)
      const PropArgs* const A = cold_args_if<COLD>();  // (cold: a ray's end record)
      const SegOut& out = COLD ? A->out : out_k;
      if constexpr (DON == 3) fin_piece = piece_of(out.pieces, ray);
      double2* rq = reinterpret_cast<double2*>(out.rec + (int64_t)ray * END_REC);
      rq[0] = make_double2(u[0], u[1]);
      rq[1] = make_double2(u[2], u[3]);
      rq[2] = make_double2(u[4], u[5]);
      rq[3] = make_double2(u[6], tau);
      int4* ri = reinterpret_cast<int4*>(rq + 4);
      ri[0] = make_int4(finish, n_acc, n_rej, ncross);
      if constexpr (SAVE) ri[1] = make_int4(save_k + 1, 0, 0, 0);  // start + interior + end
      ray = -1;
      mode = M_IDLE;
    }
    if constexpr (DON == 3) {
      // the streamed host pipelines: each finishing lane counts its ray into its wave's LDS
      // histogram over the pieces; every STREAM_FLUSH + 1 iterations (and once the queue is
      // drained) the wave releases its stores and adds the histogram to the pieces' global
      // counts, one lane per piece (stream_flush). Kept out of registers: a per-wave pending
      // count held across the loop cost the integrator 7.5% in spills
      // (profiles/r04s2_streamed_kernel_ab.jsonl)
      if (fin_piece >= 0) atomicAdd(&pend_lds[threadIdx.x >> 6][fin_piece], 1u);
      ++tick;
      if ((tick & STREAM_FLUSH) == 0 || (exhausted && (tick & DRAIN_FLUSH_MASK) == 0))
        stream_flush(COLD ? cold_args_if<COLD>()->out : out_k, pend_lds[threadIdx.x >> 6], lane);
    }
    ART_TMARK(0)  // saveat, reload, events, finish and the output stores (+ refill)
    // graduation (SegOut::graduate): a ray past `graduate` attempts, at a step boundary, leaves
    // for the tail kernel now instead of running on as one lane of this wave until the wave
    // drains; its lane takes the next ray. The record is the donation record, so the ray's
    // arithmetic does not change.
    // early graduation (SegOut::hot): a ray whose progress in ln t lags the hot rule at a
    // power-of-two attempt count, or when its drained wave donates it, leaves for the hot
    // records, which a tail_kernel launch beside this one resumes at once (one wave per ray)
    auto to_hot = [&](bool h) {
      const unsigned long long hm = __ballot(h);
      if (hm == 0ull) return;
      const int leader = __ffsll((long long)hm) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(out.hot_count, (unsigned long long)__popcll(hm));
      base = __shfl(base, leader);
      const int64_t slot = (int64_t)base + __popcll(hm & ((1ull << lane) - 1ull));
      if (h && slot < (int64_t)out.hot_cap) {  // (no slot left: the ray stays)
        write_cont_rec(out.hot + slot * CONT_REC, u, f, tau, dt, qpow, cprev, bstart, erg, ray, n_acc, n_rej, ncross,
                       iter, sprev, photon, cprev_ok, just_evented, save_k);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_store(out.hot_ready + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ray = -1;
        mode = M_IDLE;
      }
    };
    if (DON == 1 && out.hot_at > 0) {
      bool h = mode == M_STEP && iter >= out.hot_at && (iter & (iter - 1)) == 0;
      if (__ballot(h) != 0ull) {
        if (h) h = hot_lags(out, tau - in.lnt0[ray], (double)(__builtin_ctz((unsigned)iter) - 8));
        to_hot(h);
      }
    }
    // graduation (SegOut::graduate): a ray past `graduate` attempts, at a step boundary, leaves
    // for the tail kernel now instead of running on as one lane of this wave until the wave
    // drains; its lane takes the next ray. The record is the donation record, so the ray's
    // arithmetic does not change.
    if (DON == 1 && out.graduate > 0) {
      const bool g = mode == M_STEP && iter >= out.graduate;
      const unsigned long long gm = __ballot(g);
      if (gm != 0ull) {
        const int leader = __ffsll((long long)gm) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(out.grad_count, (unsigned long long)__popcll(gm));
        base = __shfl(base, leader);
        const int64_t slot = (int64_t)base + __popcll(gm & ((1ull << lane) - 1ull));
        if (g && slot < (int64_t)out.grad_cap) {  // (no slot left: the ray stays)
          write_cont_rec(out.grad + slot * CONT_REC, u, f, tau, dt, qpow, cprev, bstart, erg, ray, n_acc, n_rej,
                         ncross, iter, sprev, photon, cprev_ok, just_evented, save_k);
          ray = -1;
          mode = M_IDLE;
        }
      }
    }
    // tail donation (SegOut::donate): the drained wave's last few rays, all at a step
    // boundary, leave for the continuation launch and the wave retires
    if (DON == 1 && exhausted && out.donate > 0) {
      unsigned long long live = __ballot(mode != M_IDLE);
      if (live != 0ull && __popcll(live) <= out.donate && __ballot(mode == M_ROOT) == 0ull) {
        if (out.hot_at > 0) {  // (the lagging ones to the hot records instead)
          bool h = mode == M_STEP && iter >= out.hot_at;
          if (__ballot(h) != 0ull) {
            if (h) h = hot_lags(out, tau - in.lnt0[ray], log2((double)iter) - 8.0);
            to_hot(h);
            live = __ballot(mode != M_IDLE);
          }
        }
        if (live != 0ull) {
          const int leader = __ffsll((long long)live) - 1;
          unsigned long long base = 0;
          if (lane == leader) base = atomicAdd(out.cont_count, (unsigned long long)__popcll(live));
          base = __shfl(base, leader);
          if (mode != M_IDLE) {
            const int64_t slot = (int64_t)base + __popcll(live & ((1ull << lane) - 1ull));
            write_cont_rec(out.cont + slot * CONT_REC, u, f, tau, dt, qpow, cprev, bstart, erg, ray, n_acc, n_rej,
                           ncross, iter, sprev, photon, cprev_ok, just_evented, save_k);
            ray = -1;
            mode = M_IDLE;
          }
        }
      }
    }
  }

  // wave-reduce the statistics and add them once per wave (DON = 3: before the wave counts itself
  // done and flushes its last piece counts, so the helper that ends the call finds them complete)
  const PropArgs* const Ae = cold_args_if<COLD>();  // (COLD: nothing of this is held across the loop)
  unsigned long long* const stats_e = COLD ? Ae->stats : stats;
#if defined(ART_SECTION_TIMING)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) atomicAdd(&stats_e[k], t_sec[k]);
  }
#else
  const unsigned v[7] = {s_att, s_acc, s_root, s_scan, s_interp, s_rays, s_cert};
  const int slot[7] = {ST_ATTEMPTS, ST_ACCEPTED, ST_ROOT_STEPS, ST_SCAN_EVALS, ST_INTERP_EVALS, ST_RAYS, ST_CERT};
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    unsigned long long x = v[k];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if (lane == 0 && x) atomicAdd(&stats_e[slot[k]], x);
  }
#endif
  span_stamp(stats_e, true);
  if constexpr (DON == 3) {
    const SegOut& out = COLD ? Ae->out : out_k;
    if (out.waves_done) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      if (lane == 0) __hip_atomic_fetch_add(out.waves_done, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    stream_flush(out, pend_lds[threadIdx.x >> 6], lane);
  }
}

}  // namespace art
