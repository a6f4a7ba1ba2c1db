// art_helper.h -- helper_kernel: every initialisation and finalization, and the streamed pipeline's
// helper duty.
#pragma once
#include "art_ray_io.h"

namespace art {

// Every initialisation and finalization of the library runs in helper_kernel, through ONE call
// site of init_one and ONE of finalize_one: their arithmetic (the right-hand side's "fast"
// contraction included) is then the same machine code for every path -- the single launch, the
// chunked and CU-masked pipelines and the maskless streamed one -- so their outputs agree bit
// for bit (tests/test_edges.py). (Inlined into two kernels, the photon RHS of init_one had
// contracted differently: profiles/r04m_pytest.log.)
//   HK_INIT  rays [i0, i1): fresh state into in.u0 (grid-stride over 256-ray tiles);
//   HK_FIN   rays [i0, i1): the end state into `out` at o = i - i0, row stride i1 - i0;
//   HK_TILES the maskless streamed pipeline's helper duty (SegOut::host_ready ...): claim
//            1024-ray tiles (S3_TILE) to initialise once the host's copies of their inputs have landed,
//            and tiles of each finished piece to finalize into its blob; flag each initialised
//            chunk (chunk_ready, which the integrator's waves poll) and each finalized piece
//            (host_flags, which the host polls). init_limit >= 0: initialise only, until every
//            tile below it is claimed (the pass that starts the launch); -1: serve until every
//            tile is initialised and finalized. announce: count this block into *host_started
//            (the host launches the integrator once every persistent helper block is resident).
//            Each hand-off: the block's stores, s_waitcnt, barrier, one agent-scope release,
//            then the flag (MI355X_MICROARCH.md, inter-workgroup visibility); readers poll the
//            flag and take one agent-scope acquire.
enum { HK_INIT = 0, HK_FIN = 1, HK_TILES = 2 };
// Instantiated per geometry like the integrator (the same folded physics), for 2 waves per SIMD:
// a helper wave then shares a SIMD with one integrator wave, so the streamed pipeline's persistent
// helpers take one integrator block slot each instead of a whole CU. The builds need 158-203
// VGPRs and no scratch (-disable-machine-licm, build.py); helper_waves_per_simd checks that at
// run time, because a scratch-spilling persistent helper stalled the next launch on another
// queue for seconds (the runtime growing that queue's scratch while the helpers held theirs).
template <int GEOM>
__global__ __launch_bounds__(256, 2) void helper_kernel(
    const KParams P_in, const int64_t n, const SegIn in, const SegOut out, const int mode, const int64_t i0,
    const int64_t i1, const int64_t init_limit, const int announce, unsigned long long* __restrict__ stats) {
  const KParams P = specialize<GEOM>(P_in);
  __shared__ long long cmd[2];  // HK_TILES: [what, tile]: 0 nothing now, 1 initialise, 2 finalize, 3 done
  __shared__ double hfl[2 * FLUX_HELPER_BINS];  // (HK_TILES with SegOut::flux_hist) this block's flux counts
  __shared__ int last_out, complete;
  const int tid = threadIdx.x;
  // the persistent helpers share their SIMDs with integrator waves (2 waves per SIMD): their claims,
  // hand-offs and tiles run at the top issue priority, so the initialisation keeps ahead of the
  // integrator's chunk claims (at the integrator's priorities the idle polls starved and the calls
  // gave up); between polls they sleep
  if (mode == HK_TILES) __builtin_amdgcn_s_setprio(3);
  const bool flb = mode == HK_TILES && out.flux_hist != nullptr;
  if (flb)
    for (int b = tid; b < 2 * out.flux_nbins; b += 256) hfl[b] = 0.0;
  __syncthreads();
  const int64_t TS = mode == HK_TILES ? S3_TILE : 256;  // rays per tile
  int64_t tile = blockIdx.x;
  unsigned long long hr = 0;  // (HK_TILES, thread 0) host_ready as last read: it only grows
  long long pend = -1;  // (HK_TILES, thread 0) a claimed finalize tile whose piece is still running
  unsigned long long t_idle = __builtin_amdgcn_s_memrealtime();
  unsigned npoll = 0;  // (HK_TILES, thread 0) claim rounds: every 16th reads the abort word
  unsigned nrhs = 0;
  if (mode == HK_TILES && announce && tid == 0)
    __hip_atomic_fetch_add(out.host_flags + 64, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  while (true) {
    long long what = 0, t = -1;
    if (mode != HK_TILES) {
      t = (long long)(i0 + tile * TS);
      if (t >= i1) break;
      what = mode == HK_INIT ? 1 : 2;
      tile += gridDim.x;
    } else {
      if (tid == 0) {
        // a given-up call (the host's or a wave's abort word) ends here: every 16th claim round
        // reads the word (a host-memory load, ~2 us), every wait below reads it each time
        if ((++npoll & 15u) == 0u && ld_abort(out)) what = 3;
        const unsigned long long inext = ld_agent(out.init_next);
        if (what == 0 && init_limit >= 0 && (int64_t)inext >= init_limit) what = 3;
        if (what == 0 && (int64_t)inext < n && inext >= hr) hr = ld_sys(out.host_ready);
        if (what == 0 && (int64_t)inext < n && inext < hr) {
          if (init_limit >= 0) {
            // the pass that starts the launch claims tiles below init_limit only (compare-and-
            // swap: with a blind add, every block that saw init_next below the limit claimed a
            // tile, far past the landed inputs, and the integrator behind this pass waited for them)
            unsigned long long cur = inext;
            while ((int64_t)cur < init_limit && (int64_t)cur < n) {
              const unsigned long long seen = atomicCAS(out.init_next, cur, cur + (unsigned long long)S3_TILE);
              if (seen == cur) {
                what = 1;
                t = (long long)cur;
                break;
              }
              cur = seen;
            }
            if (what == 0) what = 3;
          } else {
            const unsigned long long c = atomicAdd(out.init_next, (unsigned long long)S3_TILE);
            if ((int64_t)c < n) {  // (a tile past the landed inputs waits for them below)
              what = 1;
              t = (long long)c;
            }
          }
        }
        if (what == 0 && init_limit < 0) {
          if (pend < 0) {
            const unsigned long long fnext = ld_agent(out.fin_next);
            if ((int64_t)fnext < n) {
              const int p = piece_of(out.pieces, (int64_t)fnext);
              if ((int64_t)ld_agent(out.piece_cnt + p) == piece_rays(out.pieces, p)) {
                const unsigned long long c = atomicAdd(out.fin_next, (unsigned long long)S3_TILE);
                if ((int64_t)c < n) pend = (long long)c;
              }
            }
          }
          if (pend >= 0) {
            const int p = piece_of(out.pieces, (int64_t)pend);
            if ((int64_t)ld_agent(out.piece_cnt + p) == piece_rays(out.pieces, p)) {
              what = 2;
              t = pend;
              pend = -1;
            }
          }
          if (what == 0 && pend < 0 && (int64_t)inext >= n && (int64_t)ld_agent(out.fin_next) >= n) what = 3;
        }
        if (what == 1) {  // the tile's inputs (bounded wait)
          const int64_t t1 = (int64_t)t + S3_TILE < n ? (int64_t)t + S3_TILE : n;
          const unsigned long long w0 = __builtin_amdgcn_s_memrealtime();
          while ((int64_t)ld_sys(out.host_ready) < t1) {
            if (__hip_atomic_load(out.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u ||
                __builtin_amdgcn_s_memrealtime() - w0 > S3_WAIT_TICKS) {
              __hip_atomic_store(out.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              what = 3;
              break;
            }
            __builtin_amdgcn_s_sleep(32);
          }
        }
        if (what == 0 && (__hip_atomic_load(out.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u ||
                          __builtin_amdgcn_s_memrealtime() - t_idle > S3_WAIT_TICKS)) {
          __hip_atomic_store(out.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          what = 3;
        }
        // aborted: drain the integrator's work queue, so each of its waves stops at its next
        // chunk claim instead of integrating every chunk the helpers had flagged
        if (what == 3 && out.queue_word && ld_abort(out)) atomicAdd(out.queue_word, 1ull << 40);
        if (what == 1 || what == 2) {
          t_idle = __builtin_amdgcn_s_memrealtime();
          // the inputs the DMA engines wrote / the end records other CUs wrote
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        cmd[0] = what;
        cmd[1] = t;
      }
      __syncthreads();
      // (block-uniform: said so, so the tile's SegOut and bounds stay in scalar registers --
      // read as per-lane values they took ~100 VGPRs across the tile loop)
      what = (long long)__builtin_amdgcn_readfirstlane((int)cmd[0]);
      {
        const unsigned long long tw = (unsigned long long)cmd[1];
        t = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(tw >> 32)) << 32) |
                        (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)tw));
      }
      __syncthreads();
      if (what == 3) break;
      if (what == 0) {
        __builtin_amdgcn_s_sleep(16);
        continue;
      }
    }
    const int64_t t1 = t + TS < (mode == HK_TILES ? n : i1) ? t + TS : (mode == HK_TILES ? n : i1);
    if (what == 1) {  // (one call site of each)
#pragma unroll 1
      for (int64_t i = t + tid; i < t1; i += 256) nrhs += init_one(P, n, i, in);
    } else {
      SegOut ol = out;
      int64_t ob = i0, m = i1 - i0;
      if (mode == HK_TILES) {
        const int p = piece_of(out.pieces, (int64_t)t);
        ol = piece_blob(out, n, p, m);
        ob = piece_lo(out.pieces, p);
      }
#pragma unroll 1
      for (int64_t i = t + tid; i < t1; i += 256) finalize_one(P, n, i, i - ob, m, in, ol, flb ? hfl : nullptr, out.flux_nbins);
    }
    if (mode == HK_TILES) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        if (what == 2 && out.blob_host) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // (the blob in host memory)
        else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (what == 1) {
          for (int64_t c = t / CHUNK; c * CHUNK < t1; ++c)
            __hip_atomic_store(out.chunk_ready + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          const int p = piece_of(out.pieces, (int64_t)t);
          const unsigned long long tiles = (unsigned long long)((piece_rays(out.pieces, p) + S3_TILE - 1) / S3_TILE);
          const unsigned long long old =
              __hip_atomic_fetch_add(out.piece_fin + p, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (old + 1ull == tiles) {  // the piece's last tile: its blob is complete in memory
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(out.host_flags + p, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
          }
        }
      }
    }
  }
  unsigned long long x = nrhs;  // init RHS evaluations -> stats[6]
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  if ((tid & 63) == 0 && x) atomicAdd(&stats[6], x);
  if (mode == HK_TILES && init_limit < 0 && out.exit_count) {
    // the end of the call (SegOut::done_host): this block's flux counts into the call's histogram
    // (sums of 1.0: exact in any order), then the last serving block out copies the statistics
    // and the flux into host memory and raises the flag the host waits for
    __syncthreads();
    if (flb)
      for (int b = tid; b < 2 * out.flux_nbins; b += 256)
        if (hfl[b] != 0.0) atomicAdd(out.flux_hist + b, hfl[b]);
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned long long old = __hip_atomic_fetch_add(out.exit_count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_out = (old + 1ull == (unsigned long long)out.exit_expected) ? 1 : 0;
    }
    __syncthreads();
    if (last_out) {
      if (tid == 0) {  // the integrator's started waves have added their statistics (they count themselves after)
        const unsigned long long w0 = __builtin_amdgcn_s_memrealtime();
        bool ok = true;
        const unsigned long long started = ld_agent(out.waves_started);
        while (ld_agent(out.waves_done) < started) {
          if (ld_abort(out) || __builtin_amdgcn_s_memrealtime() - w0 > STREAM_WAIT_TICKS) { ok = false; break; }
          __builtin_amdgcn_s_sleep(8);
        }
        complete = ok ? 1 : 2;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      __syncthreads();
      for (int k = tid; k < N_STATS_DEV; k += 256)
        __hip_atomic_store(out.done_host + DONE_STATS + k, ld_agent(stats + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (out.flux_hist)
        for (int b = tid; b < 2 * out.flux_nbins; b += 256)
          __hip_atomic_store(out.done_host + DONE_FLUX + b, ld_agent(reinterpret_cast<const unsigned long long*>(out.flux_hist) + b),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __syncthreads();
      if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // (system scope)
        __hip_atomic_store(out.done_host, (unsigned long long)complete, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

}  // namespace art
