// art_host_paths.cpp -- the host-pointer propagate calls: which path a batch takes
// (propagate_host_impl: the streamed call of art_host_stream.cpp, the chunked pipeline or one
// launch), the chunked and the single-launch paths, and the art_propagate_*_host entry points
// (declared in include/art.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "art_host.h"

namespace art {
namespace host {

// The chunked pipeline's output staging: coarse-grained (non-coherent) mapped host memory
// lets the L2 combine finalize_kernel's 8-byte stores into full-line PCIe writes; the stream
// event the host waits on makes them visible. ART_HOST_COHERENT=1: fine-grained memory (A/B).
static unsigned out_coherence() {
  return env_int("ART_HOST_COHERENT", 0) ? hipHostMallocCoherent : hipHostMallocNonCoherent;
}

// art_propagate_host for large batches: a pipeline of chunks (the reference call
// site MainRunner.jl:179-190 hands over host arrays).
//   * uploads: chunk k's inputs, gathered from the caller's arrays into pinned staging by the
//     copy pool, go to HBM on one stream, all submitted up front;
//   * compute: `slots` streams, chunk k on stream k % slots, each launch waiting for its own
//     upload only, so two chunks in flight fill each other's drain tails (tail donation);
//   * downloads: none. Each chunk's finalize_kernel writes its outputs straight into mapped
//     pinned memory over PCIe (coalesced 8-byte-per-lane stores), on a stream of its own
//     after the chunk's integrator kernels, so the outputs leave while the compute stream
//     goes on with its next chunk, and no copy waits behind a kernel.
// The host scatters the chunks' outputs into the caller's arrays in order while the later
// ones still compute. Only the first chunk's upload and the last chunk's finalize and
// scatter are not hidden behind compute, so those two chunks are a quarter of the others.
// Each chunk's scratch is carved from one preallocated buffer (a stream-ordered allocation
// per chunk blocked the submitting thread once several chunks were in flight).
// Earlier versions and why they lost (profiles/r03o_host_timeline.txt,
// profiles/r03p_host_timeline.txt, profiles/r03q_host_timeline.txt): copies on the compute
// streams (an upload waited behind the previous chunk's download on its stream), then on
// their own streams but submitted per chunk (the runtime keeps copies in submission order, so
// a download held the next uploads back until its chunk was computed), then downloads as
// copies after all uploads (the downloads ran as blit kernels competing with the compute for
// CUs, 4-15 ms per chunk). Per-ray results do not depend on the batch split
// (tests/test_edges.py), so the outputs equal the single launch's bit for bit. The statistics
// and kernel time of the call are the sums over its chunks.
static int propagate_host_chunked(DeviceCtx* c, const art_params* p, int64_t n, const double* x0, const double* k0,
                                  const double* erg, const double* dw, const double* ln_t0, const int8_t* species,
                                  int32_t max_crossings, art_segment_out* out, art_crossing_buf* xc, int nchunks,
                                  int nslots, const FluxArgs& fx) {
  const int cap = (xc && xc->count) ? xc->capacity : 0;
  const int64_t K = std::max(2, nchunks);
  const art::KParams KP = kparams(*p);
  // a chunk of m rays: its inputs as an input blob (pinned staging and HBM), its outputs as an
  // output blob (pinned) -- in_blob_bytes (art_host_plan.h), art::blob_bytes (art_pieces.h)
  // chunk boundaries: weights 1/4, 1, ..., 1, 1/4
  std::vector<int64_t> lo(K + 1);
  const double wsum = 0.5 + double(K - 2);
  for (int64_t k = 0; k <= K; ++k) {
    const double wk = k == 0 ? 0.0 : (k == K ? wsum : 0.25 + double(k - 1));
    lo[k] = (int64_t)((double)n * (wk / wsum));
  }
  lo[K] = n;
  const int32_t donate = nslots > 1 ? 16 : 0;
  std::vector<size_t> ioff(K + 1, 0), ooff(K + 1, 0), soff(K + 1, 0);
  for (int64_t k = 0; k < K; ++k) {
    const int64_t m = lo[k + 1] - lo[k];
    // the same layout propagate_device_impl will carve out of this chunk's slice (a chunk small
    // enough for the tail kernel keeps one donation record per ray, whatever `donate` says)
    const bool st = use_small_tail(p, m, TrajArgs());
    ScratchLayout SL;
    int rc0 = scratch_layout(c, m, cap, st ? 0 : donate, &SL, st);
    if (rc0) return rc0;
    ioff[k + 1] = ioff[k] + in_blob_bytes(m);
    ooff[k + 1] = ooff[k] + art::blob_bytes(m, cap);
    soff[k + 1] = soff[k] + art::blob_up(SL.total());
  }
  while ((int)c->pstreams.size() < nslots) {
    hipStream_t st = c->stream;
    if (!c->pstreams.empty()) HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    c->pstreams.push_back(st);
  }
  if (!c->h2d) HIP_OK(hipStreamCreateWithFlags(&c->h2d, hipStreamNonBlocking));
  if (!c->fin) HIP_OK(hipStreamCreateWithFlags(&c->fin, hipStreamNonBlocking));
  while ((int64_t)c->pev.size() < 2 * K) {
    hipEvent_t ev;
    HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    c->pev.push_back(ev);
  }
  hipEvent_t *ev_in = c->pev.data(), *ev_done = ev_in + K;
  int rc;
  void *pi, *po, *di_, *sc_;
  if ((rc = pinned_get(c, 0, ioff[K], &pi)) ||
      (rc = pinned_get(c, 1, ooff[K], &po, hipHostMallocMapped | out_coherence())) ||
      (rc = pool_get(c, 16, ioff[K], &di_)) || (rc = pool_get(c, 17, soff[K], &sc_)))
    return rc;
  void* po_dev = nullptr;
  HIP_OK(hipHostGetDevicePointer(&po_dev, po, 0));
  char *pin_in = (char*)pi, *pin_out = (char*)po, *out_dev = (char*)po_dev, *dev_in = (char*)di_, *scratch = (char*)sc_;
  double* hist_dev = nullptr;
  if (fx.nbins) {
    if ((rc = pool_get(c, 23, 2 * (size_t)fx.nbins * sizeof(double), (void**)&hist_dev))) return rc;
    HIP_OK(hipMemsetAsync(hist_dev, 0, 2 * (size_t)fx.nbins * sizeof(double), c->fin));
  }
  std::vector<int> rings;
  // ART_HOST_TRACE=1: the host side of every chunk to stderr (gathers, submits, waits, scatters)
  const bool trace = env_int("ART_HOST_TRACE", 0) != 0;
  auto clk = now_ms;
  const double t_start = clk();
  // Submission order: upload 0, compute 0, the other uploads, the other computes (the
  // runtime keeps copies in submission order, so no upload waits behind anything).
  auto upload = [&](int64_t k) -> int {
    const int64_t l0 = lo[k], m = lo[k + 1] - lo[k];
    char* bi = pin_in + ioff[k];
    const std::vector<Seg> g = gather_segs((double*)bi, m, (int8_t*)(bi + in_blob_species_off(m)), m, l0, n, x0, k0, erg, dw,
                                           ln_t0, species);
    const double tg0 = clk();
    copy_pool().run(g);
    const double tg1 = clk();
    HIP_OK(hipMemcpyAsync(dev_in + ioff[k], bi, in_blob_bytes(m), hipMemcpyHostToDevice, c->h2d));
    HIP_OK(hipEventRecord(ev_in[k], c->h2d));
    if (trace)
      std::fprintf(stderr, "[art-host] t=%.2f upload lo=%lld m=%lld gather %.2f ms submit %.2f ms\n", tg0 - t_start,
                   (long long)l0, (long long)m, tg1 - tg0, clk() - tg1);
    return ART_OK;
  };
  auto compute = [&](int64_t k) -> int {
    const double t0 = clk();
    hipStream_t st = c->pstreams[k % nslots];
    const int64_t m = lo[k + 1] - lo[k];
    const double* di = (const double*)(dev_in + ioff[k]);
    HIP_OK(hipStreamWaitEvent(st, ev_in[k], 0));
    BlobView dv = blob_view(out_dev + ooff[k], m, cap);  // device view of the chunk's pinned outputs
    art_segment_out& dso = dv.out;
    LaunchOpts lo_;
    lo_.donate = donate;
    lo_.scratch = scratch + soff[k];
    lo_.scratch_bytes = soff[k + 1] - soff[k];
    lo_.nan_fill = true;
    lo_.finalize_stream = c->fin;
    const int8_t* dsp = (const int8_t*)((const char*)di + in_blob_species_off(m));
    int rc2 = propagate_device_impl(p, m, di, di + 3 * m, di + 6 * m, di + 7 * m, di + 8 * m, dsp, max_crossings,
                                    &dso, dv.xcp(), st, TrajArgs(), lo_);
    if (rc2) return rc2;
    if (fx.nbins)  // the chunk's flux from its outputs (mapped pinned memory), behind its finalize
      HIP_OK(art::launch_flux(KP, m, dso.x_end, dso.k_end, dso.status, dsp, nullptr, fx.nbins, hist_dev, c->fin));
    rings.push_back(c->last);
    HIP_OK(hipEventRecord(ev_done[k], c->fin));
    if (trace) std::fprintf(stderr, "[art-host] t=%.2f compute k=%lld submit %.2f ms\n", t0 - t_start, (long long)k, clk() - t0);
    return ART_OK;
  };
  if ((rc = upload(0)) || (rc = compute(0))) return rc;
  for (int64_t k = 1; k < K; ++k)
    if ((rc = upload(k))) return rc;
  for (int64_t k = 1; k < K; ++k)
    if ((rc = compute(k))) return rc;
  // the chunks' outputs, in order: pinned staging -> the caller's arrays
  for (int64_t k = 0; k < K; ++k) {
    const double tw0 = clk();
    HIP_OK(hipEventSynchronize(ev_done[k]));
    const double tw1 = clk();
    const int64_t l0 = lo[k], m = lo[k + 1] - lo[k];
    copy_pool().run(scatter_segs(pin_out + ooff[k], m, cap, l0, n, *out, xc));
    if (trace)
      std::fprintf(stderr, "[art-host] t=%.2f drain lo=%lld wait %.2f ms scatter %.2f ms\n", tw0 - t_start,
                   (long long)l0, tw1 - tw0, clk() - tw1);
  }
  if (trace) std::fprintf(stderr, "[art-host] total %.2f ms\n", clk() - t_start);
  if (fx.nbins) {
    HIP_OK(hipMemcpyAsync(fx.hist, hist_dev, 2 * (size_t)fx.nbins * sizeof(double), hipMemcpyDeviceToHost, c->fin));
    HIP_OK(hipStreamSynchronize(c->fin));
  }
  return finish_timing_sum(c, rings);
}

// The single-launch host path: the inputs up, one propagate launch (init, integrator, finalize),
// the outputs back, all on stream s with device staging from `pool` (slots pb .. pb + 4): the
// context's own for synchronous calls, a host lane's for an asynchronous call's fallback.
int propagate_host_single(DeviceCtx* c, hipStream_t s, PoolVec& pool, size_t pb, const art_params* p, int64_t n,
                          const double* x0, const double* k0, const double* erg, const double* dw, const double* ln_t0,
                          const int8_t* species, int32_t max_crossings, art_segment_out* out, art_crossing_buf* xc,
                          const TrajArgs& htr, const FluxArgs& fx) {
  int rc;
  const int cap = (xc && xc->count) ? xc->capacity : 0;
  const size_t nd = (size_t)n;
  // staging layout: inputs 3n+3n+n+n+n doubles + n int8; outputs 3n+3n+n+n doubles + 3n int32 (+ crossings)
  void *din, *dout, *dxc = nullptr;
  const size_t in_bytes = nd * 9 * sizeof(double) + nd;
  const size_t out_bytes = nd * 8 * sizeof(double) + nd * 3 * sizeof(int32_t);
  const size_t cnt_bytes = ((nd * sizeof(int32_t) + 15) / 16) * 16;
  const size_t xc_bytes = cap ? cnt_bytes + (size_t)cap * nd * 9 * sizeof(double) : 0;
  if ((rc = pool_get_v(pool, pb + 0, in_bytes, &din))) return rc;
  if ((rc = pool_get_v(pool, pb + 1, out_bytes, &dout))) return rc;
  if (cap && (rc = pool_get_v(pool, pb + 2, xc_bytes, &dxc))) return rc;
  double* di = (double*)din;
  HIP_OK(hipMemcpyAsync(di, x0, nd * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(di + 3 * nd, k0, nd * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(di + 6 * nd, erg, nd * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(di + 7 * nd, dw, nd * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(di + 8 * nd, ln_t0, nd * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync((int8_t*)(di + 9 * nd), species, nd, hipMemcpyHostToDevice, s));
  art_segment_out dso = blob_view(dout, n, 0).out;  // (the crossings lie in a slot of their own)
  art_crossing_buf dxb{};
  art_crossing_buf* dxbp = nullptr;
  if (cap) {
    int32_t* cnt = (int32_t*)dxc;
    double* xd = (double*)((char*)dxc + cnt_bytes);
    dxb = art_crossing_buf{cap, cnt, xd, xd + 3 * cap * nd, xd + 6 * cap * nd, xd + 7 * cap * nd, xd + 8 * cap * nd};
    dxbp = &dxb;
  }
  TrajArgs dtr;
  if (htr.ntimes != 0) {
    void* dt_ = nullptr;
    const size_t nt = (size_t)htr.ntimes * nd;
    if ((rc = pool_get_v(pool, pb + 3, nt * 4 * sizeof(double) + nd * sizeof(int32_t), &dt_))) return rc;
    dtr.ntimes = htr.ntimes;
    dtr.traj = (double*)dt_;
    dtr.t = dtr.traj + 3 * nt;
    dtr.count = (int32_t*)(dtr.t + nt);
  }
  art_cyclotron_out dcy{};
  if (htr.cyc) {  // staging (saveat's slot: never both): tau n, pos 3n, ln t n doubles, then count n int32
    void* dc_ = nullptr;
    if ((rc = pool_get_v(pool, pb + 3,nd * 5 * sizeof(double) + nd * sizeof(int32_t), &dc_))) return rc;
    dcy.tau = (double*)dc_;
    dcy.pos = dcy.tau + nd;
    dcy.ln_t = dcy.tau + 4 * nd;
    dcy.count = (int32_t*)(dcy.tau + 5 * nd);
    dtr.cyc = &dcy;
  }
  // slots without a crossing come back as NaN, not as whatever the pooled staging buffer last
  // held: finalize_kernel writes them (LaunchOpts::nan_fill)
  LaunchOpts opt;
  opt.nan_fill = true;
  LaunchRec* L = nullptr;
  opt.launch_out = &L;
  rc = propagate_device_impl(p, n, di, di + 3 * nd, di + 6 * nd, di + 7 * nd, di + 8 * nd, (const int8_t*)(di + 9 * nd),
                             max_crossings, &dso, dxbp, s, dtr, opt, c);
  if (rc) return rc;
  if (fx.nbins) {  // the batch's flux from its outputs in HBM
    double* hist_dev = nullptr;
    if ((rc = pool_get_v(pool, pb + 4, 2 * (size_t)fx.nbins * sizeof(double), (void**)&hist_dev))) return rc;
    HIP_OK(hipMemsetAsync(hist_dev, 0, 2 * (size_t)fx.nbins * sizeof(double), s));
    HIP_OK(art::launch_flux(kparams(*p), n, dso.x_end, dso.k_end, dso.status, (const int8_t*)(di + 9 * nd), nullptr,
                            fx.nbins, hist_dev, s));
    HIP_OK(hipMemcpyAsync(fx.hist, hist_dev, 2 * (size_t)fx.nbins * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (htr.ntimes != 0) {
    const size_t nt = (size_t)htr.ntimes * nd;
    HIP_OK(hipMemcpyAsync(htr.traj, dtr.traj, nt * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(htr.t, dtr.t, nt * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(htr.count, dtr.count, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
  if (htr.cyc) {
    HIP_OK(hipMemcpyAsync(htr.cyc->tau, dcy.tau, nd * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(htr.cyc->count, dcy.count, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(htr.cyc->pos, dcy.pos, nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(htr.cyc->ln_t, dcy.ln_t, nd * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_OK(hipMemcpyAsync(out->x_end, dso.x_end, nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->k_end, dso.k_end, nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->u7_end, dso.u7_end, nd * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->tau_end, dso.tau_end, nd * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->status, dso.status, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->n_accept, dso.n_accept, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->n_reject, dso.n_reject, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (cap) {
    HIP_OK(hipMemcpyAsync(xc->count, dxb.count, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(xc->pos, dxb.pos, (size_t)cap * nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(xc->k, dxb.k, (size_t)cap * nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(xc->t, dxb.t, (size_t)cap * nd * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(xc->dw, dxb.dw, (size_t)cap * nd * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(xc->p_nonad, dxb.p_nonad, (size_t)cap * nd * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_OK(hipStreamSynchronize(s));
  if (htr.cyc) {  // the host contract: NaN where no crossing was found (the staging held stale values)
    for (size_t i = 0; i < nd; ++i) {
      if (htr.cyc->count[i] != 0) continue;
      htr.cyc->pos[i] = htr.cyc->pos[nd + i] = htr.cyc->pos[2 * nd + i] = NAN;
      htr.cyc->ln_t[i] = NAN;
    }
  }
  return finish_timing_slot(c, L);
}

// Synchronous host calls wait for every asynchronous one first: they share lane 0 and the
// context's staging (art_propagate_host_flux_async).
static void drain_async(DeviceCtx* c) {
  for (HostLane& H : c->lanes) {
    std::unique_lock<std::mutex> lk(H.m);
    H.cv.wait(lk, [&] { return !H.busy; });
  }
}

// Which path a host call of n rays takes: the streamed pipeline for large Vern6 batches without
// saveat (ART_HOST_CHUNK_MIN rays and more, default 2^20, so the 1.25e6-ray shard of 8 GPUs
// streams: 18.3 ms against 20.0 in one launch, profiles/r04x_shard_sizes.jsonl), the chunked one
// with ART_HOST_MODE=chunked; the single launch otherwise (and after a streamed call gave up)
HostPath host_path(const art_params* p, int64_t n, const TrajArgs& htr) {
  const char* mode_env = std::getenv("ART_HOST_MODE");
  const std::string mode = (mode_env && *mode_env) ? mode_env : "stream";
  if (htr.none() && n >= env_int("ART_HOST_CHUNK_MIN", 1 << 20)) {
    if (mode == "stream" && p->integrator == ART_VERN6) return HP_STREAM;
    if (mode == "chunked") return HP_CHUNKED;
  }
  return HP_SINGLE;
}

int host_args(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg, const double* dw,
              const double* ln_t0, const int8_t* species, art_segment_out* out, art_crossing_buf* xc, const TrajArgs& htr,
              const FluxArgs& fx, bool* empty) {
  int rc = check_segment_args(p, n, x0, k0, erg, dw, ln_t0, species, out, xc, htr, empty);
  if (rc) return rc;
  if (fx.nbins && (fx.nbins < 1 || fx.nbins > 4096 || !fx.hist)) return fail(ART_E_INVALID, "flux needs nbins in [1, 4096] and hist");
  if (fx.nbins) std::fill(fx.hist, fx.hist + 2 * (size_t)fx.nbins, 0.0);
  return ART_OK;
}

int propagate_host_impl(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                        const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                        art_segment_out* out, art_crossing_buf* xc, const TrajArgs& htr,
                        const FluxArgs& fx) {
  bool empty = false;
  int rc = host_args(p, n, x0, k0, erg, dw, ln_t0, species, out, xc, htr, fx, &empty);
  if (rc || empty) return rc;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  drain_async(c);
  g_host_cnt[HC_CALLS] += 1;
  const HostPath hp = host_path(p, n, htr);
  if (hp == HP_STREAM) {
    rc = propagate_host_stream(c, &c->lanes[0], false, -1, p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, fx);
    if (rc != STREAM_FALLBACK) {
      if (rc == ART_OK) g_host_cnt[HC_STREAMED] += 1;
      return rc;
    }
    g_host_cnt[HC_GIVEUPS] += 1;
  } else if (hp == HP_CHUNKED) {
    g_host_cnt[HC_CHUNKED] += 1;
    return propagate_host_chunked(c, p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc,
                                  std::max(2, env_int("ART_HOST_CHUNKS", 4)), std::max(1, env_int("ART_HOST_SLOTS", 2)), fx);
  }
  g_host_cnt[HC_SINGLE] += 1;
  return propagate_host_single(c, c->stream, c->pool, 0, p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc,
                               htr, fx);
}

}  // namespace host
}  // namespace art

using namespace art::host;

extern "C" {

int art_propagate_host(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                       const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                       art_segment_out* out, art_crossing_buf* xc) {
  std::lock_guard<std::mutex> lk(g_mu);
  return propagate_host_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, TrajArgs());
}

int art_propagate_host_flux(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                            const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                            art_segment_out* out, art_crossing_buf* xc, int32_t nbins, double* hist) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (nbins < 1) return fail(ART_E_INVALID, "nbins must be >= 1");
  FluxArgs fx;
  fx.nbins = nbins;
  fx.hist = hist;
  return propagate_host_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, TrajArgs(), fx);
}

int art_propagate_traj_host(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                            const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                            art_segment_out* out, art_crossing_buf* xc, int32_t ntimes, double* traj, double* traj_t,
                            int32_t* traj_n) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (ntimes < 2) return fail(ART_E_INVALID, "ntimes must be >= 2");
  TrajArgs tr;
  tr.ntimes = ntimes; tr.traj = traj; tr.t = traj_t; tr.count = traj_n;
  return propagate_host_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, tr);
}

int art_propagate_cyclotron_host(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                                 const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                                 art_segment_out* out, art_crossing_buf* xc, const art_cyclotron_out* cyc) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!cyc) return fail(ART_E_INVALID, "cyc is NULL");
  TrajArgs tr;
  tr.cyc = cyc;
  return propagate_host_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, tr);
}

}  // extern "C"
