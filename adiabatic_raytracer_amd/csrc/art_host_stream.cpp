// art_host_stream.cpp -- the streamed host call (StreamCall: the path bench.py times), the host
// lanes it runs on, the lanes' workers and the asynchronous entry points
// (art_propagate_host_flux_async, art_host_wait; declared in include/art.h).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "art_host.h"

namespace art {
namespace host {

// art_propagate_host for large batches, streamed with no CU reserved (the default; SURVEY §8b,
// the reference call site MainRunner.jl:179-190 hands over host arrays). ONE integrator launch
// (propagate_kernel<..., DON = 3>) holds every CU for the whole batch; nothing else needs a CU
// while it runs:
//   * the host gathers piece k from the caller's arrays into pinned staging (copy pool) and
//     copies it to HBM on the upload stream (DMA engines:
//     profiles/r04k_probe_*.jsonl -- 64 MB copies finish at 56 GB/s under a kernel holding
//     every CU); a host thread raises the ready counter (host memory) as each piece lands;
//   * persistent helper blocks (helper_kernel HK_TILES, a separate kernel on a stream of its own,
//     resident beside the integrator) initialise 1024-ray tiles whose inputs have landed
//     (init_one, the init_kernel arithmetic) and flag their chunks; a wave that claims a
//     chunk of 64 rays waits for its flag. Once every ray of a piece has finished, helpers
//     finalize its tiles (finalize_one) into the piece's SoA blob in HBM, and the block that
//     finalizes its last tile raises the piece's flag (host memory);
//   * the host polls the flags, copies each finished blob to pinned memory (DMA engines) and
//     scatters it into the caller's arrays.
// Before the integrator, one helper_kernel pass on the integrator's stream initialises the first
// rays with every block slot; after it, one more pass finalizes what is left.
// The two ends of a call, where the GPU stands idle (10^7 flat rays, ART_HOST_TRACE timelines
// profiles/host_trace_parent.log before and profiles/host_trace_new.log after). Start: the upload
// units ramp -- 2^16-ray units until the launch's lanes all have a ray on its way, then doubling
// to 2^18 -- and the gatherer submits the first unit's copy itself: first unit ready at 0.58 ms
// (0.89 before), 2^17 rays in HBM at 0.83 ms (2^16 until 1.76 ms before). End: the batch's last
// rays lie in fine output pieces (art_pieces.h: 35 pieces of 2^18 rays, then 26 of 2^15 over the
// last 0.8e6), so a straggler holds back 5 MB, not 39 MB: the last scatter ends 1.0 ms after the
// integrator (1.7 ms before). Pieces are still finalized in order, so the first piece with a
// straggler holds back the finalize of the pieces behind it (7 of 2^15 in that timeline).
// Interleaved A/B, seven processes each: 90.23-91.28 ms per call before, 89.31-89.85 now; 1.25e6
// rays one call at a time 16.16-16.66 -> 15.11-15.70 ms (profiles/ab_host_two_ends*.jsonl).
// Calls in flight keep the old start and one level of pieces (see fine_shift in StreamCall::plan).
// Round 3's CU-masked pipeline ran the init and finalize kernels on 8 reserved CUs, which cost
// ~10% of the integrator (profiles/r04g_stream_anatomy.jsonl); it is gone. Per-ray results
// equal the single launch's bit for bit.

constexpr size_t HSIG_WORDS = HSIG_DONE + art::DONE_FLUX + 2 * art::FLUX_HELPER_BINS;

static int lane_setup(DeviceCtx* c, HostLane* H) {
  if (!H->m_comp) {
    // the integrator's and the persistent helpers' streams each on a hardware queue of its own
    // (own_queue_stream): a stream queued behind a persistent kernel waits for that kernel to
    // end -- the integrator behind the helpers never started (profiles/r04p_maskless_hwqueue.txt)
    int rc;
    if ((rc = own_queue_stream(c, &H->m_comp)) || (rc = own_queue_stream(c, &H->m_help))) return rc;
    HIP_OK(hipStreamCreateWithFlags(&H->m_up, hipStreamNonBlocking));
    HIP_OK(hipStreamCreateWithFlags(&H->m_dn, hipStreamNonBlocking));
  }
  if (!H->hsig) {
    unsigned long long* hs = nullptr;
    HIP_OK(hipHostMalloc((void**)&hs, sizeof(unsigned long long) * HSIG_WORDS, hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(hs, 0, sizeof(unsigned long long) * HSIG_WORDS);  // ([HSIG_RESIDENT] is never reset)
    HIP_OK(hipHostGetDevicePointer((void**)&H->hsig_dev, hs, 0));
    // (published last, with release: another lane's worker reads the pointer in prev_resident)
    __atomic_store_n(&H->hsig, hs, __ATOMIC_RELEASE);
  }
  if (!H->abort_host) {
    HIP_OK(hipHostMalloc((void**)&H->abort_host, 64, hipHostMallocCoherent | hipHostMallocMapped));
    HIP_OK(hipHostGetDevicePointer((void**)&H->abort_dev, H->abort_host, 0));
  }
  return ART_OK;
}

namespace {

// A thread the call owns: leaving the scope raises its stop flag and joins it, so every return of
// the call, the early ones of HIP_OK included, is safe while it runs.
struct OwnedThread {
  std::atomic<bool> stop{false};
  std::thread t;
  void join() {
    if (t.joinable()) t.join();
  }
  ~OwnedThread() {
    stop = true;
    join();
  }
};

struct StreamArgs {
  DeviceCtx* c;
  HostLane* H;
  bool overlap;    // an asynchronous call: others may be in flight beside it
  int64_t ticket;  // ... its ticket (-1: a synchronous call)
  const art_params* p;
  int64_t n;
  const double *x0, *k0, *erg, *dw, *ln_t0;
  const int8_t* species;
  int32_t max_crossings;
  art_segment_out* out;
  art_crossing_buf* xc;
  FluxArgs fx;
};

// One streamed call: its plan, its staging, its two threads and its progress, with the steps of
// run() as member functions.
struct StreamCall : StreamArgs {
  explicit StreamCall(const StreamArgs& a) : StreamArgs(a) {}
  int run();

  // plan
  int cap = 0;
  art::KParams K;
  art::Pieces pcs;
  int np = 0;
  size_t nd = 0, in_bytes = 0, blobs = 0, ccb = 0, u0b = 0, recb = 0, xrb = 0;
  bool direct = false, serial = false, final_pass = false;
  int slots = 0, helpers = 0, iblocks = 0;
  std::vector<int64_t> ulo;  // the upload units' bounds (independent of the output pieces)
  int nu = 0;
  // staging and views
  void *po = nullptr, *dout = nullptr;  // the output blobs: pinned, and in HBM (direct: the same memory)
  char* dsc = nullptr;                  // scratch: head | chunk flags | u0 U0_REC n | rec END_REC n | xrec
  double *pin = nullptr, *di = nullptr;
  unsigned long long* words = nullptr;  // the scratch head (HeadWord)
  art::SegIn in{};
  art::SegOut so{};
  hipEvent_t *ev_up = nullptr, *ev_dn = nullptr;
  unsigned long long *hready = nullptr, *hflag = nullptr, *hdone = nullptr;  // HostLane::hsig (HostSignal)
  bool hflux = false;
  double* hist_dev = nullptr;
  bool trace = false;
  double t_start = 0.0, t_last = 0.0;
  unsigned long long* peek = nullptr;  // (trace) the device counters, copied out every 100 ms
  // progress
  int delay_ms = 0;
  bool early0 = false, launched = false;
  std::atomic<int> gathered{0}, early0_err{0}, recorded{0}, ready_err{0};
  int dk = 0, sk = 0;  // pieces whose download is queued / scattered
  // (destroyed in reverse order: the readier joins first, then the record is released, then the
  // gatherer joins -- while everything above is still alive)
  OwnedThread gatherer;
  LaunchRec* L = nullptr;
  struct ReleaseRec {  // a call that leaves before latching its record frees it for take_slot
    LaunchRec*& L;
    ~ReleaseRec() {
      if (L) L->held.store(false, std::memory_order_release);
    }
  } release_rec{L};
  OwnedThread readier;

  int64_t piece_lo(int k) const { return art::piece_lo(pcs, k); }
  size_t blob_off(int k) const { return art::piece_blob_off(pcs, k, cap); }
  double clk() const { return now_ms(); }

  void plan();
  int stage();
  void reset_signals();
  void start_gatherer();
  bool submit_unit(int u);
  int zero_counters();
  void fill_segout();
  int launch_helpers();
  bool helpers_in() const;
  bool prev_resident() const;
  int launch_main();
  int launch_if_resident();
  void start_readier();
  int progress();
  int upload_loop();
  int launch_late(int perr);
  void trace_counters();
  bool wait_pieces(int perr);
  int give_up();
  int finish();
};

void StreamCall::plan() {
  cap = (xc && xc->count) ? xc->capacity : 0;
  K = kparams(*p);
  int shift = default_piece_shift(n);  // 32..64 pieces (2^18 rays for 10^7: the last
  // piece's finalize, copy and scatter are the call's tail, 95.3-96.5 ms against 98.4-101 with 2^19,
  // profiles/r04ag_piece_shift.jsonl)
  const int shift_env = env_int("ART_HOST_PIECE_SHIFT", 0);
  if (shift_env) shift = std::max(art::PIECE_MIN_SHIFT, shift_env);  // (tests: many small pieces, one level)
  // The batch's last rays in fine pieces (art_pieces.h): a piece completes with its slowest ray, and
  // the rays still running when the queue runs dry were claimed in its last few milliseconds, so
  // each of the last coarse pieces kept 39 MB on the GPU until the integrator's very end -- the
  // call's tail of finalize, D2H and scatter. ART_HOST_FINE_RAYS: the fine region (at most so many
  // rays; default min(2^20, n / 8)), ART_HOST_FINE_SHIFT: its pieces (default 2^15 rays; 0: one
  // level). One level by default where the coarse pieces are 2^15 rays or fewer already, and
  // whenever ART_HOST_PIECE_SHIFT alone is set. The pieces number at most HSIG_NFLAG (make_pieces).
  // Calls in flight (overlap) keep one level and the plain start below by default: their two ends
  // overlap the neighbouring calls' work, so there is nothing idle to win, and with the ramped
  // start two 1.25e6-ray calls in flight took the slow way of interleaving in 22 of 24 runs
  // against 24 of 36 for the build before, ~15.1 against ~14.3 ms per call at the medians; with
  // all three defaults off, 23 of 36 (profiles/aa_host_inflight2_*.jsonl)
  const int fine_shift = env_int("ART_HOST_FINE_SHIFT", (!shift_env && shift > 15 && !overlap) ? 15 : 0);
  const int64_t fine_rays = env_int("ART_HOST_FINE_RAYS", (int)std::min((int64_t)1 << 20, n / 8));
  pcs = art::make_pieces(n, shift, fine_shift, fine_rays);
  np = pcs.count;
  nd = (size_t)n;
  in_bytes = nd * 9 * sizeof(double) + nd;  // x0 (3n) k0 (3n) erg dw lnt0 | species
  // per-piece SoA output blobs, pinned and in HBM: the partition and the layout of art_pieces.h,
  // which piece_blob (art_ray_io.h) and the integrator use too
  blobs = blob_off(np);
  const size_t nchunk = (nd + art::CHUNK - 1) / art::CHUNK;
  ccb = art::blob_up(nchunk * sizeof(unsigned));
  u0b = nd * art::U0_REC * sizeof(double);
  recb = nd * art::END_REC * sizeof(double);
  xrb = (size_t)cap * nd * art::X_REC * sizeof(double);
  // ART_HOST_DIRECT=1: the pieces' output blobs in pinned host memory (fine-grained), written by the
  // helpers over PCIe and scattered as soon as a piece is flagged -- no download copies (which a
  // profiler's tracing turns into blit kernels competing for CU slots)
  direct = env_int("ART_HOST_DIRECT", 0) != 0;
}

// The lane's streams and words, the buffers and their views, then -- with the device's CU count --
// the block counts, the upload units and the events.
int StreamCall::stage() {
  int rc;
  if ((rc = lane_setup(c, H))) return rc;
  void *pi, *din, *sc;
  if ((rc = pinned_get_v(H->pinned, 0, in_bytes, &pi)) ||
      (rc = pinned_get_v(H->pinned, 1, blobs, &po,
                         direct ? (hipHostMallocMapped | hipHostMallocCoherent) : hipHostMallocDefault)) ||
      (rc = pool_get_v(H->pool, 0, in_bytes, &din)) ||
      (!direct && (rc = pool_get_v(H->pool, 1, blobs, &dout))) ||
      (rc = pool_get_v(H->pool, 2, STREAM_HEAD_BYTES + ccb + u0b + recb + xrb, &sc)))
    return rc;
  if (direct) HIP_OK(hipHostGetDevicePointer(&dout, po, 0));
  pin = (double*)pi;
  di = (double*)din;
  dsc = (char*)sc;
  words = (unsigned long long*)sc;
  in = art::SegIn{di, di + 3 * nd, di + 6 * nd, di + 7 * nd, di + 8 * nd, (const int8_t*)(di + 9 * nd),
                  (double*)(dsc + STREAM_HEAD_BYTES + ccb)};
  int ncu = 0;
  HIP_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
  slots = std::max(2, env_int("ART_HOST_BLOCKS", 2 * ncu));  // block slots: 2 per CU
  // helper blocks beside the integrator (ART_HOST_HELPERS, default 16): launched first, and the
  // integrator only once every one of them is resident, so it cannot take their slots. Each helper
  // block (2 waves per SIMD, the top issue priority) shares a CU with one integrator block, so it
  // costs one integrator block slot, not a CU: 1e7 rays, 3 rounds on one box, the integrator 92.1-
  // 93.4 -> 88.2-89.0 ms and the call 95.3-96.0 -> 91.1-92.1 ms with 16 helpers; 8 helpers let the
  // finalize lag (109 ms calls), 12 and 24 are between (profiles/r06j_helpers.jsonl)
  const int hw = art::helper_waves_per_simd(K);
  const int helpers_wanted = env_int("ART_HOST_HELPERS", hw == 2 ? 16 : 8);
  // (dev, ART_HOST_STREAM_SERIAL=1: no persistent helpers -- every tile initialised before the
  // integrator and finalized after it, kernel by kernel: for a counter-collection run, which
  // serialises kernels; the integrator's code and traffic are the same)
  serial = env_int("ART_HOST_STREAM_SERIAL", 0) != 0;
  const StreamBlocks sb = stream_blocks(slots, hw, helpers_wanted, serial);
  helpers = sb.helpers;
  iblocks = sb.iblocks;
  // After the integrator, one pass of every block slot finalizes what is left -- unless this call
  // overlaps the next one (art_propagate_host_flux_async): then the next call's integrator would
  // hold those slots, and the helpers finalize alone
  final_pass = serial || !overlap;
  // upload units (independent of the output pieces): small first ones (2^16 rays, the integrator
  // starts soon) until the launch's lanes (iblocks x 256) all have a ray on its way -- a jump to the
  // steady size after one small unit left half the lanes waiting for a 2^18-ray unit's cold gather
  // and copy -- then units doubling up to the steady max(2^18 rays, a piece): each unit costs
  // ~0.2 ms of host-side submission, which small pieces made the bound of a 1.25e6-ray call's
  // uploads. (ART_HOST_FIRST_UNIT / ART_HOST_UNIT: tests and A/B, other first and steady sizes in
  // rays; ART_HOST_UNIT_RAMP=0, the default for calls in flight: one first unit, then the steady
  // size at once)
  const int64_t ustep = std::max(1, env_int("ART_HOST_UNIT", (int)std::max((int64_t)1 << 18, (int64_t)1 << pcs.shift)));
  const int64_t ufirst = std::max(1, env_int("ART_HOST_FIRST_UNIT", 1 << 16));
  const bool ramp = env_int("ART_HOST_UNIT_RAMP", overlap ? 0 : 1) != 0;  // (calls in flight: see fine_shift)
  ulo = upload_units(n, ufirst, ustep, ramp, (int64_t)iblocks * 256);
  nu = (int)ulo.size() - 1;
  while ((int64_t)H->pev.size() < nu + np + 2) {
    hipEvent_t ev;
    HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    H->pev.push_back(ev);
  }
  ev_up = H->pev.data();
  ev_dn = H->pev.data() + nu;
  trace = env_int("ART_HOST_TRACE", 0) != 0;
  t_start = clk();
  hready = H->hsig + HSIG_READY;
  hflag = H->hsig + HSIG_FLAGS;
  hdone = H->hsig + HSIG_DONE;
  return ART_OK;
}

void StreamCall::reset_signals() {
  __atomic_store_n(hready, 0ull, __ATOMIC_RELEASE);
  for (int k = 0; k <= HSIG_NFLAG; ++k) __atomic_store_n(hflag + k, 0ull, __ATOMIC_RELEASE);  // (+ the started count)
  __atomic_store_n(hdone, 0ull, __ATOMIC_RELEASE);
  __atomic_store_n(H->abort_host, 0u, __ATOMIC_RELEASE);
}

// one unit's H2D copies and its event: the nine double rows in one strided copy (one DMA command
// instead of nine), then the species
bool StreamCall::submit_unit(int u) {
  const int64_t lo = ulo[u], m = ulo[u + 1] - lo;
  bool bad = hipMemcpy2DAsync(di + lo, nd * sizeof(double), pin + lo, nd * sizeof(double), (size_t)m * sizeof(double), 9,
                              hipMemcpyHostToDevice, H->m_up) != hipSuccess;
  bad |= hipMemcpyAsync((int8_t*)(di + 9 * nd) + lo, (int8_t*)(pin + 9 * nd) + lo, (size_t)m, hipMemcpyHostToDevice,
                        H->m_up) != hipSuccess;
  bad |= hipEventRecord(ev_up[u], H->m_up) != hipSuccess;
  return !bad;
}

// The host gathers the upload units from the caller's arrays into pinned staging on a thread of
// its own, from the call's first moment: the set-up and launches that follow (~1.5 ms at 1.25e6 rays)
// and the first units' gathers overlap instead of adding up (profiles/r05d_shard_if1_trace.err).
void StreamCall::start_gatherer() {
  // (tests: ART_HOST_UPLOAD_DELAY_MS holds back the second upload unit, so the integrator's
  // waves outwait their 2 s bound and the device side gives the call up)
  delay_ms = env_int("ART_HOST_UPLOAD_DELAY_MS", 0);
  // The first unit's copy is what the init pass and so the integrator wait for: the gatherer submits
  // it itself the moment it is gathered, beside the caller's counter memsets, helper launch and
  // residency wait instead of after them (ART_HOST_EARLY_UNIT0=0, the default for calls in flight:
  // the caller submits it)
  early0 = env_int("ART_HOST_EARLY_UNIT0", overlap ? 0 : 1) != 0;  // (calls in flight: see fine_shift)
  const int device = c->device;
  gatherer.t = std::thread([this, device] {
    std::atomic<bool>& gstop = gatherer.stop;
    if (early0 && hipSetDevice(device) != hipSuccess) early0_err = 1;
    for (int u = 0; u < nu && !gstop.load(); ++u) {
      if (delay_ms > 0 && u == 1)
        for (int w = 0; w < delay_ms && !gstop.load(); ++w) std::this_thread::sleep_for(std::chrono::milliseconds(1));
      const int64_t lo = ulo[u], m = ulo[u + 1] - lo;
      const std::vector<Seg> g =
          gather_segs(pin + lo, n, (int8_t*)(pin + 9 * nd) + lo, m, lo, n, x0, k0, erg, dw, ln_t0, species);
      const double tg0 = clk();
      copy_pool().run(g);
      const double tg1 = clk();
      if (u == 0 && early0) {  // (before `gathered`: the caller touches the upload stream only after it)
        if (early0_err.load() == 0 && !submit_unit(0)) early0_err = 1;  // (not on another device: the caller sees the error)
        if (trace) std::fprintf(stderr, "[art-host] t=%.2f unit 0 submitted (by the gatherer)\n", clk() - t_start);
      }
      gathered.store(u + 1, std::memory_order_release);
      if (trace) std::fprintf(stderr, "[art-host] t=%.2f unit %d gathered in %.2f ms\n", tg0 - t_start, u, tg1 - tg0);
    }
  });
}

int StreamCall::zero_counters() {
  HIP_OK(hipMemsetAsync(words, 0, STREAM_HEAD_BYTES + ccb, H->m_comp));
  // the batch's flux: binned by the helpers as they finalize (bins <= FLUX_HELPER_BINS), else by
  // flux kernels over the pieces' blobs after the integrator
  hflux = fx.nbins > 0 && fx.nbins <= art::FLUX_HELPER_BINS;
  if (fx.nbins) {
    int rc;
    if ((rc = pool_get_v(H->pool, 3, 2 * (size_t)fx.nbins * sizeof(double), (void**)&hist_dev))) return rc;
    HIP_OK(hipMemsetAsync(hist_dev, 0, 2 * (size_t)fx.nbins * sizeof(double), H->m_comp));
  }
  return ART_OK;
}

void StreamCall::fill_segout() {
  so.rec = (double*)(dsc + STREAM_HEAD_BYTES + ccb + u0b);
  so.cap = cap;
  so.xrec = cap ? (double*)(dsc + STREAM_HEAD_BYTES + ccb + u0b + recb) : nullptr;
  so.xcount = cap ? (int32_t*)((char*)dout + art::blob_cnt_off(art::piece_rays(pcs, 0))) : nullptr;  // (tested for null only)
  so.piece_cnt = words + HW_PIECE_CNT;
  so.abort_word = H->abort_dev;
  so.queue_word = words + HW_QUEUE;
  // (tests: ART_HOST_WAVE_WAIT_MS shortens a wave's bound on its chunk, s_memrealtime at 100 MHz)
  so.wait_ticks = env_int("ART_HOST_WAVE_WAIT_MS", 0) > 0 ? (unsigned long long)env_int("ART_HOST_WAVE_WAIT_MS", 0) * 100000ull
                                                         : art::STREAM_WAIT_TICKS;
  so.pieces = pcs;
  so.host_ready = H->hsig_dev + HSIG_READY;
  so.host_flags = H->hsig_dev + HSIG_FLAGS;
  so.init_next = words + HW_INIT_NEXT;
  so.fin_next = words + HW_FIN_NEXT;
  so.piece_fin = words + HW_PIECE_FIN;
  so.chunk_ready = (unsigned*)(dsc + STREAM_HEAD_BYTES);
  so.blob = (char*)dout;
  so.blob_host = direct ? 1 : 0;
  so.flux_hist = hflux ? hist_dev : nullptr;
  so.flux_nbins = hflux ? fx.nbins : 0;
  so.done_host = H->hsig_dev + HSIG_DONE;
  so.exit_count = words + HW_EXIT;
  so.waves_done = words + HW_WAVES_DONE;
  so.waves_started = words + HW_WAVES_STARTED;
  so.helpers = helpers;
  so.exit_expected = (serial ? 0 : helpers) + (final_pass ? slots : 0);
}

int StreamCall::launch_helpers() {
  hipEvent_t ev_zero = H->pev[nu + np];  // (the helpers start on zeroed counters)
  HIP_OK(hipEventRecord(ev_zero, H->m_comp));
  HIP_OK(hipStreamWaitEvent(H->m_help, ev_zero, 0));
  if (!serial) HIP_OK(art::launch_helpers(K, n, in, so, helpers, -1, 1, words + HW_STATS, H->m_help));
  if (trace) std::fprintf(stderr, "[art-host] t=%.2f counters zeroed, helpers launched\n", clk() - t_start);
  return ART_OK;
}

bool StreamCall::helpers_in() const {
  return serial || __atomic_load_n(H->hsig + HSIG_STARTED, __ATOMIC_ACQUIRE) >= (unsigned long long)helpers;
}

// A call in flight launches its init pass and integrator only once the previous call's integrator
// is fully resident (its last-starting wave stores ticket + 1 into its lane's word) or that call
// has ended: launched earlier, both integrators' blocks took the slots the call before them freed,
// ran side by side at half speed each, and their downloads and scatters piled up at the end
// (1.25e6 rays: calls of 28 instead of 14 ms, profiles/r05t_ab_helpers.txt). Bounded: 200 ms.
bool StreamCall::prev_resident() const {
  if (!overlap || ticket <= 0 || c->done_ticket.load() >= ticket - 1 || clk() - t_start > 200.0) return true;
  for (const HostLane& O : c->lanes) {
    unsigned long long* const os = __atomic_load_n(&O.hsig, __ATOMIC_ACQUIRE);
    if (&O != H && os && __atomic_load_n(os + HSIG_RESIDENT, __ATOMIC_ACQUIRE) >= (unsigned long long)ticket)
      return true;
  }
  return false;
}

// The init pass, the integrator and (a lone call) the final pass on the integrator's stream, with
// the launch's ring entry around them.
int StreamCall::launch_main() {
  std::lock_guard<std::mutex> rlk(g_ring_mu);
  int r = take_slot(c, &L);
  if (r) return r;
  L->held.store(true, std::memory_order_release);  // until this call latches it (or leaves early)
  // every block slot initialises the first upload unit's rays before the integrator starts, then
  // the helpers keep ahead. (Round 4 took 258k rays, two per integrator lane: the first unit alone
  // left the integrator waiting on 8 helpers, 33 ms against 18 per 1.25e6-ray call. With the
  // units gathered from the call's start, the helpers keep up, and the first unit alone starts
  // the integrator ~1 ms sooner: 1.25e6 rays 17.2 -> 16.2 ms, 1e7 95.3 -> 94.1 ms, two boxes,
  // profiles/r05l_init_pass_sweep.txt. ART_HOST_INIT_RAYS: tests and A/B, another amount)
  const int64_t first =
      serial ? n : std::min(n, (int64_t)std::max(1, env_int("ART_HOST_INIT_RAYS", (int)(ulo[1] - ulo[0]))));
  if (env_int("ART_HOST_INITPASS", 1))  // (dev: 0 leaves the first piece to the helpers)
    HIP_OK(art::launch_helpers(K, n, in, so, iblocks, first, 0, words + HW_STATS, H->m_comp));
  HIP_OK(hipEventRecord(L->ev0, H->m_comp));
  art::LaunchPlan ran;
  if (overlap && ticket >= 0) {  // (see prev_resident)
    so.resident_host = H->hsig_dev + HSIG_RESIDENT;
    so.resident_value = (unsigned long long)ticket + 1ull;
    so.waves_total = (int32_t)std::min((n + 255) / 256, (int64_t)iblocks) * 4;
  }
  HIP_OK(art::launch_integrator_streamed(K, n, in, so, max_crossings, words + HW_QUEUE, words + HW_STATS, iblocks, H->m_comp,
                                         &ran));
  L->grid = ran.bulk_grid;
  L->path = art::plan_record(ran, true);
  HIP_OK(hipEventRecord(L->ev1, H->m_comp));
  if (final_pass) {
    HIP_OK(art::launch_helpers(K, n, in, so, slots, -1, 0, words + HW_STATS, H->m_comp));
    hipEvent_t ev_help = H->pev[nu + np + 1];  // (the persistent helpers' init counts, in the statistics)
    HIP_OK(hipEventRecord(ev_help, H->m_help));
    HIP_OK(hipStreamWaitEvent(H->m_comp, ev_help, 0));
    HIP_OK(hipMemcpyAsync(L->host_stats, words + HW_STATS, sizeof(unsigned long long) * art::N_STATS_DEV,
                          hipMemcpyDeviceToHost, H->m_comp));
  }
  // (overlapping calls: the statistics come from the helpers' completion words, and nothing
  // after the integrator waits on this stream for CU slots the next call holds)
  HIP_OK(hipEventRecord(L->done, H->m_comp));
  L->stream = H->m_comp;
  L->pending = true;
  c->last = c->next;
  c->next = (c->next + 1) % RING;
  c->launches += 1;
  launched = true;
  return ART_OK;
}

// the integrator, once every helper block is resident: before the uploads when they are at once
// (a lone call), else from the upload loop as soon as they are (a call overlapping the previous
// one, whose blocks hold the slots until its drain)
int StreamCall::launch_if_resident() {
  if ((helpers_in() && prev_resident()) || !overlap) {
    const double tw = clk();
    while (!helpers_in()) {
      if (clk() - tw > 5000.0) break;  // (never seen: the device is shared or wedged; handled in launch_late)
      std::this_thread::sleep_for(std::chrono::microseconds(5));
    }
    int rc;
    if (helpers_in() && (rc = launch_main())) return rc;
    if (trace) std::fprintf(stderr, "[art-host] t=%.2f helpers resident (%.2f ms), integrator launched\n", clk() - t_start,
                            clk() - tw);
  }
  return ART_OK;
}

// a host thread raises the ready counter as each unit's copies land
void StreamCall::start_readier() {
  readier.t = std::thread([this] {
    std::atomic<bool>& stop = readier.stop;
    for (int u = 0; u < nu && !stop.load(); ++u) {
      while (recorded.load(std::memory_order_acquire) <= u && !stop.load()) std::this_thread::sleep_for(std::chrono::microseconds(5));
      if (stop.load()) break;
      hipError_t q;  // (polled every 5 us, as the piece flags are)
      while ((q = hipEventQuery(ev_up[u])) == hipErrorNotReady && !stop.load())
        std::this_thread::sleep_for(std::chrono::microseconds(5));
      if (stop.load()) break;
      if (q != hipSuccess) {
        ready_err = 1;
        break;
      }
      __atomic_store_n(hready, (unsigned long long)ulo[u + 1], __ATOMIC_RELEASE);
      if (trace) std::fprintf(stderr, "[art-host] t=%.2f unit %d ready\n", clk() - t_start, u);
    }
  });
}

// downloads of the finished pieces, in order; scatters of the landed ones. Returns how many steps
// it made, or -1 after a HIP error.
int StreamCall::progress() {
  int moved = 0;
  while (dk < np && __atomic_load_n(hflag + dk, __ATOMIC_ACQUIRE) != 0ull) {
    if (!direct) {
      const int64_t m = piece_lo(dk + 1) - piece_lo(dk);
      if (hipMemcpyAsync((char*)po + blob_off(dk), (char*)dout + blob_off(dk), art::blob_bytes(m, cap), hipMemcpyDeviceToHost,
                         H->m_dn) != hipSuccess ||
          hipEventRecord(ev_dn[dk], H->m_dn) != hipSuccess)
        return -1;
    }
    if (trace) std::fprintf(stderr, "[art-host] t=%.2f piece %d done\n", clk() - t_start, dk);
    ++dk;
    ++moved;
  }
  while (sk < dk) {
    const hipError_t q = direct ? hipSuccess : hipEventQuery(ev_dn[sk]);
    if (q == hipErrorNotReady) break;
    if (q != hipSuccess) return -1;
    const double t0 = clk();
    const int64_t lo = piece_lo(sk), m = piece_lo(sk + 1) - lo;
    copy_pool().run(scatter_segs((const char*)po + blob_off(sk), m, cap, lo, n, *out, xc));
    if (trace) std::fprintf(stderr, "[art-host] t=%.2f piece %d scattered (%.2f ms)\n", t0 - t_start, sk, clk() - t0);
    ++sk;
    ++moved;
  }
  return moved;
}

// Submits each unit once it is gathered (the gatherer is ahead of the H2D copies), with the
// integrator's launch and the pieces' progress in between. Returns nonzero after an error.
int StreamCall::upload_loop() {
  int perr = 0;
  for (int u = 0; u < nu && !perr; ++u) {
    if (!launched && helpers_in() && prev_resident() && launch_main() != ART_OK) perr = 1;
    while (!perr && gathered.load(std::memory_order_acquire) <= u) {
      if (progress() < 0) perr = 1;
      if (!launched && helpers_in() && prev_resident() && launch_main() != ART_OK) perr = 1;
      std::this_thread::sleep_for(std::chrono::microseconds(5));
    }
    if (perr) break;
    if (u == 0 && early0) {  // (the gatherer submitted it)
      perr |= early0_err.load();
    } else {
      perr |= !submit_unit(u);
      if (trace) std::fprintf(stderr, "[art-host] t=%.2f unit %d submitted%s\n", clk() - t_start, u,
                              launched ? "" : " (integrator not launched yet)");
    }
    recorded.store(u + 1, std::memory_order_release);
    if (!perr && progress() < 0) perr = 1;
  }
  return perr;
}

// the helpers wait for CU slots the previous call still holds: the integrator after the uploads
int StreamCall::launch_late(int perr) {
  if (!perr && !launched) {
    const double tw = clk();
    while (!(helpers_in() && prev_resident()) && clk() - tw < 5000.0) {
      if (progress() < 0) break;
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    if (!helpers_in()) {
      std::fprintf(stderr, "[art] maskless streamed pipeline: helper blocks did not start; running the batch again\n");
      perr = 1;
    } else if (launch_main() != ART_OK) {
      perr = 1;
    }
  }
  return perr;
}

// (trace) the device counters, read back on the download stream
void StreamCall::trace_counters() {
  if (hipMemcpyAsync(peek, words, HW_TRACE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, H->m_dn) != hipSuccess ||
      hipStreamSynchronize(H->m_dn) != hipSuccess)
    return;
  unsigned long long fin = 0, tiles = 0;
  for (int k = 0; k < np; ++k) {
    fin += peek[HW_PIECE_CNT + k];
    tiles += peek[HW_PIECE_FIN + k];
  }
  std::fprintf(stderr, "[art-host] t=%.1f queue %llu init_next %llu fin_next %llu misses %llu finished %llu tiles %llu flags:",
               clk() - t_start, peek[HW_QUEUE], peek[HW_INIT_NEXT], peek[HW_FIN_NEXT], peek[HW_MISSES], fin, tiles);
  for (int k = 0; k < np; ++k) std::fprintf(stderr, "%llu", hflag[k]);
  std::fprintf(stderr, " ready %llu started %llu abort %u init-pass %s integrator %s\n", *hready, hflag[HSIG_NFLAG],
               *H->abort_host, hipEventQuery(L->ev0) == hipSuccess ? "done" : "running",
               hipEventQuery(L->ev1) == hipSuccess ? "done" : "running");
}

// Waits for every piece to be scattered, then for the helpers' completion words. Returns whether
// the call gave up: after an error, the abort word, or ART_HOST_STREAM_TIMEOUT_MS without progress.
bool StreamCall::wait_pieces(int perr) {
  if (trace) std::fprintf(stderr, "[art-host] t=%.2f uploads submitted\n", clk() - t_start);
  const double limit_ms = (double)env_int("ART_HOST_STREAM_TIMEOUT_MS", 30000);
  t_last = clk();
  double t_peek = clk();
  bool gave_up = perr != 0;
  bool int_logged = false;  // (trace)
  if (trace && hipHostMalloc((void**)&peek, HW_TRACE_WORDS * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
    peek = nullptr;
  while (!gave_up && sk < np) {
    if (peek && clk() - t_peek > (double)env_int("ART_HOST_PEEK_MS", 100)) {
      t_peek = clk();
      trace_counters();
    }
    if (trace && !int_logged && launched && hipEventQuery(L->ev1) == hipSuccess) {
      int_logged = true;
      std::fprintf(stderr, "[art-host] t=%.2f integrator done\n", clk() - t_start);
    }
    const int mv = progress();
    if (mv < 0 || ready_err.load()) {
      gave_up = true;
      break;
    }
    if (mv > 0) {
      t_last = clk();
      continue;
    }
    if (__atomic_load_n(H->abort_host, __ATOMIC_ACQUIRE) != 0u || clk() - t_last > limit_ms) {
      gave_up = true;
      break;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
  // the call's end: the helpers' completion words (the statistics, the flux), raised by the last
  // serving helper block once every integrator wave has counted itself (bounded like the pieces)
  if (!gave_up) {
    while (__atomic_load_n(hdone, __ATOMIC_ACQUIRE) == 0ull) {
      if (__atomic_load_n(H->abort_host, __ATOMIC_ACQUIRE) != 0u || clk() - t_last > limit_ms) {
        gave_up = true;
        break;
      }
      std::this_thread::sleep_for(std::chrono::microseconds(10));
    }
  }
  return gave_up;
}

// Stop the launch, then leave the batch to another path: every wait of the helpers and the
// waves ends on the abort word, and a helper that sees it drains the work queue (queue_word),
// so the integrator stops at each wave's next chunk claim. (The ready counter is NOT raised:
// helpers would initialise tiles whose inputs never landed)
int StreamCall::give_up() {
  if (peek) (void)hipHostFree(peek);
  __atomic_store_n(H->abort_host, 1u, __ATOMIC_RELEASE);
  readier.join();
  (void)hipStreamSynchronize(H->m_up);
  (void)hipStreamSynchronize(H->m_comp);
  (void)hipStreamSynchronize(H->m_help);
  (void)hipStreamSynchronize(H->m_dn);
  (void)hipGetLastError();
  if (trace) {  // the device counters at the give-up
    std::vector<unsigned long long> w(HW_TRACE_WORDS);
    if (hipMemcpy(w.data(), words, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
      std::fprintf(stderr, "[art-host] queue %llu init_next %llu fin_next %llu\n", w[HW_QUEUE], w[HW_INIT_NEXT], w[HW_FIN_NEXT]);
      for (int k = 0; k < np; ++k)
        std::fprintf(stderr, "[art-host] piece %d finished %llu finalized tiles %llu flag %llu\n", k, w[HW_PIECE_CNT + k],
                     w[HW_PIECE_FIN + k], hflag[k]);
    }
  }
  std::fprintf(stderr, "[art] maskless streamed pipeline gave up at piece %d of %d (abort=%u); running the batch again\n",
               sk, np, *H->abort_host);
  return STREAM_FALLBACK;
}

// the flux and the statistics of a call whose pieces are all in the caller's arrays
int StreamCall::finish() {
  readier.join();
  if (trace) std::fprintf(stderr, "[art-host] maskless total %.2f ms (%d pieces of 2^%d, %d of 2^%d)\n", clk() - t_start, pcs.ncoarse,
                          pcs.shift, np - pcs.ncoarse, pcs.fine_shift);
  if (peek) (void)hipHostFree(peek);  // (after the total: freeing pinned memory takes ~0.6 ms)
  const bool complete = __atomic_load_n(hdone, __ATOMIC_ACQUIRE) == 1ull;
  if (fx.nbins && hflux && complete) {
    for (int b = 0; b < 2 * fx.nbins; ++b) {
      const unsigned long long v = __atomic_load_n(hdone + art::DONE_FLUX + b, __ATOMIC_ACQUIRE);
      std::memcpy(fx.hist + b, &v, sizeof(double));
    }
  } else if (fx.nbins) {  // flux kernels over the pieces' blobs, once the integrator is done
    if (hflux) HIP_OK(hipMemsetAsync(hist_dev, 0, 2 * (size_t)fx.nbins * sizeof(double), H->m_comp));
    for (int k = 0; k < np; ++k) {
      const int64_t lo = piece_lo(k), m = piece_lo(k + 1) - lo;
      const art_segment_out v = blob_view((char*)dout + blob_off(k), m, 0).out;
      HIP_OK(art::launch_flux(K, m, v.x_end, v.k_end, v.status, in.species + lo, nullptr, fx.nbins, hist_dev, H->m_comp));
    }
    HIP_OK(hipMemcpyAsync(fx.hist, hist_dev, 2 * (size_t)fx.nbins * sizeof(double), hipMemcpyDeviceToHost, H->m_comp));
    HIP_OK(hipStreamSynchronize(H->m_comp));
  }
  if (complete && !final_pass) {  // the statistics from the completion words
    unsigned long long st[art::N_STATS_DEV];
    for (int i = 0; i < art::N_STATS_DEV; ++i) st[i] = __atomic_load_n(hdone + art::DONE_STATS + i, __ATOMIC_ACQUIRE);
    return latch_launch(c, L, st);
  }
  if (!final_pass) {  // (the helpers' copy timed out: the statistics as the stream has them)
    HIP_OK(hipMemcpyAsync(L->host_stats, words + HW_STATS, sizeof(unsigned long long) * art::N_STATS_DEV, hipMemcpyDeviceToHost,
                          H->m_comp));
    HIP_OK(hipStreamSynchronize(H->m_comp));
  }
  return finish_timing_slot(c, L);
}

// The steps of a call, in their order.
int StreamCall::run() {
  int rc;
  plan();
  if ((rc = stage())) return rc;
  reset_signals();
  start_gatherer();
  if ((rc = zero_counters())) return rc;
  fill_segout();
  if ((rc = launch_helpers()) || (rc = launch_if_resident())) return rc;
  start_readier();
  const int perr = launch_late(upload_loop());
  const bool gave_up = wait_pieces(perr);
  readier.stop = true;
  return gave_up ? give_up() : finish();
}

}  // namespace

int propagate_host_stream(DeviceCtx* c, HostLane* H, bool overlap, int64_t ticket, const art_params* p, int64_t n,
                          const double* x0, const double* k0, const double* erg, const double* dw, const double* ln_t0,
                          const int8_t* species, int32_t max_crossings, art_segment_out* out, art_crossing_buf* xc,
                          const FluxArgs& fx) {
  StreamCall call(StreamArgs{c, H, overlap, ticket, p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, fx});
  return call.run();
}

// The asynchronous calls' workers: one thread per host lane, one call at a time.
static void lane_worker(DeviceCtx* c, HostLane* H) {
  (void)hipSetDevice(c->device);
  for (;;) {
    std::function<int()> job;
    {
      std::unique_lock<std::mutex> lk(H->m);
      H->cv.wait(lk, [&] { return H->stop || (bool)H->job; });
      if (!H->job) return;  // (stop, nothing left)
      job = std::move(H->job);
      H->job = nullptr;
    }
    job();
    {
      std::lock_guard<std::mutex> lk(H->m);
      H->busy = false;
    }
    H->cv.notify_all();
  }
}

// Ticket t runs on lane t % HOST_LANES once that lane's previous call has ended; its result waits
// in c->results for art_host_wait.
static int64_t submit_async(DeviceCtx* c, std::function<int(HostLane*, int64_t)> body) {
  const int64_t t = c->next_ticket++;
  HostLane* H = &c->lanes[t % HOST_LANES];
  {
    std::lock_guard<std::mutex> lk(c->res_m);
    c->pending.insert(t);
  }
  {
    std::unique_lock<std::mutex> lk(H->m);
    H->cv.wait(lk, [&] { return !H->busy; });
    H->busy = true;
    H->job = [c, H, t, body] {
      g_err.clear();
      const int rc = body(H, t);
      for (int64_t d = c->done_ticket.load(); d < t && !c->done_ticket.compare_exchange_weak(d, t);) {
      }
      std::lock_guard<std::mutex> lk2(c->res_m);
      c->results[t] = {rc, g_err};
      c->res_cv.notify_all();
      return rc;
    };
    if (!H->worker.joinable()) H->worker = std::thread(lane_worker, c, H);
  }
  H->cv.notify_all();
  return t;
}

}  // namespace host
}  // namespace art

using namespace art::host;

extern "C" {

int art_propagate_host_flux_async(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                                  const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                                  art_segment_out* out, art_crossing_buf* xc, int32_t nbins, double* hist, int64_t* ticket) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!ticket) return fail(ART_E_INVALID, "ticket is NULL");
  if (nbins < 1) return fail(ART_E_INVALID, "nbins must be >= 1");
  FluxArgs fx;
  fx.nbins = nbins;
  fx.hist = hist;
  bool empty = false;
  int rc = host_args(p, n, x0, k0, erg, dw, ln_t0, species, out, xc, TrajArgs(), fx, &empty);
  if (rc) return rc;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  if (empty || host_path(p, n, TrajArgs()) != HP_STREAM) {
    // (a batch the streamed pipeline does not take runs now, in this thread; its ticket is complete)
    const int rc1 = empty ? ART_OK : propagate_host_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc,
                                                          TrajArgs(), fx);
    const std::string e1 = g_err;
    *ticket = submit_async(c, [rc1, e1](HostLane*, int64_t) {
      g_err = e1;
      return rc1;
    });
    return ART_OK;
  }
  g_host_cnt[HC_CALLS] += 1;
  const art_params pc = *p;  // (the caller's structs by value: they may go out of scope before the call ends)
  art_segment_out oc = *out;
  const bool has_xc = xc != nullptr;
  art_crossing_buf xcc = has_xc ? *xc : art_crossing_buf{};
  *ticket = submit_async(c, [=](HostLane* H, int64_t t) mutable {
    int r = propagate_host_stream(c, H, true, t, &pc, n, x0, k0, erg, dw, ln_t0, species, max_crossings, &oc,
                                    has_xc ? &xcc : nullptr, fx);
    if (r == STREAM_FALLBACK) {  // the batch again as one launch, on this lane's stream and staging
      g_host_cnt[HC_GIVEUPS] += 1;
      g_host_cnt[HC_SINGLE] += 1;
      if (fx.nbins) std::fill(fx.hist, fx.hist + 2 * (size_t)fx.nbins, 0.0);
      r = propagate_host_single(c, H->m_comp, H->pool, 4, &pc, n, x0, k0, erg, dw, ln_t0, species, max_crossings, &oc,
                                has_xc ? &xcc : nullptr, TrajArgs(), fx);
    } else if (r == ART_OK) {
      g_host_cnt[HC_STREAMED] += 1;
    }
    return r;
  });
  return ART_OK;
}

int art_host_wait(int64_t ticket) {
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  std::unique_lock<std::mutex> lk(c->res_m);
  if (!c->pending.count(ticket)) return fail(ART_E_INVALID, "unknown ticket, or one already waited for");
  c->res_cv.wait(lk, [&] { return c->results.count(ticket) > 0; });
  const std::pair<int, std::string> r = c->results[ticket];
  c->results.erase(ticket);
  c->pending.erase(ticket);
  if (r.first != ART_OK) g_err = r.second;
  return r.first;
}

}  // extern "C"
