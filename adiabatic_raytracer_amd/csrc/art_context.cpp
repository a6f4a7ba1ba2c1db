// art_context.cpp -- the state every host unit of libart.so shares (art_host.h): the device
// contexts with their launch rings and staging pools, the copy pool, the latched statistics,
// shutdown; and the small entry points that set or read them (declared in include/art.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "art_host.h"

namespace art {
namespace host {

std::mutex g_mu, g_ring_mu;
thread_local std::string g_err;
double g_last_ms = 0.0;
unsigned long long g_last_stats[art::N_STATS] = {0};
int g_last_grid = 0;
art_launch_path g_last_path{};
std::atomic<uint64_t> g_host_cnt[HC_N] = {};
// (pointers: a context never moves, so a worker thread may hold one while another device's is created)
std::vector<std::unique_ptr<DeviceCtx>> g_ctx;
static std::mutex g_ctx_mu;

int fail(int code, const char* fmt, const char* a, const char* b) {
  char buf[512];
  std::snprintf(buf, sizeof buf, fmt, a, b);
  g_err = buf;
  return code;
}

static void shutdown_at_exit();

int current_ctx(DeviceCtx** out) {
  // Release every HIP object of the library at exit, before the HIP runtime tears itself down:
  // handlers registered with atexit run in reverse order, and the runtime (loaded and
  // initialised before libart's first call) registered its teardown earlier. Left to static
  // destruction, the library's streams, signal memory and pinned buffers outlived the runtime
  // (and a profiler's finalisation), DESIGN.md §4 "exit".
  static bool at_exit = false;
  if (!at_exit) {
    std::atexit(shutdown_at_exit);
    at_exit = true;
  }
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  DeviceCtx* cp = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if ((int)g_ctx.size() <= dev) g_ctx.resize(dev + 1);
    if (!g_ctx[dev]) g_ctx[dev].reset(new DeviceCtx());
    cp = g_ctx[dev].get();
  }
  DeviceCtx& c = *cp;
  if (c.device < 0) {
    HIP_OK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    unsigned long long* hs = nullptr;
    HIP_OK(hipHostMalloc((void**)&hs, sizeof(unsigned long long) * HOST_WORDS * RING, hipHostMallocDefault));
    for (int i = 0; i < RING; ++i) {
      HIP_OK(hipEventCreate(&c.ring[i].ev0));
      HIP_OK(hipEventCreate(&c.ring[i].ev1));
      HIP_OK(hipEventCreateWithFlags(&c.ring[i].done, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&c.ring[i].hot_fork, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&c.ring[i].hot_join, hipEventDisableTiming));
      c.ring[i].host_stats = hs + i * HOST_WORDS;
    }
    // per-launch scratch comes from the stream-ordered allocator: keep what it frees cached
    // so a steady stream of launches does not go back to the driver
    hipMemPool_t mp;
    if (hipDeviceGetDefaultMemPool(&mp, dev) == hipSuccess) {
      uint64_t thr = ~0ull;
      (void)hipMemPoolSetAttribute(mp, hipMemPoolAttrReleaseThreshold, &thr);
    }
    c.device = dev;
  }
  *out = &c;
  return ART_OK;
}

// The next launch record: waits for the launch that used the slot RING launches ago.
int take_slot(DeviceCtx* c, LaunchRec** out) {
  for (int k = 0; k < RING && c->ring[c->next].held.load(std::memory_order_acquire); ++k) c->next = (c->next + 1) % RING;
  LaunchRec& L = c->ring[c->next];
  if (L.pending) {
    HIP_OK(hipEventSynchronize(L.done));
    L.pending = false;
  }
  *out = &L;
  return ART_OK;
}

int pool_get_v(PoolVec& pool, size_t slot, size_t bytes, void** p) {
  if (pool.size() <= slot) pool.resize(slot + 1, {nullptr, 0});
  auto& e = pool[slot];
  if (e.second < bytes) {
    if (e.first) HIP_OK(hipFree(e.first));
    e.first = nullptr;
    e.second = 0;
    if (hipMalloc(&e.first, bytes) != hipSuccess) return fail(ART_E_NOMEM, "hipMalloc of %s bytes failed", std::to_string(bytes).c_str());
    e.second = bytes;
  }
  *p = e.first;
  return ART_OK;
}

int pool_get(DeviceCtx* c, size_t slot, size_t bytes, void** p) { return pool_get_v(c->pool, slot, bytes, p); }

int pinned_get_v(std::vector<Pinned>& pinned, size_t slot, size_t bytes, void** p, unsigned flags) {
  if (pinned.size() <= slot) pinned.resize(slot + 1);
  auto& e = pinned[slot];
  if (e.bytes < bytes || e.flags != flags) {
    if (e.p) HIP_OK(hipHostFree(e.p));
    e.p = nullptr;
    e.bytes = 0;
    e.flags = flags;
    if (hipHostMalloc(&e.p, bytes, flags) != hipSuccess)
      return fail(ART_E_NOMEM, "hipHostMalloc of %s bytes failed", std::to_string(bytes).c_str());
    e.bytes = bytes;
  }
  *p = e.p;
  return ART_OK;
}

int pinned_get(DeviceCtx* c, size_t slot, size_t bytes, void** p, unsigned flags) {
  return pinned_get_v(c->pinned, slot, bytes, p, flags);
}

CopyPool::CopyPool(int nthreads) {
  for (int i = 0; i < nthreads; ++i) th_.emplace_back([this] { loop(); });
}
CopyPool::~CopyPool() {
  {
    std::lock_guard<std::mutex> lk(m_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& t : th_) t.join();
}
void CopyPool::run(const std::vector<Seg>& segs) {
  std::lock_guard<std::mutex> one(run_m_);
  pieces_.clear();
  for (const Seg& g : segs)
    for (size_t o = 0; o < g.bytes; o += PIECE)
      pieces_.push_back({(char*)g.dst + o, (const char*)g.src + o, std::min(PIECE, g.bytes - o)});
  if (pieces_.empty()) return;
  next_.store(0);
  {
    std::lock_guard<std::mutex> lk(m_);
    busy_ = (int)th_.size();
    ++gen_;
  }
  cv_.notify_all();
  work();
  std::unique_lock<std::mutex> lk(m_);
  done_.wait(lk, [this] { return busy_ == 0; });
}
void CopyPool::work() {
  for (size_t i; (i = next_.fetch_add(1)) < pieces_.size();) std::memcpy(pieces_[i].dst, pieces_[i].src, pieces_[i].bytes);
}
void CopyPool::loop() {
  unsigned long long seen = 0;
  for (;;) {
    {
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
    }
    work();
    std::lock_guard<std::mutex> lk(m_);
    if (--busy_ == 0) done_.notify_all();
  }
}

int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return (e && *e) ? std::atoi(e) : dflt;
}
double env_double(const char* name, double dflt) {
  const char* e = std::getenv(name);
  return (e && *e) ? std::atof(e) : dflt;
}

// (a heap object, not a function-local static: art_shutdown joins its threads before the HIP
// runtime's own teardown, and no static destructor of libart is left to run after it)
// Created under its own lock: the gatherer threads of two asynchronous calls may ask for it
// at the same time, outside g_mu.
static std::atomic<CopyPool*> g_copy_pool{nullptr};
static std::mutex g_copy_pool_mu;
CopyPool& copy_pool() {
  CopyPool* cp = g_copy_pool.load(std::memory_order_acquire);
  if (cp) return *cp;
  std::lock_guard<std::mutex> lk(g_copy_pool_mu);
  cp = g_copy_pool.load(std::memory_order_relaxed);
  // ART_HOST_THREADS: worker threads besides the caller (default 7)
  if (!cp) {
    cp = new CopyPool(std::max(0, env_int("ART_HOST_THREADS", 7)));
    g_copy_pool.store(cp, std::memory_order_release);
  }
  return *cp;
}

// Every HIP object a device context holds, released in dependency order (the streams drained
// first). Used by art_shutdown, which runs at exit ahead of the HIP runtime's teardown.
static void stop_workers(DeviceCtx& c) {
  for (HostLane& H : c.lanes) {
    if (!H.worker.joinable()) continue;
    {
      std::lock_guard<std::mutex> lk(H.m);
      H.stop = true;
    }
    H.cv.notify_all();
    H.worker.join();
  }
}

static void release_ctx(DeviceCtx& c) {
  if (c.device < 0) return;
  stop_workers(c);  // (each finishes its call first)
  (void)hipSetDevice(c.device);
  (void)hipDeviceSynchronize();
  for (LaunchRec& L : c.ring) {
    if (L.ev0) (void)hipEventDestroy(L.ev0);
    if (L.ev1) (void)hipEventDestroy(L.ev1);
    if (L.done) (void)hipEventDestroy(L.done);
    for (hipEvent_t e : {L.hot_fork, L.hot_join})
      if (e) (void)hipEventDestroy(e);
  }
  for (auto& e : c.hot_side) (void)hipStreamDestroy(e.second);
  if (c.ring[0].host_stats) (void)hipHostFree(c.ring[0].host_stats);  // one block for the ring
  for (auto& e : c.pool)
    if (e.first) (void)hipFree(e.first);
  for (auto& e : c.pinned)
    if (e.p) (void)hipHostFree(e.p);
  for (hipEvent_t e : c.pev) (void)hipEventDestroy(e);
  for (hipStream_t s : c.pstreams)
    if (s && s != c.stream) (void)hipStreamDestroy(s);
  for (hipStream_t s : {c.h2d, c.fin})
    if (s) (void)hipStreamDestroy(s);
  for (HostLane& H : c.lanes) {
    for (auto& e : H.pool)
      if (e.first) (void)hipFree(e.first);
    for (auto& e : H.pinned)
      if (e.p) (void)hipHostFree(e.p);
    for (hipEvent_t e : H.pev) (void)hipEventDestroy(e);
    for (hipStream_t s : {H.m_comp, H.m_up, H.m_dn, H.m_help})
      if (s) (void)hipStreamDestroy(s);
    if (H.hsig) (void)hipHostFree(H.hsig);
    if (H.abort_host) (void)hipHostFree(H.abort_host);
  }
  if (c.stream) (void)hipStreamDestroy(c.stream);
}

void shutdown_locked() {
  std::vector<std::unique_ptr<DeviceCtx>> all;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    all.swap(g_ctx);
  }
  for (auto& c : all)
    if (c) release_ctx(*c);
  all.clear();
  std::lock_guard<std::mutex> lk(g_copy_pool_mu);
  delete g_copy_pool.exchange(nullptr);
}

static void shutdown_at_exit() {
  // (a call still running on another thread at exit keeps its objects: releasing them under it
  // would be worse than leaving them to the runtime)
  if (!g_mu.try_lock()) return;
  shutdown_locked();
  g_mu.unlock();
}

int scratch_alloc(hipStream_t s, size_t bytes, void** p) {
  if (hipMallocAsync(p, bytes, s) != hipSuccess)
    return fail(ART_E_NOMEM, "hipMallocAsync of %s bytes failed", std::to_string(bytes).c_str());
  return ART_OK;
}

int own_queue_stream(DeviceCtx* c, hipStream_t* s) {
  int ncu_all = 0;
  HIP_OK(hipDeviceGetAttribute(&ncu_all, hipDeviceAttributeMultiprocessorCount, c->device));
  std::vector<uint32_t> all((ncu_all + 31) / 32, 0u);
  for (int i = 0; i < ncu_all; ++i) all[i / 32] |= 1u << (i % 32);
  HIP_OK(hipExtStreamCreateWithCUMask(s, (uint32_t)all.size(), all.data()));
  return ART_OK;
}

int validate(const art_params* p) {
  if (!p) return fail(ART_E_INVALID, "params is NULL");
  if (!p->melrose) return fail(ART_E_UNSUPPORTED, "melrose=0 (Ctheta_B_sphere form) is not supported; the reference hard-codes melrose=true (Gen_Samples.jl:167)");
  if (p->integrator != ART_VERN6 && p->integrator != ART_RK4) return fail(ART_E_INVALID, "unknown integrator");
  if (p->integrator == ART_RK4 && p->n_fixed < 1) return fail(ART_E_INVALID, "RK4 needs n_fixed >= 1");
  if (!(p->rNS > 0) || !(p->mass_a > 0) || !(p->omega_pul != 0)) return fail(ART_E_INVALID, "rNS, mass_a must be > 0 and omega_pul != 0");
  if (!(p->abstol > 0) || !(p->reltol >= 0)) return fail(ART_E_INVALID, "bad tolerances");
  if (p->maxiters < 1) return fail(ART_E_INVALID, "maxiters must be >= 1");
  if (p->interp_points > 65) return fail(ART_E_INVALID, "interp_points must be <= 65 (the reference uses 50)");
  return ART_OK;
}

// Kernel parameters. ART_SCAN_CERT=0 switches the certified scan steps of the integrator and
// of the sampler off (A/B tests: the results are bit-identical either way,
// tests/test_gpu_scan_cert.py).
art::KParams kparams(const art_params& p) {
  art::KParams K = art::make_kparams(p);
  if (const char* e = std::getenv("ART_SCAN_CERT"))
    if (e[0] == '0') K.cert_fac = __builtin_inf();
  return K;
}

int check_segment_args(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                       const double* dw, const double* ln_t0, const int8_t* species, const art_segment_out* out,
                       const art_crossing_buf* xc, const TrajArgs& tr, bool* empty) {
  int rc = validate(p);
  if (rc) return rc;
  if (n < 0 || n > 2147483647LL) return fail(ART_E_INVALID, "n must be in [0, 2^31)");
  if (!out || !out->x_end || !out->k_end || !out->u7_end || !out->tau_end || !out->status || !out->n_accept || !out->n_reject)
    return fail(ART_E_INVALID, "segment output buffers must be non-NULL");
  *empty = n == 0;
  if (n == 0) return ART_OK;
  if (!x0 || !k0 || !erg || !dw || !ln_t0 || !species) return fail(ART_E_INVALID, "input buffers must be non-NULL");
  const int cap = (xc && xc->count) ? xc->capacity : 0;
  if (cap && (cap < 1 || !xc->pos || !xc->k || !xc->t || !xc->dw || !xc->p_nonad))
    return fail(ART_E_INVALID, "crossing buffer incomplete");
  if (tr.ntimes != 0 && (tr.ntimes < 2 || !tr.traj || !tr.t || !tr.count))
    return fail(ART_E_INVALID, "saveat needs ntimes >= 2 and buffers");
  if (tr.cyc) {
    if (!tr.cyc->tau || !tr.cyc->count || !tr.cyc->pos || !tr.cyc->ln_t)
      return fail(ART_E_INVALID, "cyclotron output buffers must be non-NULL");
    if (p->integrator != ART_VERN6) return fail(ART_E_INVALID, "the cyclotron observation needs the Vern6 integrator");
    if (tr.ntimes != 0) return fail(ART_E_INVALID, "the cyclotron observation cannot be combined with saveat");
  }
  return ART_OK;
}

// A launch's record with its counts: the record words the launch copied back beside its statistics
// (the streamed call's integrator has none)
static art_launch_path path_with_counts(const LaunchRec& L) {
  art_launch_path r = L.path;
  if (r.streamed) return r;
  r.donated = L.host_stats[HS_DONATED];
  r.donated2 = L.host_stats[HS_DONATED2];
  r.grad_count = L.host_stats[HS_GRAD_COUNT];
  r.hot_count = L.host_stats[HS_HOT_COUNT];
  r.hot_claimed = L.host_stats[HS_HOT_QUEUE];
  return r;
}

int finish_timing_slot(DeviceCtx* c, LaunchRec* Lp) {
  std::lock_guard<std::mutex> rlk(g_ring_mu);
  if (!Lp && c->last < 0) return ART_OK;
  LaunchRec& L = Lp ? *Lp : c->ring[c->last];
  HIP_OK(hipEventSynchronize(L.done));
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, L.ev0, L.ev1));
  g_last_ms = ms;
  g_last_grid = L.grid;
  for (int i = 0; i < art::N_STATS; ++i) g_last_stats[i] = L.host_stats[i];
  g_last_path = path_with_counts(L);
  L.held.store(false, std::memory_order_release);
  return ART_OK;
}
int finish_timing(DeviceCtx* c) { return finish_timing_slot(c, nullptr); }

int finish_timing_sum(DeviceCtx* c, const std::vector<int>& slots) {
  std::lock_guard<std::mutex> rlk(g_ring_mu);
  double ms_sum = 0.0;
  unsigned long long st[art::N_STATS] = {0};
  int grid = 0;
  art_launch_path path{};  // the last launch's decisions, the counts summed (as the statistics are)
  for (int i : slots) {
    LaunchRec& L = c->ring[i];
    HIP_OK(hipEventSynchronize(L.done));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, L.ev0, L.ev1));
    ms_sum += ms;
    for (int k = 0; k < art::N_STATS; ++k) st[k] += L.host_stats[k];
    grid = std::max(grid, L.grid);
    const art_launch_path one = path_with_counts(L), sum = path;
    path = one;
    path.launches = sum.launches + one.launches;
    path.bulk_grid = std::max(sum.bulk_grid, one.bulk_grid);
    path.donated += sum.donated;
    path.donated2 += sum.donated2;
    path.grad_count += sum.grad_count;
    path.grad_cap += sum.grad_cap;
    path.hot_count += sum.hot_count;
    path.hot_cap += sum.hot_cap;
    path.hot_claimed += sum.hot_claimed;
  }
  g_last_path = path;
  g_last_ms = ms_sum;
  g_last_grid = grid;
  for (int k = 0; k < art::N_STATS; ++k) g_last_stats[k] = st[k];
  return ART_OK;
}

int latch_launch(DeviceCtx* c, LaunchRec* L, const unsigned long long* st) {
  std::lock_guard<std::mutex> rlk(g_ring_mu);
  for (int i = 0; i < art::N_STATS_DEV; ++i) L->host_stats[i] = st[i];
  HIP_OK(hipEventSynchronize(L->ev1));
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, L->ev0, L->ev1));
  g_last_ms = ms;
  g_last_grid = L->grid;
  for (int i = 0; i < art::N_STATS; ++i) g_last_stats[i] = st[i];
  g_last_path = path_with_counts(*L);
  L->held.store(false, std::memory_order_release);
  return ART_OK;
}

}  // namespace host
}  // namespace art

using namespace art::host;

extern "C" {

int art_abi_version(void) { return ART_ABI_VERSION; }
const char* art_last_error(void) { return g_err.c_str(); }

int art_device_count(int32_t* count) {
  int n = 0;
  HIP_OK(hipGetDeviceCount(&n));
  if (count) *count = n;
  return ART_OK;
}

int art_set_device(int32_t device) {
  std::lock_guard<std::mutex> lk(g_mu);
  HIP_OK(hipSetDevice(device));
  return ART_OK;
}

int art_set_tail_donation(int32_t lanes) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (lanes < -1 || lanes > 63) return fail(ART_E_INVALID, "tail donation lanes must be in [-1, 63]");
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  c->donate = lanes;
  return ART_OK;
}

int art_set_graduation(int32_t attempts) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (attempts < -1) return fail(ART_E_INVALID, "graduation attempts must be >= -1");
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  c->graduate = attempts;
  return ART_OK;
}

int art_set_sampler_waves(int32_t waves) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (waves != 0 && waves != 2 && waves != 3) return fail(ART_E_INVALID, "sampler waves must be 0, 2 or 3");
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  c->sampler_waves = waves;
  return ART_OK;
}

int art_synchronize(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  HIP_OK(hipStreamSynchronize(c->stream));
  HIP_OK(hipDeviceSynchronize());
  return finish_timing(c);
}

double art_last_kernel_ms(void) { return g_last_ms; }

// Statistics of the last propagate launch (after art_synchronize / a host entry point):
// [attempts, accepted, root re-steps, scan condition evals, interpolant-root evals, rays,
//  init RHS evals, reserved]; grid = persistent grid size.
int art_last_stats(uint64_t* stats, int32_t* grid) {
  for (int i = 0; i < art::N_STATS; ++i) stats[i] = g_last_stats[i];
  if (grid) *grid = g_last_grid;
  return ART_OK;
}

int art_last_launch_path(art_launch_path* out) {
  if (!out) return fail(ART_E_INVALID, "out is NULL");
  *out = g_last_path;
  return ART_OK;
}

// Integrator-kernel durations [ms] of the last min(n, issued, RING) propagate launches on the
// current device, oldest first (each from the HIP events around that launch on its own
// stream); waits for them. Returns the count written, or a negative ART_E* code.
int art_recent_kernel_ms(int32_t n, double* ms) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  if (n < 0 || (n > 0 && !ms)) return fail(ART_E_INVALID, "bad buffer");
  std::lock_guard<std::mutex> rlk(g_ring_mu);
  int64_t m = n;
  if (m > c->launches) m = c->launches;
  if (m > RING) m = RING;
  for (int64_t j = 0; j < m; ++j) {
    LaunchRec& L = c->ring[(int)(((int64_t)c->last - (m - 1 - j) + RING) % RING)];
    HIP_OK(hipEventSynchronize(L.done));
    float f = 0.f;
    HIP_OK(hipEventElapsedTime(&f, L.ev0, L.ev1));
    ms[j] = f;
  }
  return (int)m;
}

// The same launches' integrator spans [ms] from in-kernel clock stamps (first wave start to last
// wave end, s_memrealtime at 100 MHz; -1 where a launch left none). Returns the count written.
int art_recent_kernel_span_ms(int32_t n, double* ms) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  if (n < 0 || (n > 0 && !ms)) return fail(ART_E_INVALID, "bad buffer");
  std::lock_guard<std::mutex> rlk(g_ring_mu);
  int64_t m = n;
  if (m > c->launches) m = c->launches;
  if (m > RING) m = RING;
  for (int64_t j = 0; j < m; ++j) {
    LaunchRec& L = c->ring[(int)(((int64_t)c->last - (m - 1 - j) + RING) % RING)];
    HIP_OK(hipEventSynchronize(L.done));
    const unsigned long long t0 = ~L.host_stats[art::ST_T0], t1 = L.host_stats[art::ST_T1];
    // (-1 also for an asynchronous call still in flight: its stamps are latched at its end)
    ms[j] = (L.held.load(std::memory_order_acquire) || L.host_stats[art::ST_T0] == 0ull || t1 < t0)
                ? -1.0
                : (double)(t1 - t0) / art::STAMP_TICKS_PER_MS;
  }
  return (int)m;
}

int art_vern6_tableau(double* c, double* A, double* b, double* bhat) {
  using V = art::Vern6;
  const double cc[9] = {0.0, V::c2, V::c3, V::c4, V::c5, V::c6, V::c7, 1.0, 1.0};
  double AA[9][9] = {{0}};
  AA[1][0] = V::a21;
  AA[2][0] = V::a31; AA[2][1] = V::a32;
  AA[3][0] = V::a41; AA[3][2] = V::a43;
  AA[4][0] = V::a51; AA[4][2] = V::a53; AA[4][3] = V::a54;
  AA[5][0] = V::a61; AA[5][2] = V::a63; AA[5][3] = V::a64; AA[5][4] = V::a65;
  AA[6][0] = V::a71; AA[6][2] = V::a73; AA[6][3] = V::a74; AA[6][4] = V::a75; AA[6][5] = V::a76;
  AA[7][0] = V::a81; AA[7][2] = V::a83; AA[7][3] = V::a84; AA[7][4] = V::a85; AA[7][5] = V::a86; AA[7][6] = V::a87;
  AA[8][0] = V::a91; AA[8][3] = V::a94; AA[8][4] = V::a95; AA[8][5] = V::a96; AA[8][6] = V::a97; AA[8][7] = V::a98;
  const double bh[9] = {V::bh1, 0, 0, V::bh4, V::bh5, V::bh6, 0, V::bh8, V::bh9};
  for (int i = 0; i < 9; ++i) {
    c[i] = cc[i];
    b[i] = AA[8][i];
    bhat[i] = bh[i];
    for (int j = 0; j < 9; ++j) A[9 * i + j] = AA[i][j];
  }
  return ART_OK;
}

double art_find_conversion_surface(const art_params* p) {
  // Find_Conversion_Surface (RayTracer.jl:1250-1263) with fix_time = 0: ωp at the surface
  // point in the plane of the magnetic axis, then rNS (ωp/m_a)^(2/3) * 1.01.
  const double th = p->theta_m < art::PI / 2.0 ? p->theta_m / 2.0 : (p->theta_m + art::PI) / 2.0;
  const double x[3] = {p->rNS * std::sin(th), 0.0, p->rNS * std::cos(th)};
  const double r = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double ph = std::atan2(x[1], x[0]);
  const double t = std::acos(x[2] / r);
  const double psi = ph;
  const double Bn = p->B0 * std::pow(p->rNS / r, 3) / 2.0;
  const double Br = 2.0 * Bn * (std::cos(p->theta_m) * std::cos(t) + std::sin(p->theta_m) * std::sin(t) * std::cos(psi));
  const double Bt = Bn * (std::cos(p->theta_m) * std::sin(t) - std::sin(p->theta_m) * std::cos(t) * std::cos(psi));
  const double Bz = Br * std::cos(t) - Bt * std::sin(t);
  const double ne = std::fabs(2.0 * p->omega_pul * Bz / std::sqrt(4 * art::PI / 137) * 1.95e-2 * art::HBAR);
  const double wp = std::sqrt(4 * art::PI * ne / 137 / 5.0e5);
  return p->rNS * std::pow(wp / p->mass_a, 2.0 / 3.0) * 1.01;
}

int art_host_path_counters(uint64_t* counters, int32_t n, int32_t reset) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (n < 0 || (n > 0 && !counters)) return fail(ART_E_INVALID, "bad buffer");
  for (int i = 0; i < n && i < HC_N; ++i) counters[i] = g_host_cnt[i];
  for (int i = HC_N; i < n; ++i) counters[i] = 0;
  if (reset)
    for (auto& v : g_host_cnt) v = 0;
  return HC_N;
}

int art_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  shutdown_locked();
  return ART_OK;
}

}  // extern "C"
