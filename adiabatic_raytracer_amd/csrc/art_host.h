// art_host.h -- what the host units of libart.so share (the kernel units do not include it): the
// device context with its launch ring, pools and host lanes, the error macro, and the helpers that
// cross units. The units, each holding its share of the extern "C" boundary (include/art.h):
//   art_context.cpp      contexts, the ring, pools, the copy pool, shutdown, the setters and getters
//   art_device.cpp       the device launch layout (propagate_device_impl), art_propagate_*_device,
//                        art_grow_trees_device
//   art_host_stream.cpp  the streamed host call (StreamCall), the host lanes' workers, the
//                        asynchronous entry points
//   art_host_paths.cpp   the chunked and single-launch host paths, art_propagate_*_host
//   art_post.cpp         sampling, weights, flux, sky maps, event rows, the eval entry points
//   art_rccl.cpp         the flux reduction across ranks
// Host-pointer entry points (what a Julia ccall passes) stage through pooled device buffers on the
// library's own HIP streams; device-pointer entry points run asynchronously on the caller's stream.
// No torch types cross the boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/art.h"
#include "art_core.h"
#include "art_internal.h"
#include "art_host_plan.h"
#include "art_launch_plan.h"

namespace art {
namespace host {

// g_mu: every entry point (the calls of one process are serialised); g_ring_mu: the launch ring
// and the latched statistics, which the asynchronous host calls' worker threads also touch
// (they never take g_mu, so a caller holding it may wait for them)
extern std::mutex g_mu, g_ring_mu;
extern thread_local std::string g_err;
extern double g_last_ms;
extern unsigned long long g_last_stats[art::N_STATS];
extern int g_last_grid;
extern art_launch_path g_last_path;  // (art_last_launch_path: latched with the statistics)
// What the art_propagate_host* calls ran as (art_host_path_counters): calls, streamed
// pipeline completions, streamed give-ups (each batch then ran again as one launch), chunked
// pipeline calls, single-launch calls
enum { HC_CALLS, HC_STREAMED, HC_GIVEUPS, HC_CHUNKED, HC_SINGLE, HC_N };
extern std::atomic<uint64_t> g_host_cnt[HC_N];

// One propagate launch's bookkeeping: the HIP events around the integrator kernel, an event
// after its statistics were copied to pinned host memory, and that memory. A ring of them per
// device lets launches on different streams be in flight together; a slot is reused only after
// its previous launch completed.
constexpr int RING = 64;
// The words a device launch copies back: its statistics (head words 1 .. N_STATS_DEV) and, in the
// same copy, its record words (head words 16 .. 23: the donated, second-level, graduated and hot
// counts and their queue heads), so host_stats[w - 1] is head word w.
constexpr int HOST_WORDS = 23;
enum { HS_DONATED = 15, HS_DONATED2 = 17, HS_GRAD_COUNT = 19, HS_HOT_COUNT = 21, HS_HOT_QUEUE = 22 };
struct LaunchRec {
  hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
  hipEvent_t hot_fork = nullptr, hot_join = nullptr;  // the hot rays' side launch (art::HotSide)
  unsigned long long* host_stats = nullptr;  // HOST_WORDS words (pinned): statistics, the clock stamps, the record words
  int grid = 0;
  art_launch_path path{};  // the launch's plan as a record (plan_record); the counts are filled in when it is latched
  hipStream_t stream = nullptr;
  bool pending = false;
  // an asynchronous host call holds its record from its launch until it latches it at its end
  // (latch_launch / finish_timing_slot): take_slot skips a held record, so the ring wrapping
  // under other launches cannot hand it out twice
  std::atomic<bool> held{false};
};

struct Pinned {
  void* p = nullptr;
  size_t bytes = 0;
  unsigned flags = 0;
};
using PoolVec = std::vector<std::pair<void*, size_t>>;

// One set of the maskless streamed pipeline's resources (StreamCall, art_host_stream.cpp): the
// integrator's and the helpers' CU-masked streams (a hardware queue each), the two copy
// streams, the host words the GPU polls and raises, the pinned and device staging and the
// events. A context has HOST_LANES of them, so that many host calls can be in flight at once
// (art_propagate_host_flux_async: the next batch's uploads and first rays overlap this one's
// drain); lane 0 also serves the synchronous calls, which first wait for every async call.
constexpr int HOST_LANES = 2;
struct HostLane {
  hipStream_t m_comp = nullptr, m_up = nullptr, m_dn = nullptr, m_help = nullptr;
  unsigned long long* hsig = nullptr;  // the words of HostSignal (art_host_plan.h)
  unsigned long long* hsig_dev = nullptr;
  unsigned int* abort_host = nullptr;  // the word the waves and helpers raise (or read) when a call gives up
  unsigned int* abort_dev = nullptr;
  std::vector<hipEvent_t> pev;
  std::vector<Pinned> pinned;  // [0] gathered inputs, [1] output blobs
  PoolVec pool;                // [0] inputs, [1] output blobs, [2] scratch, [3] flux; [4..] the single-launch fallback
  // the asynchronous calls' worker: one job at a time, results kept by ticket until waited for
  std::thread worker;
  std::mutex m;
  std::condition_variable cv;
  std::function<int()> job;
  bool busy = false, stop = false;
};

struct DeviceCtx {
  int device = -1;
  hipStream_t stream = nullptr;  // the *_host entry points' stream
  LaunchRec ring[RING];
  int next = 0, last = -1;       // next ring slot; the most recent propagate launch
  int64_t launches = 0;          // propagate launches issued so far
  int32_t donate = -1;           // tail donation (art_set_tail_donation): lanes per wave, 0 = off, -1 = by geometry
  int32_t graduate = -1;         // graduation (art_set_graduation): attempts, 0 = off, -1 = the default (2048)
  int32_t sampler_waves = 0;     // art_set_sampler_waves: 0 = by line length, 2 or 3
  // the side stream of each stream that propagate launches ran on (the hot rays' tail launch,
  // art::HotSide): one per caller stream, so a launch waits on no other stream's hot rays
  std::map<hipStream_t, hipStream_t> hot_side;
  std::vector<std::pair<void*, size_t>> pool;  // host-entry staging buffers (grow-only, used under g_mu by the
                                               // synchronous *_host calls only)
  // the chunked host pipeline of art_propagate_host (propagate_host_chunked): its compute
  // streams, one stream for the uploads and one for the chunks' finalize kernels, its pinned
  // input and output staging (grow-only) and two events per chunk (inputs in HBM, outputs in
  // pinned memory)
  std::vector<hipStream_t> pstreams;
  hipStream_t h2d = nullptr, fin = nullptr;
  std::vector<Pinned> pinned;
  std::vector<hipEvent_t> pev;
  HostLane lanes[HOST_LANES];
  // asynchronous host calls: tickets in submission order (ticket t runs on lane t % HOST_LANES);
  // finished calls' results until art_host_wait takes them
  std::atomic<int64_t> next_ticket{0};
  std::atomic<int64_t> done_ticket{-1};  // the highest ticket whose call has ended
  std::mutex res_m;
  std::condition_variable res_cv;
  std::set<int64_t> pending;  // submitted, not yet waited for
  std::map<int64_t, std::pair<int, std::string>> results;
};

int fail(int code, const char* fmt, const char* a = "", const char* b = "");

#define HIP_OK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return ::art::host::fail(ART_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// ---- art_context.cpp ----
int current_ctx(DeviceCtx** out);
void shutdown_locked();
// The next launch record: waits for the launch that used the slot RING launches ago.
int take_slot(DeviceCtx* c, LaunchRec** out);
int pool_get_v(PoolVec& pool, size_t slot, size_t bytes, void** p);
int pool_get(DeviceCtx* c, size_t slot, size_t bytes, void** p);
int pinned_get_v(std::vector<Pinned>& pinned, size_t slot, size_t bytes, void** p, unsigned flags = hipHostMallocDefault);
int pinned_get(DeviceCtx* c, size_t slot, size_t bytes, void** p, unsigned flags = hipHostMallocDefault);
// Device scratch of ONE launch, allocated and freed in the order of its stream (hipMallocAsync /
// hipFreeAsync), so concurrent launches never share a work-queue word or a state buffer.
int scratch_alloc(hipStream_t s, size_t bytes, void** p);
// A stream on a hardware queue of its own (a stream with a CU mask gets one; the mask holds every
// CU): plain streams share the process's few queues (GPU_MAX_HW_QUEUES), and a stream queued behind
// a kernel that waits for it never runs (profiles/r04p_maskless_hwqueue.txt).
int own_queue_stream(DeviceCtx* c, hipStream_t* s);
int env_int(const char* name, int dflt);
double env_double(const char* name, double dflt);
inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
int validate(const art_params* p);
art::KParams kparams(const art_params& p);

// Host-side copies of the host pipelines (caller arrays <-> pinned staging): a few persistent
// worker threads share each batch of row segments, so gathering one chunk's inputs and scattering
// another's outputs runs at the host's memory bandwidth, not one core's.
class CopyPool {
 public:
  explicit CopyPool(int nthreads);
  ~CopyPool();
  // copies every segment; pieces of at most 1 MiB are shared by the workers and the caller (one
  // caller at a time: the asynchronous calls' workers take turns)
  void run(const std::vector<Seg>& segs);

 private:
  static constexpr size_t PIECE = size_t(1) << 20;
  void work();
  void loop();
  std::vector<std::thread> th_;
  std::mutex run_m_;
  std::vector<Seg> pieces_;
  std::atomic<size_t> next_{0};
  std::mutex m_;
  std::condition_variable cv_, done_;
  unsigned long long gen_ = 0;
  int busy_ = 0;
  bool stop_ = false;
};
CopyPool& copy_pool();

// saveat outputs (art_propagate_traj_*): ntimes >= 2 points per ray, or none (ntimes = 0)
// ... or the cyclotron observation's outputs (art_propagate_cyclotron_*; not with saveat)
struct TrajArgs {
  int32_t ntimes = 0;
  double *traj = nullptr, *t = nullptr;
  int32_t* count = nullptr;
  const art_cyclotron_out* cyc = nullptr;
  bool none() const { return ntimes == 0 && !cyc; }
};

// art_propagate_host_flux: the batch's binned radiated flux (flux_kernel over the outputs while
// they are still in HBM), 2 * nbins doubles into the caller's `hist`; nbins = 0: none
struct FluxArgs {
  int32_t nbins = 0;
  double* hist = nullptr;
};

// Argument checks shared by the host and device entry points, before any device call (the
// host path stages buffers of n elements, so a bad n or a NULL buffer must stop it first).
// Returns ART_OK with *empty set for n == 0 (nothing to do, nothing written).
int check_segment_args(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                       const double* dw, const double* ln_t0, const int8_t* species, const art_segment_out* out,
                       const art_crossing_buf* xc, const TrajArgs& tr, bool* empty);

// Latch one propagate launch (L; null: the most recent): its integrator kernel's duration and
// statistics, once it has completed.
int finish_timing_slot(DeviceCtx* c, LaunchRec* Lp);
int finish_timing(DeviceCtx* c);
// Latch several propagate launches (the chunks of one host call) as one: their integrator
// kernels' summed durations and summed statistics.
int finish_timing_sum(DeviceCtx* c, const std::vector<int>& slots);
// Latch one launch's statistics (the ring entry's, for art_recent_kernel_*; and the "last
// launch" figures of art_last_stats / art_last_kernel_ms) from words the host already holds.
int latch_launch(DeviceCtx* c, LaunchRec* L, const unsigned long long* st);

// ---- art_device.cpp ----
// Options of one propagate launch beyond the entry points' arguments (the host paths' own
// use): the tail-donation lanes (-1: the device's setting), caller-provided scratch of
// propagate_scratch_bytes() bytes (null: from the stream-ordered pool), and NaN in the
// crossing slots without a crossing (finalize_kernel writes them, the *_host contract).
struct LaunchOpts {
  int donate = -1;
  void* scratch = nullptr;
  size_t scratch_bytes = 0;  // the size of `scratch` (checked against the launch's layout)
  bool nan_fill = false;
  hipStream_t finalize_stream = nullptr;  // finalize_kernel on this stream (after the integrator)
  LaunchRec** launch_out = nullptr;       // the launch's ring entry (finish_timing_slot)
};

// this launch's scratch: [queue head + statistics (256 B) | u0: U0_REC n doubles of fresh state
// (init_kernel -> the integrator) | END_REC n doubles of end records | X_REC cap n doubles of
// crossing records (the integrator -> finalize_kernel) | donation records of two levels, the
// graduation and early-graduation records (and the latter's ready words) | the claim order's sort]
struct ScratchLayout {
  size_t head = 256, u0b = 0, recb = 0, xrb = 0, ncont = 0, nhot = 0, contb = 0, ordb = 0;
  size_t total() const { return head + u0b + recb + xrb + contb + ordb; }
};
int scratch_layout(DeviceCtx* c, int64_t n, int cap, int32_t donate, ScratchLayout* L, bool small_tail = false);
bool use_small_tail(const art_params* p, int64_t n, const TrajArgs& tr);

// *_device entry points run on the caller's stream exactly as given: NULL is the HIP null
// stream (torch's default stream), so the library orders correctly with the caller's
// work. Only the *_host entry points use the library's own streams.
int propagate_device_impl(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                          const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                          art_segment_out* out, art_crossing_buf* xc, void* stream, const TrajArgs& tr = TrajArgs(),
                          const LaunchOpts& opt = LaunchOpts(), DeviceCtx* cx = nullptr);

// What one art_grow_trees_device (or art_event_gather_photons_device) call holds until it returns:
// its stream-ordered device blocks and the pinned word the per-round count lands in.
struct TreeScratch {
  hipStream_t s = nullptr;
  void* block = nullptr;
  void* log = nullptr;
  int32_t* host = nullptr;  // [0] the next round's batch size, [1] the overflow word
  ~TreeScratch() {
    if (log) (void)hipFreeAsync(log, s);
    if (block) (void)hipFreeAsync(block, s);
    if (host) (void)hipHostFree(host);
  }
};

// ---- art_host_stream.cpp ----
// The streamed pipeline gave up (a wave waited too long for its inputs, or a piece for its
// signal): the call's results are discarded and the batch runs again on another path.
constexpr int STREAM_FALLBACK = 1 << 20;
int propagate_host_stream(DeviceCtx* c, HostLane* H, bool overlap, int64_t ticket, const art_params* p, int64_t n,
                          const double* x0, const double* k0, const double* erg, const double* dw, const double* ln_t0,
                          const int8_t* species, int32_t max_crossings, art_segment_out* out, art_crossing_buf* xc,
                          const FluxArgs& fx);

// ---- art_host_paths.cpp ----
enum HostPath { HP_STREAM, HP_CHUNKED, HP_SINGLE };
HostPath host_path(const art_params* p, int64_t n, const TrajArgs& htr);
int host_args(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg, const double* dw,
              const double* ln_t0, const int8_t* species, art_segment_out* out, art_crossing_buf* xc, const TrajArgs& htr,
              const FluxArgs& fx, bool* empty);
int propagate_host_single(DeviceCtx* c, hipStream_t s, PoolVec& pool, size_t pb, const art_params* p, int64_t n,
                          const double* x0, const double* k0, const double* erg, const double* dw, const double* ln_t0,
                          const int8_t* species, int32_t max_crossings, art_segment_out* out, art_crossing_buf* xc,
                          const TrajArgs& htr, const FluxArgs& fx);
int propagate_host_impl(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                        const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                        art_segment_out* out, art_crossing_buf* xc, const TrajArgs& htr, const FluxArgs& fx = FluxArgs());

}  // namespace host
}  // namespace art
