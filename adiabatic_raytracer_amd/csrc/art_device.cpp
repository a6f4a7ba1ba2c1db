// art_device.cpp -- the device launch: one propagate launch's scratch layout and kernels on the
// caller's stream (propagate_device_impl, which the host paths use too), the art_propagate_*_device
// entry points and the device-resident tree driver (declared in include/art.h).
#include <algorithm>
#include <cmath>
#include <string>

#include "art_host.h"

namespace art {
namespace host {

// The environment's share of a launch's plan, read once per launch (tests switch the variables):
// ART_SMALL_TAIL, ART_TAIL, ART_TAIL_DONATE, ART_W1, ART_GRADUATE, ART_HOT_AT, ART_HOT_ORDER.
static void plan_env(art::LaunchPlanIn* in) {
  const char* e = std::getenv("ART_SMALL_TAIL");
  in->small_tail_set = e && *e;
  in->small_tail_max = in->small_tail_set ? std::atoll(e) : 0;
  in->tail_rays = env_int("ART_TAIL", 1);
  in->tail_donate = std::min(63, std::max(1, env_int("ART_TAIL_DONATE", 4)));
  e = std::getenv("ART_W1");  // the 1-wave/SIMD builds are on unless ART_W1=0
  in->w1 = !(e && e[0] == '0');
  in->graduate_env = env_int("ART_GRADUATE", 2048);
  in->hot_at_env = env_int("ART_HOT_AT", 128);
  in->hot_order = env_int("ART_HOT_ORDER", 1) != 0;
}

// The inputs of a launch's plan (art_launch_plan.h) but for its stream and its kernel's occupancy.
// Tail donation by default goes by geometry: a Schwarzschild batch is bound by its few longest rays
// (configs[3]: ray 717277 takes 23 592 attempts), which a lone pass would run on one lane of a
// draining wave (13.5 us per attempt); donated, they finish on the one-wave-per-ray tail kernel
// (7.7 us). A flat lone pass has no such ray, and donation costs its drain 0.5-1.3%.
static int plan_inputs(DeviceCtx* c, const art_params* p, int64_t n, const TrajArgs& tr, int donate_caller,
                       art::LaunchPlanIn* in) {
  in->n = n;
  in->integrator = p->integrator;
  in->geom = art::geom_of(kparams(*p));
  in->save = tr.ntimes >= 2;
  in->cyc = tr.cyc != nullptr;
  in->donate_caller = donate_caller;
  in->donate_device = c->donate;
  in->graduate_device = c->graduate;
  HIP_OK(hipDeviceGetAttribute(&in->ncu, hipDeviceAttributeMultiprocessorCount, c->device));
  plan_env(in);
  return ART_OK;
}

// A small Vern6 batch without saveat, in flat space or Schwarzschild, runs every ray on a wave of its own (tail_kernel): the
// latency of a Julia host's per-event calls (its rays run ~40% faster per attempt than a lone
// lane of the persistent integrator), bit-identical results. One decision (lp_small_tail) for the
// launch and for every caller that lays out a launch's scratch ahead of it (the chunked host pipeline).
bool use_small_tail(const art_params* p, int64_t n, const TrajArgs& tr) {
  art::LaunchPlanIn in;
  in.n = n;
  in.integrator = p->integrator;
  in.geom = art::geom_of(kparams(*p));
  in.save = tr.ntimes != 0;
  in.cyc = tr.cyc != nullptr;
  in.small_tail_set = true;
  in.small_tail_max = art::small_tail_limit();
  return art::lp_small_tail(in);
}

int scratch_layout(DeviceCtx* c, int64_t n, int cap, int32_t donate, ScratchLayout* L, bool small_tail) {
  const size_t nd = (size_t)n;
  L->u0b = nd * art::U0_REC * sizeof(double);
  L->recb = nd * art::END_REC * sizeof(double);
  L->xrb = (size_t)cap * nd * art::X_REC * sizeof(double);
  // tail donation: at most (resident waves) x donate records of CONT_REC doubles; a small batch
  // sent to the tail kernel: one record per ray
  int ncu = 0;
  if (!small_tail && donate > 0) HIP_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
  L->ncont = art::lp_ncont(n, ncu, donate, small_tail);
  // the second level (the packed continuation's own donations, resumed by the tail kernel):
  // never more than the first level's; then as many graduation records (SegOut::grad) and the
  // early-graduation records (SegOut::hot) and their ready words
  L->nhot = art::lp_nhot(L->ncont, small_tail);
  L->contb = ((small_tail ? 2 : 3) * L->ncont + L->nhot) * art::CONT_REC * sizeof(double) + L->nhot * sizeof(unsigned);
  // (then the claim order's sort, SegOut::order)
  L->ordb = L->nhot ? art::claim_order_bytes(n) + 256 : 0;
  return ART_OK;
}

int propagate_device_impl(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                          const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                          art_segment_out* out, art_crossing_buf* xc, void* stream, const TrajArgs& tr,
                          const LaunchOpts& opt, DeviceCtx* cx) {
  bool empty = false;
  int rc = check_segment_args(p, n, x0, k0, erg, dw, ln_t0, species, out, xc, tr, &empty);
  if (rc || empty) return rc;
  DeviceCtx* c = cx;
  if (!c && (rc = current_ctx(&c))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const art::KParams K = kparams(*p);
  const int cap = (xc && xc->count) ? xc->capacity : 0;
  // the launch's plan (art_launch_plan.h): every choice below and in launch_propagate is one of its
  // fields. (Early graduation only on a non-blocking stream: its side stream is a blocking one, and
  // work on a blocking stream -- the null stream above all -- would wait for the hot launch, which
  // waits for this launch's own kernels.)
  art::LaunchPlanIn pin;
  if ((rc = plan_inputs(c, p, n, tr, opt.donate, &pin))) return rc;
  unsigned sflags = 0;
  pin.nonblocking = s != nullptr && hipStreamGetFlags(s, &sflags) == hipSuccess && (sflags & hipStreamNonBlocking);
  const art::LaunchPlan plan = art::plan_launch(pin);
  const bool small_tail = plan.small_tail;
  const int32_t donate = plan.donate;
  ScratchLayout SL;
  if ((rc = scratch_layout(c, n, cap, donate, &SL, small_tail))) return rc;
  if (opt.scratch && SL.total() > opt.scratch_bytes)
    return fail(ART_E_INVALID, "caller scratch of %s bytes is smaller than the launch needs (%s)",
                std::to_string(opt.scratch_bytes).c_str(), std::to_string(SL.total()).c_str());
  const size_t head = SL.head, u0b = SL.u0b, recb = SL.recb, xrb = SL.xrb, ncont = SL.ncont;
  std::lock_guard<std::mutex> rlk(g_ring_mu);  // (the ring, up to this launch's entry in it)
  LaunchRec* L;
  if ((rc = take_slot(c, &L))) return rc;
  if (opt.launch_out) *opt.launch_out = L;
  void* blk = opt.scratch;
  if (!blk && (rc = scratch_alloc(s, SL.total(), &blk))) return rc;
  unsigned long long* words = (unsigned long long*)blk;
  double* u0 = (double*)((char*)blk + head);
  double* rec = (double*)((char*)blk + head + u0b);
  art::SegIn in{x0, k0, erg, dw, ln_t0, species, u0};
  art::SegOut so{out->x_end, out->k_end, out->u7_end, out->tau_end, out->status, out->n_accept, out->n_reject,
                 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (cap) {
    so.cap = cap;
    so.xcount = xc->count;
    so.xpos = xc->pos; so.xk = xc->k; so.xt = xc->t; so.xdw = xc->dw; so.xp = xc->p_nonad;
    so.xrec = (double*)((char*)blk + head + u0b + recb);
    so.nan_fill = opt.nan_fill ? 1 : 0;
  }
  if (tr.ntimes != 0) {
    so.ntimes = tr.ntimes;
    so.traj = tr.traj;
    so.traj_t = tr.t;
    so.traj_n = tr.count;
  }
  if (tr.cyc) {  // (the integrator adds to tau and count in place)
    so.cyc_tau = tr.cyc->tau;
    so.cyc_count = tr.cyc->count;
    so.cyc_pos = tr.cyc->pos;
    so.cyc_lnt = tr.cyc->ln_t;
    HIP_OK(hipMemsetAsync(so.cyc_tau, 0, (size_t)n * sizeof(double), s));
    HIP_OK(hipMemsetAsync(so.cyc_count, 0, (size_t)n * sizeof(int32_t), s));
  }
  so.rec = rec;
  art::HotSide hot;
  if (ncont) {
    so.cont = (double*)((char*)blk + head + u0b + recb + xrb);
    so.cont_count = words + 16;  // head words 16 .. 19 (zeroed with the head)
    so.cont_queue = words + 17;
    so.cont2 = so.cont + ncont * art::CONT_REC;
    so.cont2_count = words + 18;
    so.cont2_queue = words + 19;
    if (plan.grad_cap > 0) {
      // graduation of a pass's outlier rays to the tail kernel (ART_GRADUATE attempts, default
      // 2048 -- about 23x the mean GR ray, never reached by a flat one; 0 = off;
      // profiles/r04av_graduation_threshold.txt): the records' place, which launch_propagate hands
      // to the kernels where the tail kernel runs (plan.grad_records)
      so.grad = so.cont2 + ncont * art::CONT_REC;
      so.grad_count = words + 20;
      so.grad_queue = words + 21;
      so.grad_cap = plan.grad_cap;
      // (the caller's setting, art_set_graduation: a host that keeps several passes in flight turns
      // it off -- each graduated ray then holds a whole tail wave while the other passes fill the
      // CUs it would free, profiles/r04al_graduation_in_flight.txt; round 4 decided this per launch
      // from the other streams' events, which made it depend on host timing)
      so.graduate = plan.graduate;
      // early graduation (SegOut::hot), with graduation only: from ART_HOT_AT attempts (default
      // 128) a ray whose progress in ln t is below ART_HOT_DTAU + ART_HOT_SLOPE log2(attempts /
      // 256) (defaults 15.95, 0.75): on configs[3] 102 rays, 90 of them past 5000 attempts, among
      // them every one of the 20 longest (tools/exp_gr_predict.py)
      if (plan.hot_records) {
        so.hot = so.grad + ncont * art::CONT_REC;
        so.hot_ready = (unsigned*)(so.hot + SL.nhot * art::CONT_REC);
        so.hot_count = words + 22;
        so.hot_queue = words + 23;
        so.hot_done = (unsigned*)(words + 26);
        so.hot_cap = plan.hot_cap;
        so.hot_at = plan.hot_at;
        so.hot_dtau = env_double("ART_HOT_DTAU", 15.95);
        so.hot_slope = env_double("ART_HOT_SLOPE", 0.75);
        if (plan.sorted) {  // (256-byte aligned)
          const uintptr_t o = (uintptr_t)blk + SL.total() - SL.ordb;
          so.order_tmp = (void*)((o + 255) & ~(uintptr_t)255);
        }
        auto it = c->hot_side.find(s);
        if (it == c->hot_side.end()) {
          // a hardware queue of its own: a plain stream may share one with s, and s's kernels would
          // then queue behind the hot launch that waits for them (own_queue_stream, lane_setup)
          hipStream_t hsd = nullptr;
          if ((rc = own_queue_stream(c, &hsd))) return rc;
          it = c->hot_side.emplace(s, hsd).first;
        }
        hot.stream = it->second;
        hot.fork = L->hot_fork;
        hot.join = L->hot_join;
        hot.zero_word = words + 24;  // (words 22 .. 26: zeroed with the head)
      }
    }
    so.donate = donate;
    so.small_tail = small_tail ? 1 : 0;
  }
  HIP_OK(hipMemsetAsync(words, 0, head, s));
  if (so.hot_ready) HIP_OK(hipMemsetAsync(so.hot_ready, 0, SL.nhot * sizeof(unsigned), s));
  art::LaunchPlan ran;  // the plan with its grids from the bulk kernel's occupancy: what was launched
  HIP_OK(art::launch_propagate(K, n, in, so, max_crossings, words, words + 1, s, pin, &ran, L->ev0, L->ev1,
                               opt.finalize_stream, hot));
  L->grid = ran.small_tail ? ran.tail_grid : ran.bulk_grid;
  L->path = art::plan_record(ran, false);
  L->path.grad_cap = ran.grad_records ? (uint64_t)ran.grad_cap : 0;
  L->path.hot_cap = ran.hot ? (uint64_t)ran.hot_cap : 0;
  // (the statistics and, in the same copy, the launch's record words: head words 1 .. HOST_WORDS)
  HIP_OK(hipMemcpyAsync(L->host_stats, words + 1, sizeof(unsigned long long) * HOST_WORDS, hipMemcpyDeviceToHost, s));
  HIP_OK(hipEventRecord(L->done, s));
  if (!opt.scratch) HIP_OK(hipFreeAsync(blk, s));
  L->stream = s;
  L->pending = true;
  c->last = c->next;
  c->next = (c->next + 1) % RING;
  c->launches += 1;
  return ART_OK;
}

}  // namespace host
}  // namespace art

using namespace art::host;

extern "C" {

int art_propagate_device(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                         const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                         art_segment_out* out, art_crossing_buf* xc, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return propagate_device_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, stream);
}

int art_propagate_cyclotron_device(const art_params* p, int64_t n, const double* x0, const double* k0,
                                   const double* erg, const double* dw, const double* ln_t0, const int8_t* species,
                                   int32_t max_crossings, art_segment_out* out, art_crossing_buf* xc,
                                   const art_cyclotron_out* cyc, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!cyc) return fail(ART_E_INVALID, "cyc is NULL");
  TrajArgs tr;
  tr.cyc = cyc;
  return propagate_device_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, stream, tr);
}

int art_propagate_traj_device(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                              const double* dw, const double* ln_t0, const int8_t* species, int32_t max_crossings,
                              art_segment_out* out, art_crossing_buf* xc, int32_t ntimes, double* traj,
                              double* traj_t, int32_t* traj_n, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (ntimes < 2) return fail(ART_E_INVALID, "ntimes must be >= 2");
  TrajArgs tr;
  tr.ntimes = ntimes; tr.traj = traj; tr.t = traj_t; tr.count = traj_n;
  return propagate_device_impl(p, n, x0, k0, erg, dw, ln_t0, species, max_crossings, out, xc, stream, tr);
}

// get_tree for n roots with every tree's state in HBM (art_tree_step.h, the tree kernels of
// art_kernels.hip): per round one pack, one batched propagate (propagate_device_impl: the
// small-batch path, donation and graduation as for any device launch), one step and one scan on
// `stream`; the host reads the next round's batch size and nothing else. g_mu is held while work is
// enqueued and released while the host waits for a round, so other streams' calls go on.
int art_grow_trees_device(const art_params* p, int64_t n, const double* x0, const double* k0, const double* erg,
                          const int8_t* species, const art_tree_opts* opts, int64_t node_capacity, art_tree_node* nodes,
                          int64_t* node_start, int32_t* counts, int32_t* infos, int64_t* n_nodes, void* stream) {
  std::unique_lock<std::mutex> lk(g_mu);
  if (!p) return fail(ART_E_INVALID, "params is NULL");
  if (!opts) return fail(ART_E_INVALID, "opts is NULL");
  if (!n_nodes) return fail(ART_E_INVALID, "n_nodes is NULL");
  if (n < 0 || n > 2147483647LL) return fail(ART_E_INVALID, "n must be in [0, 2^31)");
  if (n > 0 && (!x0 || !k0 || !erg || !species)) return fail(ART_E_INVALID, "input buffers must be non-NULL");
  if (opts->max_nodes < 0) return fail(ART_E_INVALID, "max_nodes must be >= 0");
  if (opts->crossing_cap < 0) return fail(ART_E_INVALID, "crossing_cap must be >= 0");
  const bool split_all = opts->splittings_cutoff > 0;
  if (split_all && opts->num_cutoff > 0)
    return fail(ART_E_INVALID, "splittings_cutoff > 0 with num_cutoff > 0 has no device form (art_grow_trees grows such trees)");
  int rc = validate(p);
  if (rc) return rc;
  *n_nodes = 0;
  if (n == 0 && !node_start) return ART_OK;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    HIP_OK(hipMemsetAsync(node_start, 0, sizeof(int64_t), s));
    HIP_OK(hipStreamSynchronize(s));
    return ART_OK;
  }
  const art::KParams K = kparams(*p);
  art::TreeRules R{};
  R.num_cutoff = opts->num_cutoff;
  R.mc_nodes = opts->mc_nodes;
  R.max_nodes = opts->max_nodes;
  R.split_all = split_all ? 1 : 0;
  R.cap = split_all ? std::max(1, opts->crossing_cap) : 1;
  const int64_t depth = art::tree_stack_capacity(opts->mc_nodes, opts->max_nodes, split_all);
  R.stack_cap = (int32_t)depth;
  R.tree_offset = opts->tree_offset;
  R.seed = opts->seed;
  R.prob_cutoff = opts->prob_cutoff;
  R.rNS = p->rNS;
  const double dt0 = std::exp(-30.0);  // NumerPass[1] = ln_t_start = -30 (MainRunner.jl:410)
  const double ln_dt0 = std::log(dt0);  // the double the host forest passes for its roots

  // one block: [state | stacks | two lists, flag, pos | counts (n + 1) | node_start (n + 1) | overflow
  // word | scan scratch | the round's batch], each part 256-byte aligned
  const size_t nd = (size_t)n, cap = (size_t)R.cap;
  size_t off = 0;
  auto part = [&off](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
  };
  const size_t o_state = part(nd * sizeof(art::TreeState)), o_stack = part(nd * (size_t)depth * sizeof(art::TreeEv));
  const size_t o_list0 = part(nd * 4), o_list1 = part(nd * 4), o_flag = part(nd * 4), o_pos = part(nd * 4);
  const size_t o_counts = part((nd + 1) * 4), o_start = part((nd + 1) * 8), o_err = part(4);
  const size_t tmp_bytes = art::tree_scan_bytes(n), o_tmp = part(tmp_bytes);
  const size_t o_in = part(9 * nd * 8), o_sp = part(nd), o_out = part(8 * nd * 8), o_int = part(4 * nd * 4);
  const size_t o_xc = part(9 * cap * nd * 8);
  TreeScratch ts;
  ts.s = s;
  if ((rc = scratch_alloc(s, off, &ts.block))) return rc;
  if (hipHostMalloc((void**)&ts.host, 64, hipHostMallocDefault) != hipSuccess) return fail(ART_E_NOMEM, "hipHostMalloc failed");
  char* b = (char*)ts.block;
  art::TreeState* state = (art::TreeState*)(b + o_state);
  art::TreeEv* stack = (art::TreeEv*)(b + o_stack);
  int32_t *cur = (int32_t*)(b + o_list0), *nxt = (int32_t*)(b + o_list1);
  int32_t *flag = (int32_t*)(b + o_flag), *pos = (int32_t*)(b + o_pos), *counts1 = (int32_t*)(b + o_counts);
  int32_t* err = (int32_t*)(b + o_err);
  double *din = (double*)(b + o_in), *dout = (double*)(b + o_out), *dxc = (double*)(b + o_xc);
  int32_t* dint = (int32_t*)(b + o_int);
  HIP_OK(hipMemsetAsync(err, 0, 4, s));
  HIP_OK(art::launch_tree_roots(K, R, n, x0, k0, erg, species, state, stack, cur, flag, pos, s));

  int64_t log_cap = split_all ? n : 3 * n, total = 0;
  if ((rc = scratch_alloc(s, (size_t)log_cap * sizeof(art_tree_node), &ts.log))) return rc;
  const int64_t max_rounds = (int64_t)opts->max_nodes + 2;
  int64_t m_prev = n, m = n;
  for (int64_t round = 0; m > 0; ++round) {
    if (round >= max_rounds) return fail(ART_E_HIP, "the forest did not end within max_nodes + 2 rounds");
    if (total + m > log_cap) {  // grow the node log (kept across rounds; the flatten reads it whole)
      const int64_t want = std::max(2 * log_cap, total + m);
      void* bigger = nullptr;
      if ((rc = scratch_alloc(s, (size_t)want * sizeof(art_tree_node), &bigger))) return rc;
      HIP_OK(hipMemcpyAsync(bigger, ts.log, (size_t)total * sizeof(art_tree_node), hipMemcpyDeviceToDevice, s));
      HIP_OK(hipFreeAsync(ts.log, s));
      ts.log = bigger;
      log_cap = want;
    }
    // this round's batch of m segments: SoA with stride m inside the buffers sized for n
    const size_t md = (size_t)m;
    art::TreeBatch B{};
    B.x0 = din; B.k0 = din + 3 * md; B.erg = din + 6 * md; B.dw = din + 7 * md; B.lnt0 = din + 8 * md;
    B.species = (int8_t*)(b + o_sp);
    B.x_end = dout; B.k_end = dout + 3 * md; B.u7_end = dout + 6 * md; B.tau_end = dout + 7 * md;
    B.status = dint; B.n_acc = dint + md; B.n_rej = dint + 2 * md; B.xcount = dint + 3 * md;
    B.xpos = dxc; B.xk = dxc + 3 * cap * md; B.xt = dxc + 6 * cap * md; B.xdw = dxc + 7 * cap * md; B.xp = dxc + 8 * cap * md;
    HIP_OK(art::launch_tree_pack(R, m_prev, m, cur, flag, pos, nxt, state, stack, B, dt0, ln_dt0, s));
    art_segment_out so{B.x_end, B.k_end, B.u7_end, B.tau_end, B.status, B.n_acc, B.n_rej};
    art_crossing_buf xb{R.cap, B.xcount, B.xpos, B.xk, B.xt, B.xdw, B.xp};
    if ((rc = propagate_device_impl(p, m, B.x0, B.k0, B.erg, B.dw, B.lnt0, B.species, opts->splittings_cutoff, &so, &xb,
                                    stream)))
      return rc;
    HIP_OK(art::launch_tree_step(K, R, n, m, nxt, state, stack, B, (art_tree_node*)ts.log + total, flag, pos, err,
                                 b + o_tmp, tmp_bytes, s));
    total += m;
    HIP_OK(hipMemcpyAsync(ts.host, pos + (m - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    lk.unlock();
    const hipError_t we = hipStreamSynchronize(s);
    lk.lock();
    if (we != hipSuccess) return fail(ART_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(we));
    m_prev = m;
    m = ts.host[0];
    if (m < 0 || m > m_prev) return fail(ART_E_HIP, "the forest's round count is out of range");
    std::swap(cur, nxt);
  }
  *n_nodes = total;
  const bool fits = nodes && total <= node_capacity;
  if (fits) {
    int64_t* ns = node_start ? node_start : (int64_t*)(b + o_start);
    HIP_OK(art::launch_tree_finish(R, n, state, counts1, counts, infos, ns, b + o_tmp, tmp_bytes, s));
    HIP_OK(art::launch_tree_flatten(total, (const art_tree_node*)ts.log, ns, node_capacity, nodes, s));
  }
  HIP_OK(hipMemcpyAsync(ts.host + 1, err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  lk.unlock();
  const hipError_t we = hipStreamSynchronize(s);
  lk.lock();
  if (we != hipSuccess) return fail(ART_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(we));
  if (ts.host[1]) return fail(ART_E_INVALID, "a tree's event stack left its bound (art_tree_step.h): no result");
  if (!fits && total > node_capacity)
    return fail(ART_E_NOMEM, "node_capacity is too small: %s nodes", std::to_string(total).c_str());
  return ART_OK;
}

}  // extern "C"
