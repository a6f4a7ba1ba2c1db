// art_post.cpp -- the entry points around the propagate calls (declared in include/art.h): the
// non-adiabatic probability, the sampler, event weights, flux histograms, sky maps, event rows, event moments, the coupling
// scan, the halo scan, the jackknife replicates, the coupling x halo grid, the event power spectrum, the exact tables and the eval entry points the tests compare against the oracle. Each checks its arguments, then
// launches on the caller's stream (or stages through the context's pool, the *_host ones).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>

#include "art_event_grid.h"
#include "art_event_moments.h"
#include "art_event_replicates.h"
#include "art_event_reweight.h"
#include "art_event_rows.h"
#include "art_event_spectrum.h"
#include "art_exact.h"
#include "art_host.h"

namespace art {
namespace host {

// An art_halo checked (no device is touched) and resolved for the kernels: v_prop <= 0 is
// sqrt(v0² + |v_ns|²).
static int halo_of(const art_halo* h, art::HaloK* K) {
  if (!std::isfinite(h->v0) || !(h->v0 > 0.0)) return fail(ART_E_INVALID, "halo: v0 must be finite and > 0");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(h->v_ns[i])) return fail(ART_E_INVALID, "halo: v_ns must be finite");
  if (std::isnan(h->v_prop)) return fail(ART_E_INVALID, "halo: v_prop must not be NaN");
  if (h->v_prop > 0.0 && h->v_prop < h->v0)
    return fail(ART_E_INVALID, "halo: v_prop must be >= v0 (the weights are unbounded below it)");
  K->v0 = h->v0;
  for (int i = 0; i < 3; ++i) K->v_ns[i] = h->v_ns[i];
  K->vp = h->v_prop > 0.0
              ? h->v_prop
              : std::sqrt(h->v0 * h->v0 + h->v_ns[0] * h->v_ns[0] + h->v_ns[1] * h->v_ns[1] + h->v_ns[2] * h->v_ns[2]);
  if (!(K->vp <= 3000.0))
    return fail(ART_E_INVALID, "halo: v_prop must be <= 3000 km/s (the largest draw is 6.1 v_prop, far below c)");
  return ART_OK;
}

static int sample_device_impl(const art_params* p, const art_halo* halo, double max_r, uint64_t seed, int64_t ray_offset,
                       int64_t n, double* x, double* k_init, double* erg_inf, double* vifty, int32_t* weights,
                       int32_t* attempts, hipStream_t s) {
  int rc = validate(p);
  if (rc) return rc;
  art::HaloK hk;
  if (halo && (rc = halo_of(halo, &hk))) return rc;
  if (n == 0) return ART_OK;
  if (n < 0 || n > 2147483647LL) return fail(ART_E_INVALID, "n must be in [0, 2^31)");
  if (!(max_r > p->rNS)) return fail(ART_E_INVALID, "max_r must exceed rNS (MainRunner.jl:389-396 quits otherwise)");
  if (!x || !k_init || !erg_inf || !vifty || !weights || !attempts) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  void* q = nullptr;  // this launch's work-queue word
  if ((rc = scratch_alloc(s, 256, &q))) return rc;
  HIP_OK(hipMemsetAsync(q, 0, sizeof(unsigned long long), s));
  HIP_OK(hipMemsetAsync(q, 0, 256, s));
  HIP_OK(art::launch_sample(kparams(*p), max_r, seed, ray_offset, n, x, k_init, erg_inf, vifty, weights,
                            attempts, (unsigned long long*)q, s, c->sampler_waves, halo ? &hk : nullptr));
#ifdef ART_SAMPLER_SECTIONS  // (dev build: the sampler's section cycles to stderr)
  {
    unsigned long long w[16];
    HIP_OK(hipMemcpyAsync(w, q, sizeof w, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    std::fprintf(stderr, "[sampler-sections] n=%lld setup %llu control %llu cert %llu grid %llu brackets %llu out %llu "
                 "grid_steps %llu steps %llu\n", (long long)n, w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15]);
  }
#endif
  HIP_OK(hipFreeAsync(q, s));
  return ART_OK;
}

static int event_weight_device_impl(const art_params* p, const art_halo* halo, double max_r, double rho_dm,
                             double mcmc_weight, int64_t n, const double* x, const double* k_init, const double* vifty,
                             double* out, hipStream_t s) {
  int rc = validate(p);
  if (rc) return rc;
  art::HaloK hk;
  if (halo && (rc = halo_of(halo, &hk))) return rc;
  if (n == 0) return ART_OK;
  if (n < 0) return fail(ART_E_INVALID, "n must be >= 0");
  if (!x || !k_init || !vifty || !out) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  HIP_OK(art::launch_event_weight(art::make_kparams(*p), n, x, k_init, vifty, max_r, rho_dm, mcmc_weight, out, s,
                                  halo ? &hk : nullptr));
  return ART_OK;
}

// The argument checks the two sky-map entry points share (no device is touched): the axes of a
// table of at most SKY_MAX_DOUBLES doubles, and a mode the table allows.
static int sky_axes(const int32_t nbins[3], const double lo[3], const double hi[3], bool c_all, int32_t mode,
                    art::SkyAxes* A) {
  if (mode < 0 || mode > 2) return fail(ART_E_INVALID, "sky map mode must be 0 (auto), 1 (LDS table) or 2 (global adds)");
  int64_t table = 2;
  for (int d = 0; d < 3; ++d) {
    if (nbins[d] < 1) return fail(ART_E_INVALID, "sky map bin counts must be >= 1");
    if (nbins[d] > art::SKY_MAX_DOUBLES / table) return fail(ART_E_INVALID, "sky map table exceeds 2^26 doubles");
    table *= nbins[d];
    A->n[d] = nbins[d];
    if (d == 2 && c_all) {
      A->lo[d] = A->hi[d] = 0.0;
      continue;
    }
    if (!std::isfinite(lo[d]) || !std::isfinite(hi[d]) || !(lo[d] < hi[d]))
      return fail(ART_E_INVALID, "sky map ranges need finite lo < hi");
    A->lo[d] = lo[d];
    A->hi[d] = hi[d];
  }
  A->c_all = c_all;
  if (mode == 1 && table > art::SKY_LDS_DOUBLES)
    return fail(ART_E_INVALID, "sky map mode 1: the table exceeds the LDS budget of 8192 doubles");
  return ART_OK;
}

// An art_sky_spec as the kernels take it. Without one (the event calls' optional map): a single bin, added to in
// HBM (mode 2).
struct EventSky {
  art::SkyAxes A{{1, 1, 1}, 1, {0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}};
  int cos_axis = 1, mode = 2;
  int64_t size = 0;  // the doubles of one table, 0 without a map
};
// honour_mode: the spec's mode is checked and kept, and with mode 1 the map must fit the LDS budget beside a flux
// table of nbins bins; else the tables are added to in HBM and the mode is not looked at.
static int event_sky(const art_sky_spec* spec, bool honour_mode, int32_t nbins, EventSky* S) {
  if (!spec) return ART_OK;
  if (spec->theta_axis != 0 && spec->theta_axis != 1)
    return fail(ART_E_INVALID, "theta_axis must be 0 (theta) or 1 (cos theta)");
  const int32_t nb[3] = {spec->n_theta, spec->n_phi, spec->n_dw};
  const double lo[3] = {spec->theta_axis ? -1.0 : 0.0, -art::PI, spec->dw_lo};
  const double hi[3] = {spec->theta_axis ? 1.0 : art::PI, art::PI, spec->dw_hi};
  const int rc = sky_axes(nb, lo, hi, spec->n_dw == 1, honour_mode ? spec->mode : 0, &S->A);
  if (rc) return rc;
  S->size = 2 * (int64_t)nb[0] * nb[1] * nb[2];
  if (honour_mode && spec->mode == 1 && S->size + 2 * nbins > art::SKY_LDS_DOUBLES)
    return fail(ART_E_INVALID, "sky map mode 1: the sky and flux tables exceed the LDS budget of 8192 doubles");
  S->cos_axis = spec->theta_axis;
  if (honour_mode) S->mode = spec->mode;
  return ART_OK;
}

// ---- The front end of the four event calls (rows, moments, coupling scan, halo scan): with event_sky above, the
// checks of an art_event_rows_in, the fill of EventRowsArgs, the scans' tables and the scratch carver. Each call
// keeps its own order of checks; where the calls differ on purpose the difference is a flag at the call site.

static int event_in_ranges(const art_event_rows_in* in) {
  if (in->n_events < 0) return fail(ART_E_INVALID, "n_events must be >= 0");
  if (in->n_nodes < 0 || in->n_nodes > 2147483647LL) return fail(ART_E_INVALID, "n_nodes must be in [0, 2^31)");
  return ART_OK;
}

static int event_out_ranges(int32_t reserved, int32_t nbins) {
  if (reserved != 0) return fail(ART_E_INVALID, "reserved must be 0");
  if (nbins < 0 || nbins > 4096) return fail(ART_E_INVALID, "nbins must be in [0, 4096]");
  return ART_OK;
}

static int need_node_start(const art_event_rows_in* in, const int64_t* node_start) {
  if (in->n_nodes > 0 && !node_start) return fail(ART_E_INVALID, "node_start is NULL");
  return ART_OK;
}

// What event_in_buffers asks beyond the buffers of a chunk that has nodes
enum : unsigned {
  IN_CYC_END_STATES = 1u,       // cyc_slot needs the re-run's end states too, not cyc_tau alone
  IN_EVENT_INPUTS_ALWAYS = 2u,  // x, k_init, weight5 and back are needed with n_nodes == 0 too
  IN_NODE_START_LATE = 4u,      // node_start is checked here, after the call's n_events == 0 return
};

// The buffers of an art_event_rows_in and its cyc_* rule: the last checks before the device
static int event_in_buffers(const art_event_rows_in* in, const int64_t* node_start, unsigned flags) {
  int rc;
  if ((flags & IN_NODE_START_LATE) && (rc = need_node_start(in, node_start))) return rc;
  const bool per_event = in->x && in->k_init && in->weight5 && in->back;
  const bool per_node = in->back_counts && in->nodes && in->counts && in->infos;
  if (((flags & IN_EVENT_INPUTS_ALWAYS) && !per_event) || (in->n_nodes > 0 && !(per_event && per_node)))
    return fail(ART_E_INVALID, "NULL input buffer");
  if (!in->cyc_slot) return ART_OK;
  const art_segment_out* ce = in->cyc_end;
  const bool tau = in->cyc_n == 0 || (in->cyc_n > 0 && in->cyc_tau);
  if (!(flags & IN_CYC_END_STATES)) return tau ? ART_OK : fail(ART_E_INVALID, "cyc_slot needs cyc_n >= 0 and cyc_tau");
  if (!tau || (in->cyc_n > 0 && (!ce || !ce->x_end || !ce->k_end || !ce->u7_end || !ce->tau_end || !ce->status)))
    return fail(ART_E_INVALID, "cyc_slot needs cyc_n >= 0, cyc_tau and the re-run's end states");
  return ART_OK;
}

// EventRowsArgs' inputs from p and in (13 columns, no outputs). end_states: also the cyclotron re-run's end states
static art::EventRowsArgs event_args(const art_params* p, const art_event_rows_in* in, bool end_states) {
  art::EventRowsArgs a{};
  a.n_events = in->n_events; a.event_offset = in->event_offset; a.n_nodes = in->n_nodes;
  a.x = in->x; a.k_init = in->k_init; a.weight5 = in->weight5; a.attempts = in->attempts;
  a.back = in->back; a.nodes = in->nodes; a.back_counts = in->back_counts; a.counts = in->counts; a.infos = in->infos;
  if (in->cyc_slot) {
    a.cyc_slot = in->cyc_slot; a.cyc_n = in->cyc_n; a.cyc_tau = in->cyc_tau;
    if (const art_segment_out* ce = end_states ? in->cyc_end : nullptr) {
      a.cyc_x_end = ce->x_end; a.cyc_k_end = ce->k_end; a.cyc_u7_end = ce->u7_end; a.cyc_tau_end = ce->tau_end;
      a.cyc_status = ce->status;
    }
  }
  a.mass_a = p->mass_a;
  a.ncols = art::EVENT_COLS_SHORT;
  return a;
}

// The part of a scan's out struct the two scans share (art_event_reweight_out, art_event_halo_scan_out): the checks
// of its tables after `totals`, then the tables, node_start and the sizes into the kernels' args.
template <class Out, class Args>
static int scan_tables(const Out* out, const int64_t* node_start, int32_t n_k, const EventSky& S, Args* r) {
  if (out->nbins > 0 && !out->flux) return fail(ART_E_INVALID, "flux is NULL");
  if (out->sky && !out->sky_hist) return fail(ART_E_INVALID, "sky_hist is NULL");
  const bool moments = out->moment_totals != nullptr;
  if (moments && out->nbins > 0 && (!out->flux_sq || !out->flux_xa)) return fail(ART_E_INVALID, "flux_sq or flux_xa is NULL");
  if (moments && out->sky && (!out->sky_sq || !out->sky_xa)) return fail(ART_E_INVALID, "sky_sq or sky_xa is NULL");
  r->node_start = node_start; r->n_k = n_k; r->nbins = out->nbins; r->sky_size = S.size;
  r->flux = out->flux; r->sky = out->sky ? out->sky_hist : nullptr; r->totals = out->totals;
  if (moments) {
    r->flux_sq = out->flux_sq; r->flux_xa = out->flux_xa; r->mtotals = out->moment_totals;
    if (out->sky) {
      r->sky_sq = out->sky_sq; r->sky_xa = out->sky_xa;
    }
  }
  return ART_OK;
}

// One block of scratch cut into parts that each begin at a multiple of 256 bytes: add() every part, allocate
// `bytes`, then part i lies at block + its add().
struct Carve {
  size_t bytes = 0;
  size_t add(size_t part) {
    const size_t at = (bytes + 255) & ~(size_t)255;
    bytes = at + part;
    return at;
  }
};

}  // namespace host
}  // namespace art

using namespace art::host;

extern "C" {

int art_get_prob_nonad_device(const art_params* p, int64_t nc, const double* pos, const double* kpos,
                              const double* erg_eff, int64_t n_groups, const int64_t* group_start, double* out,
                              void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (nc == 0) return ART_OK;
  if (nc < 0 || nc > 2147483647LL) return fail(ART_E_INVALID, "nc must be in [0, 2^31)");
  if (!pos || !kpos || !erg_eff || !out) return fail(ART_E_INVALID, "NULL buffer");
  if (!group_start) n_groups = nc;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  HIP_OK(art::launch_prob(art::make_kparams(*p), nc, pos, kpos, erg_eff, n_groups, group_start, out, (hipStream_t)stream));
  return ART_OK;
}

int art_get_prob_nonad_host(const art_params* p, int64_t nc, const double* pos, const double* kpos,
                            const double* erg_eff, int64_t n_groups, const int64_t* group_start, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (nc == 0) return ART_OK;
  if (nc < 0 || nc > 2147483647LL) return fail(ART_E_INVALID, "nc must be in [0, 2^31)");
  if (!pos || !kpos || !erg_eff || !out) return fail(ART_E_INVALID, "NULL buffer");
  if (!group_start) n_groups = nc;
  if (group_start) {  // groups must tile [0, nc)
    if (n_groups < 1) return fail(ART_E_INVALID, "n_groups must be >= 1");
    if (group_start[0] != 0 || group_start[n_groups] != nc) return fail(ART_E_INVALID, "group_start must span [0, nc]");
    for (int64_t g = 0; g < n_groups; ++g)
      if (group_start[g + 1] <= group_start[g]) return fail(ART_E_INVALID, "empty or unsorted group");
  }
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  void* d;
  const size_t nd = (size_t)nc;
  const size_t bytes = nd * 8 * sizeof(double) + (size_t)(n_groups + 1) * sizeof(int64_t);
  if ((rc = pool_get(c, 3, bytes, &d))) return rc;
  double* dd = (double*)d;
  int64_t* dg = group_start ? (int64_t*)(dd + 8 * nd) : nullptr;
  hipStream_t s = c->stream;
  HIP_OK(hipMemcpyAsync(dd, pos, nd * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(dd + 3 * nd, kpos, nd * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(dd + 6 * nd, erg_eff, nd * sizeof(double), hipMemcpyHostToDevice, s));
  if (dg) HIP_OK(hipMemcpyAsync(dg, group_start, (size_t)(n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  HIP_OK(art::launch_prob(art::make_kparams(*p), nc, dd, dd + 3 * nd, dd + 6 * nd, n_groups, dg, dd + 7 * nd, s));
  HIP_OK(hipMemcpyAsync(out, dd + 7 * nd, nd * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return ART_OK;
}

int art_sample_conversion_points_device(const art_params* p, double max_r, uint64_t seed, int64_t ray_offset,
                                        int64_t n, double* x, double* k_init, double* erg_inf, double* vifty,
                                        int32_t* weights, int32_t* attempts, void* stream) {
  return art_sample_conversion_points_halo_device(p, nullptr, max_r, seed, ray_offset, n, x, k_init, erg_inf, vifty,
                                                  weights, attempts, stream);
}

// The sampler with the halo velocity model (include/art.h); halo == NULL: the kernels without it.
int art_sample_conversion_points_halo_device(const art_params* p, const art_halo* halo, double max_r, uint64_t seed,
                                             int64_t ray_offset, int64_t n, double* x, double* k_init,
                                             double* erg_inf, double* vifty, int32_t* weights, int32_t* attempts,
                                             void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return sample_device_impl(p, halo, max_r, seed, ray_offset, n, x, k_init, erg_inf, vifty, weights, attempts,
                            (hipStream_t)stream);
}

// The whole stage-run-copy sequence holds the mutex, so no other thread can regrow the staging
// buffer in between.
int art_sample_conversion_points_host(const art_params* p, double max_r, uint64_t seed, int64_t ray_offset, int64_t n,
                                      double* x, double* k_init, double* erg_inf, double* vifty, int32_t* weights,
                                      int32_t* attempts) {
  return art_sample_conversion_points_halo_host(p, nullptr, max_r, seed, ray_offset, n, x, k_init, erg_inf, vifty,
                                                weights, attempts);
}

int art_sample_conversion_points_halo_host(const art_params* p, const art_halo* halo, double max_r, uint64_t seed,
                                           int64_t ray_offset, int64_t n, double* x, double* k_init,
                                           double* erg_inf, double* vifty, int32_t* weights, int32_t* attempts) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  art::HaloK hk;
  if (halo && (rc = halo_of(halo, &hk))) return rc;
  if (n == 0) return ART_OK;
  if (n < 0 || n > 2147483647LL) return fail(ART_E_INVALID, "n must be in [0, 2^31)");
  if (!(max_r > p->rNS)) return fail(ART_E_INVALID, "max_r must exceed rNS (MainRunner.jl:389-396 quits otherwise)");
  if (!x || !k_init || !erg_inf || !vifty || !weights || !attempts) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  void* d;
  const size_t nd = (size_t)n;
  if ((rc = pool_get(c, 4, nd * 10 * sizeof(double) + nd * 2 * sizeof(int32_t), &d))) return rc;
  double* dd = (double*)d;
  int32_t* di = (int32_t*)(dd + 10 * nd);
  hipStream_t s = c->stream;
  if ((rc = sample_device_impl(p, halo, max_r, seed, ray_offset, n, dd, dd + 3 * nd, dd + 6 * nd, dd + 7 * nd, di, di + nd,
                               s)))
    return rc;
  HIP_OK(hipMemcpyAsync(x, dd, nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(k_init, dd + 3 * nd, nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(erg_inf, dd + 6 * nd, nd * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(vifty, dd + 7 * nd, nd * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(weights, di, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(attempts, di + nd, nd * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return ART_OK;
}

int art_event_weight_device(const art_params* p, double max_r, double rho_dm, double mcmc_weight, int64_t n,
                            const double* x, const double* k_init, const double* vifty, double* out, void* stream) {
  return art_event_weight_halo_device(p, nullptr, max_r, rho_dm, mcmc_weight, n, x, k_init, vifty, out, stream);
}

// The event weight with the halo model's factor and vel_eng (include/art.h); halo == NULL: without.
int art_event_weight_halo_device(const art_params* p, const art_halo* halo, double max_r, double rho_dm,
                                 double mcmc_weight, int64_t n, const double* x, const double* k_init,
                                 const double* vifty, double* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  return event_weight_device_impl(p, halo, max_r, rho_dm, mcmc_weight, n, x, k_init, vifty, out, (hipStream_t)stream);
}

int art_event_weight_host(const art_params* p, double max_r, double rho_dm, double mcmc_weight, int64_t n,
                          const double* x, const double* k_init, const double* vifty, double* out) {
  return art_event_weight_halo_host(p, nullptr, max_r, rho_dm, mcmc_weight, n, x, k_init, vifty, out);
}

int art_event_weight_halo_host(const art_params* p, const art_halo* halo, double max_r, double rho_dm,
                               double mcmc_weight, int64_t n, const double* x, const double* k_init,
                               const double* vifty, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  art::HaloK hk;
  if (halo && (rc = halo_of(halo, &hk))) return rc;
  if (n == 0) return ART_OK;
  if (n < 0 || n > 2147483647LL) return fail(ART_E_INVALID, "n must be in [0, 2^31)");
  if (!x || !k_init || !vifty || !out) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  void* d;
  const size_t nd = (size_t)n;
  if ((rc = pool_get(c, 5, nd * 14 * sizeof(double), &d))) return rc;
  double* dd = (double*)d;
  hipStream_t s = c->stream;
  HIP_OK(hipMemcpyAsync(dd, x, nd * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(dd + 3 * nd, k_init, nd * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(dd + 6 * nd, vifty, nd * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  if ((rc = event_weight_device_impl(p, halo, max_r, rho_dm, mcmc_weight, n, dd, dd + 3 * nd, dd + 6 * nd, dd + 9 * nd, s)))
    return rc;
  HIP_OK(hipMemcpyAsync(out, dd + 9 * nd, nd * 5 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return ART_OK;
}

int art_flux_histogram_device(const art_params* p, int64_t n, const double* x_end, const double* k_end,
                              const int32_t* status, const int8_t* species, const double* w, int32_t nbins,
                              double* hist, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (nbins < 1 || nbins > 4096) return fail(ART_E_INVALID, "nbins must be in [1, 4096]");
  if (n == 0) return ART_OK;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  HIP_OK(art::launch_flux(art::make_kparams(*p), n, x_end, k_end, status, species, w, nbins, hist, (hipStream_t)stream));
  return ART_OK;
}

int art_flux_histogram_phi_device(int64_t n, const double* phi, const int8_t* species, const double* w, int32_t nbins,
                                  double* hist, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (nbins < 1 || nbins > 4096) return fail(ART_E_INVALID, "nbins must be in [1, 4096]");
  if (n < 0) return fail(ART_E_INVALID, "n must be >= 0");
  if (n == 0) return ART_OK;
  if (!phi || !hist) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  HIP_OK(art::launch_flux_phi(n, phi, species, w, nbins, -art::PI, art::PI, hist, (hipStream_t)stream));
  return ART_OK;
}

int art_flux_histogram_phi_range_device(int64_t n, const double* phi, const int8_t* species, const double* w,
                                        int32_t nbins, double lo, double hi, double* hist, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (nbins < 1 || nbins > 4096) return fail(ART_E_INVALID, "nbins must be in [1, 4096]");
  if (n < 0) return fail(ART_E_INVALID, "n must be >= 0");
  if (!(lo < hi) || !std::isfinite(lo) || !std::isfinite(hi)) return fail(ART_E_INVALID, "need finite lo < hi");
  if (n == 0) return ART_OK;
  if (!phi || !hist) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  HIP_OK(art::launch_flux_phi(n, phi, species, w, nbins, lo, hi, hist, (hipStream_t)stream));
  return ART_OK;
}

int art_histogram3_device(int64_t n, const double* a, const double* b, const double* c, const int8_t* species,
                          const double* w, const int32_t nbins[3], const double lo[3], const double hi[3], int32_t mode,
                          double* hist, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (n < 0) return fail(ART_E_INVALID, "n must be >= 0");
  if (!nbins || !lo || !hi) return fail(ART_E_INVALID, "NULL nbins, lo or hi");
  art::SkyAxes A;
  int rc = sky_axes(nbins, lo, hi, false, mode, &A);
  if (rc) return rc;
  if (n == 0) return ART_OK;
  if (!a || !b || !c || !hist) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  HIP_OK(art::launch_sky_map(n, a, b, c, species, w, A, mode, hist, (hipStream_t)stream));
  return ART_OK;
}

int art_sky_map_segments_device(const art_params* p, const art_sky_spec* spec, int64_t n, const double* x_end,
                                const double* k_end, const double* u7_end, const int32_t* status, const int8_t* species,
                                const double* w, const double* dw_offset, double* hist, int32_t* bin_out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (n < 0) return fail(ART_E_INVALID, "n must be >= 0");
  if (!spec) return fail(ART_E_INVALID, "NULL spec");
  EventSky S;
  if ((rc = event_sky(spec, /*honour_mode=*/true, 0, &S))) return rc;  // (no flux table beside the map)
  if (n == 0) return ART_OK;
  if (!x_end || !k_end || !u7_end || !status || !hist) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  HIP_OK(art::launch_sky_map_segments(art::make_kparams(*p), n, x_end, k_end, u7_end, status, species, w, dw_offset, S.A,
                                      S.cos_axis, S.mode, hist, bin_out, (hipStream_t)stream));
  return ART_OK;
}

// The rows, flux, sky map and totals of a chunk of events whose forests lie in HBM (include/art.h):
// a scan of the final nodes and event_rows_kernel, both on `stream`.
int art_event_rows_device(const art_params* p, const art_event_rows_in* in, const art_event_rows_out* out,
                          void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out) return fail(ART_E_INVALID, "NULL in or out");
  if ((rc = event_in_ranges(in))) return rc;
  if (out->ncols != art::EVENT_COLS_SHORT && out->ncols != art::EVENT_COLS_FULL)
    return fail(ART_E_INVALID, "ncols must be 13 or 29");
  if ((out->rows || out->bin_out) && out->row_capacity < in->n_nodes)
    return fail(ART_E_INVALID, "row_capacity must be >= n_nodes");
  if ((rc = event_out_ranges(0, out->nbins))) return rc;  // (this out struct has no reserved field)
  EventSky S;
  // honour_mode: event_rows_kernel alone can keep its tables in LDS; the other three calls add to theirs in HBM
  if ((rc = event_sky(out->sky, /*honour_mode=*/true, out->nbins, &S))) return rc;
  if (in->n_events == 0 || (in->n_nodes == 0 && !in->attempts)) return ART_OK;  // (attempts alone still add to totals)
  if (!out->totals) return fail(ART_E_INVALID, "totals is NULL");
  if (out->nbins > 0 && !out->flux) return fail(ART_E_INVALID, "flux is NULL");
  if (out->sky && !out->sky_hist) return fail(ART_E_INVALID, "sky_hist is NULL");
  // IN_CYC_END_STATES: the kernel compares each re-run's end state with its node's (totals[5])
  if ((rc = event_in_buffers(in, nullptr, IN_CYC_END_STATES))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  hipStream_t s = (hipStream_t)stream;
  art::EventRowsArgs a = event_args(p, in, /*end_states=*/true);
  a.row_capacity = out->row_capacity;
  a.ncols = out->ncols; a.nbins = out->nbins;
  a.rows = out->rows; a.flux = out->flux; a.sky_hist = out->sky ? out->sky_hist : nullptr; a.totals = out->totals;
  a.bin_out = out->sky ? out->bin_out : nullptr;
  if (in->n_nodes == 0) {
    HIP_OK(art::launch_event_rows(a, S.A, S.cos_axis, S.mode, s));
    return ART_OK;
  }
  Carve cv;  // [pos | tmp]
  const size_t tmp_bytes = art::event_scan_bytes(in->n_nodes), o_pos = cv.add((size_t)in->n_nodes * 4),
               o_tmp = cv.add(tmp_bytes);
  void* block = nullptr;
  if ((rc = scratch_alloc(s, cv.bytes, &block))) return rc;
  a.pos = (const int32_t*)((char*)block + o_pos);
  hipError_t e = art::launch_event_scan(in->n_nodes, in->nodes, false, (int32_t*)((char*)block + o_pos),
                                        (char*)block + o_tmp, tmp_bytes, s);
  if (e == hipSuccess) e = art::launch_event_rows(a, S.A, S.cos_axis, S.mode, s);
  (void)hipFreeAsync(block, s);
  HIP_OK(e);
  return ART_OK;
}

// The cyclotron re-run's batch (include/art.h): scan, one count to the host, gather.
int art_event_gather_photons_device(const art_params* p, int64_t n_events, const double* erg, int64_t n_nodes,
                                    const art_tree_node* nodes, int64_t capacity, double* x0, double* k0,
                                    double* erg_out, double* dw, double* ln_t0, int8_t* species, int32_t* slot,
                                    int64_t* n_out, void* stream) {
  std::unique_lock<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!n_out) return fail(ART_E_INVALID, "n_out is NULL");
  if (n_events < 0) return fail(ART_E_INVALID, "n_events must be >= 0");
  if (n_nodes < 0 || n_nodes > 2147483647LL) return fail(ART_E_INVALID, "n_nodes must be in [0, 2^31)");
  if (capacity < 0) return fail(ART_E_INVALID, "capacity must be >= 0");
  *n_out = 0;
  if (n_nodes == 0) return ART_OK;
  if (!erg || !nodes || !slot) return fail(ART_E_INVALID, "NULL input buffer");
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  hipStream_t s = (hipStream_t)stream;
  TreeScratch ts;  // (its block and its pinned word, released when the call returns)
  ts.s = s;
  Carve cv;  // [pos | tmp]
  const size_t tmp_bytes = art::event_scan_bytes(n_nodes + 1), o_pos = cv.add((size_t)(n_nodes + 1) * 4), o_tmp = cv.add(tmp_bytes);
  if ((rc = scratch_alloc(s, cv.bytes, &ts.block))) return rc;
  if (hipHostMalloc((void**)&ts.host, 64, hipHostMallocDefault) != hipSuccess) return fail(ART_E_NOMEM, "hipHostMalloc failed");
  int32_t* pos = (int32_t*)((char*)ts.block + o_pos);
  // the count is the sum of the last prefix and the last node's own flag: both come to the host
  HIP_OK(art::launch_event_scan(n_nodes, nodes, true, pos, (char*)ts.block + o_tmp, tmp_bytes, s));
  HIP_OK(hipMemcpyAsync(ts.host, pos + (n_nodes - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(ts.host + 2, &nodes[n_nodes - 1], 2 * sizeof(int32_t) + sizeof(int32_t), hipMemcpyDeviceToHost, s));
  lk.unlock();
  const hipError_t we = hipStreamSynchronize(s);
  lk.lock();
  if (we != hipSuccess) return fail(ART_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(we));
  // ts.host[2..4]: the last node's tree, species, is_final
  const int64_t m = (int64_t)ts.host[0] + ((ts.host[4] != 0 && ts.host[3] != ART_AXION) ? 1 : 0);
  *n_out = m;
  if (m > capacity) return fail(ART_E_NOMEM, "capacity is too small: %s final photons", std::to_string(m).c_str());
  if (m > 0 && (!x0 || !k0 || !erg_out || !dw || !ln_t0 || !species)) return fail(ART_E_INVALID, "NULL batch buffer");
  art::TreeBatch B{};
  B.x0 = x0; B.k0 = k0; B.erg = erg_out; B.dw = dw; B.lnt0 = ln_t0; B.species = species;
  const double dt0 = std::exp(-30.0), ln_dt0 = std::log(dt0);  // art_grow_trees_device's
  HIP_OK(art::launch_event_gather(n_nodes, nodes, pos, n_events, erg, m, B, slot, dt0, ln_dt0, s));
  return ART_OK;  // (ts releases pos in the stream's order, after the gather)
}

// The second moments of a chunk's binned event power (include/art.h): one entry per node record in
// scratch, then the per-tree group-by (art_event_moments.h), both on `stream`.
int art_event_moments_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                             const art_event_moments_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out) return fail(ART_E_INVALID, "NULL in or out");
  if ((rc = event_in_ranges(in)) || (rc = event_out_ranges(out->reserved, out->nbins))) return rc;
  EventSky S;
  if ((rc = event_sky(out->sky, /*honour_mode=*/false, out->nbins, &S))) return rc;  // (tables in HBM: no mode)
  if (in->n_events == 0) return ART_OK;
  if (!out->totals) return fail(ART_E_INVALID, "totals is NULL");
  if (out->nbins > 0 && (!out->flux_sq || !out->flux_xa)) return fail(ART_E_INVALID, "flux_sq or flux_xa is NULL");
  if (out->sky && (!out->sky_sq || !out->sky_xa)) return fail(ART_E_INVALID, "sky_sq or sky_xa is NULL");
  // IN_NODE_START_LATE: an empty chunk has returned above without a look at node_start (the scans look first).
  // IN_CYC_END_STATES: asked for as art_event_rows_device asks, whose chunk and re-run this call is handed; the
  // kernels read cyc_tau alone.
  if ((rc = event_in_buffers(in, node_start, IN_NODE_START_LATE | IN_CYC_END_STATES))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  art::EventMomentsArgs m{};
  m.node_start = node_start; m.nbins = out->nbins;
  m.flux_sq = out->flux_sq; m.flux_xa = out->flux_xa; m.totals = out->totals;
  if (out->sky) {
    m.sky_sq = out->sky_sq; m.sky_xa = out->sky_xa;
  }
  void* block = nullptr;
  if (in->n_nodes > 0 && (rc = scratch_alloc(s, (size_t)in->n_nodes * sizeof(art::MomentEntry), &block))) return rc;
  m.entries = (art::MomentEntry*)block;
  const hipError_t e = art::launch_event_moments(a, m, S.A, S.cos_axis, s);
  if (block) (void)hipFreeAsync(block, s);
  HIP_OK(e);
  return ART_OK;
}

// The coupling scan of a chunk (include/art.h): the per-tree reweight, then the bins and, when asked
// for, the second moments per coupling (art_event_reweight.h), all on `stream`.
int art_event_reweight_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                              const art_tree_opts* opts, int32_t n_couplings, const double* couplings,
                              const art_event_reweight_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out || !opts) return fail(ART_E_INVALID, "NULL in, out or opts");
  if (!couplings) return fail(ART_E_INVALID, "couplings is NULL");
  if (n_couplings < 1 || n_couplings > art::REWEIGHT_MAX_COUPLINGS)
    return fail(ART_E_INVALID, "n_couplings must be in [1, 32]");
  if (!(p->g_agg > 0.0) || !std::isfinite(p->g_agg)) return fail(ART_E_INVALID, "the base coupling g_agg must be finite and > 0");
  for (int k = 0; k < n_couplings; ++k)
    if (!(couplings[k] > 0.0) || !std::isfinite(couplings[k]))
      return fail(ART_E_INVALID, "every coupling must be finite and > 0");
  if ((rc = event_in_ranges(in)) || (rc = event_out_ranges(out->reserved, out->nbins))) return rc;
  EventSky S;
  if ((rc = event_sky(out->sky, /*honour_mode=*/false, out->nbins, &S))) return rc;  // (tables in HBM: no mode)
  if ((rc = need_node_start(in, node_start))) return rc;  // (before the empty return, unlike the moments call)
  if (in->n_events == 0) return ART_OK;
  if (!out->totals) return fail(ART_E_INVALID, "totals is NULL");
  if (!out->erg) return fail(ART_E_INVALID, "erg is NULL");
  art::EventReweightArgs r{};
  if ((rc = scan_tables(out, node_start, n_couplings, S, &r))) return rc;
  // IN_EVENT_INPUTS_ALWAYS: event_reweight_kernel reads x, k_init and back of every event, nodes or not.
  // No IN_CYC_END_STATES: the scan reads cyc_tau alone.
  if ((rc = event_in_buffers(in, node_start, IN_EVENT_INPUTS_ALWAYS))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  r.erg = out->erg; r.mc_nodes = opts->mc_nodes;
  for (int k = 0; k < n_couplings; ++k) {
    const double q = couplings[k] / p->g_agg;
    r.s[k] = q * q;
  }
  const bool moments = r.mtotals != nullptr;
  const size_t K = (size_t)n_couplings, nn = (size_t)in->n_nodes, ne = (size_t)in->n_events;
  Carve cv;  // [X0 | W | B | Pw | entries | 256 bytes, so the block is never empty]
  const size_t o_x0 = cv.add(nn * 8), o_w = cv.add(out->weights ? 0 : K * nn * 8), o_b = cv.add(out->back ? 0 : K * ne * 8),
               o_pw = cv.add(moments ? K * nn * 8 : 0), o_en = cv.add(moments ? nn * sizeof(art::MomentEntry) : 0);
  cv.add(256);
  void* block = nullptr;
  if ((rc = scratch_alloc(s, cv.bytes, &block))) return rc;
  char* at = (char*)block;
  r.X0 = (double*)(at + o_x0);
  r.W = out->weights ? out->weights : (double*)(at + o_w);
  r.B = out->back ? out->back : (double*)(at + o_b);
  r.Bp = out->back_prob;
  if (moments) {
    r.Pw = (double*)(at + o_pw);
    r.entries = (art::MomentEntry*)(at + o_en);
  }
  art_params pb = *p;
  pb.B0 = -p->B0;  // the backtrace's field (main_runner_tree: the backtrace runs with B0 negated)
  const hipError_t e = art::launch_event_reweight(art::make_kparams(*p), art::make_kparams(pb), a, r, S.A, S.cos_axis, s);
  (void)hipFreeAsync(block, s);
  HIP_OK(e);
  return ART_OK;
}

// The halo scan of a chunk (include/art.h): the ratios per event and model, then the bins and, when
// asked for, the second moments per model (art_event_haloscan.h), all on `stream`.
int art_event_halo_scan_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                               const art_halo* base, int32_t n_models, const art_halo* models,
                               const art_event_halo_scan_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out) return fail(ART_E_INVALID, "NULL in or out");
  if (!base || !models) return fail(ART_E_INVALID, "NULL base or models");
  if (n_models < 1 || n_models > art::HALO_SCAN_MAX_MODELS) return fail(ART_E_INVALID, "n_models must be in [1, 32]");
  art::EventHaloScanArgs h{};
  if ((rc = halo_of(base, &h.base))) return rc;
  for (int k = 0; k < n_models; ++k) {
    const art_halo& m = models[k];
    if (!std::isfinite(m.v0) || !(m.v0 > 0.0)) return fail(ART_E_INVALID, "halo scan: every model's v0 must be finite and > 0");
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(m.v_ns[i])) return fail(ART_E_INVALID, "halo scan: every model's v_ns must be finite");
    if (m.v0 > h.base.vp)
      return fail(ART_E_INVALID, "halo scan: a model's v0 must be <= the base's v_prop (the weights are unbounded above it)");
    h.models[k].v0 = m.v0;
    for (int i = 0; i < 3; ++i) h.models[k].v_ns[i] = m.v_ns[i];
    h.models[k].vp = h.base.vp;  // (the run's proposal; a model's own v_prop is ignored)
  }
  if ((rc = event_in_ranges(in)) || (rc = event_out_ranges(out->reserved, out->nbins))) return rc;
  EventSky S;
  if ((rc = event_sky(out->sky, /*honour_mode=*/false, out->nbins, &S))) return rc;  // (tables in HBM: no mode)
  if (in->n_events > 0 && !out->vifty) return fail(ART_E_INVALID, "vifty is NULL");
  if ((rc = need_node_start(in, node_start))) return rc;  // (before the empty return, unlike the moments call)
  if (in->n_events == 0) return ART_OK;
  if (!out->totals) return fail(ART_E_INVALID, "totals is NULL");
  if ((rc = scan_tables(out, node_start, n_models, S, &h))) return rc;
  // No IN_EVENT_INPUTS_ALWAYS: the ratio kernel reads vifty alone per event. No IN_CYC_END_STATES: cyc_tau alone.
  if ((rc = event_in_buffers(in, node_start, 0))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  h.vifty = out->vifty;
  const bool moments = h.mtotals != nullptr;
  const size_t K = (size_t)n_models, nn = (size_t)in->n_nodes, ne = (size_t)in->n_events;
  Carve cv;  // [R | Pw | entries | 256 bytes, so the block is never empty]
  const size_t o_r = cv.add(out->ratio ? 0 : K * ne * 8), o_pw = cv.add(moments ? K * nn * 8 : 0),
               o_en = cv.add(moments ? nn * sizeof(art::MomentEntry) : 0);
  cv.add(256);
  void* block = nullptr;
  if ((rc = scratch_alloc(s, cv.bytes, &block))) return rc;
  char* at = (char*)block;
  h.R = out->ratio ? out->ratio : (double*)(at + o_r);
  if (moments) {
    h.Pw = (double*)(at + o_pw);
    h.entries = (art::MomentEntry*)(at + o_en);
  }
  const hipError_t e = art::launch_event_halo_scan(a, h, S.A, S.cos_axis, s);
  (void)hipFreeAsync(block, s);
  HIP_OK(e);
  return ART_OK;
}

// The jackknife replicates of a chunk (include/art.h): the run's, a coupling scan's or a halo scan's first-moment
// tables per group of events (art_event_replicates.h), one kernel on `stream`.
int art_event_replicates_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                                const art_event_replicates_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out) return fail(ART_E_INVALID, "NULL in or out");
  if (out->n_groups < art::REPLICATES_MIN_GROUPS || out->n_groups > art::REPLICATES_MAX_GROUPS)
    return fail(ART_E_INVALID, "n_groups must be in [2, 64]");
  if (out->kind < 0 || out->kind >= art::REP_KIND_COUNT)
    return fail(ART_E_INVALID, "kind must be 0 (the run), 1 (a coupling scan) or 2 (a halo scan)");
  if (out->n_sets < 1 || out->n_sets > art::REPLICATES_MAX_SETS) return fail(ART_E_INVALID, "n_sets must be in [1, 32]");
  if (out->kind == art::REP_KIND_RUN && out->n_sets != 1) return fail(ART_E_INVALID, "n_sets must be 1 with kind 0");
  if (out->kind == art::REP_KIND_COUPLING && in->n_nodes > 0 && !out->node_factor)
    return fail(ART_E_INVALID, "node_factor is NULL (kind 1: the coupling scan's weights)");
  if (out->kind != art::REP_KIND_RUN && !out->event_factor)
    return fail(ART_E_INVALID, "event_factor is NULL (kind 1: the coupling scan's back, kind 2: the halo scan's ratio)");
  if ((rc = event_in_ranges(in)) || (rc = event_out_ranges(0, out->nbins))) return rc;  // (no reserved field)
  EventSky S;
  if ((rc = event_sky(out->sky, /*honour_mode=*/false, out->nbins, &S))) return rc;  // (tables in HBM: no mode)
  if (in->n_events == 0) return ART_OK;
  if (!out->totals || !out->groups) return fail(ART_E_INVALID, "totals or groups is NULL");
  if (out->nbins > 0 && !out->flux) return fail(ART_E_INVALID, "flux is NULL");
  if (out->sky && !out->sky_hist) return fail(ART_E_INVALID, "sky_hist is NULL");
  // IN_NODE_START_LATE and IN_CYC_END_STATES: the moments call's checks, whose chunk and re-run this call is handed;
  // the kernel reads cyc_tau alone.
  if ((rc = event_in_buffers(in, node_start, IN_NODE_START_LATE | IN_CYC_END_STATES))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  art::EventReplicatesArgs r{};
  r.node_start = node_start; r.n_groups = out->n_groups; r.kind = out->kind; r.n_k = out->n_sets; r.nbins = out->nbins;
  r.sky_size = S.size; r.node_factor = out->node_factor; r.event_factor = out->event_factor;
  r.flux = out->flux; r.sky = out->sky ? out->sky_hist : nullptr; r.totals = out->totals; r.groups = out->groups;
  HIP_OK(art::launch_event_replicates(a, r, S.A, S.cos_axis, (hipStream_t)stream));
  return ART_OK;
}

// The coupling x halo grid of a chunk (include/art.h): the first-moment tables at every (coupling, halo model) cell
// from the two scans' factors (art_event_grid.h), one kernel on `stream`.
int art_event_grid_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                          const art_event_grid_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out) return fail(ART_E_INVALID, "NULL in or out");
  if (out->n_couplings < 1 || out->n_couplings > art::GRID_MAX_COUPLINGS)
    return fail(ART_E_INVALID, "n_couplings must be in [1, 32]");
  if (out->n_models < 1 || out->n_models > art::GRID_MAX_MODELS) return fail(ART_E_INVALID, "n_models must be in [1, 32]");
  if (out->n_groups != 0 && (out->n_groups < art::REPLICATES_MIN_GROUPS || out->n_groups > art::REPLICATES_MAX_GROUPS))
    return fail(ART_E_INVALID, "n_groups must be 0 (no replicate tables) or in [2, 64]");
  if ((rc = event_in_ranges(in)) || (rc = event_out_ranges(0, out->nbins))) return rc;  // (no reserved field)
  if (in->n_events == 0) return ART_OK;
  if (!out->back || !out->ratio) return fail(ART_E_INVALID, "back or ratio is NULL (the two scans' factors per event)");
  if (in->n_nodes > 0 && !out->node_factor) return fail(ART_E_INVALID, "node_factor is NULL (the coupling scan's weights)");
  if (!out->totals) return fail(ART_E_INVALID, "totals is NULL");
  if (out->nbins > 0 && !out->flux) return fail(ART_E_INVALID, "flux is NULL");
  if (out->n_groups > 0 && (!out->totals_rep || !out->groups)) return fail(ART_E_INVALID, "totals_rep or groups is NULL");
  if (out->n_groups > 0 && out->nbins > 0 && !out->flux_rep) return fail(ART_E_INVALID, "flux_rep is NULL");
  // IN_NODE_START_LATE and IN_CYC_END_STATES: the moments call's checks, whose chunk and re-run this call is handed;
  // the kernel reads cyc_tau alone.
  if ((rc = event_in_buffers(in, node_start, IN_NODE_START_LATE | IN_CYC_END_STATES))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  art::EventGridArgs r{};
  r.node_start = node_start; r.n_g = out->n_couplings; r.n_h = out->n_models; r.nbins = out->nbins;
  r.n_groups = out->n_groups; r.W = out->node_factor; r.B = out->back; r.R = out->ratio;
  r.flux = out->flux; r.totals = out->totals; r.mtotals = out->moment_totals;
  if (out->n_groups > 0) {
    r.flux_rep = out->flux_rep; r.totals_rep = out->totals_rep; r.groups = out->groups;
  }
  HIP_OK(art::launch_event_grid(a, r, (hipStream_t)stream));
  return ART_OK;
}

// The event power spectrum of a chunk (include/art.h): one entry per node record and X per set, species and event in
// scratch, then the tables and the top lists (art_event_spectrum.h), three kernels on `stream`.
int art_event_spectrum_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                              const art_event_spectrum_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out) return fail(ART_E_INVALID, "NULL in or out");
  if (out->kind < 0 || out->kind >= art::REP_KIND_COUNT)
    return fail(ART_E_INVALID, "kind must be 0 (the run), 1 (a coupling scan) or 2 (a halo scan)");
  if (out->n_sets < 1 || out->n_sets > art::SPECTRUM_MAX_SETS) return fail(ART_E_INVALID, "n_sets must be in [1, 32]");
  if (out->kind == art::REP_KIND_RUN && out->n_sets != 1) return fail(ART_E_INVALID, "n_sets must be 1 with kind 0");
  if (out->sub_bits < 0 || out->sub_bits > art::SPECTRUM_MAX_SUB_BITS) return fail(ART_E_INVALID, "sub_bits must be in [0, 4]");
  if (out->top < 0 || out->top > art::SPECTRUM_MAX_TOP) return fail(ART_E_INVALID, "top must be in [0, 256]");
  if ((rc = event_in_ranges(in))) return rc;
  if (out->kind == art::REP_KIND_COUPLING && in->n_nodes > 0 && !out->node_factor)
    return fail(ART_E_INVALID, "node_factor is NULL (kind 1: the coupling scan's weights)");
  if (out->kind != art::REP_KIND_RUN && !out->event_factor)
    return fail(ART_E_INVALID, "event_factor is NULL (kind 1: the coupling scan's back, kind 2: the halo scan's ratio)");
  if ((rc = need_node_start(in, node_start))) return rc;
  if (!out->count || !out->sum || !out->sum_sq || !out->totals) return fail(ART_E_INVALID, "count, sum, sum_sq or totals is NULL");
  if (out->top > 0 && (!out->top_power || !out->top_event)) return fail(ART_E_INVALID, "top_power or top_event is NULL");
  if (in->n_events == 0) return ART_OK;
  // IN_CYC_END_STATES: the moments call's check, whose chunk and re-run this call is handed; the kernels read
  // cyc_tau alone.
  if ((rc = event_in_buffers(in, node_start, IN_CYC_END_STATES))) return rc;
  if (out->kind == art::REP_KIND_COUPLING && !in->weight5) return fail(ART_E_INVALID, "NULL input buffer");
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  art::EventSpectrumArgs r{};
  r.node_start = node_start; r.kind = out->kind; r.n_k = out->n_sets; r.sub_bits = out->sub_bits; r.top = out->top;
  r.node_factor = out->node_factor; r.event_factor = out->event_factor;
  r.count = out->count; r.sum = out->sum; r.sum_sq = out->sum_sq; r.totals = out->totals;
  r.top_power = out->top_power; r.top_event = out->top_event;
  Carve cv;  // [X | entries]
  const size_t o_x = cv.add((size_t)out->n_sets * 2 * (size_t)in->n_events * 8),
               o_en = cv.add((size_t)in->n_nodes * sizeof(art::MomentEntry));
  void* block = nullptr;
  if ((rc = scratch_alloc(s, cv.bytes, &block))) return rc;
  r.X = (double*)((char*)block + o_x);
  r.entries = (art::MomentEntry*)((char*)block + o_en);
  const hipError_t e = art::launch_event_spectrum(a, r, s);
  (void)hipFreeAsync(block, s);
  HIP_OK(e);
  return ART_OK;
}

// The emission map of a chunk (include/art.h): the powers of its final rows over their event's conversion point and,
// with an observer, jointly over their direction (art_event_origin.h), one kernel on `stream`.
int art_event_origin_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                            const art_event_origin_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out || !out->origin) return fail(ART_E_INVALID, "NULL in, out or origin");
  const art_origin_spec* og = out->origin;
  if (og->n_r < 1 || og->n_theta < 1 || og->n_phi < 1) return fail(ART_E_INVALID, "origin bin counts must be >= 1");
  if (og->theta_axis != 0 && og->theta_axis != 1) return fail(ART_E_INVALID, "theta_axis must be 0 (theta) or 1 (cos theta)");
  if (og->mode < 0 || og->mode > 2) return fail(ART_E_INVALID, "origin mode must be 0 (auto), 1 (LDS table) or 2 (global adds)");
  if (!std::isfinite(og->cm) || !std::isfinite(og->sm) || !std::isfinite(og->r_lo) || !std::isfinite(og->r_hi))
    return fail(ART_E_INVALID, "origin: cm, sm and the range of r must be finite");
  const bool r_all = og->n_r == 1 && og->r_lo == 0.0 && og->r_hi == 0.0;
  if (!r_all && !(og->r_lo < og->r_hi)) return fail(ART_E_INVALID, "origin: the range of r needs r_lo < r_hi");
  if (out->groups != 0 && (out->groups < art::REPLICATES_MIN_GROUPS || out->groups > art::REPLICATES_MAX_GROUPS))
    return fail(ART_E_INVALID, "groups must be 0 (one table) or in [2, 64]");
  if (out->observer && out->observer->n_dw != 1) return fail(ART_E_INVALID, "origin: the observer axes need n_dw == 1");
  if ((rc = event_in_ranges(in))) return rc;
  // the observer axes: the sky map's of (n_theta, n_phi, 1) with c_all; without an observer one bin per species over
  // the whole sphere
  const art_sky_spec whole{1, 1, 1, 1, 0, 0.0, 0.0};
  EventSky S;
  if ((rc = event_sky(out->observer ? out->observer : &whole, /*honour_mode=*/false, 0, &S))) return rc;
  int64_t total = (out->groups > 0 ? out->groups : 1) * S.size;  // (S.size <= 2^26, groups <= 64)
  for (const int32_t nb : {og->n_r, og->n_theta, og->n_phi}) {
    if (nb > 2147483647LL / total) return fail(ART_E_INVALID, "origin: the table has 2^31 doubles or more");
    total *= nb;
  }
  if (og->mode == 1 && total > art::SKY_LDS_DOUBLES)
    return fail(ART_E_INVALID, "origin mode 1: the table exceeds the LDS budget of 8192 doubles");
  if (!out->hist || !out->misplaced) return fail(ART_E_INVALID, "hist or misplaced is NULL");
  if (in->n_events == 0) return ART_OK;
  // IN_NODE_START_LATE and IN_CYC_END_STATES: the moments call's checks, whose chunk and re-run this call is handed;
  // the kernel reads cyc_tau alone.
  if ((rc = event_in_buffers(in, node_start, IN_NODE_START_LATE | IN_CYC_END_STATES))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  const art::OriginAxes O{{og->n_r, og->n_theta, og->n_phi}, r_all ? 1 : 0, og->theta_axis, og->r_lo, og->r_hi, og->cm,
                          og->sm};
  art::EventOriginArgs r{};
  r.node_start = node_start; r.n_groups = out->groups; r.n_origin = og->n_r * og->n_theta * og->n_phi;
  r.table = S.size * r.n_origin;
  r.hist = out->hist; r.bin_out = out->bin_out; r.power_out = out->power_out; r.misplaced = out->misplaced;
  HIP_OK(art::launch_event_origin(a, r, S.A, S.cos_axis, O, og->mode, (hipStream_t)stream));
  return ART_OK;
}

// The exact tables (include/art.h; art_exact.h): values into fixed-point accumulators, one per bin, which every call
// leaves normalised.
int art_exact_histogram_device(int64_t n, const int32_t* bins, const double* values, int32_t n_bins, int64_t* acc,
                               double* nonfinite, int32_t mode, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (n < 0) return fail(ART_E_INVALID, "n must be >= 0");
  if (n_bins < 1 || n_bins > (1 << 24)) return fail(ART_E_INVALID, "n_bins must be in [1, 2^24]");
  if (mode < 0 || mode > 2) return fail(ART_E_INVALID, "exact mode must be 0 (auto), 1 (LDS accumulators) or 2 (global adds)");
  if (mode == 1 && n_bins > art::EXACT_LDS_BINS)
    return fail(ART_E_INVALID, "exact mode 1: more than the 124 accumulators that fit the LDS budget");
  if (n == 0) return ART_OK;
  if (!bins || !values || !acc || !nonfinite) return fail(ART_E_INVALID, "NULL buffer");
  int rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  const bool lds = mode == 1 || (mode == 0 && n_bins <= art::EXACT_LDS_BINS);
  HIP_OK(art::launch_exact_histogram(n, bins, values, n_bins, acc, nonfinite, lds, (hipStream_t)stream));
  return ART_OK;
}

int art_exact_finish_device(int64_t n_bins, const int64_t* acc, double* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (n_bins < 0) return fail(ART_E_INVALID, "n_bins must be >= 0");
  if (n_bins == 0) return ART_OK;
  if (!acc || !out) return fail(ART_E_INVALID, "NULL buffer");
  int rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  HIP_OK(art::launch_exact_finish(n_bins, acc, out, (hipStream_t)stream));
  return ART_OK;
}

// the host twins: art_exact.h's functions on host arrays of limbs; no device is touched
int art_exact_add_host(int64_t n, const int32_t* bins, const double* values, int32_t n_bins, int64_t* acc,
                       int64_t* nonfinite) {
  if (n < 0 || n_bins < 1) return fail(ART_E_INVALID, "n must be >= 0 and n_bins >= 1");
  if (n > 0 && (!values || !acc)) return fail(ART_E_INVALID, "NULL buffer");
  int64_t since = 0, bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t b = bins ? bins[i] : 0;
    if (b < 0 || b >= n_bins) continue;
    if (!art::exact_add(acc + (int64_t)b * art::EXACT_LIMBS, values[i])) ++bad;
    if (++since == art::EXACT_MAX_ADDS) {  // (the headroom rule)
      for (int32_t q = 0; q < n_bins; ++q) art::exact_normalize(acc + (int64_t)q * art::EXACT_LIMBS);
      since = 0;
    }
  }
  if (n > 0)
    for (int32_t q = 0; q < n_bins; ++q) art::exact_normalize(acc + (int64_t)q * art::EXACT_LIMBS);
  if (nonfinite) *nonfinite += bad;
  return ART_OK;
}

int art_exact_normalize_host(int64_t n_bins, int64_t* acc) {
  if (n_bins < 0 || (n_bins > 0 && !acc)) return fail(ART_E_INVALID, "n_bins must be >= 0 and acc given");
  for (int64_t q = 0; q < n_bins; ++q) art::exact_normalize(acc + q * art::EXACT_LIMBS);
  return ART_OK;
}

int art_exact_round_host(int64_t n_bins, const int64_t* acc, double* out) {
  if (n_bins < 0 || (n_bins > 0 && (!acc || !out))) return fail(ART_E_INVALID, "n_bins must be >= 0, acc and out given");
  for (int64_t q = 0; q < n_bins; ++q) out[q] = art::exact_round(acc + q * art::EXACT_LIMBS);
  return ART_OK;
}

// The exact tables of a chunk (include/art.h): the run's, a coupling scan's or a halo scan's powers into fixed-point
// accumulators (art_exact.h), one kernel per set and the normalisation on `stream`.
int art_event_exact_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                           const art_event_exact_out* out, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (!in || !out) return fail(ART_E_INVALID, "NULL in or out");
  if (out->kind < 0 || out->kind >= art::REP_KIND_COUNT)
    return fail(ART_E_INVALID, "kind must be 0 (the run), 1 (a coupling scan) or 2 (a halo scan)");
  if (out->n_sets < 1 || out->n_sets > art::REPLICATES_MAX_SETS) return fail(ART_E_INVALID, "n_sets must be in [1, 32]");
  if (out->kind == art::REP_KIND_RUN && out->n_sets != 1) return fail(ART_E_INVALID, "n_sets must be 1 with kind 0");
  if (out->kind == art::REP_KIND_COUPLING && in->n_nodes > 0 && !out->node_factor)
    return fail(ART_E_INVALID, "node_factor is NULL (kind 1: the coupling scan's weights)");
  if (out->kind != art::REP_KIND_RUN && !out->event_factor)
    return fail(ART_E_INVALID, "event_factor is NULL (kind 1: the coupling scan's back, kind 2: the halo scan's ratio)");
  if (out->mode < 0 || out->mode > 2) return fail(ART_E_INVALID, "exact mode must be 0 (auto), 1 (LDS accumulators) or 2 (global adds)");
  if ((rc = event_in_ranges(in)) || (rc = event_out_ranges(0, out->nbins))) return rc;  // (no reserved field)
  constexpr int lds_nbins = art::EXACT_LDS_FLUX_BINS;
  if (out->mode == 1 && out->nbins > lds_nbins)
    return fail(ART_E_INVALID, "exact mode 1: a flux table of more than 56 bins exceeds the LDS budget");
  EventSky S;
  if ((rc = event_sky(out->sky, /*honour_mode=*/false, out->nbins, &S))) return rc;  // (the sky accumulators stay in HBM)
  if (in->n_events == 0) return ART_OK;
  if (!out->totals_acc || !out->nonfinite || !out->misplaced) return fail(ART_E_INVALID, "totals_acc, nonfinite or misplaced is NULL");
  if (out->nbins > 0 && !out->flux_acc) return fail(ART_E_INVALID, "flux_acc is NULL");
  if (out->sky && !out->sky_acc) return fail(ART_E_INVALID, "sky_acc is NULL");
  // IN_NODE_START_LATE and IN_CYC_END_STATES: the replicates call's checks
  if ((rc = event_in_buffers(in, node_start, IN_NODE_START_LATE | IN_CYC_END_STATES))) return rc;
  DeviceCtx* ctx;
  if ((rc = current_ctx(&ctx))) return rc;
  const art::EventRowsArgs a = event_args(p, in, /*end_states=*/false);
  art::EventExactArgs r{};
  r.node_start = node_start; r.kind = out->kind; r.n_k = out->n_sets; r.nbins = out->nbins; r.sky_size = S.size;
  r.node_factor = out->node_factor; r.event_factor = out->event_factor;
  r.flux = out->flux_acc; r.sky = out->sky ? out->sky_acc : nullptr; r.totals = out->totals_acc;
  r.nonfinite = out->nonfinite; r.misplaced = out->misplaced;
  const int path = out->mode == 2 ? 0 : (out->mode == 1 || out->nbins <= lds_nbins) ? 2 : 1;
  HIP_OK(art::launch_event_exact(a, r, S.A, S.cos_axis, path, (hipStream_t)stream));
  return ART_OK;
}

int art_eval_rhs_device(const art_params* p, int64_t n, const double* u, const double* tau, const double* erg,
                        const int8_t* species, double* du, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (n == 0) return ART_OK;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  HIP_OK(art::launch_eval_rhs(art::make_kparams(*p), n, u, tau, erg, species, du, (hipStream_t)stream));
  return ART_OK;
}

int art_eval_hamiltonian_device(const art_params* p, int64_t n, const double* x, const double* k, const double* T,
                                const double* E, double* H, double* dHdx, double* dHdk, double* dHdT, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (n == 0) return ART_OK;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  HIP_OK(art::launch_eval_hamiltonian(art::make_kparams(*p), n, x, k, T, E, H, dHdx, dHdk, dHdT, (hipStream_t)stream));
  return ART_OK;
}

int art_eval_condition_device(const art_params* p, int64_t n, const double* u, const double* tau, double* out,
                              void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (n == 0) return ART_OK;
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  HIP_OK(art::launch_eval_condition(art::make_kparams(*p), n, u, tau, out, (hipStream_t)stream));
  return ART_OK;
}

int art_eval_cyclotron_device(const art_params* p, int64_t n, const double* pos, const double* k, const double* t,
                              double* wc, double* tau, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = validate(p);
  if (rc) return rc;
  if (n == 0) return ART_OK;
  if (n < 0 || n > 2147483647LL) return fail(ART_E_INVALID, "n must be in [0, 2^31)");
  if (!pos || !k || !t || !wc || !tau) return fail(ART_E_INVALID, "NULL buffer");
  DeviceCtx* c;
  if ((rc = current_ctx(&c))) return rc;
  HIP_OK(art::launch_eval_cyclotron(art::make_kparams(*p), n, pos, k, t, wc, tau, (hipStream_t)stream));
  return ART_OK;
}

int art_eval_math_device(int32_t fn, int32_t tu, int64_t n, const double* a, const double* b, double* out0,
                         double* out1, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (fn < 0 || fn >= ART_MATH_COUNT) return fail(ART_E_INVALID, "unknown fn (ART_MATH_*)");
  if (tu != 0 && tu != 1) return fail(ART_E_INVALID, "tu must be 0 or 1");
  if (n < 0 || n > 2147483647LL) return fail(ART_E_INVALID, "n must be in [0, 2^31)");
  if (n == 0) return ART_OK;
  const bool two = fn == ART_MATH_MAX_ABS || fn == ART_MATH_MIN_Q || fn == ART_MATH_MAX_Q || fn == ART_MATH_RCLAMP;
  if (!a || (two && !b)) return fail(ART_E_INVALID, "NULL operand");
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  HIP_OK(art::launch_eval_math(fn, tu, n, a, b, out0, out1, (hipStream_t)stream));
  return ART_OK;
}

}  // extern "C"
