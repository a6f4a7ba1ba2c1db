// art_internal.h -- the launch wrappers and record layouts shared by the two kernel translation
// units (art_kernels.hip, art_kernels_nolicm.hip), their headers and the host units (art_host.h).
#pragma once
#include <hip/hip_runtime.h>

#include "art_core.h"
#include "art_halo.h"
#include "art_launch_plan.h"
#include "art_pieces.h"
#include "art_tree_step.h"

namespace art {
// Segment inputs / outputs (device pointers, SoA), see art_segment_out / art_crossing_buf.
struct SegIn {
  const double *x0, *k0, *erg, *dw, *lnt0;
  const int8_t* species;
  // device scratch filled by the init pass: one U0_REC-double fresh-state record per ray
  // (fresh_rec below), so a refilling lane reads its ray with 10 16-byte loads from two lines
  double* u0;
};

struct SegOut {
  double *x_end, *k_end, *u7_end, *tau_end;
  int32_t *status, *n_acc, *n_rej;
  int32_t cap;
  int32_t* xcount;
  double *xpos, *xk, *xt, *xdw, *xp;
  // saveat (RayTracer.jl:176, 383), only with ntimes >= 2: ntimes points per ray, positions
  // [(c * ntimes + k) * n + ray] (spherical from the integrator, Cartesian after finalize),
  // ln t [k * n + ray], and the number of points of each ray
  int32_t ntimes;
  double *traj, *traj_t;
  int32_t* traj_n;
  // END_REC doubles of device scratch per ray: the integrator's raw end state as one AoS
  // record per ray, [u (7) | tau | int4 {status, n_acc, n_rej, ncross} | int4 {traj_n, 0, 0, 0}],
  // which finalize_kernel spreads into the SoA outputs above with coalesced stores. A finishing
  // lane then writes 5 (saveat: 6) 16-byte stores into its own 128-byte line instead of 12
  // 4/8-byte stores into as many partly written lines.
  double* rec;
  // X_REC doubles of device scratch per (ray, crossing j < cap), the same idea for the
  // crossings affect! records: [x (3) | k (3) | t | Δω] at ((ray cap + j) X_REC), spread into
  // xpos / xk / xt / xdw by finalize_kernel
  double* xrec;
  // Tail donation (art_set_tail_donation): once the queue is drained, a wave whose live rays
  // (all at a step boundary) number at most `donate` writes their complete integrator state
  // as CONT_REC-double records to cont[] (count in *cont_count) and retires, so its CU slot
  // goes to the next launch in flight; a continuation launch (cont_mode = 1) then integrates
  // those rays packed into full waves, bit for bit as if they had never moved.
  double* cont;
  unsigned long long* cont_count;
  unsigned long long* cont_queue;
  int32_t donate, cont_mode;
  // the continuation launch (cont_mode = 1) reads the records from cont_src (count
  // *cont_src_count) and may itself donate its own drained waves' last rays into cont /
  // cont_count: the second level, which tail_kernel resumes one ray per wave
  const double* cont_src;
  const unsigned long long* cont_src_count;
  double* cont2;  // the second-level records (set on the launch's SegOut; read by launch_propagate)
  unsigned long long *cont2_count, *cont2_queue;
  // 1: finalize_kernel writes NaN into the crossing slots j >= min(count, cap) (the *_host
  // entry points' contract, include/art.h), so no fill of the outputs is needed beforehand
  int32_t nan_fill;
  // The streamed host pipeline (propagate_kernel<..., DON = 3>, art_propagate_host): piece
  // p = piece_of(pieces, ray) (art_pieces.h: coarse pieces, then fine ones over the batch's last
  // rays); every finished ray counts into piece_cnt[p]; a wave that waits too
  // long (STREAM_WAIT_TICKS of s_memrealtime) raises *abort_word and stops taking rays.
  unsigned long long* piece_cnt;
  unsigned int* abort_word;
  // the launch's work-queue word: a helper that sees the call given up adds 2^40 to it, so every
  // integrator wave's next chunk claim finds the queue drained and the launch runs out at once
  unsigned long long* queue_word;
  unsigned long long wait_ticks;  // a wave's bound on a chunk flag (STREAM_WAIT_TICKS; tests set less)
  Pieces pieces;
  // The maskless streamed pipeline (DON = 3, art_host_stream.cpp StreamCall): one launch
  // over the whole batch holds every CU; its first `helpers` blocks are helpers, not
  // integrators. *host_ready (host memory, raised by the host as each piece's copies land)
  // counts rays whose inputs are in HBM. Helpers claim 1024-ray tiles (HELPER_TILE) to initialise
  // (*init_next, init_one) and set chunk_ready[c] for each 64-ray chunk they finish; an
  // integrator wave that claims a chunk waits for its flag. Finished rays count into
  // piece_cnt[p] as in DON = 2; once a piece is complete, helpers claim its tiles to finalize
  // (*fin_next, finalize_one) into the piece's SoA blob (blob + piece_blob_off, piece_blob), and
  // the block that finalizes a piece's last tile sets host_flags[p] (host memory the host
  // polls, then copies the blob out). The helpers are a separate persistent kernel on a stream of
  // their own; one helper pass over every block slot initialises the first rays before the
  // integrator starts, and another finalizes the rest after it.
  const unsigned long long* host_ready;
  unsigned long long* host_flags;
  unsigned long long *init_next, *fin_next;
  unsigned long long* piece_fin;
  unsigned* chunk_ready;
  char* blob;
  int32_t blob_host;  // 1: the blobs are pinned host memory the helpers write over PCIe (no download copies)
  int32_t helpers;
  // The end of a streamed call without the integrator's stream (art_host.h, HostLane): the
  // helpers bin the radiated flux of the rays they finalize (flux_hist, 2 flux_nbins doubles of
  // device memory, flux_nbins <= FLUX_HELPER_BINS; 0 = none), every integrator wave counts itself
  // into *waves_started as it starts and into *waves_done after its statistics, and the last of the
  // exit_expected serving helper blocks to leave (*exit_count) -- every ray is done by then -- waits
  // until every started wave is done (blocks the next call's kernels kept from starting find the
  // queue drained and add nothing), then copies the statistics (stats[0, N_STATS_DEV)) and the flux
  // into host memory (done_host[DONE_STATS...], [DONE_FLUX...]) and raises done_host[0]. The host
  // then has the call's results without waiting on a stream.
  double* flux_hist;
  int32_t flux_nbins;
  unsigned long long* done_host;
  unsigned long long *exit_count, *waves_started, *waves_done;
  int32_t exit_expected;
  // (calls in flight) the wave that starts last of the integrator's waves_total stores
  // resident_value into host-mapped *resident_host: the next call launches its own init pass and
  // integrator only then, so its blocks queue behind this launch's instead of sharing the GPU with it
  unsigned long long* resident_host;
  unsigned long long resident_value;
  int32_t waves_total;
  // Small batches (art_device.cpp, propagate_device_impl): 1 = every fresh ray goes straight to
  // tail_kernel, one wave per ray (pack_fresh_kernel writes their CONT_REC records to cont),
  // instead of one lane per ray of the persistent integrator
  int32_t small_tail;
  // Graduation (DON = 1 launches with tail_kernel): a ray that has taken `graduate` step
  // attempts leaves its lane for the tail kernel at its next step boundary -- one wave per ray
  // from then on -- without waiting for its wave to drain: CONT_REC records in grad[0, grad_cap)
  // (count in *grad_count, which may pass grad_cap: a ray that finds no slot stays where it is),
  // taken by tail_kernel ahead of the drained waves' records. 0 = off.
  double* grad;
  unsigned long long *grad_count, *grad_queue;
  int32_t grad_cap, graduate;
  // Early graduation (DON = 1 launches with tail_kernel, art_device.cpp): a ray whose progress
  // in ln t since its start is below hot_dtau + hot_slope log2(attempts / 256) -- tested at every
  // power-of-two attempt count >= hot_at, and when its drained wave donates it -- leaves for
  // hot[0, hot_cap) at once: the count in *hot_count (it may pass hot_cap: a ray that finds no
  // slot stays where it is), each record's hot_ready word raised once it is written.
  // configs[3]'s longest rays crawl along the star's surface and are singled out this way
  // (tail_kernel "hot rays"). A tail_kernel launch beside the bulk pass and the
  // continuation claims them through *hot_queue as they arrive, until *hot_done (raised after
  // the continuation) and none is left. hot_at 0 = off.
  double* hot;
  unsigned long long *hot_count, *hot_queue;
  unsigned* hot_ready;
  unsigned* hot_done;
  int32_t hot_cap, hot_at;
  double hot_dtau, hot_slope;
  // The bulk pass's claim order with early graduation (launch_propagate sorts it; null: ray index
  // order): the rays by their initial step size, smallest first -- configs[3]'s 20 longest rays
  // are among the 1066 with the smallest (tools/exp_gr_predict.py), so they start at once and reach
  // their hot test within the first few milliseconds. order_tmp: claim_order_bytes(n) of scratch.
  const int32_t* order;
  void* order_tmp;
  // The cyclotron-resonance observation (art_propagate_cyclotron_*; null: none): per ray the summed
  // optical depth of its crossings of ω_c = ω and their number (both zeroed before the launch; the
  // integrator adds to them in place), and the first crossing's Cartesian position [c * n + ray]
  // and ln t (unwritten where the count stays 0).
  double* cyc_tau;
  int32_t* cyc_count;
  double *cyc_pos, *cyc_lnt;
};
constexpr unsigned long long STREAM_WAIT_TICKS = 200000000ull;  // 2 s at 100 MHz
constexpr int FLUX_HELPER_BINS = 256;  // flux bins the helpers bin themselves (2 x 256 doubles of LDS)
constexpr int DONE_STATS = 1, DONE_FLUX = 16;  // done_host layout: [0] flag | [1, 11) statistics | [16, 16 + 2 nbins) flux
constexpr int CHUNK = 64;  // rays a persistent wave claims from the queue at once
constexpr int HELPER_TILE = 1024;  // rays a helper block initialises or finalizes per claim
// The fresh state of ray i at u0 + i U0_REC (init_one writes it, a refilling integrator lane
// reads it): [u0 (7) | f(u0) (7) | dt | c0 | erg | ln t0 | species | 0], 160 bytes, 32-byte aligned.
constexpr int U0_REC = 20;
constexpr int END_REC = 16;
constexpr int X_REC = 8;
constexpr int CONT_REC = 24;  // [u (7) | f (7) | τ, dt, qpow, cprev, bstart, erg | int4 {ray, n_acc, n_rej, ncross} | int4 {iter, sprev, flags, save_k}]
constexpr int N_STATS = 8;  // propagate statistics: attempts, accepted, root re-steps, scan evals,
                            // interpolant-root evals, rays, init RHS, certified steps (art_last_stats)
// ... followed by the integrator's span from in-kernel clock stamps (s_memrealtime, the device's
// 100 MHz constant clock): [8] the max over waves of ~(start), [9] the max of the end
constexpr int ST_T0 = 8, ST_T1 = 9, N_STATS_DEV = 10;
constexpr double STAMP_TICKS_PER_MS = 1e5;
int persistent_blocks(const void* func, int64_t work, int block, int fallback_per_cu);
// propagate = init (u0 of every ray) -> the persistent integrator -> finalize (Cartesian
// end state, conversion probability at the crossings); ev0/ev1 (may be null) bracket the
// integrator kernels alone. With fs (and ev1) given, finalize runs on stream fs after ev1,
// so s can go on with its next launch while the outputs are written (the chunked host
// pipeline writes them over PCIe into pinned memory).
// hs: the side stream of the hot rays' tail launch (SegOut::hot), its fork and join events and two
// zeroed device words; without them the launch does not graduate early.
struct HotSide {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  unsigned long long* zero_word = nullptr;
};
size_t claim_order_bytes(int64_t n);
// 200 ms at 100 MHz: a hot wave that has waited this long for a record leaves (the records still
// to come, if any, go to the tail launch after the continuation). In a 10^6-ray GR launch the
// hot records arrive within the first ~70 ms; a profiler that serialises kernels runs the
// continuation, and so the raising of *hot_done, only after this launch has ended.
constexpr unsigned long long HOT_WAIT_TICKS = 20000000ull;
constexpr int HOT_BLOCKS = 32;  // the hot rays' tail launch: 32 blocks of 4 waves (one ray a wave)
// pin: the launch's plan inputs (art_launch_plan.h; the caller laid the scratch out from plan_launch(pin));
// launch_propagate adds the bulk kernel's occupancy, launches what the plan then names and returns
// that plan in *ran (may be null). A plan that names a build nobody instantiated is an error.
hipError_t launch_propagate(const KParams& P, int64_t n, const SegIn& in, const SegOut& out, int32_t max_crossings,
                            unsigned long long* queue, unsigned long long* stats, hipStream_t s, const LaunchPlanIn& pin,
                            LaunchPlan* ran, hipEvent_t ev0, hipEvent_t ev1, hipStream_t fs = nullptr,
                            const HotSide& hs = HotSide());
// The streamed host pipeline's integrator (DON = 3) with at most `blocks` persistent blocks
// (plan_streamed; *ran, may be null: the plan it launched).
hipError_t launch_integrator_streamed(const KParams& P, int64_t n, const SegIn& in, const SegOut& out,
                                      int32_t max_crossings, unsigned long long* queue, unsigned long long* stats,
                                      int blocks, hipStream_t s, LaunchPlan* ran);
// The maskless streamed pipeline's helper duty (helper_kernel HK_TILES, SegOut::host_ready ...):
// `blocks` blocks; init_limit >= 0 initialises only (tiles below it), -1 serves to the end;
// announce counts each block into host_flags[64] as it starts.
hipError_t launch_helpers(const KParams& P, int64_t n, const SegIn& in, const SegOut& out, int blocks, int64_t init_limit,
                          int announce, unsigned long long* stats, hipStream_t s);
// The geometry a kernel is instantiated for: the GEOM_* of art_step.h (0 any, 1 flat, 2 GR). The one
// classification both translation units select their instantiations by.
int geom_of(const KParams& P);
// The helper kernel (art_helper.h, built in art_kernels_nolicm.hip): the instantiation for these
// parameters' geometry, and its waves per SIMD (2: a helper block shares its CU with one
// integrator block; 1: it takes the whole CU).
using HFn = void (*)(const KParams, const int64_t, const SegIn, const SegOut, const int, const int64_t, const int64_t,
                     const int64_t, const int, unsigned long long*);
HFn pick_helper(const KParams& P);
// The integrator (propagate_kernel) and tail kernel builds of art_kernels_nolicm.hip: every geometry
// but flat's (nullptr for a combination no path launches). integ: ART_VERN6 / ART_RK4; geom: the
// GEOM_* of art_step.h (geom_of); don: the donation mode; wps: waves per SIMD.
using KFn = void (*)(const KParams, const int64_t, const SegIn, const SegOut, const int32_t, unsigned long long*,
                     unsigned long long*);
using TFn = void (*)(const KParams, const int64_t, const SegIn, const SegOut, const int32_t, const int32_t,
                     unsigned long long*);
// (the lists: ART_BUILDS_NL, ART_BUILDS_NL_CYC and ART_BUILDS_TAIL of art_launch_plan.h)
KFn nl_propagate(int integ, int geom, bool save, int don, int wps);
KFn nl_propagate_cyc(int geom, int don);  // (Vern6 with the cyclotron observation, SegOut::cyc_tau)
TFn nl_tail(int geom);
// the sampler (find_samples_new) builds, also in art_kernels_nolicm.hip: wps 2 or 3 waves per SIMD,
// blocks: the blocks-of-steps line scan
using SFn = void (*)(const KParams, const double, const uint64_t, const int64_t, const int64_t, double*, double*,
                     double*, double*, int32_t*, int32_t*, unsigned long long*);
SFn nl_sample(int wps, bool blocks);
// the same builds with the halo velocity model (sample_kernel's HALO, art_halo.h): one more
// argument, the proposal's speed scale
using SHFn = void (*)(const KParams, const double, const uint64_t, const int64_t, const int64_t, double*, double*,
                      double*, double*, int32_t*, int32_t*, unsigned long long*, const double);
SHFn nl_sample_halo(int wps, bool blocks);
int helper_waves_per_simd(const KParams& P);
// The batch size up to which launch_propagate runs every ray on a wave of its own (tail_kernel):
// ART_SMALL_TAIL, default one ray per SIMD of the device; 0 switches it off. (Flat space and Schwarzschild:
// the general geometry has no tail kernel, art_launch_plan.h.)
int64_t small_tail_limit();
hipError_t launch_sample(const KParams& P, double maxR, uint64_t seed, int64_t ray_offset, int64_t n, double* x,
                         double* k, double* erg, double* vifty, int32_t* w, int32_t* att, unsigned long long* queue,
                         hipStream_t s, int waves, const HaloK* halo = nullptr);  // halo: the HALO builds
hipError_t launch_prob(const KParams& P, int64_t nc, const double* pos, const double* kpos, const double* erg,
                       int64_t n_groups, const int64_t* gstart, double* out, hipStream_t s);
hipError_t launch_flux(const KParams& P, int64_t n, const double* x_end, const double* k_end, const int32_t* status,
                       const int8_t* species, const double* w, int32_t nbins, double* hist, hipStream_t s);
hipError_t launch_flux_phi(int64_t n, const double* phi, const int8_t* species, const double* w, int32_t nbins,
                           double lo, double hi, double* hist, hipStream_t s);
// Sky maps (sky_map_kernel, sky_map_segments_kernel): n[d] equal bins over [lo[d], hi[d]] on each of
// the three axes; c_all: the third axis is one bin holding every finite value (n[2] = 1).
struct SkyAxes {
  int32_t n[3];
  int32_t c_all;
  double lo[3], hi[3];
};
// The origin axes of an emission map (origin_bin_of, art_event_origin.h): n the bins of r, θ and φ of the event's
// sampled point turned about y by (cm, sm); theta_axis 0 θ over [0, π], 1 cos θ over [-1, 1]; r over [r_lo, r_hi],
// or r_all: one bin holding every finite r (n[0] = 1).
struct OriginAxes {
  int32_t n[3];
  int32_t r_all, theta_axis;
  double r_lo, r_hi, cm, sm;
};
// The largest table (2 n[0] n[1] n[2] doubles) a block keeps in LDS: 64 KiB, which leaves two
// blocks on a CU's 160 KiB; larger tables are added to in HBM.
constexpr int64_t SKY_LDS_DOUBLES = 8192;
constexpr int64_t SKY_MAX_DOUBLES = (int64_t)1 << 26;
// mode: 0 by the table's size, 1 the LDS table (the table must fit), 2 adds to HBM
hipError_t launch_sky_map(int64_t n, const double* a, const double* b, const double* c, const int8_t* species,
                          const double* w, const SkyAxes& A, int mode, double* hist, hipStream_t s);
hipError_t launch_sky_map_segments(const KParams& P, int64_t n, const double* x_end, const double* k_end,
                                   const double* u7_end, const int32_t* status, const int8_t* species, const double* w,
                                   const double* dw_offset, const SkyAxes& A, int cos_axis, int mode, double* hist,
                                   int32_t* bin_out, hipStream_t s);
hipError_t launch_eval_rhs(const KParams& P, int64_t n, const double* u, const double* tau, const double* erg,
                           const int8_t* species, double* du, hipStream_t s);
hipError_t launch_eval_hamiltonian(const KParams& P, int64_t n, const double* x, const double* k, const double* T,
                                   const double* E, double* H, double* dHdx, double* dHdk, double* dHdT,
                                   hipStream_t s);
hipError_t launch_event_weight(const KParams& P, int64_t n, const double* x, const double* k, const double* v,
                               double maxR, double rho, double mcmc, double* out, hipStream_t s,
                               const HaloK* halo = nullptr);  // halo: event_weight_halo_kernel
hipError_t launch_eval_condition(const KParams& P, int64_t n, const double* u, const double* tau, double* out,
                                 hipStream_t s);
hipError_t launch_eval_cyclotron(const KParams& P, int64_t n, const double* x, const double* k, const double* t,
                                 double* wc, double* tau, hipStream_t s);
// art_eval_math_device: fn an ART_MATH_* id; tu 0 the kernel of art_kernels.hip, 1 the same one
// compiled in art_kernels_nolicm.hip (nl_eval_math)
using MFn = void (*)(const int64_t, const double*, const double*, double*, double*);
MFn nl_eval_math(int fn);
hipError_t launch_eval_math(int fn, int tu, int64_t n, const double* a, const double* b, double* out0, double* out1,
                            hipStream_t s);
// The device-resident tree driver (art_grow_trees_device; kernels in art_kernels.hip, the per-tree
// rules in art_tree_step.h). One round's propagate inputs and outputs, device pointers, SoA with
// the round's batch size as the stride:
struct TreeBatch {
  double *x0, *k0, *erg, *dw, *lnt0;
  int8_t* species;
  double *x_end, *k_end, *u7_end, *tau_end;
  int32_t *status, *n_acc, *n_rej;
  int32_t* xcount;
  double *xpos, *xk, *xt, *xdw, *xp;
};
// scratch of the driver's two scans (over at most n trees)
size_t tree_scan_bytes(int64_t n);
// state, root events (stack, R.stack_cap per tree) and round 1's selection: list[i] = i, flag 1, pos i + 1
hipError_t launch_tree_roots(const KParams& P, const TreeRules& R, int64_t n, const double* x0, const double* k0,
                             const double* erg, const int8_t* species, TreeState* state, TreeEv* stack, int32_t* list,
                             int32_t* flag, int32_t* pos, hipStream_t s);
// pop and pack: the flagged entries of list_prev[0, m_prev) into this round's list and batch B of m
hipError_t launch_tree_pack(const TreeRules& R, int64_t m_prev, int64_t m, const int32_t* list_prev, const int32_t* flag,
                            const int32_t* pos, int32_t* list, TreeState* state, const TreeEv* stack, const TreeBatch& B,
                            double dt0, double ln_dt0, hipStream_t s);
// the step of the m trees of list: nodes into log[0, m), flag[j] whether tree list[j] goes on, pos the
// inclusive scan of flag (pos[m - 1]: the next round's batch size), *err raised on a stack overflow
hipError_t launch_tree_step(const KParams& P, const TreeRules& R, int64_t n, int64_t m, const int32_t* list, TreeState* state,
                            TreeEv* stack, const TreeBatch& B, art_tree_node* log, int32_t* flag, int32_t* pos,
                            int32_t* err, void* tmp, size_t tmp_bytes, hipStream_t s);
// counts / infos (either may be null), and node_start[0, n] as the exclusive scan of the counts (counts1: n + 1 ints)
hipError_t launch_tree_finish(const TreeRules& R, int64_t n, const TreeState* state, int32_t* counts1, int32_t* counts,
                              int32_t* infos, int64_t* node_start, void* tmp, size_t tmp_bytes, hipStream_t s);
// the log's `total` records into nodes (capacity records) at node_start[tree] + sequence
hipError_t launch_tree_flatten(int64_t total, const art_tree_node* log, const int64_t* node_start, int64_t capacity,
                               art_tree_node* nodes, hipStream_t s);
// Event rows (art_event_rows_device, art_event_gather_photons_device; event_rows_kernel and the row
// math of art_event_rows.h). Device pointers; art_event_rows_in / _out of include/art.h flattened,
// with pos the exclusive sum of is_final != 0 over the node records.
struct EventRowsArgs {
  int64_t n_events, event_offset, n_nodes, row_capacity, cyc_n;
  const double *x, *k_init, *weight5;
  const int32_t* attempts;
  const art_tree_node *back, *nodes;
  const int32_t *back_counts, *counts, *infos, *pos, *cyc_slot;
  const double *cyc_tau, *cyc_x_end, *cyc_k_end, *cyc_u7_end, *cyc_tau_end;
  const int32_t* cyc_status;
  double mass_a;
  int32_t ncols, nbins;
  double *rows, *flux, *sky_hist, *totals;
  int32_t* bin_out;
};
// scratch of the scans over n_nodes records; pos[i] = final (or final photon) nodes before record i
size_t event_scan_bytes(int64_t n_nodes);
hipError_t launch_event_scan(int64_t n_nodes, const art_tree_node* nodes, bool photons_only, int32_t* pos, void* tmp,
                             size_t tmp_bytes, hipStream_t s);
// final photon node i into slot pos[i] of the batch B of m segments (x0, k0, erg, dw, lnt0, species), slot[i] = pos[i] or -1
hipError_t launch_event_gather(int64_t n_nodes, const art_tree_node* nodes, const int32_t* pos, int64_t n_events,
                               const double* erg, int64_t m, const TreeBatch& B, int32_t* slot, double dt0, double ln_dt0,
                               hipStream_t s);
// rows, flux, sky map (A, cos_axis, mode as launch_sky_map_segments; sky_hist null: none) and totals in one pass
hipError_t launch_event_rows(const EventRowsArgs& a, const SkyAxes& A, int cos_axis, int mode, hipStream_t s);
// Event moments (art_event_moments_device; the kernels and the per-tree group-by of art_event_moments.h):
// the inputs are an EventRowsArgs (its outputs unused); node_start (n_events + 1) the forest's ranges,
// the tables of art_event_moments_out (sky_sq null: no sky tables) and entries, n_nodes MomentEntry of
// scratch (16 B each).
struct MomentEntry;
struct EventMomentsArgs {
  const int64_t* node_start;
  int32_t nbins;
  double *flux_sq, *flux_xa, *sky_sq, *sky_xa, *totals;
  MomentEntry* entries;
};
hipError_t launch_event_moments(const EventRowsArgs& a, const EventMomentsArgs& m, const SkyAxes& A, int cos_axis,
                                hipStream_t s);
// The coupling scan (art_event_reweight_device; the kernels and the per-tree reweight of
// art_event_reweight.h): the inputs are an EventRowsArgs (its outputs unused), the forests' erg and
// node_start; s the n_k scales (g_k / g0)². W (n_k n_nodes), B (n_k n_events) and X0 (n_nodes) are
// caller memory or scratch; flux, sky (sky_size per coupling; null: none) and totals are art_event_reweight_out's.
// mtotals null: no second moments; else Pw (n_k n_nodes) and entries (n_nodes) of scratch and the moment tables.
struct EventReweightArgs {
  const int64_t* node_start;
  const double* erg;
  int32_t mc_nodes, n_k, nbins;
  int64_t sky_size;
  double s[32];
  double *W, *B, *Bp, *X0;  // (Bp: n_k n_events, the back factors' first factor; null: not wanted)
  double *flux, *sky, *totals;
  double *Pw, *flux_sq, *flux_xa, *sky_sq, *sky_xa, *mtotals;
  MomentEntry* entries;
};
// P: the forward forest's parameters (g0), Pb: the backtrace's (B0 negated)
hipError_t launch_event_reweight(const KParams& P, const KParams& Pb, const EventRowsArgs& a, const EventReweightArgs& r,
                                 const SkyAxes& A, int cos_axis, hipStream_t s);
// The halo scan (art_event_halo_scan_device; the kernels of art_event_haloscan.h): the inputs are an
// EventRowsArgs (its outputs unused), the sampler's vifty (3 n_events, SoA) and the forest's node_start;
// base and models[0, n_k) travel in the kernel arguments (33 x 5 doubles). R (n_k n_events) is caller
// memory or scratch; flux, sky (sky_size per model; null: none) and totals are art_event_halo_scan_out's.
// mtotals null: no second moments; else Pw (n_k n_nodes) and entries (n_nodes) of scratch and the moment tables.
constexpr int HALO_SCAN_MAX_MODELS = 32;
struct EventHaloScanArgs {
  const int64_t* node_start;
  const double* vifty;
  int32_t n_k, nbins;
  int64_t sky_size;
  HaloK base, models[HALO_SCAN_MAX_MODELS];
  double* R;
  double *flux, *sky, *totals;
  double *Pw, *flux_sq, *flux_xa, *sky_sq, *sky_xa, *mtotals;
  MomentEntry* entries;
};
hipError_t launch_event_halo_scan(const EventRowsArgs& a, const EventHaloScanArgs& h, const SkyAxes& A, int cos_axis,
                                  hipStream_t s);
// The jackknife replicates (art_event_replicates_device; the kernel of art_event_replicates.h): the inputs are an
// EventRowsArgs (its outputs unused) and the forest's node_start; kind says whose powers the n_k sets take (0 the
// run's own, 1 a coupling scan's from node_factor (n_k n_nodes) and event_factor (n_k n_events), 2 a halo scan's
// from event_factor). flux, sky (sky_size per set and group; null: none) and totals hold set k's group g at
// k n_groups + g times the usual size; groups is 3 per group.
struct EventReplicatesArgs {
  const int64_t* node_start;
  int32_t n_groups, kind, n_k, nbins;
  int64_t sky_size;
  const double *node_factor, *event_factor;
  double *flux, *sky, *totals, *groups;
};
hipError_t launch_event_replicates(const EventRowsArgs& a, const EventReplicatesArgs& r, const SkyAxes& A, int cos_axis,
                                   hipStream_t s);
// The emission maps (art_event_origin_device; the kernel of art_event_origin.h): the inputs are an EventRowsArgs (its
// outputs unused) and the forest's node_start. One table is `table` = 2 n_obs n_origin doubles, n_origin the origin
// bins n_r n_theta n_phi; hist holds max(n_groups, 1) of them, group g at g table. bin_out and power_out (n_nodes,
// either may be null) and misplaced (1) as art_event_origin_out's. A, cos_axis: the observer axes (c_all); mode as
// launch_sky_map's, for the whole of hist.
struct EventOriginArgs {
  const int64_t* node_start;
  int32_t n_groups, n_origin;
  int64_t table;
  double* hist;
  int32_t* bin_out;
  double *power_out, *misplaced;
};
hipError_t launch_event_origin(const EventRowsArgs& a, const EventOriginArgs& r, const SkyAxes& A, int cos_axis,
                               const OriginAxes& O, int mode, hipStream_t s);
// The coupling x halo grid (art_event_grid_device; the kernel of art_event_grid.h): the inputs are an EventRowsArgs
// (its outputs unused), the forest's node_start and the factors of the two scans of the same chunk, W (n_g n_nodes),
// B (n_g n_events) and R (n_h n_events). The tables are cell-minor (art_event_grid.h): flux (2 nbins x C), totals
// (3 x C), and with n_groups > 0 flux_rep (n_groups x 2 nbins x C), totals_rep (n_groups x 2 x C) and groups (3 per
// group); mtotals (8 x C) null: no moment sums.
struct EventGridArgs {
  const int64_t* node_start;
  int32_t n_g, n_h, nbins, n_groups;
  const double *W, *B, *R;
  double *flux, *totals, *flux_rep, *totals_rep, *groups, *mtotals;
};
hipError_t launch_event_grid(const EventRowsArgs& a, const EventGridArgs& r, hipStream_t s);
// The event power spectrum (art_event_spectrum_device; the kernels of art_event_spectrum.h): the inputs are an
// EventRowsArgs (its outputs unused) and the forest's node_start; kind, node_factor and event_factor as
// EventReplicatesArgs'. count, sum and sum_sq hold (set k, species s) at (2 k + s) (2047 << sub_bits), totals at
// (2 k + s) 8, the lists top_power and top_event (carried in and out) at (2 k + s) top. Scratch: entries, n_nodes
// MomentEntry, and X, n_k 2 n_events doubles, X_{e,s} of set k at (2 k + s) n_events + e.
struct EventSpectrumArgs {
  const int64_t* node_start;
  int32_t kind, n_k, sub_bits, top;
  const double *node_factor, *event_factor;
  double *count, *sum, *sum_sq, *totals, *top_power;
  int64_t* top_event;
  MomentEntry* entries;
  double* X;
};
hipError_t launch_event_spectrum(const EventRowsArgs& a, const EventSpectrumArgs& r, hipStream_t s);
// The exact tables (art_exact_histogram_device, art_exact_finish_device, art_event_exact_device; the kernels of
// art_exact.h). An accumulator is ART_EXACT_LIMBS int64 limbs per bin. EventExactArgs: kind, node_factor and
// event_factor as EventReplicatesArgs'; flux (n_k 2 nbins bins), sky (n_k sky_size bins; null: none) and totals
// (n_k 2 bins) hold set k at k times the usual size; nonfinite is one float64 count per set, misplaced one in all.
// Every launch leaves the accumulators it added to normalised.
struct EventExactArgs {
  const int64_t* node_start;
  int32_t kind, n_k, nbins;
  int64_t sky_size;
  const double *node_factor, *event_factor;
  int64_t *flux, *sky, *totals;
  double *nonfinite, *misplaced;
};
hipError_t launch_exact_histogram(int64_t n, const int32_t* bins, const double* values, int n_bins, int64_t* acc,
                                  double* nonfinite, bool lds, hipStream_t s);
hipError_t launch_exact_finish(int64_t n_bins, const int64_t* acc, double* out, hipStream_t s);
hipError_t launch_event_exact(const EventRowsArgs& a, const EventExactArgs& r, const SkyAxes& A, int cos_axis, int path,
                              hipStream_t s);
}  // namespace art
