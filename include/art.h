/*
 * art.h -- C ABI of libart.so, the MI355X (gfx950) engine for the hot path of
 * SamWitte/Adiabatic_RayTracer: the per-ray Hamiltonian ODE of a photon/axion
 * segment around a neutron star (Goldreich-Julian plasma, rotating dipole,
 * Schwarzschild metric), its Vern6/RK4 integration, resonance detection and the
 * conversion probability at each crossing.
 *
 * Every entry point replaces a reference interface (file:line under
 * /root/reference/src):
 *
 *   art_propagate_host / _device   RT.propagate              RayTracer.jl:171-452
 *       (callers MainRunner.jl:179-182 photon, :187-190 axion)
 *   art_propagate_traj_host/_dev   RT.propagate with saveat points (RayTracer.jl:176,383,444)
 *   art_get_prob_nonad_host/_dev   get_Prob_nonAD            MainRunner.jl:67-124
 *       (-> RT.conversion_prob RayTracer.jl:1405-1473; callers MainRunner.jl:134,265)
 *   art_sample_conversion_points_* RT.find_samples_new + k_norm_Cart
 *                                  RayTracer.jl:1480-1653, MainRunner.jl:463-529
 *   art_find_conversion_surface    RT.Find_Conversion_Surface RayTracer.jl:1250-1263
 *   art_flux_histogram_device      plot/flux.py:38-48 (binned flux of segment end states)
 *   art_flux_histogram_phi_device  plot/flux.py:38-48 (binned flux of the npy rows' φf;
 *   art_flux_histogram_phi_range_device  _range: over flux.py's data-dependent bins)
 *   art_histogram3_device          np.histogramdd of rows over (θf | cos θf, φf, Δω), per species
 *   art_sky_map_segments_device    the same map of a propagated batch's end states (no reference
 *                                  counterpart: its plot scripts leave Δω "NOT implemented")
 *   art_propagate_host_flux        RT.propagate + the batch's binned flux (bench.py's step)
 *   art_propagate_host_flux_async  the same, two batches in flight; art_host_wait
 *   art_comm_* / art_flux_allreduce  the reduction of the flux and counters over the GPUs of
 *                                  a node (the reference merges files instead,
 *                                  Combine_Files.py, Gen_Samples.jl:195-239)
 *   art_grow_trees[_traj]          get_tree (MainRunner.jl:126-352) for n trees, batched
 *                                  (_traj: + saveNode data, MainRunner.jl:17-65)
 *   art_grow_trees_device          the same forest with roots, tree state and nodes in device memory
 *   art_event_weight_*             sln_prob of a sampled point: dwp_ds cos_w + g_det
 *                                  (MainRunner.jl:498-557, RayTracer.jl:734-754,1327-1403)
 *   art_eval_*_device              pointwise physics (func!, func_axion!, hamiltonian,
 *                                  GJ_Model_ωp_vecSPH, condition) for parity tests;
 *                                  art_eval_math_device: the hand-written sincos / exp / log /
 *                                  reciprocal / min / max themselves, for ulp-level tests
 *
 * Conventions
 *   - All arrays are caller-owned. Position/momentum arrays are structure-of-arrays,
 *     exactly the memory of a Julia column-major N x 3 Matrix{Float64}:
 *     x[0..n) = x-column, x[n..2n) = y-column, x[2n..3n) = z-column.
 *   - *_host entry points take host pointers and do H2D/kernel/D2H on the library's
 *     own HIP stream (a Julia ccall passes Vector/Matrix pointers straight through).
 *     *_device entry points take device (HBM) pointers plus a hipStream_t passed as
 *     void*, used exactly as given (NULL = the HIP null stream, which is also
 *     PyTorch's default stream); they are asynchronous on that stream.
 *   - Return 0 on success or a negative ART_E* code; art_last_error() describes it.
 *   - Thread safety: calls are issued under an internal mutex; one device per call
 *     (art_set_device). *_host calls are synchronous. *_device calls only enqueue work:
 *     every propagate / sampler launch allocates its own scratch (work-queue word,
 *     statistics, fresh-state and end-record buffers) from the stream-ordered allocator
 *     and frees it in stream order, so launches on different streams may run
 *     concurrently and never share device state.
 */
#ifndef ART_H
#define ART_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ART_ABI_VERSION 1

/* error codes */
#define ART_OK 0
#define ART_E_INVALID (-1)     /* bad argument / unsupported option */
#define ART_E_HIP (-2)         /* HIP runtime error */
#define ART_E_NOMEM (-3)       /* device allocation failed */
#define ART_E_UNSUPPORTED (-4) /* melrose=0 (dead code at the reference's fixed flags) */

/* integrators */
#define ART_VERN6 0 /* adaptive Verner 6(5), the reference's Vern6() (RayTracer.jl:383) */
#define ART_RK4 1   /* fixed-step classical RK4 in ln t (BASELINE config 1) */

/* per-ray segment status (the reference's sol.retcode, refined) */
#define ART_STATUS_SUCCESS 0    /* reached ln_t_end                      (:Success)    */
#define ART_STATUS_CROSSING 1   /* terminate! after max_crossings         (:Terminated) */
#define ART_STATUS_HIT_NS 2     /* photon r < 1.01 rNS (cb_r, :352-368)   (:Terminated) */
#define ART_STATUS_MAXITERS 3   /* maxiters step attempts                 (:MaxIters)   */
#define ART_STATUS_NONFINITE 4  /* NaN/Inf in state or error estimate     (:Unstable)   */

/* max_crossings of art_propagate_*: no callbacks (RT.propagate with make_tree = false) */
#define ART_NO_CALLBACKS (-2147483647 - 1)

/* species (RT.node.species; MainRunner.jl:175-191) */
#define ART_AXION 0
#define ART_PHOTON 1

typedef struct art_params {
  /* physics: Gen_Samples.jl:139-170, Mvars of MainRunner.jl:177-178,185-186 */
  double theta_m;   /* θm misalignment angle [rad]                                  */
  double omega_pul; /* ωPul rotation frequency [1/s]                                */
  double B0;        /* surface dipole field [G]                                     */
  double rNS;       /* neutron-star radius [km]                                     */
  double mass_ns;   /* Mass_NS [solar masses]; get_Prob_nonAD always uses this GR   */
                    /* mass, even when flat != 0 (MainRunner.jl:75, global)         */
  double mass_a;    /* axion mass [eV]                                              */
  double g_agg;     /* axion-photon coupling Ax_g [1/GeV]                          */
  double bndry_lyr; /* boundary-layer index; <= 0 disables (Gen_Samples.jl:130)    */
  /* numerics: NumerP = [ln_tstart, ln_tend, ode_err] (MainRunner.jl:411-413),       */
  /* solve(...) keywords RayTracer.jl:383-384                                        */
  double ln_t_end;  /* log(1/ωPul)                                                  */
  double abstol;    /* ode_err = 1e-6                                               */
  double reltol;    /* 1e-7                                                         */
  double dtmin;     /* 1e-13 with force_dtmin = true                                */
  int64_t maxiters; /* 1e5 step attempts                                            */
  int32_t flat;     /* 1: Mass_NS -> 0 in the ray equations (RayTracer.jl:77,187)   */
  int32_t isotropic;/* 1: k_par -> 0                                                */
  int32_t melrose;  /* must be 1 (Gen_Samples.jl:167)                               */
  int32_t integrator;    /* ART_VERN6 or ART_RK4                                    */
  int32_t n_fixed;       /* RK4: steps per segment                                  */
  int32_t interp_points; /* ContinuousCallback interp_points (RayTracer.jl:358 = 50),*/
                         /* at most 65                                             */
} art_params;

/* Outputs of one batch of segments (the 14-tuple of RayTracer.jl:448, per ray). */
typedef struct art_segment_out {
  double* x_end;     /* 3n  final Cartesian position [km]       (x_reshaped[:, :, end]) */
  double* k_end;     /* 3n  final Cartesian momentum [eV]       (v_reshaped[:, :, end]) */
  double* u7_end;    /* n   final u[7] = erg*Δω                 (dt[:, end], :431)      */
  double* tau_end;   /* n   final ln t                          (times[end], :444)      */
  int32_t* status;   /* n   ART_STATUS_*                                               */
  int32_t* n_accept; /* n   accepted steps                                             */
  int32_t* n_reject; /* n   rejected steps                                             */
} art_segment_out;

/* Resonance crossings (xc..Δωc of RayTracer.jl:325-342), layout [(c*cap + j)*n + i]
 * for component c, crossing j < capacity, ray i. Slots j >= min(count[i], capacity) hold no
 * crossing (the reference's arrays simply end there): the *_device entry points leave them
 * unwritten, the *_host entry points fill them with NaN. */
typedef struct art_crossing_buf {
  int32_t capacity; /* crossings stored per ray (1 for forward trees)               */
  int32_t* count;   /* n  crossings recorded (> capacity means overflow)            */
  double* pos;      /* 3*cap*n  xc, yc, zc [km]                                     */
  double* k;        /* 3*cap*n  kxc, kyc, kzc [eV]                                  */
  double* t;        /* cap*n    tc = exp(τ) [s]                                     */
  double* dw;       /* cap*n    Δωc = u7/erg                                        */
  double* p_nonad;  /* cap*n    get_Prob_nonAD at the crossing, Nc = 1 semantics   */
} art_crossing_buf;

/* ---- library / device ---- */
int art_abi_version(void);
const char* art_last_error(void);
int art_device_count(int32_t* count);
int art_set_device(int32_t device);
int art_synchronize(void);
/* Releases every device object the library holds (streams, events, pooled HBM and pinned
 * staging, the host-mapped flags of the streamed pipeline, the host copy threads) after
 * draining its work; the next call re-creates what it needs. The library registers this to run at process exit, before the HIP
 * runtime's own teardown; a host may also call it itself. */
int art_shutdown(void);
/* Duration [ms] of the last propagate kernel, from HIP events recorded on the stream
 * the kernel ran on. */
double art_last_kernel_ms(void);
/* Counters of the last propagate launch: [step attempts, accepted steps, root re-steps,
 * scan condition evals, interpolant-root condition evals, rays, init RHS evals, 0] and the
 * persistent grid size; they feed the roofline accounting of bench.py. */
int art_last_stats(uint64_t* stats, int32_t* grid);

/* the geometry an integrator or tail kernel is built for */
#define ART_GEOM_ANY 0  /* the general one: boundary layer, isotropic plasma, RK4 outside flat space */
#define ART_GEOM_FLAT 1 /* flat space, anisotropic plasma, no boundary layer                       */
#define ART_GEOM_GR 2   /* Schwarzschild, anisotropic plasma, no boundary layer                    */

/* Which kernels the last propagate launch ran (latched with art_last_stats: after
 * art_synchronize or a host entry point). The decisions are the launch plan's own values, the
 * ones the kernels were selected by; the counts are the launch's record words, read back with its
 * statistics. A host call made of several launches (the chunked pipeline) reports what
 * art_last_stats reports for it: one record for the call, `launches` its number of launches, the
 * counts summed over them, bulk_grid the largest, every other decision the last launch's. The
 * streamed host call reports streamed = 1, don = 3 and zero counts. */
typedef struct art_launch_path {
  /* decisions */
  int32_t launches;    /* launches this record covers                                          */
  int32_t streamed;    /* 1: the streamed host call's integrator                              */
  int32_t small_tail;  /* 1: every ray on a wave of its own, tail_kernel alone (no bulk pass)  */
  int32_t bulk;        /* 1: the persistent integrator (propagate_kernel) ran ...              */
  int32_t integrator;  /* ... its template arguments: ART_VERN6 / ART_RK4,                     */
  int32_t geom;        /*     ART_GEOM_* (small_tail: the tail kernel's),                      */
  int32_t save;        /*     saveat,                                                          */
  int32_t don;         /*     DON: 0 none, 1 donating, 3 streamed,                             */
  int32_t wps;         /*     waves per SIMD,                                                  */
  int32_t cyc;         /*     the cyclotron observation                                        */
  int32_t bulk_grid;   /* ... and its grid                                                     */
  int32_t donate;      /* first-level donation lanes of the launch                             */
  int32_t cont;        /* 1: the packed continuation ran; its waves per SIMD and the lanes     */
  int32_t cont_wps;    /*    its drained waves hand to the tail kernel (0: no second level)    */
  int32_t cont_donate;
  int32_t tail;        /* 1: tail_kernel ran; its geometry and grid                            */
  int32_t tail_geom;
  int32_t tail_grid;
  int32_t hot;         /* 1: the early-graduation side launch ran                              */
  int32_t sorted;      /* 1: the bulk pass claimed its rays in sorted order                    */
  int32_t graduate;    /* the effective graduate threshold [attempts], 0: no graduation        */
  int32_t hot_at;      /* the effective early-graduation threshold [attempts], 0: off          */
  /* counts */
  uint64_t donated;     /* first-level donated records (small_tail: the batch's rays)          */
  uint64_t donated2;    /* second-level donated records                                        */
  uint64_t grad_count;  /* rays that asked to graduate (may pass grad_cap: the rest stayed)     */
  uint64_t grad_cap;
  uint64_t hot_count;   /* rays that asked for a hot record (may pass hot_cap)                 */
  uint64_t hot_cap;
  uint64_t hot_claimed; /* hot records claimed by the side launch and the tail kernel          */
} art_launch_path;
int art_last_launch_path(art_launch_path* out);
/* Integrator-kernel durations [ms] of the last min(n, 64) propagate launches on the current
 * device, oldest first, each from the HIP events around that launch on its own stream (waits
 * for them). Returns the number written (>= 0) or a negative ART_E* code. */
int art_recent_kernel_ms(int32_t n, double* ms);
/* The same launches' integrator spans [ms] from in-kernel clock stamps: the first wave's start
 * to the last wave's end on the device's 100 MHz constant clock (s_memrealtime), so free of a
 * profiler's per-dispatch completion signals; -1 where a launch left none. Returns the number
 * written (>= 0) or a negative ART_E* code. (No reference counterpart: measurement) */
int art_recent_kernel_span_ms(int32_t n, double* ms);
/* Tail donation for propagate launches that are pipelined with others (several batches in
 * flight on different streams): once a launch's work queue is drained, a wave with at most
 * `lanes` live rays (all between steps) hands them to a continuation launch on the same
 * stream and retires, so its CU slot goes to the next batch instead of idling behind one
 * long ray. The continuation launch integrates the donated rays packed into full waves, and
 * its own last rays finish one per wave (the tail kernel); results are bit-identical to
 * lanes = 0 (off). -1 (the default) chooses by geometry: 16 for Schwarzschild Vern6 batches,
 * whose few longest rays set a lone batch's wall time (configs[3]), 0 otherwise. Applies to
 * the current device's subsequent launches (the streamed host pipeline never donates). No
 * reference counterpart (an execution policy). */
int art_set_tail_donation(int32_t lanes);
/* Graduation for Vern6 launches with tail donation (the Schwarzschild default): a ray still
 * stepping after `attempts` step attempts leaves its lane at its next step boundary for the
 * one-wave-per-ray tail kernel, so a batch's longest rays run at lone-wave speed without waiting
 * for their waves to drain (configs[3] as one batch: 260-297 -> 230 ms). 0 switches it off -- for
 * a host that keeps several batches in flight, where each graduated ray would hold a whole tail
 * wave while the other batches fill the CUs it frees; -1 (the default) = 2048 attempts (or
 * ART_GRADUATE). Per device; results are bit-identical either way.
 * With graduation on, a launch on a non-blocking stream also graduates early: from 128 attempts
 * on, a ray whose progress in ln t lags 15.95 + 0.75 log2(attempts / 256) (ART_HOT_AT,
 * ART_HOT_DTAU, ART_HOT_SLOPE) -- on configs[3] the rays that crawl along the star's surface,
 * every one of its 20 longest among them -- leaves at once for a tail-kernel launch that runs on
 * a side stream beside the bulk pass, and the bulk pass claims its rays smallest initial step
 * first (configs[3] as one batch: 226 -> 188 ms). Not on the null stream or another blocking
 * stream, whose work would wait for that side launch. */
int art_set_graduation(int32_t attempts);
/* Waves per SIMD of the conversion-point sampler (art_sample_conversion_points*): 0 (the default)
 * chooses by line length -- 3 for lines up to 2.2 x 60 km, walked step by step, else 2 with blocks
 * of 3 steps, the faster builds for one launch at a time; 3 takes the 3-wave build for every line,
 * which packs better beside other sampler launches in flight on other streams (the 32-point scan's
 * sampling on 8 streams: 0.503-0.508 -> 0.484 s, profiles/r05ah_scan_sampler_waves.txt). Per
 * device; samples are bit-identical either way. No reference counterpart (an execution policy). */
int art_set_sampler_waves(int32_t waves);
/* The Vern6 tableau the kernel uses: c[9], A[81] row-major, b[9], bhat[9]. */
int art_vern6_tableau(double* c, double* A, double* b, double* bhat);

/* ---- RT.Find_Conversion_Surface (RayTracer.jl:1250-1263), pure host math ---- */
double art_find_conversion_surface(const art_params* p);

/* ---- RT.propagate for a batch of n segments (RayTracer.jl:171-452) ----
 * x0, k0   : 3n Cartesian start position [km] / momentum (rescaled onto the axion
 *            mass shell in-kernel exactly as k_norm_Cart, RayTracer.jl:179-186)
 * erg      : n  Mvars erg (erg_inf_ini) [eV]
 * dw       : n  Δω (u0[7] = erg*Δω, RayTracer.jl:216)
 * ln_t0    : n  NumerP[1] = log(max(event.t, e^-30)) (MainRunner.jl:166)
 * species  : n  ART_PHOTON (func!) or ART_AXION (func_axion!)
 * max_crossings : terminate! once this many crossings are recorded (RayTracer.jl:346);
 *            <= 0 means "stop at the first new crossing" exactly like the reference's
 *            splittings_cutoff = -1 (MainRunner.jl:128). ART_NO_CALLBACKS integrates the
 *            plain ODE with no callbacks, as the reference does for make_tree = false
 *            (RayTracer.jl:361-377): no crossing is recorded and photons are not stopped
 *            at 1.01 rNS.
 * xc may be NULL when crossings are not wanted (the segment still stops on them).
 * art_propagate_host streams Vern6 batches of 2^20 rays and more: one
 * integrator launch while the inputs are still being copied in and finished pieces already
 * copied out; the outputs are those of one launch bit for bit, and a streamed call that outlasts
 * its bounds runs again as one launch (counted by art_host_path_counters). */
int art_propagate_host(const art_params* p, int64_t n, const double* x0, const double* k0,
                       const double* erg, const double* dw, const double* ln_t0,
                       const int8_t* species, int32_t max_crossings,
                       art_segment_out* out, art_crossing_buf* xc);
int art_propagate_device(const art_params* p, int64_t n, const double* x0, const double* k0,
                         const double* erg, const double* dw, const double* ln_t0,
                         const int8_t* species, int32_t max_crossings,
                         art_segment_out* out, art_crossing_buf* xc, void* stream);
/* art_propagate_host plus the batch's binned radiated flux (plot/flux.py:38-48, the quantity
 * MainRunner.jl:749 normalises): hist[2*nbins] (host, overwritten; row 0 axions, row 1
 * photons) counts the segments that end without a crossing beyond 1.1 rNS (MainRunner.jl:
 * 203-209) by the azimuth atan2(k_y, k_x) of their final momentum, in nbins equal bins of
 * [-pi, pi] with np.histogram's bin assignment. It is binned on the device while the outputs
 * are still in HBM, so it costs no second pass over them; a multi-process run sums hist over
 * its ranks (art_flux_allreduce_host). */
int art_propagate_host_flux(const art_params* p, int64_t n, const double* x0, const double* k0,
                            const double* erg, const double* dw, const double* ln_t0,
                            const int8_t* species, int32_t max_crossings, art_segment_out* out,
                            art_crossing_buf* xc, int32_t nbins, double* hist);
/* art_propagate_host_flux, asynchronous: checks the arguments, returns at once with *ticket, and
 * runs the call on a library worker thread; art_host_wait(ticket) returns the call's result code.
 * Two calls per device can be in flight (a third waits for the lane of the one two before it),
 * each with its own streams and staging, so the next batch's uploads and first rays overlap this
 * batch's drain (MainRunner.jl:179-190 calls RT.propagate batch after batch; a host that has the
 * next batch ready submits it before waiting for this one). Every buffer of a call must stay
 * valid and untouched until its art_host_wait returns; wait on the device the call was submitted
 * on. A batch the streamed pipeline does not take (below ART_HOST_CHUNK_MIN rays, default 2^20)
 * runs inside the submitting call and its ticket is complete. Synchronous host calls first wait
 * for every asynchronous one. Results equal art_propagate_host_flux's bit for bit. */
int art_propagate_host_flux_async(const art_params* p, int64_t n, const double* x0, const double* k0,
                                  const double* erg, const double* dw, const double* ln_t0,
                                  const int8_t* species, int32_t max_crossings, art_segment_out* out,
                                  art_crossing_buf* xc, int32_t nbins, double* hist, int64_t* ticket);
/* Waits for an asynchronous host call and returns its result (ART_OK or the ART_E* code it
 * failed with; art_last_error() then says why). Each ticket is waited for once. */
int art_host_wait(int64_t ticket);
/* What the art_propagate_host* calls of this process ran as, since load or the last reset:
 * [0] calls, [1] streamed-pipeline completions, [2] streamed-pipeline give-ups (a wait
 * outlasted its bound; the batch then ran again as one launch, same results), [3] chunked-
 * pipeline calls, [4] single-launch calls (a give-up counts there too). Writes min(n, 5)
 * counters (0 beyond), resets them when reset != 0, and returns 5. No reference counterpart
 * (execution-path bookkeeping; bench.py asserts no give-up inside its timed passes). */
int art_host_path_counters(uint64_t* counters, int32_t n, int32_t reset);

/* ---- RT.propagate with its saved points (saveat, RayTracer.jl:176, 383, 427-444) ----
 * As art_propagate_*, plus up to ntimes (>= 2) saved points per ray: the start, the
 * interior times ln_t0 + k (ln_t_end - ln_t0)/(ntimes - 1) that the segment reached before
 * it ended (from the step's cubic Hermite interpolant), and the end state -- the
 * reference's x_reshaped[:, :, k] and times = sol.t, without the duplicate points DiffEq
 * adds at callback events. Used by saveMode 3 tree dumps (saveNode, MainRunner.jl:17-65).
 * traj: 3*ntimes*n Cartesian positions [(c*ntimes + k)*n + i]; traj_t: ntimes*n ln t
 * [k*n + i]; traj_n: n points per ray (2 .. ntimes). */
int art_propagate_traj_host(const art_params* p, int64_t n, const double* x0, const double* k0,
                            const double* erg, const double* dw, const double* ln_t0,
                            const int8_t* species, int32_t max_crossings, art_segment_out* out,
                            art_crossing_buf* xc, int32_t ntimes, double* traj, double* traj_t,
                            int32_t* traj_n);
int art_propagate_traj_device(const art_params* p, int64_t n, const double* x0, const double* k0,
                              const double* erg, const double* dw, const double* ln_t0,
                              const int8_t* species, int32_t max_crossings, art_segment_out* out,
                              art_crossing_buf* xc, int32_t ntimes, double* traj, double* traj_t,
                              int32_t* traj_n, void* stream);

/* ---- RT.propagate with the cyclotron-resonance optical depth of each ray ----
 * Beyond the reference: it writes opticalDepth = 0 into every npy row (MainRunner.jl:703-708)
 * and keeps the formula as dead code (cyclotronF / tau_cyc, RayTracer.jl:792-851). As
 * art_propagate_*, and while a photon is integrated every crossing of omega_c = omega
 * (omega_c = 0.3/5.11e5*(1.95e-20*1e18) eV/G * |B| of the rotating dipole, omega the ray's erg) is
 * located on the step's cubic Hermite interpolant and its optical depth
 * tau = pi omega_p^2 / |khat . grad omega_c| / (c hbar) added up (khat = k/|k| Cartesian, the GJ
 * omega_p there; a ray running along a surface of constant omega_c gets +inf). The observation
 * is passive: every art_segment_out / art_crossing_buf output equals art_propagate_*'s bit for
 * bit. Vern6 only (RK4: ART_E_INVALID); cyc and its four buffers must be non-NULL.
 * tau and count are written for every ray (axions: 0); pos and ln_t hold the first crossing and
 * follow the crossing-buffer convention: the device entry point leaves them unwritten where
 * count = 0, the host entry point fills NaN there. */
typedef struct art_cyclotron_out {
  double*  tau;    /* n   sum of tau over the segment's cyclotron crossings (0 when none) */
  int32_t* count;  /* n   crossings of omega_c = omega found                              */
  double*  pos;    /* 3n  Cartesian position of the first one [km], [c*n + i]             */
  double*  ln_t;   /* n   its ln t                                                        */
} art_cyclotron_out;
int art_propagate_cyclotron_host(const art_params* p, int64_t n, const double* x0, const double* k0,
                                 const double* erg, const double* dw, const double* ln_t0,
                                 const int8_t* species, int32_t max_crossings, art_segment_out* out,
                                 art_crossing_buf* xc, const art_cyclotron_out* cyc);
int art_propagate_cyclotron_device(const art_params* p, int64_t n, const double* x0, const double* k0,
                                   const double* erg, const double* dw, const double* ln_t0,
                                   const int8_t* species, int32_t max_crossings, art_segment_out* out,
                                   art_crossing_buf* xc, const art_cyclotron_out* cyc, void* stream);

/* ---- get_Prob_nonAD (MainRunner.jl:67-124) ----
 * One call of the reference per group: group g covers crossings
 * [group_start[g], group_start[g+1]) and reproduces the reference's column-major
 * linear indexing of ksphere/Bsphere inside conversion_prob (RayTracer.jl:1432-1443)
 * for groups with more than one crossing. group_start == NULL means n_groups == nc
 * groups of one crossing each (forward-tree semantics).
 * pos, kpos: 3nc Cartesian; erg_eff: nc = erg_inf_ini .* abs.(Δωc). out: nc P_nonAD. */
int art_get_prob_nonad_host(const art_params* p, int64_t nc, const double* pos,
                            const double* kpos, const double* erg_eff,
                            int64_t n_groups, const int64_t* group_start, double* out);
int art_get_prob_nonad_device(const art_params* p, int64_t nc, const double* pos,
                              const double* kpos, const double* erg_eff,
                              int64_t n_groups, const int64_t* group_start, double* out,
                              void* stream);

/* ---- conversion-surface sampler (find_samples_new, RayTracer.jl:1480-1653) ----
 * Draws one accepted sample per ray i in [0, n) with a Philox4x32-10 stream keyed by
 * (seed, ray_offset + i): attempts are repeated until accepted (MainRunner.jl:463-495).
 * Outputs (n or 3n, SoA): x [km], k_init (k_norm_Cart onto the axion shell, :529),
 * erg_inf_ini [eV] (:526), vifty = vIfty/c (unitless, :1651), weights (# crossings on
 * the accepted line, :1636), attempts (# find_samples_new calls, feeds f_inx :469). */
int art_sample_conversion_points_host(const art_params* p, double max_r, uint64_t seed,
                                      int64_t ray_offset, int64_t n, double* x, double* k_init,
                                      double* erg_inf, double* vifty, int32_t* weights,
                                      int32_t* attempts);
int art_sample_conversion_points_device(const art_params* p, double max_r, uint64_t seed,
                                        int64_t ray_offset, int64_t n, double* x,
                                        double* k_init, double* erg_inf, double* vifty,
                                        int32_t* weights, int32_t* attempts, void* stream);

/* ---- batched tree driver: get_tree (MainRunner.jl:126-352) for n trees at once ----
 * Roots are RT.node(x0, k0, t = 0, Δω = -1, species, prob = 1, weight = 1, -1, -1, -1) with
 * root.prob replaced by 1 - exp(-P_nonAD) at the root (:132-137), as main_runner_tree
 * builds both its backtrace (axion, -k, -B0: pass p with B0 negated) and its forward
 * (photon) trees (:578-590, :653-667). Every round propagates the next node of every
 * active tree in one batched launch. Per tree the reference's rules are kept: pop the
 * highest-weight event (stable sort by weight), stop each segment at its first crossing
 * when splittings_cutoff <= 0, full splitting while count <= mc_nodes and one
 * Monte-Carlo branch after (Philox4x32-10 keyed by (seed, tree, count) in place of
 * rand(Float64)), the |kc| > 1 rule, the 1e-5 km crossing merge, the stop rules and the
 * info codes 1..4 (negative once Monte-Carlo). */
typedef struct art_tree_opts {
  int32_t num_cutoff;        /* 5   (Gen_Samples.jl default)                       */
  int32_t mc_nodes;          /* 5                                                  */
  int32_t max_nodes;         /* 50                                                 */
  int32_t splittings_cutoff; /* -1: forward trees; 100000: backtrace (:588)        */
  int32_t crossing_cap;      /* crossings stored per segment when splittings > 0   */
  int32_t tree_offset;       /* global id of tree 0: the Monte-Carlo draws are keyed */
                             /* by (seed, tree_offset + i, count), so a run sharded */
                             /* over ranks by event id draws what one process would */
  double prob_cutoff;        /* 1e-10                                              */
  uint64_t seed;             /* key of the Monte-Carlo draws                        */
} art_tree_opts;

/* One RT.node of a finished tree, in the order get_tree pushed it onto `tree`. */
typedef struct art_tree_node {
  int32_t tree;      /* index of its root                                          */
  int32_t species;   /* ART_AXION / ART_PHOTON                                     */
  int32_t is_final;  /* no crossing and |x_end| > 1.1 rNS (:200-207)               */
  int32_t n_cross;   /* crossings kept on its segment (after the 1e-5 km merge)    */
  int32_t status;    /* ART_STATUS_* of its segment                                */
  int32_t pad;
  double weight, prob, parent_weight, prob_conv, prob_conv0;
  double x0[3], k0[3], t0, dw0;               /* node.x .. node.Δω (start)          */
  double x_end[3], k_end[3], u7_end, tau_end; /* traj[end], mom[end], erg[end], ln t */
  double xc[3], kc[3], tc, dwc, pc;           /* first crossing, Pc = 1 - e^-P_nonAD */
} art_tree_node;

/* x0, k0: 3n SoA; erg: n erg_inf_ini; species: n. nodes: caller-owned, node_capacity
 * records; *n_nodes receives the number of nodes (returns ART_E_NOMEM with the needed
 * count when node_capacity is too small). counts, infos (n, may be NULL): get_tree's
 * `count` and `info`. Host pointers; synchronous. */
int art_grow_trees(const art_params* p, int64_t n, const double* x0, const double* k0,
                   const double* erg, const int8_t* species, const art_tree_opts* opts,
                   int64_t node_capacity, art_tree_node* nodes, int64_t* n_nodes,
                   int32_t* counts, int32_t* infos);

/* art_grow_trees with every tree's state in device memory (HBM): the roots come as device arrays
 * (the sampler's outputs, say) and the nodes are left in device memory, in art_grow_trees' layout:
 * trees in order, each tree's nodes in the order it processed them. A round is one pack kernel, one
 * batched art_propagate_device launch, one step kernel (one lane per active tree) and one scan, all
 * on `stream`; the host reads one number per round, the count of trees still active, and runs at
 * most max_nodes + 2 rounds.
 *   - x0, k0, erg, species, nodes, node_start, counts, infos: device pointers. p, opts, n_nodes: host.
 *   - node_start (n + 1 entries, may be NULL): tree i owns nodes[node_start[i] .. node_start[i + 1]).
 *     counts, infos (n, may be NULL) as art_grow_trees'. *n_nodes receives the number of nodes;
 *     ART_E_NOMEM with the needed count in *n_nodes when node_capacity is too small (nothing else
 *     is written then).
 *   - Every kernel and every scratch allocation (the stream-ordered allocator) goes on `stream`.
 *   - Unlike the other *_device entry points it BLOCKS: it returns when the forest is done and its
 *     outputs are written. It reads a count between rounds, so it cannot be captured into a graph.
 *     Calls on other streams from other threads proceed while it waits.
 *   - Forward trees (splittings_cutoff <= 0) and the backtrace form main_runner_tree uses
 *     (splittings_cutoff > 0 with num_cutoff <= 0: only the root is processed, every crossing up
 *     to crossing_cap is merged and grouped, the root's weight becomes prod(1 - P_j)).
 *     splittings_cutoff > 0 with num_cutoff > 0 is ART_E_INVALID here, and trajectory dumps
 *     (art_grow_trees_traj) have no device form.
 *   - ART_E_INVALID before any device is touched: NULL p, opts or n_nodes; n < 0; n > 0 with a NULL
 *     input; max_nodes < 0; crossing_cap < 0; the unsupported mode.
 *   - Against art_grow_trees: the integrator and the probabilities are the same kernels; exp and
 *     log of the bookkeeping are the device's (each within 1 ulp of the host's), and a "rare fail"
 *     node (|kc| > 1) is recorded as the reference leaves it, without crossings (n_cross = 0). */
int art_grow_trees_device(const art_params* p, int64_t n, const double* x0, const double* k0,
                          const double* erg, const int8_t* species, const art_tree_opts* opts,
                          int64_t node_capacity, art_tree_node* nodes, int64_t* node_start,
                          int32_t* counts, int32_t* infos, int64_t* n_nodes, void* stream);

/* saveMode 3 tree dumps (saveNode, MainRunner.jl:17-65, called at :612 and :671): per node,
 * its saved trajectory points (art_propagate_traj_*) and all of its crossings after the
 * 1e-5 km merge. Arrays are caller-owned, node_capacity records each. */
typedef struct art_tree_traj {
  int32_t ntimes;       /* saved points per segment, >= 2 (Gen_Samples.jl:164: 3)            */
  int32_t crossing_cap; /* crossings kept per node in xc                                      */
  double* traj;         /* node_capacity*ntimes*3 Cartesian positions [node][k][c]            */
  double* times;        /* node_capacity*ntimes   ln t of each point (sol.t, RayTracer.jl:444) */
  int32_t* count;       /* node_capacity          points of each node                         */
  double* xc;           /* node_capacity*crossing_cap*4 (x, y, z, tc) [node][j][c]             */
} art_tree_traj;
/* art_grow_trees plus the saveNode data of every node. */
int art_grow_trees_traj(const art_params* p, int64_t n, const double* x0, const double* k0,
                        const double* erg, const int8_t* species, const art_tree_opts* opts,
                        int64_t node_capacity, art_tree_node* nodes, int64_t* n_nodes,
                        int32_t* counts, int32_t* infos, const art_tree_traj* traj);

/* ---- event weight of sampled points (MainRunner.jl:498-557) ----
 * For n sampled conversion points (x, k_init, vifty: 3n SoA, as returned by the
 * sampler) computes out (5n SoA): cos_w of dwp_ds (RayTracer.jl:1327-1403),
 * jacobian_GR = g_det (:734-754, 1 when flat), sln_prob (the incoming axion rate,
 * npy column 8 before the division by f_inx, :549-552), erg_inf_ini (:517) and
 * vel_eng (:513). rho_dm [GeV/cm^3] defaults to 0.45 and mcmc_weight = n_maxSample = 6
 * in the reference (MainRunner.jl:356-362,480). */
int art_event_weight_host(const art_params* p, double max_r, double rho_dm, double mcmc_weight, int64_t n,
                          const double* x, const double* k_init, const double* vifty, double* out);
int art_event_weight_device(const art_params* p, double max_r, double rho_dm, double mcmc_weight, int64_t n,
                            const double* x, const double* k_init, const double* vifty, double* out,
                            void* stream);

/* ---- halo velocity model (beyond the reference: its sampler draws every axion at one speed) ----
 * f_inf(u) ~ exp(-|u + v_ns|^2 / v0^2) in the star's frame: u the axion's velocity at infinity,
 * v0 the most probable speed (the reference's 220), v_ns the star's velocity in the halo frame.
 * With a non-NULL halo the sampler draws the speed at infinity s = v_prop sqrt(-log(1 - U[6]))
 * per attempt (the ten uniforms are drawn as without it), vifty is u/c with u the incoming
 * asymptote of the Newtonian Kepler orbit through the accepted point (|u| = s), and the event
 * weight's sln_prob is the reference's expression times
 *   F = (220/v0) (v_prop/v0)^2 exp(s^2/v_prop^2 - |u + v_ns|^2/v0^2),
 * with vel_eng = |vifty|^2 / 2 (the reference divides by c once more; not here, so that the rows'
 * column 12 is the line position). F is 1 for v_ns = 0, v_prop = v0 = 220.
 * halo == NULL: the entry points without _halo, bit for bit. ART_E_INVALID before any device is
 * touched: v0 <= 0 or not finite, a v_ns that is not finite, 0 < v_prop < v0, v_prop > 3000. */
typedef struct art_halo {
  double v0;       /* km/s */
  double v_ns[3];  /* km/s */
  double v_prop;   /* <= 0: sqrt(v0^2 + |v_ns|^2) */
} art_halo;

int art_sample_conversion_points_halo_host(const art_params* p, const art_halo* halo, double max_r, uint64_t seed,
                                           int64_t ray_offset, int64_t n, double* x, double* k_init,
                                           double* erg_inf, double* vifty, int32_t* weights, int32_t* attempts);
int art_sample_conversion_points_halo_device(const art_params* p, const art_halo* halo, double max_r, uint64_t seed,
                                             int64_t ray_offset, int64_t n, double* x, double* k_init,
                                             double* erg_inf, double* vifty, int32_t* weights, int32_t* attempts,
                                             void* stream);
int art_event_weight_halo_host(const art_params* p, const art_halo* halo, double max_r, double rho_dm,
                               double mcmc_weight, int64_t n, const double* x, const double* k_init,
                               const double* vifty, double* out);
int art_event_weight_halo_device(const art_params* p, const art_halo* halo, double max_r, double rho_dm,
                                 double mcmc_weight, int64_t n, const double* x, const double* k_init,
                                 const double* vifty, double* out, void* stream);

/* ---- binned flux (plot/flux.py:38-48): histogram of the final momentum azimuth
 * φf = atan2(ky, kx) over [-π, π) in nbins bins, separately for axions (row 0) and
 * photons (row 1), weight w[i] (NULL = 1), only rays that ended without a crossing
 * (status != ART_STATUS_CROSSING) and whose final radius exceeds 1.1 rNS -- the
 * reference's is_final (MainRunner.jl:200-207), whatever the retcode. hist (2*nbins, device,
 * float64) is ACCUMULATED into (zero it first). */
int art_flux_histogram_device(const art_params* p, int64_t n, const double* x_end,
                              const double* k_end, const int32_t* status,
                              const int8_t* species, const double* w, int32_t nbins,
                              double* hist, void* stream);

/* ---- binned flux of the npy rows (plot/flux.py:38-48): np.histogram(phif, nbins,
 * range = (-π, π), weights = w) of the given azimuths φf (npy column 4, MainRunner.jl:715),
 * axions (species 0) into row 0 and photons into row 1 of hist (2*nbins, device, float64),
 * with numpy's bin assignment (edges linspace(-π, π, nbins + 1), the right edge in the last
 * bin, values outside [-π, π] dropped). hist is ACCUMULATED into. The reference's radiated
 * flux is row 1 with w = weight * sln_prob (columns 9 and 8). */
int art_flux_histogram_phi_device(int64_t n, const double* phi, const int8_t* species, const double* w,
                                  int32_t nbins, double* hist, void* stream);
/* The same over [lo, hi] (finite, lo < hi): plot/flux.py:43-47 itself calls np.histogram(phif,
 * bins=50) without a range, i.e. over [min φf, max φf] of the rows, and this reproduces those
 * bins (edges linspace(lo, hi, nbins + 1), numpy's bin assignment). */
int art_flux_histogram_phi_range_device(int64_t n, const double* phi, const int8_t* species, const double* w,
                                        int32_t nbins, double lo, double hi, double* hist, void* stream);

/* ---- sky maps: a weighted 3-D histogram per species (beyond the reference, whose plot scripts
 * stop at the 1-D azimuth histogram above). hist[((s*na + ia)*nb + ib)*nc + ic] (device, float64,
 * ACCUMULATED into; ordinary device memory), s = 0 axions, 1 photons. Each axis has nbins[d]
 * equal bins over the closed range [lo[d], hi[d]] with numpy's bin assignment, so
 * np.histogramdd(range =, bins =) of one species' items is the same table; an item outside the
 * range, or NaN, on any axis is dropped. w NULL = 1; species NULL = photons. Counts are exact;
 * weighted sums depend on the order the adds arrive in and differ in the last bits between runs.
 * mode: 0 picks the accumulation path by the table's size, 1 forces the block-private LDS table
 * (2*na*nb*nc <= 8192), 2 forces adds to device memory. ART_E_INVALID, before any device is
 * touched: n < 0, a bin count < 1, a non-finite or empty range, an unknown mode, a table of more
 * than 2^26 doubles, mode 1 with a table over the LDS budget. */
int art_histogram3_device(int64_t n, const double* a, const double* b, const double* c,
                          const int8_t* species, const double* w,
                          const int32_t nbins[3], const double lo[3], const double hi[3],
                          int32_t mode, double* hist, void* stream);

/* The sky map of a propagated batch, straight from the device-resident outputs of
 * art_propagate_device: the final segments (art_flux_histogram_device's rule) binned over
 * (θf or cos θf, φf, Δω) of the final momentum: cos θf = kz / |k|, θf = acos(cos θf),
 * φf = atan2(ky, kx) over [-π, π], Δω = u7_end / mass_a + dw_offset (NULL = 0; the rows' column 13,
 * MainRunner.jl:709). bin_out (n, int32, may be NULL): each ray's flat index into hist, -1 for
 * not counted. */
typedef struct art_sky_spec {
  int32_t n_theta, n_phi, n_dw;   /* each >= 1 */
  int32_t theta_axis;             /* 0: θf over [0, π]; 1: cos θf over [-1, 1] (equal solid angle) */
  int32_t mode;                   /* 0 auto, 1 LDS table, 2 global adds */
  double  dw_lo, dw_hi;           /* range of Δω; ignored when n_dw == 1 (one bin holding every finite Δω) */
} art_sky_spec;
int art_sky_map_segments_device(const art_params* p, const art_sky_spec* spec, int64_t n,
                                const double* x_end, const double* k_end, const double* u7_end,
                                const int32_t* status, const int8_t* species, const double* w,
                                const double* dw_offset, double* hist, int32_t* bin_out, void* stream);

/* ---- event rows: main_runner_tree's npy rows, flux and sky map from forests held in HBM ----
 * One pass over the forward forest's node records (art_grow_trees_device's layout) selects the
 * final nodes (is_final != 0), writes each one's row (MainRunner.jl:690-747, 715-761) in node
 * order -- row r is the r-th final node -- and, while the row is in registers, adds
 * column 8 * column 7 (weight * sln_prob) to the azimuth flux table and to the sky map and sums
 * the run's totals. Columns, 0-based: 0 event_offset + node.tree + 1; 1 species (0 axion,
 * 1 photon); 2, 3 θf, φf of k_end; 4-6 θ, φ, |.| of x_end; 7 sln_prob, raw (the division by the
 * run's f_inx comes later); 8 node.weight * (back.prob * back.weight) [* exp(-τ)]; 9-11 the sampled
 * x; 12 u7_end / mass_a + vel_eng; and with ncols = 29: 13 column 8 without exp(-τ); 14 τ; 15 1;
 * 16-18 k_init; 19 cos_w; 20, 21 the forward tree's count and info; 22-24 prob, prob_conv,
 * prob_conv0; 25 back.prob * back.weight; 26 column 6; 27 the backtrace tree's count; 28 back.prob.
 * Every operation is rounded on its own, as numpy rounds them: |v| = sqrt((x² + y²) + z²),
 * θ = acos(z / |v|), φ = atan2(y, x).
 * All array pointers are device pointers; the structs and p are host memory. */
typedef struct art_event_rows_in {
  int64_t n_events;            /* events (trees) of this chunk                                        */
  int64_t event_offset;        /* global id of the chunk's event 0 (column 0)                         */
  const double* x;             /* 3n  the sampler's x (SoA)                                           */
  const double* k_init;        /* 3n  the sampler's k_init                                            */
  const int32_t* attempts;     /* n   the sampler's attempts; may be NULL (totals[4] stays)           */
  const double* weight5;       /* 5n  the output of art_event_weight_device                           */
  const art_tree_node* back;   /* n   the backtrace forest's nodes, one per event                     */
  const int32_t* back_counts;  /* n   its counts (column 27)                                          */
  const art_tree_node* nodes;  /* n_nodes  the forward forest's nodes                                 */
  int64_t n_nodes;             /* < 2^31                                                              */
  const int32_t* counts;       /* n   the forward forest's counts (column 20)                         */
  const int32_t* infos;        /* n   its infos (column 21)                                           */
  /* cyclotron (all NULL / 0 without): the re-run of the final photon segments that
   * art_event_gather_photons_device packed and art_propagate_cyclotron_device ran */
  const int32_t* cyc_slot;     /* n_nodes  each node's segment in that batch, -1 for none             */
  int64_t cyc_n;               /* segments in the batch                                               */
  const double* cyc_tau;       /* cyc_n  art_cyclotron_out::tau: column 14, and exp(-τ) into column 8 */
  const art_segment_out* cyc_end; /* the batch's end states (x_end, k_end, u7_end, tau_end, status),  */
                               /* compared with the nodes' bitwise, NaN equal to NaN: totals[5]       */
} art_event_rows_in;
/* Every table is ACCUMULATED into (zero it first); ordinary device memory.
 * totals (6 float64; counts are exact below 2^53): [0] rows, [1] photon rows, [2] Σ column 8 *
 * column 7 of the axion rows, [3] of the photon rows, [4] Σ (attempts - 1) over the events,
 * [5] cyclotron re-runs that did not reproduce their node's end state (must stay 0). */
typedef struct art_event_rows_out {
  int32_t ncols;               /* 13 or 29                                                            */
  int32_t nbins;               /* bins of the azimuth flux over [-π, π], 0 .. 4096 (0: no flux)       */
  double* rows;                /* row_capacity * ncols, row-major; NULL: bin only (large runs)        */
  int64_t row_capacity;        /* rows that `rows` and `bin_out` hold: >= n_nodes when either is given */
  double* flux;                /* 2 * nbins: axions, photons (np.histogram's bins, np_hist_bin)       */
  const art_sky_spec* sky;     /* NULL: no sky map. θ axis from kz / |k| or column 2, φf = column 3,  */
  double* sky_hist;            /*   Δω = column 12; the table of art_sky_map_segments_device          */
  int32_t* bin_out;            /* may be NULL: each row's flat sky bin, -1 for not counted            */
  double* totals;              /* 6                                                                   */
} art_event_rows_out;
/* Asynchronous on `stream` like the other *_device calls; its scratch (one int32 per node and the
 * scan's) comes from the stream-ordered allocator. The flux table is block-private in LDS; the sky
 * table too when 2 n_theta n_phi n_dw + 2 nbins <= 8192 doubles (mode 0) and otherwise added to in
 * device memory, as art_sky_map_segments_device chooses. ART_E_INVALID before any device is touched:
 * a NULL p, in or out; n_events < 0; n_nodes < 0 or >= 2^31; ncols not 13 or 29; rows or bin_out
 * given with row_capacity < n_nodes; nbins < 0 or > 4096; a bad sky spec by
 * art_sky_map_segments_device's rules (mode 1: the two tables together exceed the LDS budget);
 * a NULL buffer that the call needs. */
int art_event_rows_device(const art_params* p, const art_event_rows_in* in, const art_event_rows_out* out,
                          void* stream);
/* The cyclotron re-run's inputs, a second small entry point (art_event_rows_device itself stays
 * asynchronous): packs the final photon nodes of `nodes` in node order into a segment batch --
 * x0, k0 (3m SoA, stride m), erg = erg[node.tree], dw = dw0, ln_t0 = log(max(t0, e^-30)) by the
 * function and constants art_grow_trees_device packed its rounds with, species = photon -- so
 * art_propagate_cyclotron_device(max_crossings = -1) starts from the forest's own inputs bit for
 * bit. slot (n_nodes): each node's segment, -1 for none. It BLOCKS, because it reads one count on
 * the host, m = *n_out, the stride of the batch and the n the propagate call takes by value. The
 * batch buffers hold `capacity` segments (3 capacity for x0 and k0); n_nodes always suffices, a
 * smaller capacity than m is ART_E_NOMEM with m in *n_out and nothing packed. erg: n_events. */
int art_event_gather_photons_device(const art_params* p, int64_t n_events, const double* erg, int64_t n_nodes,
                                    const art_tree_node* nodes, int64_t capacity, double* x0, double* k0,
                                    double* erg_out, double* dw, double* ln_t0, int8_t* species, int32_t* slot,
                                    int64_t* n_out, void* stream);

/* ---- event moments: the Monte-Carlo errors of the flux table, the sky map and the totals ----
 * The independent unit of a run is the event; the rows of one event (the leaves of one forward tree)
 * are correlated. With p_r = column 8 * column 7 of final row r (what art_event_rows_device adds to
 * its tables, exp(-τ) included with cyclotron) and the same bins, per event e:
 *   a_e     = (attempts[e] - 1) + (final photon rows of e)   (Σ_e a_e is the run's f_inx; attempts
 *             NULL: the photon rows only),
 *   X_{e,b} = Σ p_r over e's final rows in bin b, summed in node order,
 *   X_{e,s} = Σ p_r over all of e's final rows of species s, binned or not,
 * and the call ADDS, per table, Q_b = Σ_e X_{e,b}² to *_sq and C_b = Σ_e X_{e,b} a_e to *_xa, each
 * (event, bin) group once, and to totals [0] the events n, [1] A1 = Σ a_e, [2] A2 = Σ a_e²,
 * [3], [4] Q of axions and photons, [5], [6] C of axions and photons, [7] records that lie in the range
 * of a tree other than their own (skipped; must stay 0). All of these add over chunks and ranks.
 * With S_b the first-moment table, f = f_inx and F_b = S_b / f, the delta-method standard error of
 * F_b is sqrt(max(Q_b - 2 F_b C_b + F_b² A2, 0) n / (n - 1)) / f  (n >= 2, f > 0).
 * in: art_event_rows_device's input (cyclotron fields included; cyc_end is not read).
 * node_start (n_events + 1, device): tree e owns records node_start[e] .. node_start[e + 1], as
 * art_grow_trees_device leaves them; required when n_nodes > 0. */
typedef struct art_event_moments_out {
  int32_t nbins;               /* flux bins over [-π, π], 0 .. 4096 (0: no flux tables)            */
  int32_t reserved;            /* 0                                                                 */
  double* flux_sq; double* flux_xa;   /* 2 nbins each: Q_b, C_b                                     */
  const art_sky_spec* sky;     /* NULL: no sky tables; mode is ignored                              */
  double* sky_sq;  double* sky_xa;    /* 2 n_theta n_phi n_dw each                                  */
  double* totals;              /* 8: n, A1, A2, Q_axion, Q_photon, C_axion, C_photon, bad nodes     */
} art_event_moments_out;
/* Asynchronous on `stream`; its scratch (16 B per node record) comes from the stream-ordered
 * allocator; no host synchronisation. Every table is ordinary device memory and takes float64
 * hardware adds. ART_E_INVALID before any device is touched: art_event_rows_device's argument faults
 * on p, in and the sky spec; reserved != 0; nbins < 0 or > 4096; a NULL node_start with n_nodes > 0;
 * a NULL table that the call needs. n_events == 0: ART_OK, nothing touched. */
int art_event_moments_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                             const art_event_moments_out* out, void* stream);

/* ---- coupling scan: one forest grown at the base coupling g0 = p->g_agg reweighted to many ----
 * No ray depends on g_agg; it enters only as the factor (g 1e-9 |B|)² of P_nonAD, so at coupling g_k
 * every crossing's exponent is s_k = (g_k / g0)² times the one at g0, and the tree weights follow
 * through P = 1 - exp(-P_nonAD). Per forward tree (node_start's ranges, records in the order the tree
 * processed them): the parent of a record is the one earlier record with n_cross > 0 whose (tc, xc)
 * equal its (t0, x0) bit for bit; a child of the other species is the converted branch. With x0 the
 * P_nonAD of the parent's stored first crossing, recomputed at g0, f_k = 1 - exp(-s_k x0) (converted)
 * or exp(-s_k x0) (unconverted); a record with n_cross > 1 took pc from the group of its segment's
 * crossings, so there x0 = -log(1 - pc), which is also ∝ g², and pc == 1 keeps the probabilities 1 and 0
 * (art_grow_trees and art_grow_trees_device store one crossing per forward segment: n_cross <= 1).
 * W_k(root) = 1, W_k = f_k W_k(parent) for a child pushed while the tree
 * split fully (the parent was pop number <= opts->mc_nodes), W_k = W_k(parent) (f_k / f_0) for a
 * Monte-Carlo child (f_0 at s = 1: the likelihood ratio of the drawn branch). The event's backtrace
 * factor is B_k = (1 - exp(-s_k x_root)) bweight^s_k, x_root the backtrace root's P_nonAD (parameters
 * with B0 negated, the sampled x, -k_init), bweight the backtrace node's stored weight (0 stays 0, 1
 * stays 1; a backtrace with exactly one crossing stores it, and bweight^s_k is then exp(-s_k x_c) from
 * its recomputed exponent). The power of a final row at g_k is W_k B_k [exp(-τ)] sln_prob, in art_event_rows_device's
 * bins. Every table is ACCUMULATED into (zero it first), ordinary device memory, coupling k's part at
 * k times the usual size. totals, 6 per coupling: [0], [1] Σ power of the axion and of the photon
 * rows; [2] the coverage, Σ_trees Σ W_k over the records that added to tot_prob (n_cross == 0): 1 per
 * tree explored to its end, less where the g0 run's stop rules cut what matters at g_k; [3] events
 * with bweight == 0 plus grouped forward records with pc == 1 (`saturated`: their exponents were lost
 * to underflow at g0); [4] records without
 * exactly one parent (`unlinked`; their weights are 0; must stay 0); [5] recomputed probabilities,
 * 1 - exp(-x0) against pc, the root's against back.prob and a single backtrace crossing's against its pc,
 * that are not bit-equal. [3]-[5] do not
 * depend on k and are repeated for each. */
typedef struct art_event_reweight_out {
  const double* erg;           /* n   INPUT: the forests' erg (the sampler's; art_event_rows_in has none) */
  int32_t nbins;               /* flux bins over [-π, π], 0 .. 4096 (0: no flux table)               */
  int32_t reserved;            /* 0                                                                   */
  double* flux;                /* K * 2 nbins                                                         */
  const art_sky_spec* sky;     /* NULL: no sky map; mode is ignored                                   */
  double* sky_hist;            /* K * 2 n_theta n_phi n_dw                                            */
  double* totals;              /* K * 6                                                               */
  double* weights;             /* may be NULL: K * n_nodes, W_k of every record (written, not added)  */
  double* back;                /* may be NULL: K * n_events, B_k of every event (written)             */
  double* back_prob;           /* may be NULL: K * n_events, its first factor 1 - exp(-s_k x_root)    */
  /* the second moments per coupling (art_event_moments_device's tables, a_e and bins those of the g0
   * forest); moment_totals NULL: none */
  double* flux_sq; double* flux_xa;   /* K * 2 nbins each                                            */
  double* sky_sq;  double* sky_xa;    /* K * 2 n_theta n_phi n_dw each                               */
  double* moment_totals;       /* K * 8 (slot 7, misplaced records, in the first coupling's only)     */
} art_event_reweight_out;
/* Asynchronous on `stream`, no host read; scratch (8 B per record, and per coupling 8 B per record
 * and per event for the weights and back factors not handed out, 8 B per record more with moments)
 * comes from the stream-ordered allocator. couplings: n_couplings values on the HOST. ART_E_INVALID
 * before any device is touched: a NULL p, in, out, opts or couplings; n_couplings < 1 or > 32; a
 * coupling or p->g_agg that is not finite and positive; reserved != 0; a NULL node_start or erg with
 * nodes present; art_event_moments_device's faults on the sky spec and nbins; a NULL table that the
 * call needs. n_events == 0: ART_OK, nothing touched. */
int art_event_reweight_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                              const art_tree_opts* opts, int32_t n_couplings, const double* couplings,
                              const art_event_reweight_out* out, void* stream);

/* ---- halo scan: one run drawn and weighted under a base halo model reweighted to many ----
 * With a halo model the sampler takes only the proposal scale v_prop and the integrator sees the drawn
 * speed through erg; v0 and v_ns enter only in the factor F of sln_prob. Two runs with the same seed and
 * the same v_prop draw the same events, grow the same forests and write the same rows but for column 7,
 * so a target model h seen from the run of the base model b is one scalar per event,
 *   R_h = F_h / F_b = (v0_b/v0_h)^3 exp(|u + v_b|^2/v0_b^2 - |u + v_h|^2/v0_h^2),   u = c vifty,
 * and the power of a final row under h is the run's own column 8 * column 7 (exp(-tau) included with the
 * cyclotron fields of `in`) times R_h of its event, in art_event_rows_device's bins. Column 12, the line
 * position, does not depend on the model. `base` must be the halo the run was sampled and weighted
 * with (its v_prop resolved as there); a model's own v_prop is ignored. Every table is ACCUMULATED into
 * (zero it first), ordinary device memory, model k's part at k times the usual size. */
typedef struct art_event_halo_scan_out {
  const double* vifty;         /* 3n INPUT: the sampler's vifty (SoA), the one the base run was weighted with */
  int32_t nbins;               /* flux bins over [-π, π], 0 .. 4096 (0: no flux table)               */
  int32_t reserved;            /* 0                                                                   */
  double* flux;                /* K * 2 nbins                                                         */
  const art_sky_spec* sky;     /* NULL: no sky map; mode is ignored                                   */
  double* sky_hist;            /* K * 2 n_theta n_phi n_dw                                            */
  double* totals;              /* K * 5: Σ power of the axion rows, of the photon rows, Σ_e R, Σ_e R²,
                                  records outside their tree's range (must stay 0; repeated for each k) */
  double* ratio;               /* may be NULL: K * n_events, R of every event (written, not added)    */
  /* the second moments per model (art_event_moments_device's tables, a_e and bins the run's own);
   * moment_totals NULL: none */
  double* flux_sq; double* flux_xa;   /* K * 2 nbins each                                            */
  double* sky_sq;  double* sky_xa;    /* K * 2 n_theta n_phi n_dw each                               */
  double* moment_totals;       /* K * 8 (slot 7, misplaced records, in the first model's only)        */
} art_event_halo_scan_out;
/* Asynchronous on `stream`, no host read; the base and the models (HOST memory) travel in the kernel
 * arguments; scratch (per model 8 B per event for the ratios not handed out, and with moments 8 B per
 * record per model and 16 B per record) comes from the stream-ordered allocator. ART_E_INVALID before
 * any device is touched: a NULL p, in, out, base or models; n_models < 1 or > 32; a base that the
 * sampler would refuse; a model whose v0 is not finite and positive or whose v_ns is not finite; a
 * model with v0 above the base's resolved v_prop (its weights are unbounded in the drawn speed under that
 * proposal); reserved != 0; art_event_moments_device's faults on nbins and the sky spec; a NULL vifty
 * with events or a NULL node_start with nodes present; a NULL table that the call needs.
 * n_events == 0: ART_OK, nothing touched. */
int art_event_halo_scan_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                               const art_halo* base, int32_t n_models, const art_halo* models,
                               const art_event_halo_scan_out* out, void* stream);

/* ---- jackknife replicates: the first-moment tables per group of events, for the error of ANY function of them ----
 * The events of a run are split into n_groups groups by global id, g = (event_offset + tree) mod n_groups (in a
 * row file (column 0 - 1) mod n_groups); the events are independent draws keyed by that id, so the groups are
 * exchangeable and do not depend on the chunks or the ranks. Per set k and group g the call ADDS the powers of g's
 * final rows to flux[k][g], sky_hist[k][g] and totals[k][g] (2: Σ power of all final axion rows and of all final
 * photon rows, binned or not), in art_event_rows_device's bins, and per group alone to groups[g] (3): [0] the
 * events n_g, [1] a_g = Σ_e a_e with art_event_moments_device's a_e = (attempts[e] - 1) + (final photon rows of
 * e), so Σ_g a_g is the run's f_inx (attempts NULL: the photon rows only), [2] the records inside the forest's
 * range that lie in the range of a tree other than their own (skipped; must stay 0). The powers by kind:
 *   0  the run's own, column 8 * column 7 (exp(-τ) included with the cyclotron fields of `in`); n_sets = 1;
 *   1  a coupling scan's, W_k B_k [exp(-τ)] sln_prob, from node_factor = art_event_reweight_out::weights and
 *      event_factor = art_event_reweight_out::back of the same chunk;
 *   2  a halo scan's, column 8 * column 7 times R_k, from event_factor = art_event_halo_scan_out::ratio.
 * With S a table summed over the groups, T_g its group g and f = Σ_g a_g, the estimate of a function φ is
 * φ(S / f), its leave-one-out g is φ((S - T_g) / (f - a_g)), and σ² = (R' - 1) / R' Σ_g (θ_g - mean θ)² over
 * the R' groups with n_g > 0. Everything adds over chunks and ranks. */
typedef struct art_event_replicates_out {
  int32_t n_groups;            /* R, 2 .. 64                                                          */
  int32_t kind;                /* 0 the run, 1 a coupling scan, 2 a halo scan                         */
  int32_t n_sets;              /* K, 1 .. 32; 1 with kind 0                                           */
  int32_t nbins;               /* flux bins over [-π, π], 0 .. 4096 (0: no flux table)               */
  const double* node_factor;   /* K * n_nodes  INPUT, kind 1: W_k of every record                    */
  const double* event_factor;  /* K * n_events INPUT, kind 1: B_k; kind 2: R_k of every event         */
  double* flux;                /* K * R * 2 nbins                                                     */
  const art_sky_spec* sky;     /* NULL: no sky map; mode is ignored                                   */
  double* sky_hist;            /* K * R * 2 n_theta n_phi n_dw                                        */
  double* totals;              /* K * R * 2                                                           */
  double* groups;              /* R * 3: n_g, a_g, misplaced records                                  */
} art_event_replicates_out;
/* Asynchronous on `stream`, no host read and no scratch. Every table is ordinary device memory and takes float64
 * hardware adds. ART_E_INVALID before any device is touched: a NULL p, in or out; n_groups outside 2 .. 64; an
 * unknown kind; n_sets outside 1 .. 32, or not 1 with kind 0; a NULL event_factor with kind 1 or 2, a NULL
 * node_factor with kind 1 and n_nodes > 0; art_event_moments_device's faults on nbins, the sky spec and
 * node_start; a NULL table that the call needs. n_events == 0: ART_OK, nothing touched. */
int art_event_replicates_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                                const art_event_replicates_out* out, void* stream);

/* ---- coupling x halo grid: the first-moment tables at every (coupling, halo model) cell, from the two scans' factors ----
 * The halo ratio is one scalar per event and does not depend on g, so at cell (kg, kh) the power of final row i of
 * event e is  pw = (W_kg[i] B_kg[e] [exp(-τ)] sln_prob) * R_kh[e]:  the coupling scan's power at g_kg, then ONE
 * multiplication by the halo scan's ratio, rounded on its own. node_factor = art_event_reweight_out::weights,
 * back = art_event_reweight_out::back and ratio = art_event_halo_scan_out::ratio, all three of the same chunk. The
 * rows counted and their bins are art_event_replicates_device's: a final record inside its own tree's range, in
 * art_event_rows_device's flux bins; a record in the range of a tree other than its own is skipped and counted.
 * With C = n_couplings n_models cells, cell = kg n_models + kh, every table is CELL-MINOR (the cell is the fastest
 * index: the kernel's lanes cover consecutive cells, so one instruction adds to 512 contiguous bytes) and
 * ACCUMULATED into (zero it first); ordinary device memory. The call ADDS
 *   flux[(sp nbins + fb) C + cell] += pw      for a row of species sp (0 axion, 1 photon) in flux bin fb,
 *   totals[sp C + cell]            += pw      for every final row, binned or not; totals[2 C + 0] += the misplaced
 *                                             records (the first cell's only; must stay 0),
 * with n_groups = R, g = (event_offset + tree) mod R:
 *   flux_rep[((g 2 + sp) nbins + fb) C + cell] += pw,   totals_rep[(g 2 + sp) C + cell] += pw,
 *   groups[g 3 + q]: art_event_replicates_device's n_g, a_g and misplaced records,
 * and with moment_totals non-NULL, per cell art_event_moments_device's 8 totals,
 *   moment_totals[q C + cell]: [0] the events n, [1] A1, [2] A2, [3], [4] Q of axions and photons, [5], [6] C of
 *   axions and photons, [7] the misplaced records (the first cell's only),
 * with X_{e,s}(kg, kh) = Σ pw over e's final rows of species s, summed in node order, and a_e the moments' a_e; so
 * the delta-method σ of a cell's totals follows as for art_event_moments_device, and n_eff = S_photon² / Q_photon.
 * There is NO sky map in the grid: 64 x 128 x 16 bins per cell would be 2 GiB at 32 x 32 cells, and the line shape
 * per model is already in the halo scan. Everything adds over chunks and ranks. */
typedef struct art_event_grid_out {
  int32_t n_couplings;         /* K_g, 1 .. 32                                                        */
  int32_t n_models;            /* K_h, 1 .. 32                                                        */
  int32_t nbins;               /* flux bins over [-π, π], 0 .. 4096 (0: no flux tables)              */
  int32_t n_groups;            /* R: 0 (no replicate tables) or 2 .. 64                               */
  const double* node_factor;   /* K_g * n_nodes  INPUT: W_kg of every record                          */
  const double* back;          /* K_g * n_events INPUT: B_kg of every event                           */
  const double* ratio;         /* K_h * n_events INPUT: R_kh of every event                           */
  double* flux;                /* 2 nbins * C                                                         */
  double* totals;              /* 3 * C: Σ power of the axion rows, of the photon rows, misplaced     */
  double* flux_rep;            /* R * 2 nbins * C (n_groups > 0)                                      */
  double* totals_rep;          /* R * 2 * C       (n_groups > 0)                                      */
  double* groups;              /* R * 3           (n_groups > 0): n_g, a_g, misplaced records         */
  double* moment_totals;       /* may be NULL: 8 * C                                                  */
} art_event_grid_out;
/* Asynchronous on `stream`, no host read, no scratch and no carried state. Every table is ordinary device memory and
 * takes float64 hardware adds. ART_E_INVALID before any device is touched: a NULL p, in or out; n_couplings or
 * n_models outside 1 .. 32; n_groups of 1, negative or above 64; art_event_moments_device's faults on nbins; a NULL
 * back or ratio with events, a NULL node_factor or node_start with n_nodes > 0; a NULL table that the call needs.
 * n_events == 0: ART_OK, nothing touched. */
int art_event_grid_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                          const art_event_grid_out* out, void* stream);

/* ---- event power spectrum: the distribution of the per-event power, its tail and its largest events ----
 * Every product of a run is a sum over events of X_{e,s}, art_event_moments_device's X: the powers of event e's final
 * rows of species s (0 axion, 1 photon), binned or not, summed in node order (a record in the range of a tree other
 * than its own is skipped and counted). This call keeps the DISTRIBUTION of X per set k and species s; the sets and
 * their powers by kind are art_event_replicates_device's (0 the run's own, n_sets = 1; 1 a coupling scan's from
 * node_factor and event_factor; 2 a halo scan's from event_factor). Everything is ACCUMULATED into (zero it first),
 * ordinary device memory, float64, and adds over chunks and ranks; entry (k, s) of a table lies at 2 k + s times
 * the table's size.
 *   Bins need no range: for a finite X > 0, bin = bits(X) >> (52 - sub_bits), the top 11 + sub_bits bits of the
 *   IEEE-754 pattern: 2^sub_bits bins per octave, NB = 2047 << sub_bits bins from the subnormals to the largest
 *   finite double, monotone in X; the lower edge of bin b is the double with the pattern b << (52 - sub_bits).
 *   count[b], sum[b], sum_sq[b]: the events whose X falls in bin b, their Σ X and Σ X².
 *   totals (8): [0] events, [1] events with finite X > 0, [2] with X == 0, [3] bad ones (negative, NaN, infinite:
 *   counted, and kept out of every table and list), [4] S = Σ X and [5] Q = Σ X² over [1], [6] misplaced records (in
 *   entry (0, 0) only; must stay 0), [7] reserved, 0. n_eff = S² / Q.
 *   The list: the `top` events with the largest finite X > 0, ordered by (X descending, global id ascending), as
 *   top_power and top_event (the 0-based id event_offset + tree, column 0 - 1 of a row), unused entries (0.0, -1).
 *   It is carried IN and OUT: the entries with id >= 0 found in the buffers are candidates of the call, so after any
 *   number of calls the list is a function of the multiset of (X, id) seen, whatever the chunks and their order.
 *   Start it as (0.0, -1). */
typedef struct art_event_spectrum_out {
  int32_t kind;                /* art_event_replicates_out's: 0 the run, 1 a coupling scan, 2 a halo scan */
  int32_t n_sets;              /* K, 1 .. 32; 1 with kind 0                                           */
  int32_t sub_bits;            /* m, 0 .. 4                                                           */
  int32_t top;                 /* T, 0 .. 256 (0: no list)                                            */
  const double* node_factor;   /* K * n_nodes  INPUT, kind 1: W_k of every record                    */
  const double* event_factor;  /* K * n_events INPUT, kind 1: B_k; kind 2: R_k of every event         */
  double* count;               /* K * 2 * (2047 << m)                                                 */
  double* sum;                 /* K * 2 * (2047 << m)                                                 */
  double* sum_sq;              /* K * 2 * (2047 << m)                                                 */
  double* totals;              /* K * 2 * 8                                                           */
  double* top_power;           /* K * 2 * T, IN and OUT                                               */
  int64_t* top_event;          /* K * 2 * T, IN and OUT                                               */
} art_event_spectrum_out;
/* Asynchronous on `stream`, no host read and no host synchronisation; scratch (K 2 n_events doubles and 16 B per
 * record) comes from the stream-ordered allocator. Every table takes float64 hardware adds. ART_E_INVALID before any
 * device is touched: a NULL p, in or out; an unknown kind; n_sets outside 1 .. 32, or not 1 with kind 0; sub_bits
 * outside 0 .. 4; top outside 0 .. 256; a NULL event_factor with kind 1 or 2, a NULL node_factor with kind 1 and
 * n_nodes > 0; a NULL node_start with n_nodes > 0; a NULL count, sum, sum_sq or totals; a NULL top_power or
 * top_event with top > 0. n_events == 0: ART_OK, nothing touched. */
int art_event_spectrum_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                              const art_event_spectrum_out* out, void* stream);

/* ---- exact tables: sums that do not depend on the order of the adds, the chunks or the ranks ----
 * The float tables above are sums of per-row powers with float64 hardware adds, so their last bits depend on the
 * order the adds arrive in. These calls keep the SAME sums exactly, in a fixed-point accumulator per bin, and round
 * once at the end: the result is round-to-nearest-even of the infinitely precise sum, a function of the multiset of
 * the powers alone, equal to float(sum(Fraction(v) for v in powers)) on the host.
 *   A finite double is ± m 2^q 2^-1074 with an integer m < 2^53 and q = max(e, 1) - 1 in 0 .. 2045 (e the biased
 *   exponent; a subnormal takes q = 0 without the implicit bit). A bin is ART_EXACT_LIMBS int64 limbs (528 bytes),
 *   limb j carrying the bits [32 j, 32 j + 32) above 2^-1074. Adding a value is at most three 64-bit integer adds:
 *   m << (q & 31), cut into 32-bit pieces, goes to the limbs q >> 5, + 1 and + 2, negated for a negative value.
 *   NORMALISED: every limb but the top one lies in [0, 2^32); the top one is signed and carries the sign and the
 *   headroom. Normalising changes the representation and never the value; normalised accumulators of the same
 *   multiset of values are equal limb by limb, and normalised accumulators add limb by limb (chunks, ranks, files),
 *   the sum to be normalised again before 2^30 of them are added.
 *   THE HEADROOM RULE: every entry point below LEAVES THE ACCUMULATORS IT ADDED TO NORMALISED and expects them
 *   normalised (zeros are), and normalises at least every 2^30 values inside a call, so no limb below the top one can
 *   overflow whatever the number of calls and rows. The top limb wraps only when the magnitude of a running sum
 *   reaches 2^1069, 2^45 times the largest double (a sum beyond the largest double finishes as ±inf long before).
 *   A NaN or an infinity is not added; it is counted in `nonfinite` (float64, ADDED to, one vector add per wave).
 * acc: n_bins * ART_EXACT_LIMBS int64, ACCUMULATED into (zero it first), ordinary device memory.
 * mode: 0 picks the path by the size, 1 forces the block-private LDS accumulators (n_bins <= 124, what 64 KiB hold)
 * flushed once per block, 2 forces adds to device memory; the limbs are the same on both. A bin < 0 or >= n_bins
 * is skipped. ART_E_INVALID before any device is touched: n < 0, n_bins < 1 or > 2^24, an unknown mode, mode 1 with
 * n_bins > 124, a NULL buffer that the call needs. n == 0: ART_OK, nothing touched. */
#define ART_EXACT_LIMBS 66
int art_exact_histogram_device(int64_t n, const int32_t* bins, const double* values, int32_t n_bins, int64_t* acc,
                               double* nonfinite, int32_t mode, void* stream);
/* out[b] = the correctly rounded double of bin b, one lane per bin: carry-propagate, take the sign from the top,
 * negate if negative, find the leading bit, take 53 bits with guard and sticky, round to nearest even, assemble the
 * pattern. A sum below 2^-1022 is exact; one that rounds to 2^1024 or beyond is ±inf; a sum of zero is +0.0. The
 * accumulator is only read: more can be added afterwards. */
int art_exact_finish_device(int64_t n_bins, const int64_t* acc, double* out, void* stream);
/* The host twins, the same functions compiled for the host (art_exact.h): add n values to the bins named (bins NULL:
 * all to bin 0) and leave every bin normalised, *nonfinite += the NaNs and infinities skipped (may be NULL);
 * normalise n_bins bins; round n_bins bins. They touch no device. */
int art_exact_add_host(int64_t n, const int32_t* bins, const double* values, int32_t n_bins, int64_t* acc,
                       int64_t* nonfinite);
int art_exact_normalize_host(int64_t n_bins, int64_t* acc);
int art_exact_round_host(int64_t n_bins, const int64_t* acc, double* out);

/* The exact tables of a chunk: art_event_replicates_device's contract without the groups. Per set k (kind 0 the
 * run's own powers, n_sets = 1; 1 a coupling scan's from node_factor and event_factor; 2 a halo scan's from
 * event_factor) the power of every final record inside its own tree's range -- formed by the same products in the
 * same order as the float kernels form it -- is added to totals_acc[k][species], to flux_acc[k] in
 * art_event_rows_device's flux bin and to sky_acc[k] in its sky bin. A record in the range of a tree other than its
 * own is skipped and counted in *misplaced (must stay 0). */
typedef struct art_event_exact_out {
  int32_t kind;                /* art_event_replicates_out's: 0 the run, 1 a coupling scan, 2 a halo scan */
  int32_t n_sets;              /* K, 1 .. 32; 1 with kind 0                                           */
  int32_t nbins;               /* flux bins over [-π, π], 0 .. 4096 (0: no flux table)               */
  int32_t mode;                /* 0 auto: totals, and the flux table when nbins <= 56, block-private in LDS;
                                  1 forces both into LDS (nbins <= 56); 2 forces every add to device memory */
  const double* node_factor;   /* K * n_nodes  INPUT, kind 1: W_k of every record                    */
  const double* event_factor;  /* K * n_events INPUT, kind 1: B_k; kind 2: R_k of every event         */
  int64_t* flux_acc;           /* K * 2 nbins * ART_EXACT_LIMBS                                       */
  const art_sky_spec* sky;     /* NULL: no sky map; its mode is ignored (the sky accumulators stay in HBM) */
  int64_t* sky_acc;            /* K * 2 n_theta n_phi n_dw * ART_EXACT_LIMBS                          */
  int64_t* totals_acc;         /* K * 2 * ART_EXACT_LIMBS: all final axion rows, all final photon rows */
  double* nonfinite;           /* K: powers that were NaN or infinite (not added anywhere)            */
  double* misplaced;           /* 1: records in the range of a tree other than their own              */
} art_event_exact_out;
/* Asynchronous on `stream`, no host read and no scratch: one launch per set and one normalisation of the tables, by
 * the headroom rule above. ART_E_INVALID before any device is touched: art_event_replicates_device's faults on p, in,
 * kind, n_sets, the factor arrays, nbins, the sky spec and node_start; an unknown mode, mode 1 with nbins > 56; a
 * NULL table or count that the call needs. n_events == 0: ART_OK, nothing touched. */
int art_event_exact_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                           const art_event_exact_out* out, void* stream);

/* ---- emission maps: the power over WHERE it was produced, and optionally jointly over where it goes ----
 * Per species the powers of a chunk's final rows (column 8 * column 7, what every other table adds) binned over the
 * conversion point of their event, the sampled x of columns 9 to 11, and with `observer` jointly over the direction
 * the row left in, C order:
 *   hist[species][obs_theta][obs_phi][r][origin_theta][origin_phi]     (no observer: the two observer extents are 1).
 * The origin: v = (x cm - z sm, y, x sm + z cm), each product and the add or subtract rounded on its own; r = |v| as
 * np.linalg.norm sums it, θ = acos(v_z / r), φ = atan2(v_y, v_x); the θ axis is θ over [0, π] or cos θ = v_z / r over
 * [-1, 1], φ is over [-π, π], r over [r_lo, r_hi], every axis binned as np.histogram bins its closed range. (cm, sm) =
 * (cos θm, sin θm) makes the magnetic axis the pole, (1, 0) leaves x as it is. A NaN or a value outside a range on any
 * axis drops the row from this table only. The observer bin and the species are art_event_rows_device's sky map's
 * for (n_theta, n_phi, n_dw = 1) of `observer`, so the table summed over its origin axes is that sky map. The
 * records counted are art_event_replicates_device's: a final record inside its own tree's range; a record in the
 * range of another tree is skipped and counted in misplaced. With groups = R the table has a leading group axis and a
 * row goes to group (event_offset + tree) mod R: R tables and no ungrouped one. */
typedef struct art_origin_spec {
  int32_t n_r, n_theta, n_phi;   /* each >= 1 */
  int32_t theta_axis;            /* 0: θ over [0, π]; 1: cos θ over [-1, 1] */
  int32_t mode;                  /* 0 auto, 1 LDS, 2 global */
  double  r_lo, r_hi;            /* ignored when n_r == 1 and r_lo == r_hi == 0: one bin, every finite r */
  double  cm, sm;                /* the rotation about y; (1, 0) leaves x as it is */
} art_origin_spec;
typedef struct art_event_origin_out {
  const art_origin_spec* origin;
  const art_sky_spec* observer;  /* NULL: no observer axes; n_dw must be 1; its mode is ignored */
  int32_t groups;                /* 0, or 2 .. 64 */
  double* hist;                  /* max(groups,1) * 2 * n_obs * n_r n_theta n_phi, ADDED to */
  int32_t* bin_out;              /* n_nodes, may be NULL: per record the flat bin without the group, -1: not counted */
  double* power_out;             /* n_nodes, may be NULL: per record the power, 0 where not final */
  double* misplaced;             /* 1, ADDED to; must stay 0 */
} art_event_origin_out;
/* Asynchronous on `stream`, no host read and no scratch. mode: a table (all groups) of at most 8192 doubles is
 * block-private in LDS and flushed once per block, a larger one takes float64 hardware adds in HBM; 1 and 2 force
 * either. ART_E_INVALID before any device is touched: art_event_replicates_device's faults on p, in and node_start;
 * a NULL out or origin; an axis below 1; an unknown theta_axis or mode; mode 1 with a table over 8192 doubles;
 * r_lo >= r_hi unless n_r == 1 and both are 0; a non-finite cm, sm or range; an observer with n_dw != 1 or a bad
 * axis; groups of 1, below 0 or above 64; a flat size of 2^31 or more; a NULL hist or misplaced.
 * n_events == 0: ART_OK, nothing touched. */
int art_event_origin_device(const art_params* p, const art_event_rows_in* in, const int64_t* node_start,
                            const art_event_origin_out* out, void* stream);

/* ---- reduction over the GPUs of a node (RCCL over xGMI) ----
 * One process per GPU. Rank 0 calls art_comm_unique_id and shares the 128 bytes with the
 * other ranks (a file, MPI, the launcher); every rank then calls art_comm_init on its device.
 * art_flux_allreduce sums count float64 values of a device buffer in place over all ranks,
 * asynchronously on `stream` (the binned flux and the run's counters f_inx, Σ weight, ...).
 * RCCL is opened on first use; without it these return ART_E_UNSUPPORTED. */
typedef struct art_rccl_id {
  char internal[128]; /* ncclUniqueId */
} art_rccl_id;
int art_comm_unique_id(art_rccl_id* id);
int art_comm_init(int32_t rank, int32_t world, const art_rccl_id* id);
int art_flux_allreduce(double* buf, int64_t count, void* stream);
/* the same for a host buffer (staged through HBM; synchronous) */
int art_flux_allreduce_host(double* buf, int64_t count);
int art_comm_destroy(void);

/* ---- pointwise physics on device, for parity tests (u: 7n SoA r,θ,φ,w_r,w_θ,w_φ,u7) */
/* func!/func_axion! (RayTracer.jl:71-123): du (7n) */
int art_eval_rhs_device(const art_params* p, int64_t n, const double* u, const double* tau,
                        const double* erg, const int8_t* species, double* du, void* stream);
/* hamiltonian (RayTracer.jl:530-556) at spherical x (3n), covariant k (3n), time T (n),
 * energy E (n): H (n), dH/dx (3n), dH/dk (3n), dH/dT (n). bndry_lyr applies to all. */
int art_eval_hamiltonian_device(const art_params* p, int64_t n, const double* x,
                                const double* k, const double* T, const double* E,
                                double* H, double* dHdx, double* dHdk, double* dHdT,
                                void* stream);
/* resonance condition (RayTracer.jl:254-298): value (n) */
int art_eval_condition_device(const art_params* p, int64_t n, const double* u,
                              const double* tau, double* out, void* stream);
/* cyclotron frequency omega_c [eV] (n) and the optical depth tau (n) of a crossing at Cartesian
 * pos / k (3n SoA) and time t (n) [s] */
int art_eval_cyclotron_device(const art_params* p, int64_t n, const double* pos, const double* k,
                              const double* t, double* wc, double* tau, void* stream);
/* the hand-written scalar functions of art_core.h themselves, one thread per element, for
 * ulp-level tests against the true value: out0[i] (and out1[i]) = fn(a[i], b[i]). b is read by
 * the two-operand ids only, out1 written by ART_MATH_SINCOS only; an output that is NULL is not
 * written. tu picks the translation unit the kernel was compiled in: 0 art_kernels.hip,
 * 1 art_kernels_nolicm.hip (eval_math_kernel of art_eval_math.h in each; the functions must round
 * alike in both). An unknown fn or tu is ART_E_INVALID. */
enum {
  ART_MATH_SINCOS = 0,  /* msincos(a): out0 = sin, out1 = cos */
  ART_MATH_EXP = 1,     /* fexp(a) */
  ART_MATH_LOG = 2,     /* flog(a) */
  ART_MATH_RCP = 3,     /* frcp(a) */
  ART_MATH_POW120 = 4,  /* fexp(flog(a) * (1.0 / 120.0)), the step-size controller's EEst2^(1/120) */
  ART_MATH_MAX_ABS = 5, /* fmax_abs(a, b) */
  ART_MATH_MIN_Q = 6,   /* fmin_q(a, b) */
  ART_MATH_MAX_Q = 7,   /* fmax_q(a, b) */
  ART_MATH_RCLAMP = 8,  /* rclamp(a, b): radius a clamped to rNS = b */
  ART_MATH_COUNT = 9
};
int art_eval_math_device(int32_t fn, int32_t tu, int64_t n, const double* a, const double* b,
                         double* out0, double* out1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ART_H */
