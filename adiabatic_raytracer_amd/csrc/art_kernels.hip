// art_kernels.hip -- the translation unit compiled with MachineLICM (build.py: -sink-insts-to-avoid-spills):
// flat's integrator instantiations (art_propagate.h), the small non-template kernels (fresh-record packing,
// post-processing, the pointwise probes) and every host-side launcher (art_internal.h). Every other
// integrator, the tail kernel, the helper kernel and the sampler are built in art_kernels_nolicm.hip.
// The event kernels come last: art_event_record.h (the record rule they share) before event_rows_kernel,
// then, under ART_EVENT_KERNELS, the kernels of the six art_event_*.h headers.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "art_core.h"
#include "art_event.h"
#include "art_internal.h"
#include <hipcub/hipcub.hpp>  // (the claim order's radix sort: this unit only)

#include "art_step.h"
#include "art_ray_io.h"
#include "art_propagate.h"
#include "art_helper.h"
#include "art_eval_math.h"
#include "art_tree_step.h"
#include "art_event_rows.h"

namespace art {

// Small batches (SegOut::small_tail): every fresh ray as a CONT_REC record for tail_kernel, the
// state the persistent integrator gives a ray it takes from the queue (its refill: u0, f0, dt
// and c0 from init_kernel, the controller's qold power at qoldinit = 1e-4, no b at the step
// start, counters at zero, the sign memory from c0), so a ray's arithmetic is the same whether
// a lane or a wave of its own integrates it (tests/test_edges.py compares small batches with
// large ones bit for bit).
__global__ __launch_bounds__(256) void pack_fresh_kernel(const int64_t n, const SegIn in, const SegOut out,
                                                         unsigned long long* __restrict__ stats) {
  const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ray == 0) {
    *out.cont_count = (unsigned long long)n;
    atomicAdd(&stats[ST_RAYS], (unsigned long long)n);
  }
  if (ray >= n) return;
  const double qpow_init = pow(1e-4, 1.0 / 15.0);
  double v[20];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    v[i] = in.u0[ray * U0_REC + i];
    v[7 + i] = in.u0[ray * U0_REC + 7 + i];
  }
  const double cprev = in.u0[ray * U0_REC + 15];
  v[14] = in.lnt0[ray];
  v[15] = in.u0[ray * U0_REC + 14];
  v[16] = qpow_init;
  v[17] = cprev;
  v[18] = NAN;
  v[19] = in.erg[ray];
  double2* rq = reinterpret_cast<double2*>(out.cont + ray * CONT_REC);
#pragma unroll
  for (int i = 0; i < 10; ++i) rq[i] = make_double2(v[2 * i], v[2 * i + 1]);
  const int photon = in.species[ray] != ART_AXION;
  const int sprev = isnan(cprev) ? 0 : sgn(cprev);
  int4* ri = reinterpret_cast<int4*>(rq + 10);
  ri[0] = make_int4((int)ray, 0, 0, 0);
  ri[1] = make_int4(0, sprev, photon | 2 /* cprev_ok */, 1 /* save_k */);
}

// ---------------------------------------------------------------------------
// get_Prob_nonAD over groups; one thread per group (groups are one segment's crossings).
__global__ __launch_bounds__(256) void prob_kernel(const KParams P, const int64_t nc, const double* __restrict__ pos,
                                                   const double* __restrict__ kpos, const double* __restrict__ erg,
                                                   const int64_t n_groups, const int64_t* __restrict__ gstart,
                                                   double* __restrict__ outp) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const int64_t a = gstart ? gstart[g] : g;
  const int64_t b = gstart ? gstart[g + 1] : g + 1;
  const int64_t m = b - a;
  if (m <= 0) return;
  // linear-indexed group values (column-major m x 3): index q -> row q % m, col q / m
  double ks_lin[3], B_lin[3], x0pl_lin[2];
  for (int q = 0; q < 3; ++q) {
    const int64_t row = q % m, col = q / m;
    const double p3[3] = {pos[a + row], pos[nc + a + row], pos[2 * nc + a + row]};
    const double k3[3] = {kpos[a + row], kpos[nc + a + row], kpos[2 * nc + a + row]};
    const ProbLocal<double> Lq = prob_local(P, p3, k3, erg[a + row]);
    ks_lin[q] = Lq.ks[col];
    B_lin[q] = Lq.B[col];
    if (q < 2) {
      const double sph[3] = {Lq.r, Lq.th, Lq.ph};
      x0pl_lin[q] = sph[col];
    }
  }
  ProbLin<double> G;
  G.k1 = ks_lin[0]; G.k2 = ks_lin[1]; G.k3 = ks_lin[2];
  G.B1 = B_lin[0]; G.B2 = B_lin[1]; G.B3 = B_lin[2];
  G.r_c = x0pl_lin[0]; G.th_c = x0pl_lin[1];
  for (int64_t i = a; i < b; ++i) {
    const double p3[3] = {pos[i], pos[nc + i], pos[2 * nc + i]};
    const double k3[3] = {kpos[i], kpos[nc + i], kpos[2 * nc + i]};
    const ProbLocal<double> L = prob_local(P, p3, k3, erg[i]);
    outp[i] = prob_eval(P, P.g_agg, L, G);
  }
}


// ---------------------------------------------------------------------------
// Binned flux (plot/flux.py:38-48): φf = atan2(k_y, k_x) of final particles, per species.
__global__ __launch_bounds__(256) void flux_kernel(const KParams P, const int64_t n, const double* __restrict__ x_end,
                                                   const double* __restrict__ k_end, const int32_t* __restrict__ status,
                                                   const int8_t* __restrict__ species, const double* __restrict__ w,
                                                   const int32_t nbins, double* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x) sh[i] = 0.0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double x[3] = {x_end[i], x_end[n + i], x_end[2 * n + i]}, k[3] = {k_end[i], k_end[n + i], k_end[2 * n + i]};
    const int bin = flux_bin_of(P, x, k, status[i], nbins);
    if (bin < 0) continue;
    const int row = (species && species[i] == ART_AXION) ? 0 : 1;
    atomicAdd(&sh[row * nbins + bin], w ? w[i] : 1.0);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x)
    if (sh[i] != 0.0) atomicAdd(&hist[i], sh[i]);
}

// Binned flux of npy rows (plot/flux.py:38-48): histogram of the given φf with weights w.
__global__ __launch_bounds__(256) void flux_phi_kernel(const int64_t n, const double* __restrict__ phi,
                                                       const int8_t* __restrict__ species,
                                                       const double* __restrict__ w, const int32_t nbins,
                                                       const double lo, const double hi,
                                                       double* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x) sh[i] = 0.0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int bin = np_hist_bin(phi[i], nbins, lo, hi);
    if (bin < 0) continue;
    const int row = (species && species[i] == ART_AXION) ? 0 : 1;
    atomicAdd(&sh[row * nbins + bin], w ? w[i] : 1.0);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x)
    if (sh[i] != 0.0) atomicAdd(&hist[i], sh[i]);
}

// ---------------------------------------------------------------------------
// Sky maps: a weighted 3-D histogram per species, hist[((s na + ia) nb + ib) nc + ic] (axions
// s = 0, photons s = 1), every axis np_hist_bin over its closed range -- np.histogramdd(range =,
// bins =) per species. An item outside the range (or NaN) on any axis is dropped.
__device__ inline int sky_bin_of(const SkyAxes& A, double a, double b, double c, int row) {
  const int ia = np_hist_bin(a, A.n[0], A.lo[0], A.hi[0]);
  const int ib = np_hist_bin(b, A.n[1], A.lo[1], A.hi[1]);
  // (c_all: one bin that holds every finite c, a range no pair of doubles spans)
  const int ic = A.c_all ? ((c - c == 0.0) ? 0 : -1) : np_hist_bin(c, A.n[2], A.lo[2], A.hi[2]);
  if ((ia | ib | ic) < 0) return -1;
  return ((row * A.n[0] + ia) * A.n[1] + ib) * A.n[2] + ic;
}

// The accumulation both sky-map kernels share. item(i, v) gives item i's flat bin (-1: not
// counted) and its weight. LDS: a block-private table of `table` doubles, zeroed, added to with
// LDS atomics and flushed once per block (its non-zero bins), as flux_phi_kernel does. Otherwise
// float64 adds straight to the table in HBM (hist must be ordinary device memory: the hardware
// add is not defined on fine-grained host memory); lanes of a wave in the same bin are not
// combined first: on a flat batch's directions that changed nothing ("sky maps").
template <bool LDS, class Item>
__device__ inline void sky_accumulate(const int64_t n, const int table, double* __restrict__ hist, double* sh,
                                      const Item& item) {
  if (LDS) {
    for (int b = threadIdx.x; b < table; b += blockDim.x) sh[b] = 0.0;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
    const int64_t i = i0 + threadIdx.x;
    double v = 0.0;
    int idx = i < n ? item(i, v) : -1;
    if (LDS) {
      if (idx >= 0) atomicAdd(&sh[idx], v);
      continue;
    }
    if (idx >= 0) unsafeAtomicAdd(&hist[idx], v);
  }
  if (LDS) {
    __syncthreads();
    for (int b = threadIdx.x; b < table; b += blockDim.x)
      if (sh[b] != 0.0) unsafeAtomicAdd(&hist[b], sh[b]);
  }
}

// The histogram of n items with coordinates (a, b, c), species flag and weight w (null: 1).
template <bool LDS>
__global__ __launch_bounds__(1024) void sky_map_kernel(const int64_t n, const double* __restrict__ a,
                                                        const double* __restrict__ b, const double* __restrict__ c,
                                                        const int8_t* __restrict__ species,
                                                        const double* __restrict__ w, const SkyAxes A,
                                                        double* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  sky_accumulate<LDS>(n, 2 * A.n[0] * A.n[1] * A.n[2], hist, sh, [&](int64_t i, double& v) {
    v = w ? w[i] : 1.0;
    return sky_bin_of(A, a[i], b[i], c[i], (species && species[i] == ART_AXION) ? 0 : 1);
  });
}

// The sky map of a propagated batch from its end states in HBM: the final segments (flux_bin_of's
// rule) binned over (θf or cos θf, φf, Δω) of trees.py's rows: |k| = sqrt(kx² + ky² + kz²),
// cos θf = kz / |k|, θf = acos(cos θf), φf = atan2(ky, kx), Δω = u7_end / mass_a + dw_offset,
// every operation rounded on its own as numpy rounds them. bin_out (may be null): each ray's
// flat bin, -1 for not counted.
template <bool LDS>
__global__ __launch_bounds__(1024) void sky_map_segments_kernel(
    const KParams P, const int64_t n, const double* __restrict__ x_end, const double* __restrict__ k_end,
    const double* __restrict__ u7_end, const int32_t* __restrict__ status, const int8_t* __restrict__ species,
    const double* __restrict__ w, const double* __restrict__ dw_offset, const SkyAxes A, const int cos_axis,
    double* __restrict__ hist, int32_t* __restrict__ bin_out) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  sky_accumulate<LDS>(n, 2 * A.n[0] * A.n[1] * A.n[2], hist, sh, [&](int64_t i, double& v) {
    const double x[3] = {x_end[i], x_end[n + i], x_end[2 * n + i]};
    int idx = -1;
    if (end_is_final(P, x, status[i])) {
#pragma clang fp contract(off)
      const double kx = k_end[i], ky = k_end[n + i], kz = k_end[2 * n + i];
      const double ct = kz / sqrt(kx * kx + ky * ky + kz * kz);
      const double dw = u7_end[i] / P.mass_a + (dw_offset ? dw_offset[i] : 0.0);
      idx = sky_bin_of(A, cos_axis ? ct : acos(ct), atan2(ky, kx), dw, (species && species[i] == ART_AXION) ? 0 : 1);
    }
    if (bin_out) bin_out[i] = idx;
    v = w ? w[i] : 1.0;
    return idx;
  });
}

// ---------------------------------------------------------------------------
// Pointwise physics for parity tests.
__global__ void eval_rhs_kernel(const KParams P, const int64_t n, const double* __restrict__ u,
                                const double* __restrict__ tau, const double* __restrict__ erg,
                                const int8_t* __restrict__ species, double* __restrict__ du) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double ui[7], d[7];
  for (int c = 0; c < 7; ++c) ui[c] = u[c * n + i];
  rhs(P, species[i] != ART_AXION, ui, tau[i], erg[i], d);
  for (int c = 0; c < 7; ++c) du[c * n + i] = d[c];
}

__global__ void eval_hamiltonian_kernel(const KParams P, const int64_t n, const double* __restrict__ x,
                                        const double* __restrict__ k, const double* __restrict__ Tm,
                                        const double* __restrict__ E, double* __restrict__ H,
                                        double* __restrict__ dHdx, double* __restrict__ dHdk,
                                        double* __restrict__ dHdT) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xi[3] = {x[i], x[n + i], x[2 * n + i]};
  const double ki[3] = {k[i], k[n + i], k[2 * n + i]};
  double h, gx[3], gk[3], gT;
  hamiltonian_full(P, xi, ki, Tm[i], E[i], &h, gx, gk, &gT);
  H[i] = h;
  dHdT[i] = gT;
  for (int c = 0; c < 3; ++c) {
    dHdx[c * n + i] = gx[c];
    dHdk[c * n + i] = gk[c];
  }
}

__global__ void eval_condition_kernel(const KParams P, const int64_t n, const double* __restrict__ u,
                                      const double* __restrict__ tau, double* __restrict__ outc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double ui[7];
  for (int c = 0; c < 7; ++c) ui[c] = u[c * n + i];
  outc[i] = condition(P, ui, tau[i]);
}

// ω_c and the optical depth of a crossing (cyclotron_wc_cart / cyclotron_tau) at n points
__global__ void eval_cyclotron_kernel(const KParams P, const int64_t n, const double* __restrict__ x,
                                      const double* __restrict__ k, const double* __restrict__ t,
                                      double* __restrict__ wc, double* __restrict__ tauc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xi[3] = {x[i], x[n + i], x[2 * n + i]};
  const double ki[3] = {k[i], k[n + i], k[2 * n + i]};
  wc[i] = cyclotron_wc_cart(P, xi, t[i]);
  tauc[i] = cyclotron_tau(P, xi, ki, t[i]);
}

// Event weight of every sampled point (MainRunner.jl:498-557, art_event.h); out: 5n SoA.
__global__ __launch_bounds__(256) void event_weight_kernel(const KParams P, const int64_t n, const double* __restrict__ x,
                                                           const double* __restrict__ k, const double* __restrict__ v,
                                                           const double maxR, const double rho, const double mcmc,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xi[3] = {x[i], x[n + i], x[2 * n + i]};
  const double ki[3] = {k[i], k[n + i], k[2 * n + i]};
  const double vi[3] = {v[i], v[n + i], v[2 * n + i]};
  const EventW E = event_weight(P, xi, ki, vi, maxR, rho, mcmc);
  out[i] = E.cos_w;
  out[n + i] = E.jacobian_GR;
  out[2 * n + i] = E.sln_prob;
  out[3 * n + i] = E.erg_inf_ini;
  out[4 * n + i] = E.vel_eng;
}

// The same with the halo model's factor and vel_eng (event_weight_halo, art_event.h).
__global__ __launch_bounds__(256) void event_weight_halo_kernel(const KParams P, const int64_t n,
                                                                const double* __restrict__ x,
                                                                const double* __restrict__ k,
                                                                const double* __restrict__ v, const double maxR,
                                                                const double rho, const double mcmc, const HaloK H,
                                                                double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xi[3] = {x[i], x[n + i], x[2 * n + i]};
  const double ki[3] = {k[i], k[n + i], k[2 * n + i]};
  const double vi[3] = {v[i], v[n + i], v[2 * n + i]};
  const EventW E = event_weight_halo(P, xi, ki, vi, maxR, rho, mcmc, H);
  out[i] = E.cos_w;
  out[n + i] = E.jacobian_GR;
  out[2 * n + i] = E.sln_prob;
  out[3 * n + i] = E.erg_inf_ini;
  out[4 * n + i] = E.vel_eng;
}

// ---------------------------------------------------------------------------
// host-side launch wrappers (art_internal.h)
// Resident blocks of `func` per CU from its own resource use: the unified 512-entry VGPR file
// of a CDNA SIMD (arch VGPRs + AGPRs, granule 8), 8 waves per SIMD at most, and the 160 KB of
// LDS per CU.
static int blocks_per_cu_from_attributes(const void* func, int block, int fallback) {
  hipFuncAttributes a{};
  if (hipFuncGetAttributes(&a, func) != hipSuccess) {
    (void)hipGetLastError();
    return fallback;
  }
  const int regs = a.numRegs > 0 ? ((a.numRegs + 7) / 8) * 8 : 8;
  int wps = 512 / regs;
  wps = wps > 8 ? 8 : wps;
  const int waves = (block + 63) / 64;
  int per_cu = (4 * wps) / waves;
  if (a.sharedSizeBytes > 0) {
    const int by_lds = (int)(163840 / a.sharedSizeBytes);
    per_cu = per_cu < by_lds ? per_cu : by_lds;
  }
  return per_cu < 1 ? 1 : per_cu;
}

// Compute units of the calling thread's current device (queried per call: the device may change)
static int cu_count() {
  int dev = 0, ncu = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  return ncu;
}

// resident blocks of `func` per CU
static int resident_blocks_per_cu(const void* func, int block, int fallback_per_cu) {
  int per_cu = 0;
  const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, func, block, 0);
  if (oe != hipSuccess || per_cu < 1) {
    // The runtime's occupancy calculator returns hipErrorUnknown (and 0 blocks) for the
    // 1-wave/SIMD flat integrator (270 unified VGPRs: 256 arch + 14 AGPRs), a kernel that
    // launches and runs correctly. That error stays the thread's last error, and the
    // hipGetLastError() after the next launch then reported the launch as failed (round 2's
    // "unknown error" on a 2000-ray flat batch, profiles/r03a_w1_launch_debug.txt). Clear it
    // and size the grid from the kernel's own resource use instead.
    (void)hipGetLastError();
    per_cu = blocks_per_cu_from_attributes(func, block, fallback_per_cu);
  }
  return per_cu;
}

int persistent_blocks(const void* func, int64_t work, int block, int fallback_per_cu) {
  const int ncu = cu_count();
  const int per_cu = resident_blocks_per_cu(func, block, fallback_per_cu);
  const int64_t need = (work + block - 1) / block;
  const int64_t full = (int64_t)ncu * per_cu;
  return (int)(need < full ? need : full);
}


// The geometry whose folded physics a kernel is instantiated for (specialize): flat space or
// Schwarzschild, each without boundary layer and with the anisotropic plasma, else the general one.
int geom_of(const KParams& P) {
  if (P.bndry_lyr > 0.0 || P.isotropic) return GEOM_ANY;
  return P.rs_eff == 0.0 ? GEOM_FLAT : (P.rs_eff > 0.0 ? GEOM_GR : GEOM_ANY);
}

// The propagate_kernel instantiation a plan names (art_launch_plan.h): flat's live here
// (ART_BUILDS_FLAT); every other one comes from art_kernels_nolicm.hip (nl_propagate,
// nl_propagate_cyc), where RK4 has the general geometry's builds only. nullptr: nobody instantiated it.
static KFn kernel_of(const LaunchBuild& b) {
  if (b.geom == GEOM_FLAT) {
#define ART_FL(I, G, S, D, W, C) \
  if (b == LaunchBuild{I, G, S, D, W, C}) return propagate_kernel<I, G, S, D, W, C>;
    ART_BUILDS_FLAT(ART_FL)
#undef ART_FL
    return nullptr;
  }
  if (b.cyc) return (b.integrator == ART_VERN6 && !b.save && b.wps == ART_WAVES_PER_SIMD) ? nl_propagate_cyc(b.geom, b.don) : nullptr;
  return nl_propagate(b.integrator, b.geom, b.save, b.don, b.wps);
}
static_assert(GEOM_ANY == LP_GEOM_ANY && GEOM_FLAT == LP_GEOM_FLAT && GEOM_GR == LP_GEOM_GR && ART_WAVES_PER_SIMD == LP_WPS &&
                  BLOCK == LP_BLOCK && HOT_BLOCKS == LP_HOT_BLOCKS,
              "art_launch_plan.h plans with the kernels' own constants");

int64_t small_tail_limit() {
  const char* e = std::getenv("ART_SMALL_TAIL");  // read per launch (tests switch it)
  if (e && *e) return std::atoll(e);
  return (int64_t)cu_count() * 4;
}

// The claim order (SegOut::order): 32-bit keys of the rays' initial step sizes (positive floats sort
// as their bits), the ray ids beside them, one stable radix sort.
__global__ void order_keys_kernel(int64_t n, const double* __restrict__ u0, unsigned* __restrict__ keys,
                                  int32_t* __restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    keys[i] = __float_as_uint((float)u0[i * U0_REC + 14]);
    ids[i] = (int32_t)i;
  }
}
struct OrderLayout {
  size_t keys_in, keys_out, ids_in, ids_out, tmp, tmp_bytes, total;
};
static OrderLayout order_layout(int64_t n) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  OrderLayout L{};
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const unsigned*)nullptr, (unsigned*)nullptr,
                                           (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  const size_t k = al((size_t)n * 4);
  L.keys_in = 0;
  L.keys_out = k;
  L.ids_in = 2 * k;
  L.ids_out = 3 * k;
  L.tmp = 4 * k;
  L.tmp_bytes = tb;
  L.total = 4 * k + al(tb);
  return L;
}
size_t claim_order_bytes(int64_t n) { return n > 0 && n < INT32_MAX ? order_layout(n).total : 0; }

// Raises a launch's *hot_done once the kernels that write hot records have ended (stream order).
__global__ void hot_done_kernel(unsigned* w) {
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_store(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

hipError_t launch_propagate(const KParams& P, int64_t n, const SegIn& in, const SegOut& out_arg, int32_t max_crossings,
                            unsigned long long* queue, unsigned long long* stats, hipStream_t s, const LaunchPlanIn& pin_arg,
                            LaunchPlan* ran, hipEvent_t ev0, hipEvent_t ev1, hipStream_t fs, const HotSide& hs) {
  const int64_t gr = (n + 255) / 256;
  const unsigned g1 = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(pick_helper(P), dim3((unsigned)(gr < 2048 ? gr : 2048)), dim3(256), 0, s, P, n, in, out_arg, (int)HK_INIT,
                     (int64_t)0, n, (int64_t)-1, 0, stats);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // The plan (art_launch_plan.h): first for the bulk kernel it names, then again with that kernel's
  // resident blocks per CU, which size the grids (the choice of kernels does not depend on them).
  LaunchPlanIn pin = pin_arg;
  LaunchPlan plan = plan_launch(pin);
  KFn fn = nullptr, cfn = nullptr;
  const TFn tfn = (plan.tail || plan.hot) ? nl_tail(plan.tail_geom) : nullptr;
  if (plan.bulk) {
    if (!(fn = kernel_of(plan.bulk_build))) return hipErrorInvalidDeviceFunction;
    pin.blocks_per_cu = resident_blocks_per_cu((const void*)fn, BLOCK, plan.bulk_build.wps == 1 ? 1 : ART_WAVES_PER_SIMD * 4 / (BLOCK / 64));
    plan = plan_launch(pin);
    if (plan.cont && !(cfn = kernel_of(plan.cont_build))) return hipErrorInvalidDeviceFunction;
  }
  // (the side stream and its events come from the caller: without them no launch graduates early)
  if ((plan.tail || plan.hot) && !tfn) return hipErrorInvalidDeviceFunction;
  if (plan.hot && !(out_arg.hot && out_arg.hot_ready && out_arg.hot_done && hs.stream && hs.fork && hs.join && hs.zero_word))
    return hipErrorInvalidValue;
  if (ran) *ran = plan;
  // graduation (SegOut::grad) only where the tail kernel runs after the continuation to resume
  // the graduated rays
  // (saveat and the cyclotron observation: the persistent integrator and its packed continuation
  // alone -- no tail kernel, graduation, hot side stream or 1-wave build)
  SegOut out = out_arg;
  if (!plan.grad_records) {
    out.grad = nullptr;
    out.graduate = 0;
  }
  // early graduation (SegOut::hot): only with graduation, and with the side stream that the hot
  // rays' tail launch runs on beside the bulk pass and the continuation
  const bool hot = plan.hot;
  if (!hot) {
    out.hot = nullptr;
    out.hot_at = 0;
  }
  out.order = nullptr;
  if (plan.sorted) {
    // the bulk pass claims the rays smallest initial step first (SegOut::order)
    const OrderLayout L = order_layout(n);
    char* b = (char*)out.order_tmp;
    hipLaunchKernelGGL(order_keys_kernel, dim3(g1), dim3(256), 0, s, n, in.u0, (unsigned*)(b + L.keys_in),
                       (int32_t*)(b + L.ids_in));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = L.tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(b + L.tmp, tb, (const unsigned*)(b + L.keys_in),
                                                (unsigned*)(b + L.keys_out), (const int32_t*)(b + L.ids_in),
                                                (int32_t*)(b + L.ids_out), (int)n, 0, 32, s)) != hipSuccess)
      return e;
    out.order = (const int32_t*)(b + L.ids_out);
  }
  if (plan.small_tail) {  // a small Vern6 batch: every ray on a wave of its own (tail_kernel)
    SegOut ot = out;
    ot.cont_count = out.cont_count;
    ot.cont_queue = out.cont_queue;
    hipLaunchKernelGGL(pack_fresh_kernel, dim3(g1), dim3(256), 0, s, n, in, ot, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int waves = plan.tail_waves;
    if (ev0 && (e = hipEventRecord(ev0, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(tfn, dim3(plan.tail_grid), dim3(64), 0, s, P, n, in, ot, max_crossings, waves, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev1 && (e = hipEventRecord(ev1, s)) != hipSuccess) return e;
    hipStream_t sf = s;
    if (fs && ev1 && fs != s) {
      if ((e = hipStreamWaitEvent(fs, ev1, 0)) != hipSuccess) return e;
      sf = fs;
    }
    hipLaunchKernelGGL(pick_helper(P), dim3(g1), dim3(256), 0, sf, P, n, in, out, (int)HK_FIN, (int64_t)0, n,
                       (int64_t)-1, 0, stats);
    return hipGetLastError();
  }
  // (the plan's bulk build: a batch that fits one ray per lane of 1 wave per SIMD runs the 1-wave/SIMD
  // build, which does not spill: lone GR tail ray -3%, flat -4.5% per attempt, bit-identical,
  // profiles/r02j_small_batch_w1_ab.txt, tests/test_edges.py; ART_W1=0 switches it off. Its grid: the
  // hot rays' launch is HOT_BLOCKS blocks of 4 waves, each beside one integrator block on a CU, one
  // wave of each per SIMD, so the bulk pass gives up that many of its blocks)
  const int grid = plan.bulk_grid;
  if (ev0 && (e = hipEventRecord(ev0, s)) != hipSuccess) return e;
  if (hot) {
    // on the side stream from the bulk pass's start: each wave resumes a hot record as soon as
    // one is written (one wave per ray, the tail kernel's arithmetic) and leaves once *hot_done is
    // raised after the continuation and none is left
    if ((e = hipEventRecord(hs.fork, s)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(hs.stream, hs.fork, 0)) != hipSuccess) return e;
    SegOut oh = out;
    oh.grad = nullptr;
    oh.graduate = 0;
    oh.hot_at = 0;
    oh.cont_count = hs.zero_word;  // (no drained-wave records: word 0 stays zero, word 1 is its queue)
    oh.cont_queue = hs.zero_word + 1;
    hipLaunchKernelGGL(tfn, dim3(HOT_BLOCKS), dim3(256), 0,
                       hs.stream, P, n, in, oh, max_crossings, 4 * HOT_BLOCKS, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(hs.join, hs.stream)) != hipSuccess) return e;
  }
  // (from here on every return raises *hot_done first, so the hot waves never wait past it)
  auto hot_done = [&](hipError_t err) {
    if (hot) {
      hipLaunchKernelGGL(hot_done_kernel, dim3(1), dim3(64), 0, s, out.hot_done);
      if (err == hipSuccess) err = hipGetLastError();
    }
    return err;
  };
  hipLaunchKernelGGL(fn, dim3(grid), dim3(BLOCK), 0, s, P, n, in, out, max_crossings, queue, stats);
  if ((e = hipGetLastError()) != hipSuccess) return hot_done(e);
  if (plan.cont) {  // the donated tail rays, packed into full waves (at most waves x donate of them)
    // with the tail kernel (ART_TAIL != 0, Vern6 without saveat) the packed continuation donates
    // in its turn: its drained waves' last rays (at most ART_TAIL_DONATE each, default 4) go to
    // the second-level records, and tail_kernel resumes each of those on a wave of its own
    SegOut oc = out;  // (the continuation sends its lagging rays to the hot records too)
    oc.cont_mode = 1;
    oc.cont_src = out.cont;
    oc.cont_src_count = out.cont_count;
    oc.donate = plan.cont_donate;
    oc.cont = out.cont2;
    oc.cont_count = out.cont2_count;
    // GR continuations at 1 wave/SIMD: no spills (68 VGPRs spill to scratch at 2). A/B on the
    // configs[3] bench line: 3.21e8 -> 3.35e8 ray-steps/s, bit-identical
    // (profiles/r02h_continuation_w1_ab.txt); flat stays at 2 (measured -3.5% at 1).
    hipLaunchKernelGGL(cfn, dim3(plan.cont_grid), dim3(BLOCK), 0, s, P, n, in, oc, max_crossings, queue, stats);
    if ((e = hipGetLastError()) != hipSuccess) return hot_done(e);
    if ((e = hot_done(hipSuccess)) != hipSuccess) return e;
    if (plan.tail) {
      // one wave per ray, at most one per SIMD of the device (ART_TAIL=k: k waves); more
      // second-level rays queue behind them
      SegOut ot = out;
      ot.cont = out.cont2;
      ot.cont_count = out.cont2_count;
      ot.cont_queue = out.cont2_queue;
      hipLaunchKernelGGL(tfn, dim3(plan.tail_grid), dim3(64), 0, s, P, n, in, ot, max_crossings, plan.tail_waves, stats);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  } else if ((e = hot_done(hipSuccess)) != hipSuccess) {
    return e;
  }
  if (hot && (e = hipStreamWaitEvent(s, hs.join, 0)) != hipSuccess) return e;
  if (ev1 && (e = hipEventRecord(ev1, s)) != hipSuccess) return e;
  hipStream_t sf = s;
  if (fs && ev1 && fs != s) {
    if ((e = hipStreamWaitEvent(fs, ev1, 0)) != hipSuccess) return e;
    sf = fs;
  }
  hipLaunchKernelGGL(pick_helper(P), dim3(g1), dim3(256), 0, sf, P, n, in, out, (int)HK_FIN, (int64_t)0, n, (int64_t)-1,
                     0, stats);
  return hipGetLastError();
}

// The streamed pipeline's integrator: Vern6 (flat / GR / general geometry), no saveat, no
// donation, at most `blocks` persistent blocks (the block slots it leaves free run the init and
// finalize kernels of the pieces).
hipError_t launch_integrator_streamed(const KParams& P, int64_t n, const SegIn& in, const SegOut& out,
                                      int32_t max_crossings, unsigned long long* queue, unsigned long long* stats,
                                      int blocks, hipStream_t s, LaunchPlan* ran) {
  const LaunchPlan plan = plan_streamed(n, geom_of(P), blocks);
  const KFn fn = kernel_of(plan.bulk_build);
  if (!fn) return hipErrorInvalidDeviceFunction;
  const int grid = plan.bulk_grid;
  if (ran) *ran = plan;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(BLOCK), 0, s, P, n, in, out, max_crossings, queue, stats);
  return hipGetLastError();
}

hipError_t launch_helpers(const KParams& P, int64_t n, const SegIn& in, const SegOut& out, int blocks, int64_t init_limit,
                          int announce, unsigned long long* stats, hipStream_t s) {
  hipLaunchKernelGGL(pick_helper(P), dim3((unsigned)blocks), dim3(256), 0, s, P, n, in, out, (int)HK_TILES, (int64_t)0, n,
                     init_limit, announce, stats);
  return hipGetLastError();
}

hipError_t launch_sample(const KParams& P, double maxR, uint64_t seed, int64_t ray_offset, int64_t n, double* x,
                         double* k, double* erg, double* vifty, int32_t* w, int32_t* att, unsigned long long* queue,
                         hipStream_t s, int waves, const HaloK* halo) {
  // lines of up to 2.2 x 60 km (264 steps): the 3-wave build, step by step (blocks of steps: no
  // faster there, 118 vs 119 ms per 1e7 flat samples); longer lines, mostly certified far from the
  // conversion surface: 2 waves, blocks of 3 steps (the scan's largest-maxR point 55 -> 43 ms,
  // profiles/r05h_ab_sampler.txt). waves (art_set_sampler_waves) = 2 or 3 takes that build for every
  // line; ART_SAMPLER_WPS=2|3 and ART_SAMPLER_BLOCKS=0|1 force a build (A/B)
  int wps = waves == 2 || waves == 3 ? waves : (maxR <= 60.0 ? 3 : 2);
  bool blocks = maxR > 60.0;
  if (const char* e = std::getenv("ART_SAMPLER_WPS"))
    if (e[0] == '2' || e[0] == '3') wps = e[0] - '0';
  if (const char* e = std::getenv("ART_SAMPLER_BLOCKS"))
    if (e[0] == '0' || e[0] == '1') blocks = e[0] == '1';

  if (halo) {  // the HALO builds: the same choice of build, the proposal scale as one more argument
    const SHFn fh = nl_sample_halo(wps, blocks);
    const int gh = persistent_blocks((const void*)fh, n, 256, 1);
    hipLaunchKernelGGL(fh, dim3(gh), dim3(256), 0, s, P, maxR, seed, ray_offset, n, x, k, erg, vifty, w, att, queue,
                       halo->vp);
    return hipGetLastError();
  }
  const SFn fn = nl_sample(wps, blocks);
  const int grid = persistent_blocks((const void*)fn, n, 256, 1);
  hipLaunchKernelGGL(fn, dim3(grid), dim3(256), 0, s, P, maxR, seed, ray_offset, n, x, k, erg, vifty, w, att, queue);
  return hipGetLastError();
}

hipError_t launch_prob(const KParams& P, int64_t nc, const double* pos, const double* kpos, const double* erg,
                       int64_t n_groups, const int64_t* gstart, double* out, hipStream_t s) {
  const int64_t grid = (n_groups + 255) / 256;
  hipLaunchKernelGGL(prob_kernel, dim3((unsigned)grid), dim3(256), 0, s, P, nc, pos, kpos, erg, n_groups, gstart, out);
  return hipGetLastError();
}

hipError_t launch_flux(const KParams& P, int64_t n, const double* x_end, const double* k_end, const int32_t* status,
                       const int8_t* species, const double* w, int32_t nbins, double* hist, hipStream_t s) {
  int64_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(flux_kernel, dim3((unsigned)grid), dim3(256), 2 * nbins * sizeof(double), s, P, n, x_end, k_end,
                     status, species, w, nbins, hist);
  return hipGetLastError();
}

hipError_t launch_flux_phi(int64_t n, const double* phi, const int8_t* species, const double* w, int32_t nbins,
                           double lo, double hi, double* hist, hipStream_t s) {
  int64_t grid = (n + 255) / 256;
  if (grid > 1024) grid = 1024;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(flux_phi_kernel, dim3((unsigned)grid), dim3(256), 2 * nbins * sizeof(double), s, n, phi, species, w,
                     nbins, lo, hi, hist);
  return hipGetLastError();
}

// The sky-map launches' geometry. LDS path (mode 1, or 0 with a table within SKY_LDS_DOUBLES): the
// blocks that are resident at once and no more, since each pays for zeroing and flushing its
// table: 256 threads while 8 tables fit a CU's 160 KiB, else 1024 (two 64 KiB tables still leave
// two blocks, 32 waves, on a CU). Global path: flux_kernel's grid. Every thread takes at least 4
// items, so small batches also run the grid-stride loop.
struct SkyLaunch {
  bool lds;
  int block;
  unsigned grid;
  size_t shmem;
};
static SkyLaunch sky_launch(int64_t n, const SkyAxes& A, int mode) {
  const int64_t table = 2 * (int64_t)A.n[0] * A.n[1] * A.n[2];
  SkyLaunch L;
  L.lds = mode == 1 || (mode == 0 && table <= SKY_LDS_DOUBLES);
  L.shmem = L.lds ? (size_t)table * sizeof(double) : 0;
  L.block = L.shmem > 16384 ? 1024 : 256;
  int64_t per_cu = 2048 / L.block;
  if (L.lds && (int64_t)(163840 / L.shmem) < per_cu) per_cu = 163840 / L.shmem;
  int64_t grid = (n + 4 * L.block - 1) / (4 * L.block);
  if (grid > 256 * per_cu) grid = 256 * per_cu;
  L.grid = (unsigned)(grid < 1 ? 1 : grid);
  return L;
}

hipError_t launch_sky_map(int64_t n, const double* a, const double* b, const double* c, const int8_t* species,
                          const double* w, const SkyAxes& A, int mode, double* hist, hipStream_t s) {
  const SkyLaunch L = sky_launch(n, A, mode);
  const auto fn = L.lds ? &sky_map_kernel<true> : &sky_map_kernel<false>;
  hipLaunchKernelGGL(fn, dim3(L.grid), dim3(L.block), L.shmem, s, n, a, b, c, species, w, A, hist);
  return hipGetLastError();
}

hipError_t launch_sky_map_segments(const KParams& P, int64_t n, const double* x_end, const double* k_end,
                                   const double* u7_end, const int32_t* status, const int8_t* species, const double* w,
                                   const double* dw_offset, const SkyAxes& A, int cos_axis, int mode, double* hist,
                                   int32_t* bin_out, hipStream_t s) {
  const SkyLaunch L = sky_launch(n, A, mode);
  const auto fn = L.lds ? &sky_map_segments_kernel<true> : &sky_map_segments_kernel<false>;
  hipLaunchKernelGGL(fn, dim3(L.grid), dim3(L.block), L.shmem, s, P, n, x_end, k_end, u7_end, status, species, w, dw_offset,
                     A, cos_axis, hist, bin_out);
  return hipGetLastError();
}

hipError_t launch_eval_rhs(const KParams& P, int64_t n, const double* u, const double* tau, const double* erg,
                           const int8_t* species, double* du, hipStream_t s) {
  hipLaunchKernelGGL(eval_rhs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n, u, tau, erg, species, du);
  return hipGetLastError();
}

hipError_t launch_eval_hamiltonian(const KParams& P, int64_t n, const double* x, const double* k, const double* T,
                                   const double* E, double* H, double* dHdx, double* dHdk, double* dHdT,
                                   hipStream_t s) {
  hipLaunchKernelGGL(eval_hamiltonian_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n, x, k, T, E, H,
                     dHdx, dHdk, dHdT);
  return hipGetLastError();
}

hipError_t launch_event_weight(const KParams& P, int64_t n, const double* x, const double* k, const double* v,
                               double maxR, double rho, double mcmc, double* out, hipStream_t s, const HaloK* halo) {
  if (halo) {
    hipLaunchKernelGGL(event_weight_halo_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n, x, k, v, maxR,
                       rho, mcmc, *halo, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(event_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n, x, k, v, maxR, rho,
                     mcmc, out);
  return hipGetLastError();
}

hipError_t launch_eval_cyclotron(const KParams& P, int64_t n, const double* x, const double* k, const double* t,
                                 double* wc, double* tau, hipStream_t s) {
  hipLaunchKernelGGL(eval_cyclotron_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n, x, k, t, wc, tau);
  return hipGetLastError();
}

hipError_t launch_eval_condition(const KParams& P, int64_t n, const double* u, const double* tau, double* out,
                                 hipStream_t s) {
  hipLaunchKernelGGL(eval_condition_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n, u, tau, out);
  return hipGetLastError();
}

hipError_t launch_eval_math(int fn, int tu, int64_t n, const double* a, const double* b, double* out0, double* out1,
                            hipStream_t s) {
  const MFn k = tu ? nl_eval_math(fn) : pick_eval_math<0>(fn);
  if (!k) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, a, b, out0, out1);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The device-resident tree driver (art_grow_trees_device, art_device.cpp): every tree's state and
// event stack stay in HBM (art_tree_step.h); a round is pack -> one batched propagate -> step ->
// an inclusive scan of the trees that go on, whose last value -- the next round's batch size -- is
// the only thing the host reads. Ordering comes from the stream alone.

// Roots (:132-137): state, the root event with prob = 1 - exp(-P_nonAD), and round 1's selection
// (every tree, in order).
__global__ __launch_bounds__(256) void tree_root_kernel(const KParams P, const TreeRules R, const int64_t n,
                                                        const double* __restrict__ x0, const double* __restrict__ k0,
                                                        const double* __restrict__ erg,
                                                        const int8_t* __restrict__ species, TreeState* __restrict__ state,
                                                        TreeEv* __restrict__ stack, int32_t* __restrict__ list,
                                                        int32_t* __restrict__ flag, int32_t* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x[3] = {x0[i], x0[n + i], x0[2 * n + i]}, k[3] = {k0[i], k0[n + i], k0[2 * n + i]};
  TreeState T{};
  T.erg = erg[i];
  T.info = 1;
  T.active = 1;
  T.depth = 1;
  state[i] = T;
  stack[i * R.stack_cap] = tree_root(x, k, species[i], tree_root_prob(P, x, k, T.erg));
  list[i] = (int32_t)i;
  flag[i] = 1;
  pos[i] = (int32_t)i + 1;
}

// Pop and pack: entry jp of the last round's list that goes on (flag) pops its tree's next event
// into slot pos[jp] - 1 of this round's batch of m segments (SoA, stride m) and of its list.
__global__ __launch_bounds__(256) void tree_pack_kernel(const TreeRules R, const int64_t m_prev, const int64_t m,
                                                        const int32_t* __restrict__ list_prev,
                                                        const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                        int32_t* __restrict__ list, TreeState* __restrict__ state,
                                                        const TreeEv* __restrict__ stack, const TreeBatch B,
                                                        const double dt0, const double ln_dt0) {
  const int64_t jp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (jp >= m_prev || !flag[jp]) return;
  const int64_t j = (int64_t)pos[jp] - 1;
  if (j < 0 || j >= m) return;
  const int32_t tree = list_prev[jp];
  TreeState T = state[tree];
  if (!tree_pop(T)) return;
  state[tree] = T;
  const TreeEv e = stack[(int64_t)tree * R.stack_cap + T.depth];
  for (int c = 0; c < 3; ++c) {
    B.x0[c * m + j] = e.x[c];
    B.k0[c * m + j] = e.k[c];
  }
  B.erg[j] = T.erg;
  B.dw[j] = e.dw;
  B.lnt0[j] = tree_ln_t0(e.t, dt0, ln_dt0);
  B.species[j] = (int8_t)e.species;
  list[j] = tree;
}

// The step: lane j takes the results of segment j for its tree, appends the finished node to the
// log (its tree and its sequence number in it inside the record) and says whether the tree goes on.
__global__ __launch_bounds__(256) void tree_step_kernel(const KParams P, const TreeRules R, const int64_t n, const int64_t m,
                                                        const int32_t* __restrict__ list, TreeState* __restrict__ state,
                                                        TreeEv* __restrict__ stack, const TreeBatch B,
                                                        art_tree_node* __restrict__ log, int32_t* __restrict__ flag,
                                                        int32_t* __restrict__ err) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int32_t tree = list[j];
  flag[j] = 0;
  // (neither happens: pack fills every slot of the list, and a popped event lies below the
  // capacity. Should one, no access leaves the arrays: the call fails, the log gets a record of tree 0)
  const bool in_list = tree >= 0 && tree < n;
  if (!in_list || state[tree].depth < 0 || state[tree].depth >= R.stack_cap) {
    *err = 1;
    art_tree_node none{};
    log[j] = none;
    return;
  }
  TreeState T = state[tree];
  SegEnd S;
  for (int c = 0; c < 3; ++c) {
    S.x_end[c] = B.x_end[c * m + j];
    S.k_end[c] = B.k_end[c * m + j];
  }
  S.u7_end = B.u7_end[j];
  S.tau_end = B.tau_end[j];
  S.status = B.status[j];
  S.count = B.xcount[j];
  const XcView X{R.cap, m, j, B.xpos, B.xk, B.xt, B.xdw, B.xp};
  GroupProbPhysics gp{P, {}};
  art_tree_node node;
  const bool go = tree_step(R, (int64_t)tree, T, stack + (int64_t)tree * R.stack_cap, S, X, gp, node);
  state[tree] = T;
  log[j] = node;
  flag[j] = go ? 1 : 0;
  if (T.overflow) *err = 1;
}

// The end: get_tree's count and info of every tree, and the counts (n + 1 of them, the last 0) that
// the exclusive scan turns into node_start.
__global__ __launch_bounds__(256) void tree_finish_kernel(const TreeRules R, const int64_t n,
                                                          const TreeState* __restrict__ state,
                                                          int32_t* __restrict__ counts1, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ infos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    counts1[n] = 0;
    return;
  }
  const TreeState T = state[i];
  counts1[i] = T.count;
  if (counts) counts[i] = T.count;
  if (infos) infos[i] = tree_info(T, R.mc_nodes);
}

// Flatten: log record q goes to nodes[node_start[its tree] + its sequence number] -- trees in
// order, each tree's nodes in the order it processed them -- one 8-byte word per thread, pad zeroed.
constexpr int TREE_NODE_WORDS = (int)(sizeof(art_tree_node) / 8);
static_assert(sizeof(art_tree_node) % 8 == 0 && offsetof(art_tree_node, pad) == 20, "art_tree_node layout");
__global__ __launch_bounds__(256) void tree_flatten_kernel(const int64_t total, const art_tree_node* __restrict__ log,
                                                           const int64_t* __restrict__ node_start,
                                                           const int64_t capacity, art_tree_node* __restrict__ nodes) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= total * TREE_NODE_WORDS) return;
  const int64_t q = w / TREE_NODE_WORDS;
  const int wi = (int)(w - q * TREE_NODE_WORDS);
  const int64_t dst = node_start[log[q].tree] + log[q].pad;
  if (dst < 0 || dst >= capacity) return;
  unsigned long long v = reinterpret_cast<const unsigned long long*>(log + q)[wi];
  if (wi == 2) v &= 0xffffffffull;  // {status, pad}
  reinterpret_cast<unsigned long long*>(nodes + dst)[wi] = v;
}

struct ToI64 {
  __host__ __device__ int64_t operator()(const int32_t& v) const { return (int64_t)v; }
};
using CountIt = hipcub::TransformInputIterator<int64_t, ToI64, const int32_t*>;

size_t tree_scan_bytes(int64_t n) {
  size_t a = 0, b = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, a, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, CountIt(nullptr, ToI64()), (int64_t*)nullptr, (int)(n + 1));
  return a > b ? a : b;
}

hipError_t launch_tree_roots(const KParams& P, const TreeRules& R, int64_t n, const double* x0, const double* k0,
                             const double* erg, const int8_t* species, TreeState* state, TreeEv* stack, int32_t* list,
                             int32_t* flag, int32_t* pos, hipStream_t s) {
  hipLaunchKernelGGL(tree_root_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, R, n, x0, k0, erg, species,
                     state, stack, list, flag, pos);
  return hipGetLastError();
}

hipError_t launch_tree_pack(const TreeRules& R, int64_t m_prev, int64_t m, const int32_t* list_prev, const int32_t* flag,
                            const int32_t* pos, int32_t* list, TreeState* state, const TreeEv* stack, const TreeBatch& B,
                            double dt0, double ln_dt0, hipStream_t s) {
  hipLaunchKernelGGL(tree_pack_kernel, dim3((unsigned)((m_prev + 255) / 256)), dim3(256), 0, s, R, m_prev, m, list_prev,
                     flag, pos, list, state, stack, B, dt0, ln_dt0);
  return hipGetLastError();
}

hipError_t launch_tree_step(const KParams& P, const TreeRules& R, int64_t n, int64_t m, const int32_t* list, TreeState* state,
                            TreeEv* stack, const TreeBatch& B, art_tree_node* log, int32_t* flag, int32_t* pos,
                            int32_t* err, void* tmp, size_t tmp_bytes, hipStream_t s) {
  hipLaunchKernelGGL(tree_step_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, P, R, n, m, list, state, stack,
                     B, log, flag, err);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, (const int32_t*)flag, pos, (int)m, s);
}

hipError_t launch_tree_finish(const TreeRules& R, int64_t n, const TreeState* state, int32_t* counts1, int32_t* counts,
                              int32_t* infos, int64_t* node_start, void* tmp, size_t tmp_bytes, hipStream_t s) {
  hipLaunchKernelGGL(tree_finish_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, s, R, n, state, counts1, counts,
                     infos);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, CountIt(counts1, ToI64()), node_start, (int)(n + 1), s);
}

hipError_t launch_tree_flatten(int64_t total, const art_tree_node* log, const int64_t* node_start, int64_t capacity,
                               art_tree_node* nodes, hipStream_t s) {
  const int64_t words = total * TREE_NODE_WORDS;
  if (words <= 0) return hipSuccess;
  hipLaunchKernelGGL(tree_flatten_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, total, log, node_start,
                     capacity, nodes);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Event rows (art_event_rows_device): one pass over the forward forest's node records turns its
// final nodes into main_runner_tree's npy rows (art_event_rows.h), in node order, and bins them
// into the azimuth flux table and the sky map while they are in registers. The order comes from an
// exclusive sum of is_final != 0 over the records (read through an iterator: no flag array), so
// row r is the r-th final node, as tree[tree["is_final"] != 0] orders them.
struct FinalOf {
  __host__ __device__ int32_t operator()(const art_tree_node& nd) const { return nd.is_final != 0 ? 1 : 0; }
};
struct FinalPhotonOf {
  __host__ __device__ int32_t operator()(const art_tree_node& nd) const {
    return (nd.is_final != 0 && nd.species != ART_AXION) ? 1 : 0;
  }
};
using FinalIt = hipcub::TransformInputIterator<int32_t, FinalOf, const art_tree_node*>;
using FinalPhotonIt = hipcub::TransformInputIterator<int32_t, FinalPhotonOf, const art_tree_node*>;

size_t event_scan_bytes(int64_t n_nodes) {
  size_t a = 0, b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, FinalIt(nullptr, FinalOf()), (int32_t*)nullptr, (int)n_nodes);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, FinalPhotonIt(nullptr, FinalPhotonOf()), (int32_t*)nullptr,
                                         (int)n_nodes);
  return a > b ? a : b;
}

hipError_t launch_event_scan(int64_t n_nodes, const art_tree_node* nodes, bool photons_only, int32_t* pos, void* tmp,
                             size_t tmp_bytes, hipStream_t s) {
  if (photons_only)
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, FinalPhotonIt(nodes, FinalPhotonOf()), pos, (int)n_nodes, s);
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, FinalIt(nodes, FinalOf()), pos, (int)n_nodes, s);
}

// The cyclotron re-run's inputs: final photon node i goes to slot pos[i] of a segment batch of m
// (SoA, stride m) with the forest's own inputs -- x0, k0, its tree's erg, dw0, and ln t0 by
// tree_pack_kernel's function and constants -- and slot[i] says where (-1: no re-run).
__global__ __launch_bounds__(256) void event_gather_kernel(const int64_t n_nodes, const art_tree_node* __restrict__ nodes,
                                                           const int32_t* __restrict__ pos, const int64_t n_events,
                                                           const double* __restrict__ erg, const int64_t m,
                                                           const TreeBatch B, int32_t* __restrict__ slot, const double dt0,
                                                           const double ln_dt0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const art_tree_node& nd = nodes[i];
  const int64_t j = pos[i];
  const bool take = FinalPhotonOf()(nd) && j >= 0 && j < m && nd.tree >= 0 && nd.tree < n_events;
  slot[i] = take ? (int32_t)j : -1;
  if (!take) return;
  for (int c = 0; c < 3; ++c) {
    B.x0[c * m + j] = nd.x0[c];
    B.k0[c * m + j] = nd.k0[c];
  }
  B.erg[j] = erg[nd.tree];
  B.dw[j] = nd.dw0;
  B.lnt0[j] = tree_ln_t0(nd.t0, dt0, ln_dt0);
  B.species[j] = (int8_t)ART_PHOTON;
}

hipError_t launch_event_gather(int64_t n_nodes, const art_tree_node* nodes, const int32_t* pos, int64_t n_events,
                               const double* erg, int64_t m, const TreeBatch& B, int32_t* slot, double dt0, double ln_dt0,
                               hipStream_t s) {
  hipLaunchKernelGGL(event_gather_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, n_nodes, nodes, pos,
                     n_events, erg, m, B, slot, dt0, ln_dt0);
  return hipGetLastError();
}

}  // namespace art

// EventLoad and what the event kernels at the end of this file share: the record rule, a tree's range, the wave add
#include "art_event_record.h"

namespace art {

// One lane per node record (grid-stride). LDS holds [the flux table, 2 nbins | the sky table when
// LDS]; the sky map goes through sky_accumulate, the flux table is block-private beside it and
// flushed like it, the totals are summed per lane, then per wave, and added once per wave.
// Its rule is not event_record's: a row needs no tree range, so every final record with a `tree` in
// [0, n_events) gives one, wherever it lies, and the re-run's slot j is kept for the mismatch count.
template <bool LDS>
__global__ __launch_bounds__(1024) void event_rows_kernel(const EventRowsArgs a, const SkyAxes A, const int cos_axis,
                                                           const int sky_table) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  double* sh_flux = sh;
  double* sh_sky = sh + 2 * a.nbins;
  for (int b = threadIdx.x; b < 2 * a.nbins; b += blockDim.x) sh_flux[b] = 0.0;
  if (!LDS) __syncthreads();  // (the LDS path syncs inside sky_accumulate, after zeroing its table)
  double tot[EV_TOT_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  sky_accumulate<LDS>(n, LDS ? sky_table : 0, a.sky_hist, sh_sky, [&](int64_t i, double& v) {
    if (i < a.n_events && a.attempts) tot[EV_TOT_ATTEMPTS] += (double)((int64_t)a.attempts[i] - 1);
    if (i >= a.n_nodes) return -1;
    const art_tree_node& nd = a.nodes[i];
    const int64_t e = nd.tree;
    if (nd.is_final == 0 || e < 0 || e >= a.n_events) return -1;
    const int64_t r = a.pos[i];
    const EventLoad E{a, e};
    double tau = 0.0;
    if (a.cyc_slot) {
      const int64_t j = a.cyc_slot[i], m = a.cyc_n;
      if (j >= 0 && j < m) {
        tau = a.cyc_tau[j];
        bool same = a.cyc_status[j] == nd.status && event_same(a.cyc_u7_end[j], nd.u7_end) &&
                    event_same(a.cyc_tau_end[j], nd.tau_end);
        for (int c = 0; c < 3; ++c)
          same = same && event_same(a.cyc_x_end[c * m + j], nd.x_end[c]) && event_same(a.cyc_k_end[c * m + j], nd.k_end[c]);
        if (!same) tot[EV_TOT_MISMATCH] += 1.0;
      } else if (nd.species != ART_AXION) {
        tot[EV_TOT_MISMATCH] += 1.0;  // a final photon without its re-run
      }
    }
    double* dst = (a.rows && r >= 0 && r < a.row_capacity) ? a.rows + r * a.ncols : nullptr;
    const EventRowBins B = event_row(nd, E, a.event_offset, a.mass_a, tau, a.cyc_slot != nullptr, a.ncols, dst);
    const int sp = B.species;
    v = B.power;
    tot[EV_TOT_ROWS] += 1.0;
    tot[EV_TOT_PHOTONS] += (double)sp;
    tot[EV_TOT_SUM_AXION + sp] += v;
    if (a.nbins > 0) {
      const int fb = np_hist_bin(B.phi, a.nbins);
      if (fb >= 0) atomicAdd(&sh_flux[sp * a.nbins + fb], v);
    }
    int idx = -1;
    if (a.sky_hist) idx = sky_bin_of(A, cos_axis ? B.cos_theta : B.theta, B.phi, B.dw, sp);
    if (a.bin_out && r >= 0 && r < a.row_capacity) a.bin_out[r] = idx;
    return idx;
  });
  __syncthreads();
  for (int b = threadIdx.x; b < 2 * a.nbins; b += blockDim.x)
    if (sh_flux[b] != 0.0) unsafeAtomicAdd(&a.flux[b], sh_flux[b]);
  for (int q = 0; q < EV_TOT_COUNT; ++q) {
    double t = tot[q];
    for (int off = warpSize / 2; off > 0; off >>= 1) t += __shfl_down(t, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && t != 0.0) unsafeAtomicAdd(&a.totals[q], t);
  }
}

hipError_t launch_event_rows(const EventRowsArgs& a, const SkyAxes& A, int cos_axis, int mode, hipStream_t s) {
  const int64_t n = a.n_nodes > a.n_events ? a.n_nodes : a.n_events;
  if (n <= 0) return hipSuccess;
  // the sky launches' geometry; without a sky map, its HBM path's (no table in LDS)
  SkyLaunch L = sky_launch(n, A, a.sky_hist ? mode : 2);
  const int64_t table = 2 * (int64_t)A.n[0] * A.n[1] * A.n[2];
  // the two tables share the 64 KiB a block takes (mode 1 beyond it is refused by the caller)
  if (L.lds && table + 2 * a.nbins > SKY_LDS_DOUBLES) {
    const SkyLaunch G = sky_launch(n, A, 2);
    L = G;
  }
  const size_t shmem = L.shmem + 2 * (size_t)a.nbins * sizeof(double);
  const auto fn = L.lds ? &event_rows_kernel<true> : &event_rows_kernel<false>;
  hipLaunchKernelGGL(fn, dim3(L.grid), dim3(L.block), shmem, s, a, A, cos_axis, (int)table);
  return hipGetLastError();
}

}  // namespace art

// The kernels and launchers of the six event headers (ART_EVENT_KERNELS; without it a header is its
// __host__ __device__ functions alone, which the host builds of the CPU tests include): the event moments
// (art_event_moments_device), the coupling scan (art_event_reweight_device), the halo scan
// (art_event_halo_scan_device), the jackknife replicates (art_event_replicates_device), the coupling x halo grid
// (art_event_grid_device) and the event power spectrum (art_event_spectrum_device). All take their records through
// art_event_record.h above.
#define ART_EVENT_KERNELS
#include "art_event_moments.h"
#include "art_event_reweight.h"
#include "art_event_haloscan.h"
#include "art_event_replicates.h"
#include "art_event_grid.h"
#include "art_event_spectrum.h"
// the emission maps (art_event_origin_device): the power over its origin and observer, through event_record and
// sky_accumulate
#include "art_event_origin.h"
// the exact tables (art_exact_histogram_device, art_exact_finish_device, art_event_exact_device): a seventh kernel of
// the family, on integer limbs
#include "art_exact.h"
