// art_event_grid.h -- the coupling x halo grid (art_event_grid_device): the first-moment tables of a chunk at every
// cell (coupling kg, halo model kh) of a K_g x K_h grid, from the factors the two scans hand out. The halo ratio is
// one scalar per event and does not depend on g, so the power of final record i of event e at cell (kg, kh) is
//   pw = reweight_power(W[kg, i], B[kg, e], cyclotron, τ, sln_prob) * R[kh, e],
// the coupling scan's power times the halo scan's ratio, one multiplication rounded on its own. The records counted
// are event_replicates_kernel's, by the rule of art_event_record.h: a final record of its own tree's range, its bin
// and its event's values taken once; a misplaced record is skipped and counted. Per cell the call adds pw to the
// flux table and the two species' totals, with n_groups = R the same per
// group g = (event_offset + tree) mod R (and art_event_replicates_device's groups, 3 per group), and with
// moment_totals art_event_moments_device's 8 totals per cell, from X_{e,s}(kg, kh) = Σ pw over e's final rows of
// species s in node order (the sum of the per-record products: the first and the second moments are sums of the
// same terms). There is NO sky map in the grid: a 64 x 128 x 16 map per cell would be 2 GiB at 32 x 32 cells, and
// the line shape per model is already in the halo scan.
//
// Tables are CELL-MINOR, cell = kg K_h + kh the fastest index (C = K_g K_h cells):
//   flux        [(sp nbins + fb) C + cell]                  totals      [q C + cell], q = GRID_TOT_*
//   flux_rep    [((g 2 + sp) nbins + fb) C + cell]          totals_rep  [(g 2 + sp) C + cell]
//   moment_totals [q C + cell], q = EM_TOT_*                 groups      [g 3 + q], q = REP_GRP_*
// so that the lanes of a wave, which cover 64 consecutive cells, add to 512 contiguous bytes with one instruction
// and no two lanes of one instruction share an address.
//
// The per-cell arithmetic is written once as __host__ __device__ functions: the kernel below and a host build for
// the CPU tests (tools/eventgrid.cpp) compile the same source. The kernel takes its records through
// art_event_record.h and is compiled only in art_kernels.hip (ART_EVENT_KERNELS).
#pragma once
#include "art_core.h"
#include "art_event_moments.h"
#include "art_event_replicates.h"
#include "art_event_reweight.h"

namespace art {

constexpr int GRID_MAX_COUPLINGS = 32, GRID_MAX_MODELS = 32;
constexpr int GRID_EVENTS_PER_WAVE = 32;  // the events of one wave's slice
// art_event_grid_out::totals, per cell
enum { GRID_TOT_SUM_AXION = 0, GRID_TOT_SUM_PHOTON, GRID_TOT_MISPLACED, GRID_TOT_COUNT };

// the power of a final record at one cell: the coupling scan's power, then the halo ratio
__host__ __device__ inline double grid_power(double W, double B, double R, int cyclotron, double tau, double sln) {
#pragma clang fp contract(off)
  const double pw_g = reweight_power(W, B, cyclotron, tau, sln);
  return pw_g * R;
}

// where the tables keep a cell's entries (header comment); C: the cells
__host__ __device__ inline int64_t grid_flux_at(int64_t C, int nbins, int sp, int fb, int64_t cell) {
  return ((int64_t)sp * nbins + fb) * C + cell;
}
__host__ __device__ inline int64_t grid_flux_rep_at(int64_t C, int nbins, int g, int sp, int fb, int64_t cell) {
  return (((int64_t)g * 2 + sp) * nbins + fb) * C + cell;
}
__host__ __device__ inline int64_t grid_totals_rep_at(int64_t C, int g, int sp, int64_t cell) {
  return ((int64_t)g * 2 + sp) * C + cell;
}

// What one cell keeps while its records go by: the open event's X of the two species, and the sums over the events
// closed so far -- Σ X (the totals), Σ X² and Σ X a_e. On the device these are one lane's registers.
struct GridCell {
  double xa, xp;          // X_{e,axion}, X_{e,photon} of the open event
  double sa, sp, qa, qp, ca, cp;
};

// a final record of the open event: its power into the event's X, in node order
__host__ __device__ inline void grid_cell_record(GridCell& c, int species, double pw) {
  if (species) c.xp += pw;
  else c.xa += pw;
}

// the open event ends: with a_e its part of f_inx, X, X² and X a_e go to the sums, each product rounded on its own
__host__ __device__ inline void grid_cell_event(GridCell& c, double ae) {
#pragma clang fp contract(off)
  c.sa += c.xa;
  c.sp += c.xp;
  c.qa += c.xa * c.xa;
  c.qp += c.xp * c.xp;
  c.ca += c.xa * ae;
  c.cp += c.xp * ae;
  c.xa = c.xp = 0.0;
}

}  // namespace art

#ifdef ART_EVENT_KERNELS
namespace art {

// The lanes of a wave cover 64 consecutive CELLS (blockIdx.y picks which 64), not records: a wave takes slices of
// GRID_EVENTS_PER_WAVE events (grid-stride over the slices) and walks their trees in node order. The records of a
// tree are prepared 64 at a time, one lane per record (event_record: no sky bin; final only when it names e), and then
// the final ones are taken one at a time: bins and base factors are broadcast and wave-uniform, every lane forms
// its own cell's power and the wave adds it to 512 contiguous bytes of the flux table (and of the group's). The
// sums that take every record of the chunk -- the totals and the moment sums, 6 per cell -- stay in the lane's
// registers (GridCell) and are added to HBM once per wave, when its slices are done; the per-group totals go to HBM
// once per event and species. The per-group counts are kept by lane g for group g (n_groups <= 64 = the wave) and by
// the waves of the first 64 cells only. No LDS, no scratch memory, no host read.
__global__ __launch_bounds__(256) void event_grid_kernel(const EventRowsArgs a, const EventGridArgs r) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (warpSize - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / warpSize));
  const int waves = blockDim.x / warpSize;
  const int64_t C = (int64_t)r.n_g * r.n_h;
  const int64_t cell = (int64_t)blockIdx.y * warpSize + lane;
  const bool live = cell < C;
  const int kg = live ? (int)(cell / r.n_h) : 0, kh = live ? (int)(cell % r.n_h) : 0;
  const bool first = blockIdx.y == 0;  // these waves also count the events, the groups and the misplaced records
  const int R = r.n_groups;
  const int cyclotron = a.cyc_slot != nullptr;
  GridCell c{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double ev_n = 0.0, ev_a1 = 0.0, ev_a2 = 0.0, bad = 0.0;  // (wave-uniform)
  double grp_n = 0.0, grp_a = 0.0;                         // lane g: group g
  const int64_t n_slices = (a.n_events + GRID_EVENTS_PER_WAVE - 1) / GRID_EVENTS_PER_WAVE;
  for (int64_t sl = (int64_t)blockIdx.x * waves + wave; sl < n_slices; sl += (int64_t)gridDim.x * waves) {
    const int64_t e0 = sl * GRID_EVENTS_PER_WAVE;
    const int64_t e1 = e0 + GRID_EVENTS_PER_WAVE < a.n_events ? e0 + GRID_EVENTS_PER_WAVE : a.n_events;
    for (int64_t e = e0; e < e1; ++e) {
      int64_t s0;
      const int64_t s1 = tree_range(r.node_start, a.n_nodes, e, &s0) + s0;
      const int g = R > 0 ? replicate_group(a.event_offset + e, R) : 0;
      const double Bk = live ? r.B[(int64_t)kg * a.n_events + e] : 0.0;
      const double Rk = live ? r.R[(int64_t)kh * a.n_events + e] : 0.0;
      int photons = 0;
      bool any_axion = false, any_photon = false;
      for (int64_t base = s0; base < s1; base += warpSize) {
        const int64_t i = base + lane;
        const EventRecord rec = i < s1 ? event_record(a, r.node_start, i, r.nbins, false, SkyAxes{}, 0) : EventRecord{};
        const bool mis = rec.state == RECORD_MISPLACED, fin = rec.state == RECORD_FINAL && rec.e == e;
        const int sp = rec.species, fb = rec.fb;
        const double tau = rec.tau, sln = rec.sln;
        if (mis && first && R > 0)
          unsafeAtomicAdd(&r.groups[replicate_group(a.event_offset + rec.e, R) * REP_GRP_COUNT + REP_GRP_MISPLACED], 1.0);
        bad += (double)__popcll(__ballot(mis));
        unsigned long long todo = __ballot(fin);
        while (todo) {  // the final records of these 64, in node order
          const int j = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int spj = __shfl(sp, j), fbj = __shfl(fb, j);
          const double tauj = __shfl(tau, j), slnj = __shfl(sln, j);
          photons += spj;
          if (spj) any_photon = true;
          else any_axion = true;
          if (live) {
            const double pw = grid_power(r.W[(int64_t)kg * a.n_nodes + base + j], Bk, Rk, cyclotron, tauj, slnj);
            grid_cell_record(c, spj, pw);
            if (fbj >= 0) {
              unsafeAtomicAdd(&r.flux[grid_flux_at(C, r.nbins, spj, fbj, cell)], pw);
              if (R > 0) unsafeAtomicAdd(&r.flux_rep[grid_flux_rep_at(C, r.nbins, g, spj, fbj, cell)], pw);
            }
          }
        }
      }
      const double ae = (double)(event_attempts_m1(a, e) + photons);
      if (live) {
        if (R > 0 && any_axion) unsafeAtomicAdd(&r.totals_rep[grid_totals_rep_at(C, g, 0, cell)], c.xa);
        if (R > 0 && any_photon) unsafeAtomicAdd(&r.totals_rep[grid_totals_rep_at(C, g, 1, cell)], c.xp);
        grid_cell_event(c, ae);
      }
      ev_n += 1.0;
      ev_a1 += ae;
      ev_a2 += ae * ae;
      if (lane == g) {
        grp_n += 1.0;
        grp_a += ae;
      }
    }
  }
  if (live) {
    if (c.sa != 0.0) unsafeAtomicAdd(&r.totals[GRID_TOT_SUM_AXION * C + cell], c.sa);
    if (c.sp != 0.0) unsafeAtomicAdd(&r.totals[GRID_TOT_SUM_PHOTON * C + cell], c.sp);
    if (r.mtotals && ev_n != 0.0) {
      unsafeAtomicAdd(&r.mtotals[EM_TOT_EVENTS * C + cell], ev_n);
      unsafeAtomicAdd(&r.mtotals[EM_TOT_A1 * C + cell], ev_a1);
      unsafeAtomicAdd(&r.mtotals[EM_TOT_A2 * C + cell], ev_a2);
      unsafeAtomicAdd(&r.mtotals[EM_TOT_Q_AXION * C + cell], c.qa);
      unsafeAtomicAdd(&r.mtotals[EM_TOT_Q_PHOTON * C + cell], c.qp);
      unsafeAtomicAdd(&r.mtotals[EM_TOT_C_AXION * C + cell], c.ca);
      unsafeAtomicAdd(&r.mtotals[EM_TOT_C_PHOTON * C + cell], c.cp);
    }
  }
  if (first && lane == 0 && bad != 0.0) {  // (cell 0)
    unsafeAtomicAdd(&r.totals[GRID_TOT_MISPLACED * C], bad);
    if (r.mtotals) unsafeAtomicAdd(&r.mtotals[EM_TOT_BAD * C], bad);
  }
  if (first && lane < R && grp_n != 0.0) {
    unsafeAtomicAdd(&r.groups[lane * REP_GRP_COUNT + REP_GRP_EVENTS], grp_n);
    if (grp_a != 0.0) unsafeAtomicAdd(&r.groups[lane * REP_GRP_COUNT + REP_GRP_A], grp_a);
  }
}

hipError_t launch_event_grid(const EventRowsArgs& a, const EventGridArgs& r, hipStream_t s) {
  if (a.n_events <= 0) return hipSuccess;
  const int64_t C = (int64_t)r.n_g * r.n_h;
  const int64_t n_slices = (a.n_events + GRID_EVENTS_PER_WAVE - 1) / GRID_EVENTS_PER_WAVE;
  const int64_t blocks = (n_slices + 3) / 4;  // 4 waves, each with a slice of its own
  hipLaunchKernelGGL(event_grid_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)((C + 63) / 64)),
                     dim3(256), 0, s, a, r);
  return hipGetLastError();
}

}  // namespace art
#endif  // ART_EVENT_KERNELS
