// art_event_rows.h -- one npy row of main_runner_tree (MainRunner.jl:690-747; trees.py's `cols`)
// from ONE final node of the forward forest and its event's data, written once as
// __host__ __device__ functions: event_rows_kernel (art_kernels.hip, one lane per node) and a host
// build for the CPU tests (tools/eventrows.cpp) compile the same source.
//
// Arithmetic is rounded as numpy rounds trees.py's expressions: no contraction into FMAs, the norm
// as np.linalg.norm sums it, sqrt((x² + y²) + z²); θ = acos(z / norm), φ = atan2(y, x); products
// in the order trees.py writes them. The row, 0-based (ncols 13, or 29 with saveMode > 0):
//    0 event_offset + node.tree + 1     1 0 axion, 1 photon        2, 3 θf, φf of k_end
//    4, 5, 6 θ, φ, |.| of x_end         7 sln_prob (raw: the division by f_inx comes later)
//    8 node.weight (back.prob back.weight) [exp(-τ)]               9-11 the sampled x
//   12 u7_end / mass_a + vel_eng       13 col 8 before exp(-τ)    14 τ    15 1.0
//   16-18 k_init   19 cos_w   20, 21 the forward tree's count, info   22-24 prob, prob_conv,
//   prob_conv0     25 back.prob back.weight   26 col 6   27 the backtrace tree's count   28 back.prob
#pragma once
#include "art_core.h"

namespace art {

constexpr int EVENT_COLS_SHORT = 13, EVENT_COLS_FULL = 29;
// art_event_rows_out::totals
enum { EV_TOT_ROWS = 0, EV_TOT_PHOTONS, EV_TOT_SUM_AXION, EV_TOT_SUM_PHOTON, EV_TOT_ATTEMPTS, EV_TOT_MISMATCH, EV_TOT_COUNT };

// What a row takes from its event (one sampled conversion point: sampler, event weight, backtrace
// tree and the forward tree's count and info). event_row reads its event through accessors of this
// shape, each value where its column is written: the kernel's source loads from HBM there (a row
// held whole in registers spilled), the host tool's is this struct.
struct EventOfRow {
  double xs[3], ks[3];
  double sln, vel, cosw;
  double bprob, bweight;
  double bcount, fcount, finfo;
  __host__ __device__ double x(int c) const { return xs[c]; }
  __host__ __device__ double k(int c) const { return ks[c]; }
  __host__ __device__ double sln_prob() const { return sln; }
  __host__ __device__ double vel_eng() const { return vel; }
  __host__ __device__ double cos_w() const { return cosw; }
  __host__ __device__ double back_prob() const { return bprob; }
  __host__ __device__ double back_weight() const { return bweight; }
  __host__ __device__ double back_count() const { return bcount; }
  __host__ __device__ double count() const { return fcount; }
  __host__ __device__ double info() const { return finfo; }
};

// What the flux table, the sky map and the totals take from a row: exactly the values written
// into it (columns 1, 2, 3, 12 and column 8 * column 7), and cos θf = kz / |k| from column 2's norm.
struct EventRowBins {
  int species;
  double theta, cos_theta, phi, dw, power;
};

// trees._angles: (θ, φ, |v|) of a Cartesian vector
__host__ __device__ inline void event_angles(const double* v, double& theta, double& phi, double& norm) {
#pragma clang fp contract(off)
  const double xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
  const double s = xx + yy;
  norm = sqrt(s + zz);
  theta = acos(v[2] / norm);
  phi = atan2(v[1], v[0]);
}

// The row of final node `nd` of event E (event_offset: the global id of the chunk's event 0).
// tau: the cyclotron optical depth of its last segment (cyclotron != 0; 0 for axions), which
// multiplies column 8 by exp(-tau). Writes ncols values to row unless it is null (binning only).
template <class Ev>
__host__ __device__ inline EventRowBins event_row(const art_tree_node& nd, const Ev& E, int64_t event_offset, double mass_a,
                                                  double tau, int cyclotron, int ncols, double* row) {
#pragma clang fp contract(off)
  EventRowBins b;
  double absf, thx, phx, absx;
  event_angles(nd.k_end, b.theta, b.phi, absf);
  b.cos_theta = nd.k_end[2] / absf;
  b.species = nd.species == ART_AXION ? 0 : 1;
  const double bp = E.back_prob();
  const double back = bp * E.back_weight();  // samp_back_weight (:635)
  const double w_tree = nd.weight * back;    // tree[ii].weight *= samp_back_weight (:690)
  const double w = cyclotron ? w_tree * fexp(-tau) : w_tree;
  const double sln = E.sln_prob();
  b.dw = nd.u7_end / mass_a + E.vel_eng();  // (:713)
  b.power = w * sln;
  if (!row) return b;
  row[0] = (double)(event_offset + (int64_t)nd.tree) + 1.0;
  row[1] = (double)b.species;
  row[2] = b.theta;
  row[3] = b.phi;
  event_angles(nd.x_end, thx, phx, absx);
  row[4] = thx;
  row[5] = phx;
  row[6] = absx;
  row[7] = sln;
  row[8] = w;
  row[9] = E.x(0);
  row[10] = E.x(1);
  row[11] = E.x(2);
  row[12] = b.dw;
  if (ncols > EVENT_COLS_SHORT) {
    row[13] = w_tree;
    row[14] = cyclotron ? 0.0 + tau : 0.0;
    row[15] = 1.0;
    row[16] = E.k(0);
    row[17] = E.k(1);
    row[18] = E.k(2);
    row[19] = E.cos_w();
    row[20] = E.count();
    row[21] = E.info();
    row[22] = nd.prob;
    row[23] = nd.prob_conv;
    row[24] = nd.prob_conv0;
    row[25] = back;
    row[26] = absx;
    row[27] = E.back_count();
    row[28] = bp;
  }
  return b;
}

// Two doubles with the same bits, or both NaN (np.array_equal(equal_nan=True) on a re-run that
// must reproduce its node)
__host__ __device__ inline bool event_same(double a, double b) {
  union {
    double d;
    unsigned long long u;
  } ua{a}, ub{b};
  return ua.u == ub.u || (a != a && b != b);
}

}  // namespace art
