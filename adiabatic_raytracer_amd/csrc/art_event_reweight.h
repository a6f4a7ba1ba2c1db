// art_event_reweight.h -- the coupling scan (art_event_reweight_device): one forward forest grown at
// the base coupling g0 reweighted to a list of couplings g_k. No ray depends on g; g enters only as
// the factor (g 1e-9 |B|)² at the end of prob_eval, so P_nonAD(g_k) = s_k P_nonAD(g0) with
// s_k = (g_k / g0)² exactly, and from there the tree weights through P = 1 - exp(-P_nonAD).
//
// One tree's records t[0, c) lie in the order the tree processed them (record j was its j-th pop).
//   parent   of record j > 0: the one earlier record with n_cross > 0 whose (tc, xc) equal j's
//            (t0, x0) bit for bit (tree_push copies them). A child of the other species is the
//            converted branch, one of the same species the unconverted branch. No such record, or
//            more than one: the record is `unlinked`, its weights are 0.
//   exponent x0 = P_nonAD(g0) at the parent's stored first crossing (prob_nonad_single of xc, kc and
//            erg |dwc|, the expression art_ray_io.h evaluates for the crossing buffer), once per
//            crossing record. f_k = 1 - fexp(-s_k x0) converted, fexp(-s_k x0) unconverted.
//            A record with n_cross > 1 took its pc from the GROUP of its segment's kept crossings
//            (tree_step's gp.eval: the reference's Nc > 1 indexing mixes the first three), which the
//            one stored crossing cannot reproduce; the grouped exponent is ∝ g² all the same, so there
//            x0 = -flog(1 - pc), exact in s, and pc == 1 (the exponent is lost) keeps its branch
//            probabilities 1 and 0 at every coupling and is counted (`*grouped_lost`). The device
//            driver and the host forest store one crossing per forward segment (TreeRules::cap = 1), so
//            their forward records have n_cross <= 1; the rule serves forests from elsewhere.
//   weights  W_k(root) = 1. A child pushed while the tree split fully (the parent was pop number
//            <= mc_nodes) gets f_k W_k(parent), tree_step's product. A child drawn in the Monte-Carlo
//            regime gets W_k(parent) (f_k / f_0), the likelihood ratio of the branch that was drawn
//            (f_0: the factor at s = 1), which keeps the estimator unbiased and is exactly 1 at s = 1.
//   back     of event e: bprob_k = 1 - fexp(-s_k x_root) with x_root the backtrace root's P_nonAD
//            (tree_root_prob's exponent), and bweight_k = bweight^s_k = fexp(s_k flog(bweight)) from
//            the stored product of exp(-P_nonAD) over the backtrace's crossings; 0 stays 0 (its
//            exponents were lost to underflow at g0: `saturated`), 1 stays 1, and s_k = 1 takes the
//            stored value itself. A backtrace with ONE crossing stores it (xc, kc, dwc), so its
//            exponent x_c is recomputed like a forward one and bweight_k = fexp(-s_k x_c): the stored
//            factor 1 - P carries an absolute error of u/2, which is large beside a small bweight.
// Written once as __host__ __device__ functions: the kernels below and a host build for the CPU
// tests (tools/eventreweight.cpp, x0 through an accessor) compile the same source. The kernels take
// their records through art_event_record.h and their moments through art_event_moments.h's pass A and
// entries, and are compiled only in art_kernels.hip (ART_EVENT_KERNELS).
#pragma once
#include "art_core.h"
#include "art_event_moments.h"

namespace art {

constexpr int REWEIGHT_MAX_COUPLINGS = 32;
constexpr double REWEIGHT_LOST = 1.7976931348623157e308;  // the exponent of a grouped crossing whose pc is 1.0
// art_event_reweight_out::totals, per coupling
enum { RW_TOT_SUM_AXION = 0, RW_TOT_SUM_PHOTON, RW_TOT_COVERAGE, RW_TOT_SATURATED, RW_TOT_UNLINKED, RW_TOT_DIFFERS,
       RW_TOT_COUNT };

__host__ __device__ inline bool reweight_same_bits(double a, double b) {
  union {
    double d;
    unsigned long long u;
  } ua{a}, ub{b};
  return ua.u == ub.u;
}

// The parent of record j of the tree t, or -1 for the root, an orphan and a record with two candidates
__host__ __device__ inline int64_t reweight_parent(const art_tree_node* t, int64_t j) {
  const art_tree_node& c = t[j];
  int64_t parent = -1;
  int found = 0;
  for (int64_t i = 0; i < j; ++i) {
    const art_tree_node& p = t[i];
    if (p.n_cross > 0 && reweight_same_bits(p.tc, c.t0) && reweight_same_bits(p.xc[0], c.x0[0]) &&
        reweight_same_bits(p.xc[1], c.x0[1]) && reweight_same_bits(p.xc[2], c.x0[2])) {
      parent = i;
      found += 1;
    }
  }
  return found == 1 ? parent : -1;
}

// the branch probability at scale s of a crossing whose exponent at the base coupling is x0
__host__ __device__ inline double reweight_factor(bool converted, double s, double x0) {
#pragma clang fp contract(off)
  const double e = x0 == REWEIGHT_LOST ? 0.0 : fexp(-(s * x0));  // (a lost exponent: the crossing always converts)
  return converted ? 1.0 - e : e;
}

// does a record add its weight to its tree's tot_prob (tree_step: no crossing, or the rare fail)?
__host__ __device__ inline bool reweight_in_coverage(const art_tree_node& nd) { return nd.n_cross == 0; }

// The weights of one tree at nk scales: W[k stride + j] for record j. x0of(nd, j): the exponent of
// crossing record j with n_cross == 1, asked once per record and kept in x0[j] (c doubles); a record
// with n_cross > 1 takes -flog(1 - pc). *unlinked, *differs and *grouped_lost take the records without
// exactly one parent, the single-crossing records whose 1 - fexp(-x0) is not the stored pc bit for
// bit, and the grouped records whose pc is 1.0.
template <class X0>
__host__ __device__ inline void reweight_tree(const art_tree_node* t, int64_t c, int32_t mc_nodes, int nk, const double* s,
                                              X0& x0of, double* x0, double* W, int64_t stride, double* unlinked,
                                              double* differs, double* grouped_lost) {
#pragma clang fp contract(off)
  for (int64_t j = 0; j < c; ++j) {
    const art_tree_node& nd = t[j];
    double xj = 0.0;
    if (nd.n_cross == 1) {
      xj = x0of(nd, j);
      if (!reweight_same_bits(reweight_factor(true, 1.0, xj), nd.pc)) *differs += 1.0;
    } else if (nd.n_cross > 1) {
      if (nd.pc < 1.0) {
        xj = -flog(1.0 - nd.pc);
      } else {
        xj = REWEIGHT_LOST;
        *grouped_lost += 1.0;
      }
    }
    x0[j] = xj;
    if (j == 0) {
      for (int k = 0; k < nk; ++k) W[k * stride] = 1.0;
      continue;
    }
    const int64_t p = reweight_parent(t, j);
    if (p < 0) {
      *unlinked += 1.0;
      for (int k = 0; k < nk; ++k) W[k * stride + j] = 0.0;
      continue;
    }
    const bool converted = nd.species != t[p].species;
    const bool mc = p + 1 > (int64_t)mc_nodes;  // the parent's pop number is p + 1 (tree_step: count > mc_nodes)
    const double xp = x0[p];
    const double f0 = reweight_factor(converted, 1.0, xp);
    for (int k = 0; k < nk; ++k) {
      const double f = reweight_factor(converted, s[k], xp);
      const double wp = W[k * stride + p];
      // (a branch of probability 0 at the base coupling cannot have been drawn: it carries nothing)
      W[k * stride + j] = mc ? wp * (f0 > 0.0 ? f / f0 : 0.0) : f * wp;
    }
  }
}

__host__ __device__ inline double reweight_back_prob(double s, double x_root) { return reweight_factor(true, s, x_root); }
// single: the backtrace has one crossing, whose exponent at the base coupling is x_single
__host__ __device__ inline double reweight_back_weight(double s, double bweight, bool single, double x_single) {
#pragma clang fp contract(off)
  if (bweight == 0.0 || bweight == 1.0 || s == 1.0) return bweight;
  if (single) return fexp(-(s * x_single));
  return fexp(s * flog(bweight));
}
// column 8 * column 7 of a final row at another coupling: event_row's products in its order, with
// W_k in the place of node.weight and B_k = bprob_k bweight_k in that of back.prob back.weight
__host__ __device__ inline double reweight_power(double W, double B, int cyclotron, double tau, double sln) {
#pragma clang fp contract(off)
  const double w_tree = W * B;
  const double w = cyclotron ? w_tree * fexp(-tau) : w_tree;
  return w * sln;
}

}  // namespace art

#ifdef ART_EVENT_KERNELS
namespace art {

struct ReweightPhysics {
  const KParams& P;
  const double erg;
  __device__ double operator()(const art_tree_node& nd, int64_t) const {
    return prob_nonad_single(P, nd.xc, nd.kc, erg * fabs(nd.dwc));
  }
};

// One lane per tree: the weights of its records at every coupling (reweight_tree), its event's back
// factors, and the counters, summed per lane, then per wave, and added once per wave.
__global__ __launch_bounds__(256) void event_reweight_kernel(const KParams P, const KParams Pb, const EventRowsArgs a,
                                                             const EventReweightArgs r) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double cnt[3] = {0.0, 0.0, 0.0};  // saturated (lost exponents: bweight 0, grouped pc 1), unlinked, differs
  if (e < a.n_events) {
    const double erg = r.erg[e];
    int64_t first;
    const int64_t c = tree_range(r.node_start, a.n_nodes, e, &first);
    if (c > 0) {
      ReweightPhysics x0of{P, erg};
      reweight_tree(a.nodes + first, c, r.mc_nodes, r.n_k, r.s, x0of, r.X0 + first, r.W + first, a.n_nodes, &cnt[1],
                    &cnt[2], &cnt[0]);
    }
    const int64_t n = a.n_events;
    const double x[3] = {a.x[e], a.x[n + e], a.x[2 * n + e]};
    const double k[3] = {-a.k_init[e], -a.k_init[n + e], -a.k_init[2 * n + e]};
    const double xr = prob_nonad_single(Pb, x, k, erg);  // tree_root_prob's exponent
    if (!reweight_same_bits(reweight_back_prob(1.0, xr), a.back[e].prob)) cnt[2] += 1.0;
    const art_tree_node& bn = a.back[e];
    const double bw = bn.weight;
    if (bw == 0.0) cnt[0] += 1.0;
    const bool single = bn.n_cross == 1 && bw != 0.0 && bw != 1.0;
    double xs = 0.0;
    if (single) {
      xs = prob_nonad_single(Pb, bn.xc, bn.kc, erg * fabs(bn.dwc));
      if (!reweight_same_bits(reweight_factor(true, 1.0, xs), bn.pc)) cnt[2] += 1.0;
    }
    for (int q = 0; q < r.n_k; ++q) {
      const double bp = reweight_back_prob(r.s[q], xr);
      r.B[q * n + e] = bp * reweight_back_weight(r.s[q], bw, single, xs);
      if (r.Bp) r.Bp[q * n + e] = bp;
    }
  }
  for (int q = 0; q < 3; ++q) {
    double t = cnt[q];
    for (int off = warpSize / 2; off > 0; off >>= 1) t += __shfl_down(t, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && t != 0.0)
      for (int k = 0; k < r.n_k; ++k) unsafeAtomicAdd(&r.totals[k * RW_TOT_COUNT + RW_TOT_SATURATED + q], t);
  }
}

// One lane per node record. A final record of its own tree's range takes its bins and its event's
// values once (event_record, art_event_record.h); then per coupling its power goes to flux[k], sky[k]
// and the totals, and every record of its own range that added to tot_prob, final or not, adds W_k to
// the coverage. Misplaced records are not counted here (the moments' pass A counts them).
__global__ __launch_bounds__(256) void event_reweight_bins_kernel(const EventRowsArgs a, const EventReweightArgs r,
                                                                  const SkyAxes A, const int cos_axis) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const EventRecord rec = event_record(a, r.node_start, i, r.nbins, r.sky != nullptr, A, cos_axis);
  const bool fin = rec.state == RECORD_FINAL, cov = rec.state >= RECORD_OWN && reweight_in_coverage(a.nodes[i]);
  const int sp = rec.species, fb = rec.fb, sb = rec.sb;
  const double tau = rec.tau, sln = rec.sln;
  const int64_t e = rec.e;
  for (int k = 0; k < r.n_k; ++k) {
    double tot[3] = {0.0, 0.0, 0.0};  // Σ power of axions, of photons, coverage
    double pw = 0.0;
    if (cov || fin) {
      const double W = r.W[k * a.n_nodes + i];
      if (cov) tot[2] = W;
      if (fin) {
        pw = reweight_power(W, r.B[k * a.n_events + e], a.cyc_slot != nullptr, tau, sln);
        tot[sp] = pw;
        if (fb >= 0) unsafeAtomicAdd(&r.flux[(int64_t)k * 2 * r.nbins + sp * r.nbins + fb], pw);
        if (sb >= 0) unsafeAtomicAdd(&r.sky[k * r.sky_size + sb], pw);
      }
    }
    if (r.Pw && i < a.n_nodes) r.Pw[k * a.n_nodes + i] = pw;
    for (int q = 0; q < 3; ++q) wave_add(&r.totals[k * RW_TOT_COUNT + q], tot[q]);
  }
}

// The second moments per coupling, one lane per node record and per event: event_moments_kernel's
// group-by over the entries of pass A, event_entries_kernel (bins and a_e are those of the g0 forest
// for every k), with the powers of coupling k (Pw) in the place of the entries' own
// (moment_scan_tables, art_event_moments.h).
__global__ __launch_bounds__(256) void event_reweight_moments_kernel(const EventRowsArgs a, const EventMomentsArgs m,
                                                                     const EventReweightArgs r) {
  moment_scan_tables(a, m, r);
}

hipError_t launch_event_reweight(const KParams& P, const KParams& Pb, const EventRowsArgs& a, const EventReweightArgs& r,
                                 const SkyAxes& A, int cos_axis, hipStream_t s) {
  if (a.n_events <= 0) return hipSuccess;
  hipLaunchKernelGGL(event_reweight_kernel, dim3((unsigned)((a.n_events + 255) / 256)), dim3(256), 0, s, P, Pb, a, r);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.n_nodes > 0) {
    hipLaunchKernelGGL(event_reweight_bins_kernel, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a, r, A,
                       cos_axis);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (!r.mtotals) return hipSuccess;
  return launch_scan_moments(event_reweight_moments_kernel, a, r, A, cos_axis, s);
}

}  // namespace art
#endif  // ART_EVENT_KERNELS
