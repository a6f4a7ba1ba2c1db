// art_tree_step.h -- what get_tree (MainRunner.jl:199-350) does to ONE tree between two
// propagations, written once as __host__ __device__ functions: the device-resident tree driver
// (art_grow_trees_device: tree_step_kernel of art_kernels.hip, one lane per active tree) and a
// host build for the CPU tests (tools/treestep.cpp) compile the same source. art_forest.cpp, the
// host forest, restates the same rules over std::vector and is the comparator of the GPU tests.
//
// A tree's state in HBM: one TreeState, and its event stack, a fixed-capacity array of TreeEv
// (RT.node's fields that get_tree reads) kept in ascending weight, so the next pop -- the last
// element -- is the highest weight, a later push above an equal earlier one (sort!, :348, stable).
//
// The stack's capacity. A round pops one event and then pushes two children only while
// count <= mc_nodes (full splitting, :294-305), one at most afterwards (the Monte-Carlo branch,
// :281-292), none on a segment without a crossing or after the "rare fail" (:213-225). So the
// depth grows by at most one per round, and only in rounds with count <= mc_nodes, of which there
// are at most max(mc_nodes, 0); and no tree sees more than max_nodes + 1 rounds, because
// count > max_nodes stops it (:340-345). From the root's depth of 1:
//     depth <= min(max(mc_nodes, 0), max_nodes + 1) + 1            (tree_stack_capacity)
// The backtrace form (splittings_cutoff > 0, num_cutoff <= 0) processes its root only; its
// children would never be popped and are not stored: capacity 1. A push beyond the capacity is not
// dropped: it raises TreeState::overflow, which stops the tree and fails the host's call.
#pragma once
#include "art_core.h"

namespace art {

struct TreeEv {  // 128 bytes
  double x[3], k[3], t, dw;
  double prob, weight, parent_weight, prob_conv, prob_conv0;
  int32_t species, pad0;
  double pad1[2];
};

struct TreeState {
  double tot_prob, erg;
  int32_t count, count_main, info, active, depth, overflow;
};

// art_tree_opts as the step reads it
struct TreeRules {
  int32_t num_cutoff, mc_nodes, max_nodes, split_all;
  int32_t cap;        // crossings a segment stores: 1 for forward trees, max(1, crossing_cap) else
  int32_t stack_cap;  // tree_stack_capacity
  int64_t tree_offset;
  uint64_t seed;
  double prob_cutoff, rNS;
};

__host__ __device__ inline int64_t tree_stack_capacity(int32_t mc_nodes, int32_t max_nodes, bool split_all) {
  if (split_all) return 1;
  const int64_t a = mc_nodes > 0 ? mc_nodes : 0, b = (int64_t)max_nodes + 1;
  return (a < b ? a : b) + 1;
}

// One segment's crossings in an art_crossing_buf of a batch of m rays, ray j: component a of
// crossing q at [(a cap + q) m + j]. Only slots q < min(count, cap) are read: the *_device entry
// points leave the rest unwritten.
struct XcView {
  int32_t cap;
  int64_t m, j;
  const double *pos, *k, *t, *dw, *pn;
  __host__ __device__ double x(int a, int q) const { return pos[((int64_t)a * cap + q) * m + j]; }
  __host__ __device__ double kk(int a, int q) const { return k[((int64_t)a * cap + q) * m + j]; }
  __host__ __device__ double tc(int q) const { return t[(int64_t)q * m + j]; }
  __host__ __device__ double dwc(int q) const { return dw[(int64_t)q * m + j]; }
  __host__ __device__ double p_nonad(int q) const { return pn[(int64_t)q * m + j]; }
};

// The segment's end state and its crossing count (art_segment_out, art_crossing_buf::count)
struct SegEnd {
  double x_end[3], k_end[3], u7_end, tau_end;
  int32_t status, count;
};

// The draw of the Monte-Carlo branch: Philox4x32-10 keyed (seed, tree, count, "TREE"), the host
// forest's mc_uniform.
__host__ __device__ inline double tree_mc_uniform(uint64_t seed, uint64_t tree, uint32_t count) {
  uint32_t ctr[4] = {(uint32_t)tree, (uint32_t)(tree >> 32), count, 0x54524545u /* "TREE" */};
  philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
  return u01(ctr[0], ctr[1]);
}

// get_Prob_nonAD of one group of mk > 1 crossings (:265) with prob_kernel's arithmetic: the group
// values ksphere[1..3], Bsphere[1..3], x0_pl[1..2] by the reference's column-major linear index
// (q -> row q % mk, column q / mk), then prob_local / prob_eval per crossing with
// erg_eff = erg |Δωc|. rows: the buffer slots of the group's first min(mk, 3) crossings.
struct GroupProbPhysics {
  const KParams& P;
  ProbLin<double> G;
  __host__ __device__ void prepare(const XcView& X, const int rows[3], int mk, double erg) {
    double ks_lin[3], B_lin[3], x0pl_lin[2];
    for (int q = 0; q < 3; ++q) {
      const int row = rows[q % mk], col = q / mk;
      const double p3[3] = {X.x(0, row), X.x(1, row), X.x(2, row)};
      const double k3[3] = {X.kk(0, row), X.kk(1, row), X.kk(2, row)};
      const ProbLocal<double> Lq = prob_local(P, p3, k3, erg * fabs(X.dwc(row)));
      ks_lin[q] = Lq.ks[col];
      B_lin[q] = Lq.B[col];
      if (q < 2) {
        const double sph[3] = {Lq.r, Lq.th, Lq.ph};
        x0pl_lin[q] = sph[col];
      }
    }
    G.k1 = ks_lin[0]; G.k2 = ks_lin[1]; G.k3 = ks_lin[2];
    G.B1 = B_lin[0]; G.B2 = B_lin[1]; G.B3 = B_lin[2];
    G.r_c = x0pl_lin[0]; G.th_c = x0pl_lin[1];
  }
  // P_nonAD of the crossing in slot q, the pos-th of the group
  __host__ __device__ double eval(const XcView& X, int q, int /*pos*/, int /*mk*/, double erg) const {
    const double p3[3] = {X.x(0, q), X.x(1, q), X.x(2, q)};
    const double k3[3] = {X.kk(0, q), X.kk(1, q), X.kk(2, q)};
    const ProbLocal<double> L = prob_local(P, p3, k3, erg * fabs(X.dwc(q)));
    return prob_eval(P, P.g_agg, L, G);
  }
};

// the root's prob = 1 - exp(-P_nonAD) (:132-137), a group of one with erg_eff = erg |Δω| = erg
__host__ __device__ inline double tree_root_prob(const KParams& P, const double* x, const double* k, double erg) {
  const ProbLocal<double> L = prob_local(P, x, k, erg);
  ProbLin<double> G;
  G.k1 = L.ks[0]; G.k2 = L.ks[1]; G.k3 = L.ks[2];
  G.B1 = L.B[0]; G.B2 = L.B[1]; G.B3 = L.B[2];
  G.r_c = L.r; G.th_c = L.th;
  return 1.0 - fexp(-prob_eval(P, P.g_agg, L, G));
}

__host__ __device__ inline TreeEv tree_root(const double* x, const double* k, int species, double prob) {
  TreeEv r{};
  for (int a = 0; a < 3; ++a) {
    r.x[a] = x[a];
    r.k[a] = k[a];
  }
  r.t = 0.0;
  r.dw = -1.0;
  r.species = species == ART_AXION ? ART_AXION : ART_PHOTON;
  r.prob = prob;
  r.weight = 1.0;
  r.parent_weight = -1.0;
  r.prob_conv = -1.0;
  r.prob_conv0 = -1.0;
  return r;
}

// The start of a round: whether the tree takes part (active with an event left; a tree that
// ran out of events ends here, :158), and if so the popped event (left in place at
// stack[depth]: tree_step reads it there) with count advanced.
__host__ __device__ inline bool tree_pop(TreeState& T) {
  if (!T.active) return false;
  if (T.depth <= 0) {
    T.active = 0;
    return false;
  }
  T.count += 1;
  T.depth -= 1;
  return true;
}

// NumerPass[1] = log(max(event.t, dt0)) (:164). The root's (t = 0) is the host's double
// ln_dt0 = log(exp(-30)), handed in, so the first round's inputs equal the host forest's bit for bit.
__host__ __device__ inline double tree_ln_t0(double t, double dt0, double ln_dt0) { return t > dt0 ? flog(t) : ln_dt0; }

__host__ __device__ inline bool tree_push(const TreeRules& R, TreeState& T, TreeEv* stack, const XcView& X, int q,
                                          int species, double prob, double weight, double parent_weight,
                                          double prob_conv, double prob_conv0) {
  if (T.depth >= R.stack_cap) {
    T.overflow = 1;
    return false;
  }
  TreeEv c{};
  for (int a = 0; a < 3; ++a) {
    c.x[a] = X.x(a, q);
    c.k[a] = X.kk(a, q);
  }
  c.t = X.tc(q);
  c.dw = X.dwc(q);
  c.species = species;
  c.prob = prob;
  c.weight = weight;
  c.parent_weight = parent_weight;
  c.prob_conv = prob_conv;
  c.prob_conv0 = prob_conv0;
  stack[T.depth] = c;
  T.depth += 1;
  return true;
}

// Is crossing q of nc kept by the merge of neighbours closer than 1e-5 km (:227-245)? The last
// one always is; an earlier one when the next lies further than epsabs from it.
__host__ __device__ inline bool tree_keeps(const XcView& X, int q, int nc) {
  if (q + 1 >= nc) return true;
  const double d0 = fabs(X.x(0, q + 1) - X.x(0, q)), d1 = fabs(X.x(1, q + 1) - X.x(1, q)),
               d2 = fabs(X.x(2, q + 1) - X.x(2, q));
  const double s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2;
  return sqrt(s0 + s1 + s2) > 1e-5;
}

// The step: tree `tree` (index within the call), after tree_pop, takes its segment's results S
// and crossings X, and `node` receives the finished node (every field; pad holds the node's
// sequence number in its tree, count - 1). gp gives a group's probabilities (GroupProbPhysics; the
// CPU tests put a table in its place). Returns whether the tree goes on to another round.
// A "rare fail" node is recorded as the reference leaves it: without crossings (n_cross = 0).
template <class GroupProb>
__host__ __device__ inline bool tree_step(const TreeRules& R, int64_t tree, TreeState& T, TreeEv* stack, const SegEnd& S,
                                          const XcView& X, GroupProb& gp, art_tree_node& node) {
  TreeEv e = stack[T.depth];  // the popped event
  node.tree = (int32_t)tree;
  node.species = e.species;
  node.is_final = 0;
  node.n_cross = 0;
  node.status = S.status;
  node.pad = T.count - 1;
  node.prob = e.prob;
  node.parent_weight = e.parent_weight;
  node.prob_conv = e.prob_conv;
  node.prob_conv0 = e.prob_conv0;
  for (int a = 0; a < 3; ++a) {
    node.x0[a] = e.x[a];
    node.k0[a] = e.k[a];
    node.x_end[a] = S.x_end[a];
    node.k_end[a] = S.k_end[a];
    node.xc[a] = 0.0;
    node.kc[a] = 0.0;
  }
  node.t0 = e.t;
  node.dw0 = e.dw;
  node.u7_end = S.u7_end;
  node.tau_end = S.tau_end;
  node.tc = 0.0;
  node.dwc = 0.0;
  node.pc = 0.0;
  node.weight = e.weight;

  const int nc = S.count < X.cap ? S.count : X.cap;
  if (nc <= 0) {  // no crossings (:200-207)
    T.count_main += 1;
    T.tot_prob += e.weight;
    const double s0 = S.x_end[0] * S.x_end[0], s1 = S.x_end[1] * S.x_end[1], s2 = S.x_end[2] * S.x_end[2];
    if (sqrt(s0 + s1 + s2) > R.rNS * 1.1) node.is_final = 1;
  } else {
    bool rare = false;  // |kc| > 1 (:213-225), judged on the unmerged crossings
    for (int q = 0; q < nc; ++q)
      for (int a = 0; a < 3; ++a) rare = rare || fabs(X.kk(a, q)) > 1.0;
    if (rare) {
      T.tot_prob += e.weight;
      if (T.depth <= 0) T.active = 0;
      return T.active != 0;  // no stop checks, no sort (the reference's `continue`)
    }
    // the kept crossings: their number and the slots of the first three
    int mk = 0, rows[3] = {0, 0, 0};
    for (int q = 0; q < nc; ++q)
      if (tree_keeps(X, q, nc)) {
        if (mk < 3) rows[mk] = q;
        mk += 1;
      }
    const int q0 = rows[0];
    const bool grouped = mk > 1;  // one get_Prob_nonAD call with Nc > 1: the reference's indexing (:265)
    if (grouped) gp.prepare(X, rows, mk, T.erg);
    const double P1 = 1.0 - fexp(-(grouped ? gp.eval(X, q0, 0, mk, T.erg) : X.p_nonad(q0)));
    node.n_cross = mk;
    for (int a = 0; a < 3; ++a) {
      node.xc[a] = X.x(a, q0);
      node.kc[a] = X.kk(a, q0);
    }
    node.tc = X.tc(q0);
    node.dwc = X.dwc(q0);
    node.pc = P1;
    const int new_species = e.species == ART_PHOTON ? ART_AXION : ART_PHOTON;
    bool ok = true;
    if (!R.split_all) {
      if (T.count > R.mc_nodes) {  // pure MC (:281-292)
        const double r = tree_mc_uniform(R.seed, (uint64_t)(R.tree_offset + tree), (uint32_t)T.count);
        if (r < P1)
          ok = tree_push(R, T, stack, X, q0, new_species, P1, e.weight, e.weight, P1, P1);
        else
          ok = tree_push(R, T, stack, X, q0, e.species, 1.0 - P1, e.weight, e.weight, P1, e.prob_conv);
      } else {  // full tree (:294-305)
        ok = tree_push(R, T, stack, X, q0, new_species, P1, P1 * e.weight, e.weight, P1, P1) &&
             tree_push(R, T, stack, X, q0, e.species, 1.0 - P1, (1.0 - P1) * e.weight, e.weight, P1, e.prob_conv);
      }
    } else {  // follow one particle over all its crossings (:309-316); the children are never popped
      int pos = 0;
      for (int q = 0; q < nc; ++q) {
        if (!tree_keeps(X, q, nc)) continue;
        const double Pq = pos == 0 ? P1 : 1.0 - fexp(-gp.eval(X, q, pos, mk, T.erg));
        e.weight = e.weight * (1.0 - Pq);
        pos += 1;
      }
      T.tot_prob += e.weight;
      node.weight = e.weight;
    }
    if (!ok) {  // stack overflow: the tree stops and the host's call fails
      T.active = 0;
      return false;
    }
  }
  // stop rules (:325-345)
  if (T.tot_prob >= 1.0 - R.prob_cutoff) {
    T.info = 2;
    T.active = 0;
  } else if (R.num_cutoff <= 0 && R.split_all) {
    T.active = 0;
  } else if (T.count_main >= R.num_cutoff) {
    T.info = 3;
    T.active = 0;
  } else if (T.count > R.max_nodes) {
    T.info = 4;
    T.active = 0;
  } else {
    // sort!(events, by = weight) (:348), stable: insertion from the left keeps equal weights in
    // push order (the prefix is already sorted, so this moves the new children only)
    for (int i = 1; i < T.depth; ++i) {
      if (!(stack[i].weight < stack[i - 1].weight)) continue;
      const TreeEv key = stack[i];
      int j = i - 1;
      while (j >= 0 && key.weight < stack[j].weight) {
        stack[j + 1] = stack[j];
        j -= 1;
      }
      stack[j + 1] = key;
    }
    if (T.depth <= 0) T.active = 0;  // out of events (:158)
  }
  return T.active != 0;
}

// get_tree's `info` as it returns it: negative once the tree went Monte-Carlo (:350)
__host__ __device__ inline int32_t tree_info(const TreeState& T, int32_t mc_nodes) {
  const int32_t a = T.info < 0 ? -T.info : T.info;
  return T.count > mc_nodes ? -a : T.info;
}

}  // namespace art
