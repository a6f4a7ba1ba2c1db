// TEST TOOL ONLY: host build of the product's per-tree step (art_tree_step.h) with a driver loop of
// its own, so the CPU tests can hold get_tree's rules -- children, Monte-Carlo draw, stop rules, info
// codes, the stable order of the event stack and its bound -- against oracle/tree.py without a GPU.
// The integrator and the probabilities are not under test here: every segment's outcome comes from a
// table indexed by (tree, count), and a group's probabilities are a fixed function of that table.
// Never loaded by the product (adiabatic_raytracer_amd).
#include <cmath>
#include <vector>

#include "../adiabatic_raytracer_amd/csrc/art_tree_step.h"

using namespace art;

namespace {
// P_nonAD of a group's crossing: ((0.05 + 0.1 pos) + 0.01 mk) + 1e-3 |x|, each operation rounded on
// its own (tests/test_device_forest.py computes the same)
struct GroupProbTable {
  void prepare(const XcView&, const int*, int, double) {}
  double eval(const XcView& X, int q, int pos, int mk, double) const {
    const double a = 0.1 * pos;
    const double b = 0.01 * mk;
    const double c = 1e-3 * std::fabs(X.x(0, q));
    double s = 0.05 + a;
    s = s + b;
    s = s + c;
    return s;
  }
};
}  // namespace

extern "C" {

int64_t ts_stack_capacity(int32_t mc_nodes, int32_t max_nodes, int32_t split_all) {
  return tree_stack_capacity(mc_nodes, max_nodes, split_all != 0);
}

// Grows n trees one after the other. Tables, row-major: root_pn[tree]; ncross[tree][step] (step =
// count - 1 < steps), xc[tree][step][slot < xcap][9] = pos (3), k (3), t, Δω, P_nonAD;
// r_end[tree][step], the end radius. stack_cap <= 0: tree_stack_capacity. max_depth receives the
// deepest stack seen, overflow whether a push found it full. Returns 0, or -3 with *n_nodes when
// node_capacity is too small, or -1 when a tree outruns the table.
int ts_run(int64_t n, const art_tree_opts* o, double rNS, int32_t stack_cap, int32_t steps, int32_t xcap,
           const double* root_pn, const int32_t* ncross, const double* xc, const double* r_end, int64_t node_capacity,
           art_tree_node* nodes, int64_t* n_nodes, int32_t* counts, int32_t* infos, int32_t* max_depth,
           int32_t* overflow) {
  TreeRules R{};
  R.num_cutoff = o->num_cutoff;
  R.mc_nodes = o->mc_nodes;
  R.max_nodes = o->max_nodes;
  R.split_all = o->splittings_cutoff > 0;
  R.cap = R.split_all ? (o->crossing_cap > 1 ? o->crossing_cap : 1) : 1;
  R.stack_cap = stack_cap > 0 ? stack_cap : (int32_t)tree_stack_capacity(o->mc_nodes, o->max_nodes, R.split_all);
  R.tree_offset = o->tree_offset;
  R.seed = o->seed;
  R.prob_cutoff = o->prob_cutoff;
  R.rNS = rNS;
  *max_depth = 0;
  *overflow = 0;
  std::vector<art_tree_node> all;
  const double nan = std::nan("");
  for (int64_t i = 0; i < n; ++i) {
    TreeState T{};
    T.erg = 1e-5;
    T.info = 1;
    T.active = 1;
    T.depth = 1;
    std::vector<TreeEv> stack((size_t)R.stack_cap);
    const double x[3] = {20.0 + (double)i, 0.0, 0.0}, k[3] = {1e-5, 0.0, 0.0};
    stack[0] = tree_root(x, k, ART_PHOTON, 1.0 - fexp(-root_pn[i]));
    while (tree_pop(T)) {
      const int64_t e = i * steps + (T.count - 1);
      if (T.count > steps) return -1;
      // the segment's crossing buffer as a device launch leaves it: slots beyond the count unwritten
      std::vector<double> pos(3 * (size_t)R.cap, nan), kk(3 * (size_t)R.cap, nan), t(R.cap, nan), dw(R.cap, nan),
          pn(R.cap, nan);
      for (int q = 0; q < R.cap && q < ncross[e] && q < xcap; ++q) {
        const double* c = xc + (e * xcap + q) * 9;
        for (int a = 0; a < 3; ++a) {
          pos[(size_t)a * R.cap + q] = c[a];
          kk[(size_t)a * R.cap + q] = c[3 + a];
        }
        t[q] = c[6];
        dw[q] = c[7];
        pn[q] = c[8];
      }
      SegEnd S{};
      S.x_end[0] = r_end[e];
      S.k_end[2] = 1e-5;
      S.u7_end = -1e-5;
      S.tau_end = 0.0;
      S.status = ncross[e] > 0 ? ART_STATUS_CROSSING : ART_STATUS_SUCCESS;
      S.count = ncross[e];
      const XcView X{R.cap, 1, 0, pos.data(), kk.data(), t.data(), dw.data(), pn.data()};
      GroupProbTable gp;
      art_tree_node node;
      tree_step(R, i, T, stack.data(), S, X, gp, node);
      all.push_back(node);
      if (T.depth > *max_depth) *max_depth = T.depth;
      if (T.overflow) *overflow = 1;
    }
    if (counts) counts[i] = T.count;
    if (infos) infos[i] = tree_info(T, R.mc_nodes);
  }
  *n_nodes = (int64_t)all.size();
  if (*n_nodes > node_capacity) return -3;
  for (size_t q = 0; q < all.size(); ++q) nodes[q] = all[q];
  return 0;
}

}  // extern "C"
