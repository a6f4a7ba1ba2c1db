// TEST TOOL ONLY: host build of the product's coupling-scan reweight (art_event_reweight.h) and of the
// scaled group-by of the second moments (art_event_moments.h), so the CPU tests can hold them against
// trees.reweight_nodes without a GPU and without physics: each crossing record's exponent comes from a
// table. Never loaded by the product (adiabatic_raytracer_amd).
#include "../adiabatic_raytracer_amd/csrc/art_event_reweight.h"

using namespace art;

namespace {
struct X0Table {
  const double* x;  // the tree's records' exponents
  double operator()(const art_tree_node&, int64_t j) const { return x[j]; }
};
}  // namespace

extern "C" {

int rw_node_bytes() { return (int)sizeof(art_tree_node); }

// The weights of a forest of n_trees trees: tree e owns records start[e] .. start[e + 1] of nodes
// (n_nodes = start[n_trees]) and of x_nonad, each crossing record's P_nonAD at the base coupling.
// Writes W (nk n_nodes, W[k n_nodes + i]) and coverage (nk n_trees); counters (3) take the unlinked
// records, the single-crossing records whose recomputed probability is not the stored pc bit for bit,
// and the grouped records (n_cross > 1) whose pc is 1.0.
int rw_forest(int64_t n_trees, const int64_t* start, const art_tree_node* nodes, const double* x_nonad, int32_t mc_nodes,
              int32_t nk, const double* s, double* W, double* coverage, double* counters) {
  if (nk < 1 || nk > REWEIGHT_MAX_COUPLINGS) return -1;
  const int64_t n_nodes = start[n_trees];
  for (int64_t e = 0; e < n_trees; ++e) {
    const int64_t first = start[e], c = start[e + 1] - start[e];
    double* x0 = new double[c > 0 ? c : 1];
    X0Table x0of{x_nonad + first};
    reweight_tree(nodes + first, c, mc_nodes, nk, s, x0of, x0, W + first, n_nodes, &counters[0], &counters[1],
                  &counters[2]);
    delete[] x0;
    for (int k = 0; k < nk; ++k) {
      double cov = 0.0;
      for (int64_t j = 0; j < c; ++j)
        if (reweight_in_coverage(nodes[first + j])) cov += W[k * n_nodes + first + j];
      coverage[k * n_trees + e] = cov;
    }
  }
  return 0;
}

// B (nk n) of n events: reweight_back_prob reweight_back_weight, the kernel's product. x_single[e]: the
// exponent of the backtrace's crossing when it has exactly one, NaN otherwise
void rw_back(int64_t n, const double* x_root, const double* bweight, const double* x_single, int32_t nk, const double* s,
             double* B) {
  for (int k = 0; k < nk; ++k)
    for (int64_t e = 0; e < n; ++e)
      B[k * n + e] = reweight_back_prob(s[k], x_root[e]) *
                     reweight_back_weight(s[k], bweight[e], x_single[e] == x_single[e], x_single[e]);
}

double rw_power(double W, double B, int32_t cyclotron, double tau, double sln) { return reweight_power(W, B, cyclotron, tau, sln); }

// tools/eventmoments.cpp's em_forest at nk couplings: the groups of the entries (flux, sky: a
// MomentEntry's fields) with the powers pw[k n_nodes + i] in the place of the entries' own. The tables
// are nk times em_forest's (totals: nk 8). Returns 0, or -1 for a key outside its table.
int rw_tables(int64_t n_trees, const int64_t* start, const int32_t* flux, const int32_t* sky, const double* pw,
              const int64_t* a, int32_t nbins, int64_t sky_size, int32_t nk, double* flux_sq, double* flux_xa, double* sky_sq,
              double* sky_xa, double* totals) {
  const int64_t n_nodes = start[n_trees];
  for (int64_t e = 0; e < n_trees; ++e) {
    const int64_t first = start[e], c = start[e + 1] - start[e];
    MomentEntry* t = new MomentEntry[c > 0 ? c : 1];
    for (int64_t j = 0; j < c; ++j) t[j] = MomentEntry{flux[first + j], sky[first + j], 0.0};
    const double ae = (double)(a[e] + moment_photon_rows(t, c, nbins));
    for (int k = 0; k < nk; ++k) {
      double* tot = totals + k * EM_TOT_COUNT;
      tot[EM_TOT_EVENTS] += 1.0;
      tot[EM_TOT_A1] += ae;
      tot[EM_TOT_A2] += ae * ae;
      for (int64_t j = 0; j < c; ++j)
        for (int which = MOMENT_KEY_FLUX; which <= MOMENT_KEY_SPECIES; ++which) {
          double X;
          const int key = moment_group_scaled(t, pw + k * n_nodes + first, c, j, which, nbins, &X);
          if (key < 0) continue;
          if (key >= (which == MOMENT_KEY_FLUX ? 2 * (int64_t)nbins : which == MOMENT_KEY_SKY ? sky_size : 2)) {
            delete[] t;
            return -1;
          }
          if (which == MOMENT_KEY_FLUX) {
            flux_sq[k * 2 * (int64_t)nbins + key] += X * X;
            flux_xa[k * 2 * (int64_t)nbins + key] += X * ae;
          } else if (which == MOMENT_KEY_SKY) {
            sky_sq[k * sky_size + key] += X * X;
            sky_xa[k * sky_size + key] += X * ae;
          } else {
            tot[EM_TOT_Q_AXION + key] += X * X;
            tot[EM_TOT_C_AXION + key] += X * ae;
          }
        }
    }
    delete[] t;
  }
  return 0;
}

}  // extern "C"
