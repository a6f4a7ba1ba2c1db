// TEST TOOL ONLY: host build of the product's row math (art_event_rows.h), so the CPU tests can hold
// the columns of one npy row against the numpy expressions of trees.main_runner_tree without a GPU.
// Never loaded by the product (adiabatic_raytracer_amd).
#include <cmath>

#include "../adiabatic_raytracer_amd/csrc/art_event_rows.h"

using namespace art;

extern "C" {

// Rows of n final nodes, node q of event nodes[q].tree < n_events. Per event, row-major:
// ev[e][14] = x (3), k_init (3), sln_prob, vel_eng, cos_w, back.prob, back.weight, the backtrace
// count, the forward count and info. tau: n, or NULL for no cyclotron. rows: n * ncols; cos_t: n, the
// returned kz / |k|. Returns 0, or -1 for a node outside the events.
int er_rows(int64_t n, const art_tree_node* nodes, int64_t n_events, const double* ev, int64_t event_offset,
            double mass_a, const double* tau, int32_t ncols, double* rows, double* cos_t) {
  for (int64_t q = 0; q < n; ++q) {
    const int64_t e = nodes[q].tree;
    if (e < 0 || e >= n_events) return -1;
    const double* v = ev + 14 * e;
    EventOfRow E;
    for (int c = 0; c < 3; ++c) {
      E.xs[c] = v[c];
      E.ks[c] = v[3 + c];
    }
    E.sln = v[6];
    E.vel = v[7];
    E.cosw = v[8];
    E.bprob = v[9];
    E.bweight = v[10];
    E.bcount = v[11];
    E.fcount = v[12];
    E.finfo = v[13];
    double* row = rows + q * ncols;
    const EventRowBins B = event_row(nodes[q], E, event_offset, mass_a, tau ? tau[q] : 0.0, tau != nullptr, ncols, row);
    // what the kernel bins is what the row holds
    if (!event_same(B.theta, row[2]) || !event_same(B.phi, row[3]) || (double)B.species != row[1] ||
        !event_same(B.dw, row[12]) || !event_same(B.power, row[8] * row[7]))
      return -2;
    cos_t[q] = B.cos_theta;
  }
  return 0;
}

// event_same on pairs: out[i] = 1 when a[i] and b[i] have the same bits or are both NaN
void er_same(int64_t n, const double* a, const double* b, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = event_same(a[i], b[i]) ? 1 : 0;
}

}  // extern "C"
