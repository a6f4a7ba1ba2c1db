// TEST TOOL ONLY: host build of the coupling x halo grid's per-record and per-event functions (art_event_grid.h:
// grid_power, grid_cell_record, grid_cell_event and the tables' index functions), so the CPU tests can hold them
// against trees.grid_tables without a GPU. Never loaded by the product (adiabatic_raytracer_amd).
#include "../adiabatic_raytracer_amd/csrc/art_event_grid.h"

using namespace art;

extern "C" {

// The tables of a forest of n_trees trees whose records lie in node order, walked as the kernel walks them, one cell
// after the other: tree e owns start[e] .. start[e + 1]. Per record: tree (the tree it names), fin (is it final),
// species (0 / 1), fb (its flux bin, -1 for none), tau; per tree: sln and a (attempts - 1). W (n_g, n_nodes), B
// (n_g, n_trees) and R (n_h, n_trees) are the scans' factors. Adds to the cell-minor tables of art_event_grid_out;
// flux_rep, totals_rep and groups are read with n_groups > 0, mtotals when non-null.
int eg_forest(int64_t n_trees, int64_t event_offset, const int64_t* start, const int64_t* tree, const int32_t* fin,
              const int32_t* species, const int32_t* fb, const double* tau, const double* sln, const int64_t* a,
              int32_t cyclotron, int32_t n_g, int32_t n_h, int32_t nbins, int32_t n_groups, const double* W,
              const double* B, const double* R, double* flux, double* totals, double* flux_rep, double* totals_rep,
              double* groups, double* mtotals) {
  const int64_t C = (int64_t)n_g * n_h, n_nodes = start[n_trees];
  for (int64_t cell = 0; cell < C; ++cell) {
    const int kg = (int)(cell / n_h), kh = (int)(cell % n_h);
    GridCell c{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double ev_n = 0.0, ev_a1 = 0.0, ev_a2 = 0.0, bad = 0.0;
    for (int64_t e = 0; e < n_trees; ++e) {
      const int g = n_groups > 0 ? replicate_group(event_offset + e, n_groups) : 0;
      int photons = 0;
      bool any[2] = {false, false};
      for (int64_t i = start[e]; i < start[e + 1]; ++i) {
        const int64_t t = tree[i];
        if (!(t >= 0 && t < n_trees && start[t] <= i && i < start[t + 1])) {
          bad += 1.0;
          if (cell == 0 && n_groups > 0)
            groups[replicate_group(event_offset + t, n_groups) * REP_GRP_COUNT + REP_GRP_MISPLACED] += 1.0;
          continue;
        }
        if (t != e || !fin[i]) continue;
        const int sp = species[i];
        photons += sp;
        any[sp] = true;
        const double pw = grid_power(W[(int64_t)kg * n_nodes + i], B[(int64_t)kg * n_trees + e], R[(int64_t)kh * n_trees + e],
                                     cyclotron, tau[i], sln[e]);
        grid_cell_record(c, sp, pw);
        if (fb[i] >= 0) {
          if (fb[i] >= nbins) return -1;
          flux[grid_flux_at(C, nbins, sp, fb[i], cell)] += pw;
          if (n_groups > 0) flux_rep[grid_flux_rep_at(C, nbins, g, sp, fb[i], cell)] += pw;
        }
      }
      const double ae = (double)(a[e] + photons);
      if (n_groups > 0 && any[0]) totals_rep[grid_totals_rep_at(C, g, 0, cell)] += c.xa;
      if (n_groups > 0 && any[1]) totals_rep[grid_totals_rep_at(C, g, 1, cell)] += c.xp;
      grid_cell_event(c, ae);
      ev_n += 1.0;
      ev_a1 += ae;
      ev_a2 += ae * ae;
      if (cell == 0 && n_groups > 0) {
        groups[g * REP_GRP_COUNT + REP_GRP_EVENTS] += 1.0;
        groups[g * REP_GRP_COUNT + REP_GRP_A] += ae;
      }
    }
    totals[GRID_TOT_SUM_AXION * C + cell] += c.sa;
    totals[GRID_TOT_SUM_PHOTON * C + cell] += c.sp;
    if (cell == 0) totals[GRID_TOT_MISPLACED * C] += bad;
    if (mtotals) {
      const double m[EM_TOT_COUNT] = {ev_n, ev_a1, ev_a2, c.qa, c.qp, c.ca, c.cp, cell == 0 ? bad : 0.0};
      for (int q = 0; q < EM_TOT_COUNT; ++q) mtotals[q * C + cell] += m[q];
    }
  }
  return 0;
}

int eg_limits(int which) {
  const int v[] = {GRID_MAX_COUPLINGS, GRID_MAX_MODELS, GRID_TOT_COUNT, GRID_EVENTS_PER_WAVE};
  return which >= 0 && which < 4 ? v[which] : -1;
}

}  // extern "C"
