// capi_main.cpp -- TEST INFRASTRUCTURE ONLY: the host code of the C boundary
// (the host units of art_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, in a container
// without a GPU: the pure host entry points, every argument check, and the paths that
// reach the HIP runtime (which then reports that no device is present). The kernels'
// launch wrappers are replaced by stubs (launch_stubs.cpp). Prints "capi OK".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/art.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  art_params p{};
  p.theta_m = 0.2; p.omega_pul = 1.0; p.B0 = 1e14; p.rNS = 10.0; p.mass_ns = 1.0; p.mass_a = 1e-5;
  p.g_agg = 1e-12; p.bndry_lyr = -1.0; p.ln_t_end = 0.0; p.abstol = 1e-6; p.reltol = 1e-7; p.dtmin = 1e-13;
  p.maxiters = 100000; p.flat = 1; p.melrose = 1; p.integrator = ART_VERN6; p.n_fixed = 2000; p.interp_points = 50;
  CHECK(art_abi_version() == ART_ABI_VERSION);
  CHECK(art_last_error() != nullptr);
  const double mr = art_find_conversion_surface(&p);
  CHECK(mr > 25.0 && mr < 26.0);  // 25.167 km
  double c[9], A[81], b[9], bh[9];
  CHECK(art_vern6_tableau(c, A, b, bh) == ART_OK);
  double sb = 0.0;
  for (double v : b) sb += v;
  CHECK(std::fabs(sb - 1.0) < 1e-14);
  const int64_t n = 4;
  std::vector<double> x(3 * n, 20.0), k(3 * n, 1e-6), e(n, 1e-5), dw(n, -1.0), lt(n, -30.0), xe(3 * n), ke(3 * n),
      u7(n), tau(n);
  std::vector<int8_t> sp(n, ART_PHOTON);
  std::vector<int32_t> st(n), acc(n), rej(n);
  art_segment_out so{xe.data(), ke.data(), u7.data(), tau.data(), st.data(), acc.data(), rej.data()};
  CHECK(art_propagate_host(nullptr, n, x.data(), k.data(), e.data(), dw.data(), lt.data(), sp.data(), -1, &so,
                           nullptr) == ART_E_INVALID);
  art_params q = p;
  q.melrose = 0;
  CHECK(art_propagate_host(&q, n, x.data(), k.data(), e.data(), dw.data(), lt.data(), sp.data(), -1, &so, nullptr) ==
        ART_E_UNSUPPORTED);
  q = p; q.interp_points = 70;
  CHECK(art_propagate_host(&q, n, x.data(), k.data(), e.data(), dw.data(), lt.data(), sp.data(), -1, &so, nullptr) ==
        ART_E_INVALID);
  q = p; q.integrator = ART_RK4; q.n_fixed = 0;
  CHECK(art_propagate_host(&q, n, x.data(), k.data(), e.data(), dw.data(), lt.data(), sp.data(), -1, &so, nullptr) ==
        ART_E_INVALID);
  q = p; q.abstol = 0.0;
  CHECK(art_propagate_host(&q, n, x.data(), k.data(), e.data(), dw.data(), lt.data(), sp.data(), -1, &so, nullptr) ==
        ART_E_INVALID);
  CHECK(std::strlen(art_last_error()) > 0);
  CHECK(art_propagate_host(&p, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, -1, &so, nullptr) == ART_OK);
  CHECK(art_propagate_device(&p, n, x.data(), k.data(), e.data(), dw.data(), lt.data(), sp.data(), -1, nullptr,
                             nullptr, nullptr) == ART_E_INVALID);
  // reaches the HIP runtime: no device in this container
  int rc = art_propagate_host(&p, n, x.data(), k.data(), e.data(), dw.data(), lt.data(), sp.data(), -1, &so, nullptr);
  CHECK(rc == ART_E_HIP || rc == ART_E_NOMEM || rc == ART_OK);
  // get_Prob_nonAD groups must tile [0, nc)
  std::vector<double> out(n);
  int64_t bad[3] = {0, 3, 2};
  CHECK(art_get_prob_nonad_host(&p, n, x.data(), k.data(), e.data(), 2, bad, out.data()) == ART_E_INVALID);
  CHECK(art_get_prob_nonad_host(&p, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == ART_OK);
  // sampler / event weight / flux argument checks
  std::vector<int32_t> wi(n), ai(n);
  CHECK(art_sample_conversion_points_host(&p, 5.0, 1, 0, n, x.data(), k.data(), e.data(), x.data(), wi.data(),
                                          ai.data()) != ART_OK);
  CHECK(art_sample_conversion_points_host(&p, mr, 1, 0, -1, x.data(), k.data(), e.data(), x.data(), wi.data(),
                                          ai.data()) == ART_E_INVALID);
  CHECK(art_event_weight_host(&p, mr, 0.45, 6.0, 0, nullptr, nullptr, nullptr, nullptr) == ART_OK);
  CHECK(art_flux_histogram_device(&p, n, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) ==
        ART_E_INVALID);
  CHECK(art_flux_histogram_phi_device(n, nullptr, nullptr, nullptr, 50, nullptr, nullptr) == ART_E_INVALID);
  CHECK(art_flux_histogram_phi_device(-1, nullptr, nullptr, nullptr, 50, nullptr, nullptr) == ART_E_INVALID);
  // the sky maps: every argument check comes before the device, n = 0 touches nothing
  {
    const int32_t nb[3] = {3, 5, 2}, nb0[3] = {3, 0, 2}, big[3] = {4096, 4096, 4}, wide[3] = {64, 128, 16};
    const double l3[3] = {0.0, -1.0, 0.0}, h3[3] = {1.0, 1.0, 2.0}, hnan[3] = {1.0, NAN, 2.0}, hempty[3] = {1.0, -1.0, 2.0};
    double* d = x.data();
    CHECK(art_histogram3_device(-1, d, d, d, nullptr, nullptr, nb, l3, h3, 0, d, nullptr) == ART_E_INVALID);
    CHECK(art_histogram3_device(n, d, d, d, nullptr, nullptr, nb0, l3, h3, 0, d, nullptr) == ART_E_INVALID);
    CHECK(art_histogram3_device(n, d, d, d, nullptr, nullptr, nb, l3, hnan, 0, d, nullptr) == ART_E_INVALID);
    CHECK(art_histogram3_device(n, d, d, d, nullptr, nullptr, nb, l3, hempty, 0, d, nullptr) == ART_E_INVALID);
    CHECK(art_histogram3_device(n, d, d, d, nullptr, nullptr, nb, l3, h3, 3, d, nullptr) == ART_E_INVALID);
    CHECK(art_histogram3_device(n, d, d, d, nullptr, nullptr, big, l3, h3, 0, d, nullptr) == ART_E_INVALID);
    CHECK(art_histogram3_device(n, d, d, d, nullptr, nullptr, wide, l3, h3, 1, d, nullptr) == ART_E_INVALID);
    CHECK(art_histogram3_device(0, nullptr, nullptr, nullptr, nullptr, nullptr, nb, l3, h3, 0, nullptr, nullptr) == ART_OK);
    art_sky_spec sk{32, 64, 1, 1, 0, 0.0, 0.0};
    CHECK(art_sky_map_segments_device(&p, &sk, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr) == ART_OK);
    sk.theta_axis = 2;
    CHECK(art_sky_map_segments_device(&p, &sk, n, d, d, d, st.data(), nullptr, nullptr, nullptr, d, nullptr, nullptr) ==
          ART_E_INVALID);
    sk.theta_axis = 0; sk.n_dw = 4;  // n_dw > 1 needs a range
    CHECK(art_sky_map_segments_device(&p, &sk, n, d, d, d, st.data(), nullptr, nullptr, nullptr, d, nullptr, nullptr) ==
          ART_E_INVALID);
    // event rows: the struct checks, the sky spec's and the shared LDS budget, all before the device
    art_event_rows_in ei{};
    art_event_rows_out eo{};
    ei.n_events = ei.n_nodes = 4;
    eo.ncols = 13; eo.nbins = 50; eo.row_capacity = 4; eo.rows = d;
    CHECK(art_event_rows_device(&p, nullptr, &eo, nullptr) == ART_E_INVALID);
    CHECK(art_event_rows_device(&p, &ei, nullptr, nullptr) == ART_E_INVALID);
    eo.sky = &sk;  // still n_dw = 4 without a range
    CHECK(art_event_rows_device(&p, &ei, &eo, nullptr) == ART_E_INVALID);
    art_sky_spec full{16, 32, 8, 1, 1, 0.0, 1.0};  // 8192 doubles: fits alone, not beside the flux table
    eo.sky = &full;
    CHECK(art_event_rows_device(&p, &ei, &eo, nullptr) == ART_E_INVALID);
    eo.sky = nullptr; eo.ncols = 14;
    CHECK(art_event_rows_device(&p, &ei, &eo, nullptr) == ART_E_INVALID);
    eo.ncols = 29; eo.row_capacity = 3;
    CHECK(art_event_rows_device(&p, &ei, &eo, nullptr) == ART_E_INVALID);
    ei.n_events = ei.n_nodes = 0;
    CHECK(art_event_rows_device(&p, &ei, &eo, nullptr) == ART_OK);
    int64_t m = -1;
    CHECK(art_event_gather_photons_device(&p, 4, d, -1, nullptr, 4, d, d, d, d, d, nullptr, nullptr, &m, nullptr) ==
          ART_E_INVALID);
    CHECK(art_event_gather_photons_device(&p, 4, d, 0, nullptr, 4, d, d, d, d, d, nullptr, nullptr, &m, nullptr) == ART_OK &&
          m == 0);
    // event moments: the same struct and sky checks, reserved, node_start and the tables, all before the device
    art_event_moments_out mo{};
    mo.nbins = 50; mo.flux_sq = mo.flux_xa = mo.totals = d;
    ei.n_events = ei.n_nodes = 4;
    CHECK(art_event_moments_device(&p, nullptr, nullptr, &mo, nullptr) == ART_E_INVALID);
    CHECK(art_event_moments_device(&p, &ei, nullptr, nullptr, nullptr) == ART_E_INVALID);
    CHECK(art_event_moments_device(&p, &ei, nullptr, &mo, nullptr) == ART_E_INVALID);  // node_start
    mo.reserved = 1;
    CHECK(art_event_moments_device(&p, &ei, nullptr, &mo, nullptr) == ART_E_INVALID);
    mo.reserved = 0; mo.sky = &sk;  // n_dw = 4 without a range
    CHECK(art_event_moments_device(&p, &ei, nullptr, &mo, nullptr) == ART_E_INVALID);
    mo.sky = &full;  // a good spec (mode is not looked at) without its tables
    CHECK(art_event_moments_device(&p, &ei, nullptr, &mo, nullptr) == ART_E_INVALID);
    ei.n_events = ei.n_nodes = 0;
    CHECK(art_event_moments_device(&p, &ei, nullptr, &mo, nullptr) == ART_OK);
    // the coupling scan: the couplings (host memory, read before the device), the base coupling, node_start,
    // the sky spec and the tables, all before the device
    art_event_reweight_out ro{};
    art_tree_opts to{5, 5, 50, -1, 64, 0, 1e-10, 1769};
    ro.erg = d; ro.nbins = 50; ro.flux = ro.totals = d;
    double g[33];
    for (double& v : g) v = 1e-12;
    int64_t ns[5] = {0, 1, 2, 3, 4};
    ei.n_events = ei.n_nodes = 4;
    CHECK(art_event_reweight_device(nullptr, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID);
    CHECK(art_event_reweight_device(&p, nullptr, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID);
    CHECK(art_event_reweight_device(&p, &ei, ns, nullptr, 2, g, &ro, nullptr) == ART_E_INVALID);
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, g, nullptr, nullptr) == ART_E_INVALID);
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, nullptr, &ro, nullptr) == ART_E_INVALID);
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 0, g, &ro, nullptr) == ART_E_INVALID);
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 33, g, &ro, nullptr) == ART_E_INVALID);
    g[31] = 0.0;  // the last of 32 is read too
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 32, g, &ro, nullptr) == ART_E_INVALID);
    g[31] = std::nan("");
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 32, g, &ro, nullptr) == ART_E_INVALID);
    g[31] = 1e-12;
    art_params p0 = p;
    p0.g_agg = 0.0;
    CHECK(art_event_reweight_device(&p0, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID);
    CHECK(art_event_reweight_device(&p, &ei, nullptr, &to, 2, g, &ro, nullptr) == ART_E_INVALID);  // node_start
    ro.reserved = 1;
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID);
    ro.reserved = 0; ro.sky = &sk;  // n_dw = 4 without a range
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID);
    ro.sky = &full;  // a good spec without its table
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID);
    ro.sky = nullptr; ro.moment_totals = d;  // moments without their tables
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID);
    ro.moment_totals = nullptr;
    ei.n_events = ei.n_nodes = 0;
    CHECK(art_event_reweight_device(&p, &ei, nullptr, &to, 32, g, &ro, nullptr) == ART_OK);
    // the halo scan: the base and the models (host memory, every one of n_models read before the device),
    // node_start, vifty, the sky spec and the tables, all before the device
    art_event_halo_scan_out ho{};
    ho.vifty = d; ho.nbins = 50; ho.flux = ho.totals = d;
    const art_halo hb{260.0, {0.0, 230.0, 0.0}, -1.0};
    art_halo hm[33];
    for (art_halo& v : hm) v = art_halo{220.0, {0.0, 230.0, 0.0}, -1.0};
    ei.n_events = ei.n_nodes = 4;
    CHECK(art_event_halo_scan_device(nullptr, &ei, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);
    CHECK(art_event_halo_scan_device(&p, nullptr, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);
    CHECK(art_event_halo_scan_device(&p, &ei, ns, nullptr, 2, hm, &ho, nullptr) == ART_E_INVALID);
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, nullptr, &ho, nullptr) == ART_E_INVALID);
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, nullptr, nullptr) == ART_E_INVALID);
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 0, hm, &ho, nullptr) == ART_E_INVALID);
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 33, hm, &ho, nullptr) == ART_E_INVALID);
    hm[31].v0 = 400.0;  // the last of 32 is read too: above the base's resolved v_prop
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 32, hm, &ho, nullptr) == ART_E_INVALID);
    hm[31].v0 = 220.0; hm[31].v_ns[2] = std::nan("");
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 32, hm, &ho, nullptr) == ART_E_INVALID);
    hm[31].v_ns[2] = 0.0;
    const art_halo bad_base{260.0, {0.0, 230.0, 0.0}, 100.0};  // v_prop below v0
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &bad_base, 2, hm, &ho, nullptr) == ART_E_INVALID);
    CHECK(art_event_halo_scan_device(&p, &ei, nullptr, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);  // node_start
    ho.vifty = nullptr;
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);
    ho.vifty = d; ho.reserved = 1;
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);
    ho.reserved = 0; ho.sky = &sk;  // n_dw = 4 without a range
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);
    ho.sky = &full;  // a good spec without its table
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);
    ho.sky = nullptr; ho.moment_totals = d;  // moments without their tables
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID);
    ho.moment_totals = nullptr;
    ei.n_events = ei.n_nodes = 0;
    CHECK(art_event_halo_scan_device(&p, &ei, nullptr, &hb, 32, hm, &ho, nullptr) == ART_OK);
    // the jackknife replicates: the group count, the kind, the sets and its factor arrays, then the moments call's
    // checks, all before the device
    art_event_replicates_out po{};
    po.n_groups = 8; po.kind = 0; po.n_sets = 1; po.nbins = 50; po.flux = po.totals = po.groups = d;
    ei.n_events = ei.n_nodes = 4;
    CHECK(art_event_replicates_device(nullptr, &ei, ns, &po, nullptr) == ART_E_INVALID);
    CHECK(art_event_replicates_device(&p, nullptr, ns, &po, nullptr) == ART_E_INVALID);
    CHECK(art_event_replicates_device(&p, &ei, ns, nullptr, nullptr) == ART_E_INVALID);
    for (int bad_groups : {-1, 0, 1, 65}) {
      po.n_groups = bad_groups;
      CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    }
    po.n_groups = 64; po.kind = 3;
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    po.kind = 0; po.n_sets = 2;  // the run has one set
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    po.kind = 1; po.n_sets = 33; po.node_factor = po.event_factor = d;
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    po.n_sets = 32; po.node_factor = nullptr;  // a coupling scan's weights
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    po.kind = 2; po.event_factor = nullptr;  // a halo scan's ratios
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    po.kind = 0; po.n_sets = 1;
    CHECK(art_event_replicates_device(&p, &ei, nullptr, &po, nullptr) == ART_E_INVALID);  // node_start
    po.sky = &sk;  // n_dw = 4 without a range
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    po.sky = &full;  // a good spec without its table
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    po.sky = nullptr; po.groups = nullptr;
    CHECK(art_event_replicates_device(&p, &ei, ns, &po, nullptr) == ART_E_INVALID);
    ei.n_events = ei.n_nodes = 0;
    CHECK(art_event_replicates_device(&p, &ei, nullptr, &po, nullptr) == ART_OK);
    // the coupling x halo grid: the three counts, its factor arrays, then the moments call's checks on nbins and
    // node_start and the tables it needs, all before the device
    art_event_grid_out go{};
    go.n_couplings = 3; go.n_models = 2; go.nbins = 50; go.n_groups = 8;
    go.node_factor = go.back = go.ratio = d;
    go.flux = go.totals = go.flux_rep = go.totals_rep = go.groups = d;
    ei.n_events = ei.n_nodes = 4;
    CHECK(art_event_grid_device(nullptr, &ei, ns, &go, nullptr) == ART_E_INVALID);
    CHECK(art_event_grid_device(&p, nullptr, ns, &go, nullptr) == ART_E_INVALID);
    CHECK(art_event_grid_device(&p, &ei, ns, nullptr, nullptr) == ART_E_INVALID);
    for (int bad_count : {-1, 0, 33}) {
      go.n_couplings = bad_count;
      CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
      go.n_couplings = 32; go.n_models = bad_count;
      CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
      go.n_models = 32;
    }
    for (int bad_groups : {-1, 1, 65}) {
      go.n_groups = bad_groups;
      CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    }
    go.n_groups = 64; go.nbins = 4097;
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.nbins = 50; go.node_factor = nullptr;  // the coupling scan's weights
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.node_factor = d; go.back = nullptr;  // its back factors
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.back = d; go.ratio = nullptr;  // the halo scan's ratios
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.ratio = d;
    CHECK(art_event_grid_device(&p, &ei, nullptr, &go, nullptr) == ART_E_INVALID);  // node_start
    go.totals = nullptr;
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.totals = d; go.flux = nullptr;
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.flux = d; go.flux_rep = nullptr;
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.flux_rep = d; go.groups = nullptr;
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID);
    go.n_groups = 0;  // no replicate tables: theirs are not asked for, and the checks reach the chunk's own buffers
    go.flux_rep = go.totals_rep = nullptr;
    CHECK(art_event_grid_device(&p, &ei, ns, &go, nullptr) == ART_E_INVALID &&
          std::strstr(art_last_error(), "NULL input buffer") != nullptr);
    ei.n_events = ei.n_nodes = 0;
    go.node_factor = go.back = go.ratio = nullptr; go.flux = go.totals = nullptr;
    CHECK(art_event_grid_device(&p, &ei, nullptr, &go, nullptr) == ART_OK);
    // the event power spectrum: the kind, the sets, the bins, the list and its factor arrays, node_start and the
    // tables, all before the device
    art_event_spectrum_out so{};
    so.kind = 0; so.n_sets = 1; so.sub_bits = 3; so.top = 64;
    so.count = so.sum = so.sum_sq = so.totals = so.top_power = d; so.top_event = (int64_t*)d;
    ei.n_events = ei.n_nodes = 4;
    CHECK(art_event_spectrum_device(nullptr, &ei, ns, &so, nullptr) == ART_E_INVALID);
    CHECK(art_event_spectrum_device(&p, nullptr, ns, &so, nullptr) == ART_E_INVALID);
    CHECK(art_event_spectrum_device(&p, &ei, ns, nullptr, nullptr) == ART_E_INVALID);
    so.kind = 3;
    CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    so.kind = 0; so.n_sets = 2;  // the run has one set
    CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    so.n_sets = 1;
    for (int bad_bits : {-1, 5}) {
      so.sub_bits = bad_bits;
      CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    }
    so.sub_bits = 4;
    for (int bad_top : {-1, 257}) {
      so.top = bad_top;
      CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    }
    so.top = 256; so.kind = 1; so.n_sets = 33; so.node_factor = so.event_factor = d;
    CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    so.n_sets = 32; so.node_factor = nullptr;  // a coupling scan's weights
    CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    so.kind = 2; so.event_factor = nullptr;  // a halo scan's ratios
    CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    so.kind = 0; so.n_sets = 1;
    CHECK(art_event_spectrum_device(&p, &ei, nullptr, &so, nullptr) == ART_E_INVALID);  // node_start
    so.sum_sq = nullptr;
    CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    so.sum_sq = d; so.top_event = nullptr;
    CHECK(art_event_spectrum_device(&p, &ei, ns, &so, nullptr) == ART_E_INVALID);
    so.top = 0; so.top_power = nullptr;  // no list: its buffers are not asked for
    ei.n_events = ei.n_nodes = 0;
    CHECK(art_event_spectrum_device(&p, &ei, nullptr, &so, nullptr) == ART_OK);
    // the exact tables: the host twins on limbs, then the device calls' checks, all before the device
    {
      std::vector<int64_t> acc(3 * ART_EXACT_LIMBS, 0);
      const double v[6] = {1e308, 1.0, -1e308, std::nan(""), 5e-324, -1.5};
      const int32_t b[6] = {0, 0, 0, 1, 1, 7};  // (bin 7 of 3: skipped)
      int64_t bad = 0;
      double out[3];
      CHECK(art_exact_add_host(6, b, v, 3, acc.data(), &bad) == ART_OK && bad == 1);
      CHECK(art_exact_normalize_host(3, acc.data()) == ART_OK && art_exact_round_host(3, acc.data(), out) == ART_OK);
      CHECK(out[0] == 1.0 && out[1] == 5e-324 && out[2] == 0.0);
      CHECK(art_exact_add_host(1, nullptr, v, 3, acc.data(), nullptr) == ART_OK);  // (bins NULL: bin 0; no count asked for)
      CHECK(art_exact_add_host(-1, b, v, 3, acc.data(), &bad) == ART_E_INVALID);
      CHECK(art_exact_add_host(1, b, nullptr, 3, acc.data(), &bad) == ART_E_INVALID);
      CHECK(art_exact_round_host(1, nullptr, out) == ART_E_INVALID && art_exact_normalize_host(-1, acc.data()) == ART_E_INVALID);
      CHECK(art_exact_histogram_device(-1, b, v, 3, acc.data(), out, 0, nullptr) == ART_E_INVALID);
      CHECK(art_exact_histogram_device(6, b, v, 0, acc.data(), out, 0, nullptr) == ART_E_INVALID);
      CHECK(art_exact_histogram_device(6, b, v, 3, acc.data(), out, 3, nullptr) == ART_E_INVALID);
      CHECK(art_exact_histogram_device(6, b, v, 125, acc.data(), out, 1, nullptr) == ART_E_INVALID);
      CHECK(art_exact_histogram_device(6, b, v, 3, acc.data(), nullptr, 0, nullptr) == ART_E_INVALID);
      CHECK(art_exact_histogram_device(0, nullptr, nullptr, 3, nullptr, nullptr, 0, nullptr) == ART_OK);
      CHECK(art_exact_finish_device(-1, acc.data(), out, nullptr) == ART_E_INVALID);
      CHECK(art_exact_finish_device(3, nullptr, out, nullptr) == ART_E_INVALID);
      art_event_exact_out xo{};
      xo.kind = 0; xo.n_sets = 1; xo.nbins = 50; xo.flux_acc = xo.totals_acc = acc.data(); xo.nonfinite = xo.misplaced = d;
      ei.n_events = ei.n_nodes = 4;
      CHECK(art_event_exact_device(nullptr, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      CHECK(art_event_exact_device(&p, nullptr, ns, &xo, nullptr) == ART_E_INVALID);
      CHECK(art_event_exact_device(&p, &ei, ns, nullptr, nullptr) == ART_E_INVALID);
      xo.kind = 3;
      CHECK(art_event_exact_device(&p, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      xo.kind = 0; xo.n_sets = 2;  // the run has one set
      CHECK(art_event_exact_device(&p, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      xo.kind = 1; xo.n_sets = 32;  // a coupling scan without its factors
      CHECK(art_event_exact_device(&p, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      xo.kind = 0; xo.n_sets = 1; xo.mode = 3;
      CHECK(art_event_exact_device(&p, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      xo.mode = 1; xo.nbins = 57;  // the LDS path holds 56 flux bins
      CHECK(art_event_exact_device(&p, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      xo.mode = 0; xo.nbins = 50;
      CHECK(art_event_exact_device(&p, &ei, nullptr, &xo, nullptr) == ART_E_INVALID);  // node_start
      xo.sky = &full;  // a good spec without its accumulators
      CHECK(art_event_exact_device(&p, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      xo.sky = nullptr; xo.nonfinite = nullptr;
      CHECK(art_event_exact_device(&p, &ei, ns, &xo, nullptr) == ART_E_INVALID);
      ei.n_events = ei.n_nodes = 0;
      CHECK(art_event_exact_device(&p, &ei, nullptr, &xo, nullptr) == ART_OK);
    }
    // where the four event calls differ on purpose (art_post.cpp's front-end flags). A call that passes its
    // argument checks goes on to the device, which this container does not have.
    auto went_on = [](int r) { return r == ART_E_HIP || r == ART_E_NOMEM || r == ART_OK; };
    auto said = [](const char* what) { return std::strstr(art_last_error(), what) != nullptr; };
    // an empty chunk with nodes and no node_start: moments returns before it looks, the scans look first
    mo.sky = nullptr;
    ei.n_events = 0; ei.n_nodes = 4;
    CHECK(art_event_moments_device(&p, &ei, nullptr, &mo, nullptr) == ART_OK);
    CHECK(art_event_reweight_device(&p, &ei, nullptr, &to, 2, g, &ro, nullptr) == ART_E_INVALID && said("node_start is NULL"));
    CHECK(art_event_halo_scan_device(&p, &ei, nullptr, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID && said("node_start is NULL"));
    // only the rows call looks at the spec's mode
    art_sky_spec odd{4, 8, 1, 1, 7, 0.0, 0.0};
    ei.n_nodes = 0;
    eo.sky = &odd; mo.sky = &odd; ro.sky = &odd; ho.sky = &odd;
    CHECK(art_event_rows_device(&p, &ei, &eo, nullptr) == ART_E_INVALID && said("sky map mode"));
    CHECK(art_event_moments_device(&p, &ei, nullptr, &mo, nullptr) == ART_OK);
    CHECK(art_event_reweight_device(&p, &ei, nullptr, &to, 2, g, &ro, nullptr) == ART_OK);
    CHECK(art_event_halo_scan_device(&p, &ei, nullptr, &hb, 2, hm, &ho, nullptr) == ART_OK);
    eo.sky = mo.sky = ro.sky = ho.sky = nullptr;
    // cyc_slot with a batch and its cyc_tau but no end states: rows and moments refuse, the scans need cyc_tau alone
    std::vector<art_tree_node> nd(4);
    ei.n_events = ei.n_nodes = 4;
    ei.x = ei.k_init = ei.weight5 = d; ei.attempts = ai.data();
    ei.back = ei.nodes = nd.data(); ei.back_counts = ei.counts = ei.infos = st.data();
    ei.cyc_slot = st.data(); ei.cyc_n = 2; ei.cyc_tau = d; ei.cyc_end = nullptr;
    eo.ncols = 13; eo.row_capacity = 4; eo.flux = eo.totals = d;
    CHECK(art_event_rows_device(&p, &ei, &eo, nullptr) == ART_E_INVALID && said("the re-run's end states"));
    CHECK(art_event_moments_device(&p, &ei, ns, &mo, nullptr) == ART_E_INVALID && said("the re-run's end states"));
    CHECK(went_on(art_event_reweight_device(&p, &ei, ns, &to, 2, g, &ro, nullptr)));
    CHECK(went_on(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr)));
    ei.cyc_tau = nullptr;  // (that much the scans do ask for, in their own words)
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID && said("cyc_n >= 0 and cyc_tau"));
    CHECK(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr) == ART_E_INVALID && said("cyc_n >= 0 and cyc_tau"));
    // events without nodes: the coupling scan still reads its per-event buffers, the halo scan only vifty
    ei.cyc_slot = nullptr; ei.cyc_n = 0;
    ei.n_nodes = 0; ei.weight5 = nullptr;
    CHECK(art_event_reweight_device(&p, &ei, ns, &to, 2, g, &ro, nullptr) == ART_E_INVALID && said("NULL input buffer"));
    CHECK(went_on(art_event_halo_scan_device(&p, &ei, ns, &hb, 2, hm, &ho, nullptr)));
  }
  // the device forest: every argument check comes before the device; with roots it reaches the HIP runtime
  {
    art_tree_opts to{5, 5, 50, -1, 64, 0, 1e-10, 1769};
    int64_t nn = -1;
    double* d = x.data();
    CHECK(art_grow_trees_device(nullptr, n, d, d, d, sp.data(), &to, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_E_INVALID);
    CHECK(art_grow_trees_device(&p, n, d, d, d, sp.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_E_INVALID);
    CHECK(art_grow_trees_device(&p, n, d, d, d, sp.data(), &to, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ART_E_INVALID);
    CHECK(art_grow_trees_device(&p, -1, d, d, d, sp.data(), &to, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_E_INVALID);
    CHECK(art_grow_trees_device(&p, n, d, d, nullptr, sp.data(), &to, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_E_INVALID);
    art_tree_opts bad_opts = to;
    bad_opts.max_nodes = -1;
    CHECK(art_grow_trees_device(&p, n, d, d, d, sp.data(), &bad_opts, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_E_INVALID);
    bad_opts = to; bad_opts.crossing_cap = -2;
    CHECK(art_grow_trees_device(&p, n, d, d, d, sp.data(), &bad_opts, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_E_INVALID);
    bad_opts = to; bad_opts.splittings_cutoff = 100000;
    CHECK(art_grow_trees_device(&p, n, d, d, d, sp.data(), &bad_opts, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_E_INVALID);
    CHECK(nn == -1);
    CHECK(art_grow_trees_device(&p, 0, nullptr, nullptr, nullptr, nullptr, &to, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr) == ART_OK);
    CHECK(nn == 0);
    rc = art_grow_trees_device(&p, n, d, d, d, sp.data(), &to, 0, nullptr, nullptr, nullptr, nullptr, &nn, nullptr);
    CHECK(rc == ART_E_HIP || rc == ART_E_NOMEM);
  }
  // the reduction: nothing to reduce without a communicator, bad ranks rejected
  double h[4] = {1, 2, 3, 4};
  CHECK(art_flux_allreduce(h, 4, nullptr) == ART_E_INVALID);
  CHECK(art_flux_allreduce_host(h, 4) == ART_E_INVALID);
  art_rccl_id id{};
  CHECK(art_comm_init(2, 2, &id) == ART_E_INVALID);
  CHECK(art_comm_init(0, 0, &id) == ART_E_INVALID);
  CHECK(art_comm_init(0, 1, nullptr) == ART_E_INVALID);
  CHECK(art_comm_destroy() == ART_OK);
  double ms[2];
  CHECK(art_recent_kernel_ms(-1, ms) != ART_OK);
  // the scalar-function entry: an unknown fn or tu is refused before any device call, n = 0 touches nothing
  CHECK(art_eval_math_device(ART_MATH_COUNT, 0, 4, h, h, h, nullptr, nullptr) == ART_E_INVALID);
  CHECK(art_eval_math_device(-1, 0, 4, h, h, h, nullptr, nullptr) == ART_E_INVALID);
  CHECK(art_eval_math_device(ART_MATH_EXP, 2, 4, h, nullptr, h, nullptr, nullptr) == ART_E_INVALID);
  CHECK(art_eval_math_device(ART_MATH_MAX_Q, 0, 4, h, nullptr, h, nullptr, nullptr) == ART_E_INVALID);
  CHECK(art_eval_math_device(ART_MATH_EXP, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ART_OK);
  std::printf("capi OK\n");
  return 0;
}
