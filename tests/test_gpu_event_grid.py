"""The coupling x halo grid on the GPU (art_event_grid_device, Engine.event_grid, run_events(grid=True),
main_runner_tree(device_events=True, grid=True)) against trees.grid_tables, the numpy statement of its definition,
on the rows and the factors the device itself hands out, against the coupling scan's own tables, and against a
direct run under a target halo model.

Integer factors (the synthetic forest): every power W B sln R is an integer of at most 3⁴ and every sum, X² and X a_e
an integer below 2^53, so the device tables are np.array_equal to numpy's, whatever the order of the adds.

Weighted tables. The power of a row at a cell is formed by the same three products in the same order on both sides
(reweight_power, then the ratio), so the terms are bit-equal and an entry is a sum of the same non-negative terms in
another order: two such sums differ by at most 2 (cnt + 1) u max(got, ref) with cnt the entry's rows and u = 2^-53
(tests/test_gpu_replicates.py). Σ over the groups of an entry adds at most one rounding per group that holds a row of
it, which the same bound with the rows of all groups covers. An event's X is summed in node order on both sides and
is bit-equal; Q = Σ X² and C = Σ X a_e are then sums over the events in another order, within
tests/test_gpu_event_moments.py's 2 (E + 2 m + 2) u max(got, ref) with E the events and m the most rows of one event.

Against a direct run under target model h (the same seed and proposal: the same events, forests and rows but column
7): column 7 of the base run times R_h is within β relative of the direct run's (tests/test_halo_scan.py's beta), so an
entry differs by the add-order bound plus Σ β p over its rows.

ART_PARITY_REPORT=path collects the JSON lines the tests print. Measured on an MI355X
(profiles/event_grid_parity.jsonl; DESIGN.md §3, "Coupling x halo grid"): the synthetic forest exact in all 48
cases; 600 events give 2151 records and 1102 rows; every cell against numpy 0.26 of the add-order bound, the base
column against the coupling scan 0.23, Σ over the groups 0.17, chunks 0.25, Q and C 0.02 of their bound; against
the direct run under Halo(220, (0, 230, 0)) 0.06 of the bound, photon totals to 6.7e-16 relative, slopes at least
1.77, the limit equal to the direct run's crossing (1.414e-12, σ 6.6e-14); band hi / lo = 1.044 +- 0.011 with
the limits of the base and the target correlated at 0.98; main_runner_tree 0.24; off by default 0.14."""
import json
import os

import numpy as np
import pytest

from test_gpu_event_moments import SIZES, _synthetic_forest
from test_gpu_event_moments import _bound as _moment_bound
from test_gpu_event_moments import _groups
from test_gpu_event_rows import SEED, U, _np, _params
from test_gpu_halo_scan import C_KM, _eng, _halos, _pipe
from test_halo_scan import beta

pytestmark = pytest.mark.gpu

N, R, NBINS = 600, 7, 50
LO = 1003
_cache = {}


def _report(what, **vals):
    line = json.dumps({"test": "event_grid", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _raw(grid):
    from adiabatic_raytracer_amd import trees as T
    return T.grid_raw(grid)


def _tables(raw):
    from adiabatic_raytracer_amd import trees as T
    return [k for k in T.GRID_KEYS if raw.get(k) is not None]


# ---- 1. the synthetic forest: exact

def _synthetic():
    """the synthetic forest, its rows from event_rows (computed once) and the record index of every row"""
    if "syn" not in _cache:
        from test_gpu_event_rows import _engine
        parts, nd, recs = _synthetic_forest()
        er = _engine().event_rows(*parts, event_offset=LO, nbins=NBINS)
        rows = er["rows"].cpu().numpy()
        fin = np.flatnonzero(nd["is_final"] != 0)
        assert len(rows) == len(fin) and np.array_equal(rows[:, 0], nd["tree"][fin] + 1.0 + LO)
        rows.setflags(write=False)
        _cache["syn"] = (_engine(), parts, nd, recs, rows, fin)
    return _cache["syn"]


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("nbins", [0, 50])
@pytest.mark.parametrize("groups", [None, 2, 64])
@pytest.mark.parametrize("Kg,Kh", [(1, 1), (3, 2), (5, 13), (32, 32)])
def test_synthetic_forest_is_exact(Kg, Kh, groups, nbins, moments):
    import torch
    from adiabatic_raytracer_amd import trees as T
    eng, parts, nd, recs, rows, fin = _synthetic()
    s, w5, back, fwd = parts
    n, nn = len(SIZES), sum(SIZES)
    rng = np.random.default_rng(1000 * Kg + Kh)
    W, B, Rt = (rng.integers(0, 4, shape).astype(np.float64) for shape in ((Kg, nn), (Kg, n), (Kh, n)))
    up = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
    base = _halos()[0]
    kw = dict(weights=up(W), back_factor=up(B), ratio=up(Rt), g=[1e-12 * (k + 1) for k in range(Kg)],
              models=[(200.0 + k, (0.0, 10.0 * k, 0.0)) for k in range(Kh)], base=base, event_offset=LO, nbins=nbins,
              replicates=groups, errors=moments)
    att = s["attempts"].cpu().numpy()
    grid = eng.event_grid(*parts, **kw)
    got = _raw(grid)
    want = T.grid_tables(rows, W, B, Rt, fin, nbins, groups, att, LO)
    names = _tables(got)
    assert names == [k for k in T.GRID_KEYS if k in want and (moments or k != "moment_totals")]
    assert ("groups" in names) == (groups is not None) and ("moment_totals" in names) == moments
    for k in names:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["flux"].shape == (Kg, Kh, 2 * nbins) and want["totals"][..., :2].sum() > 0 and not want["totals"][..., 2].any()
    if nbins:
        assert 0 < want["flux"].sum() < want["totals"][..., :2].sum()  # (rows with a NaN direction are in no bin)
    if groups:
        assert got["groups"][:, 0].sum() == n and (got["groups"][:, 0] == 0).sum() == max(0, groups - n)
    # accumulated into: a second call doubles every table
    twice = _raw(eng.event_grid(*parts, grid=grid, **kw))
    for k in names:
        assert np.array_equal(twice[k], 2.0 * want[k]), k
    # a final record of tree 3 inside the range of tree 7: counted, for the group of the tree it names, and skipped
    start = np.r_[0, np.cumsum(SIZES)]
    q = fin[(fin >= start[7] + 100)][0]
    bad = nd.copy()
    bad["tree"][q] = 3
    got_bad = _raw(eng.event_grid(s, w5, back, dict(fwd, nodes=recs(bad)), **kw))
    keep = fin != q
    want_bad = T.grid_tables(rows[keep], W, B, Rt, fin[keep], nbins, groups, att, LO)
    want_bad["totals"][0, 0, 2] = want_bad["moment_totals"][0, 0, 7] = 1.0
    if groups:
        want_bad["groups"][(LO + 3) % groups, 2] = 1.0
    for k in names:
        assert np.array_equal(got_bad[k], want_bad[k]), k
    assert T.grid_result(got_bad, 1)["misplaced"] == 1


def test_event_grid_value_errors():
    import torch
    eng, parts, nd, recs, rows, fin = _synthetic()
    n, nn = len(SIZES), sum(SIZES)
    base = _halos()[0]
    z = lambda *d: torch.zeros(*d, dtype=torch.float64, device=eng.device)  # noqa: E731
    good = dict(weights=z(2, nn), back_factor=z(2, n), ratio=z(3, n), g=[1e-12, 2e-12], models=[base, base, base], base=base)
    grid = eng.event_grid(*parts, **good)
    for name, t in (("weights", z(2, nn + 1)), ("weights", z(nn, 2).t()), ("back_factor", z(3, n)), ("ratio", z(3, n + 1)),
                    ("ratio", z(3, n).float()), ("back_factor", z(2, 2 * n)[:, ::2])):
        with pytest.raises(ValueError, match=f"event_grid: {name} must be a contiguous float64 tensor"):
            eng.event_grid(*parts, **dict(good, **{name: t}))
    for change in (dict(g=[1e-12, 3e-12]), dict(models=[base, base, (200.0, (0.0, 0.0, 0.0))]), dict(replicates=4),
                   dict(errors=True), dict(nbins=10)):
        with pytest.raises(ValueError, match="`grid` was made for other couplings, models, groups or tables"):
            eng.event_grid(*parts, grid=grid, **dict(good, **change))


# ---- 2. a real forest: 600 flat events under the halo tests' base model, 3 couplings x 3 models

def _couplings():
    g0 = _eng()[0].params.g_agg
    return [g0, 2.0 * g0, 0.5 * g0]


def _factors(lo=0, c=N):
    """the two scans of events [lo, lo + c) with their factors, and event_rows' rows: (scan, halo scan, rows, fin)"""
    if ("factors", lo, c) not in _cache:
        from adiabatic_raytracer_amd.engine import nodes_to_numpy
        eng = _eng()[0]
        base, models = _halos()
        parts = _pipe(lo, c)
        kw = dict(event_offset=lo, nbins=NBINS)
        er = eng.event_rows(*parts, **kw)
        sc = eng.event_reweight(*parts, _couplings(), mc_nodes=5, return_weights=True, **kw)
        hs = eng.event_halo_scan(*parts, base, models, return_ratio=True, **kw)
        rows = er["rows"].cpu().numpy()
        nodes = nodes_to_numpy(parts[3]["nodes"])
        fin = np.flatnonzero(nodes["is_final"] != 0)
        assert len(fin) == len(rows) and np.array_equal(nodes["tree"][fin], rows[:, 0].astype(np.int64) - 1 - lo)
        _cache[("factors", lo, c)] = (sc, hs, rows, fin)
    return _cache[("factors", lo, c)]


def _grid_of(lo=0, c=N, grid=None, **kw):
    sc, hs, _, _ = _factors(lo, c)
    base, models = _halos()
    return _eng()[0].event_grid(*_pipe(lo, c), weights=sc["weights"], back_factor=sc["back"], ratio=hs["ratio"],
                                g=_couplings(), models=models, base=base, event_offset=lo, nbins=NBINS, grid=grid, **kw)


def _counts(rows, groups):
    """the rows of every entry of the first-moment tables: per flux bin, per species, and per group of each"""
    from adiabatic_raytracer_amd import trees as T
    sp = rows[:, 1].astype(np.int64)
    g = (rows[:, 0].astype(np.int64) - 1) % groups
    fb = T.hist_bins(rows[:, 3], NBINS)
    k = fb >= 0
    lab = sp * NBINS + fb
    return {"flux": np.bincount(lab[k], minlength=2 * NBINS), "totals": np.bincount(sp, minlength=2),
            "flux_rep": np.bincount(g[k] * 2 * NBINS + lab[k], minlength=groups * 2 * NBINS).reshape(groups, 2 * NBINS),
            "totals_rep": np.bincount(g * 2 + sp, minlength=2 * groups).reshape(groups, 2)}


def _within(what, got, ref, cnt, extra=None):
    """the module docstring's add-order bound per entry (cnt broadcasts over the cells; extra: what the terms
    themselves may differ by); returns the largest measured / bound"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    cnt = np.broadcast_to(cnt, got.shape)
    assert got.shape == ref.shape and np.all(ref >= 0) and np.all(got >= 0), what
    err, bound = np.abs(got - ref), 2 * (cnt + 1) * U * np.maximum(got, ref) + (0.0 if extra is None else extra)
    f = (cnt > 0) & (bound > 0)
    ratio = float(np.max(err[f] / bound[f])) if f.any() else 0.0
    assert np.all(err <= bound), (what, ratio)
    assert np.all(got[cnt == 0] == 0) and np.all(ref[cnt == 0] == 0), what
    return ratio


def _first_moments_within(what, got, ref, cnt):
    """every first-moment table of two raw dicts; the largest share of the bound"""
    worst = _within(f"{what}_flux", got["flux"], ref["flux"], cnt["flux"])
    worst = max(worst, _within(f"{what}_totals", got["totals"][..., :2], ref["totals"][..., :2], cnt["totals"]))
    if ref.get("flux_rep") is not None:
        worst = max(worst, _within(f"{what}_flux_rep", got["flux_rep"], ref["flux_rep"], cnt["flux_rep"]),
                    _within(f"{what}_totals_rep", got["totals_rep"], ref["totals_rep"], cnt["totals_rep"]))
        assert np.array_equal(got["groups"], ref["groups"]), what
    assert np.array_equal(got["totals"][..., 2], ref["totals"][..., 2]), what
    return worst


def _moments_within(what, got, ref, rows):
    """moment totals: slots 0, 1, 2 and 7 exact, Q and C within tests/test_gpu_event_moments.py's bound"""
    ev, sp = rows[:, 0].astype(np.int64) - 1, rows[:, 1].astype(np.int64)
    grp = _groups(ev, sp, 2)
    assert np.array_equal(got[..., [0, 1, 2, 7]], ref[..., [0, 1, 2, 7]]), what
    worst = 0.0
    for q in (3, 4, 5, 6):
        a, b = got[..., q], ref[..., q]
        gq = tuple(v[(q - 3) % 2] for v in grp)
        err, bound = np.abs(a - b), _moment_bound(a, b, gq)
        assert np.all(err <= bound), (what, q)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0)
    return worst


def test_real_forest_against_numpy_the_scan_and_chunks():
    from adiabatic_raytracer_amd import trees as T
    sc, hs, rows, fin = _factors()
    base, models = _halos()
    parts = _pipe(0, N)
    assert parts[3]["n_nodes"] > 3 * 256 and len(rows) > 1000
    W, B, ratio = (v.cpu().numpy() for v in (sc["weights"], sc["back"], hs["ratio"]))
    att = parts[0]["attempts"].cpu().numpy()
    got = _raw(_grid_of(replicates=R, errors=True))
    assert got["flux"].shape == (3, 3, 2 * NBINS) and got["flux_rep"].shape == (3, 3, R, 2 * NBINS)
    assert got["totals_rep"].shape == (3, 3, R, 2) and got["moment_totals"].shape == (3, 3, 8)
    cnt = _counts(rows, R)
    # every cell against the numpy statement, from the device's own weights, back, ratio and rows
    ref = T.grid_tables(rows, W, B, ratio, fin, NBINS, R, att, 0)
    a = _first_moments_within("numpy", got, ref, cnt)
    m = _moments_within("numpy_moments", got["moment_totals"], ref["moment_totals"], rows)
    assert got["totals"][..., 1].min() > 0 and got["groups"][:, 0].sum() == N and not got["totals"][..., 2].any()
    # column kh = base: R is exactly 1 there, so the powers are the coupling scan's own bit for bit
    assert np.array_equal(ratio[0], np.ones(N))
    sf, st = sc["flux"].cpu().numpy(), sc["totals"].cpu().numpy()
    b = max(_within("scan_flux", got["flux"][:, 0], sf, cnt["flux"]), _within("scan_totals", got["totals"][:, 0, :2], st[:, :2], cnt["totals"]))
    # Σ over the groups of the replicate tables
    c = max(_within("sum_flux", got["flux_rep"].sum(axis=2), got["flux"], cnt["flux"]),
            _within("sum_totals", got["totals_rep"].sum(axis=2), got["totals"][..., :2], cnt["totals"]))
    # one chunk against chunks of 250
    acc = None
    for lo, n in ((0, 250), (250, 250), (500, 100)):
        acc = _grid_of(lo, n, grid=acc, replicates=R, errors=True)
    acc = _raw(acc)
    assert acc["n_events"] == N
    d = _first_moments_within("chunks", acc, got, cnt)
    e = _moments_within("chunks_moments", acc["moment_totals"], got["moment_totals"], rows)
    # without the replicate and the moment tables: the same first moments
    lean = _raw(_grid_of())
    assert _tables(lean) == ["flux", "totals"]
    f = _first_moments_within("lean", lean, {k: got[k] for k in ("flux", "totals")}, cnt)
    _report("real_forest", rows=int(len(rows)), nodes=int(parts[3]["n_nodes"]), numpy=a, numpy_moments=m, base_column_vs_scan=b,
            sum_over_groups=c, chunks=d, chunks_moments=e, lean=f)


# ---- 3. end to end: run_events(grid=True) against a direct run under a target model, and main_runner_tree

G4 = (0.5, 1.0, 2.0, 4.0)  # times g0: the two middle couplings bracket the threshold
H = 1                      # the target model of the direct run


def _runs():
    if "runs" not in _cache:
        import adiabatic_raytracer_amd as A
        eng = _eng()[0]
        base, models = _halos()
        g = [q * eng.params.g_agg for q in G4]
        h = models[H]
        r = _np(eng.run_events(N, seed=SEED, halo=base, couplings=g, halos=models, grid=True, replicates=8, errors=True,
                               nbins=NBINS))
        d = _np(eng.run_events(N, seed=SEED, halo=A.Halo(h.v0, h.v_ns, v_prop=base.vp()), couplings=g, replicates=8,
                               nbins=NBINS))
        _cache["runs"] = (g, r, d)
    return _cache["runs"]


def test_run_events_column_against_a_direct_run():
    from adiabatic_raytracer_amd import trees as T
    base, models = _halos()
    h = models[H]
    g, r, d = _runs()
    grid = r["grid"]
    assert set(grid) == {"g", "models", "base", "flux", "sum_weight_sln_prob", "misplaced", "raw", "f_inx",
                         "sum_weight_sln_prob_sigma", "n_eff", "replicates"}
    assert grid["flux"].shape == (4, 3, 2, NBINS) and grid["sum_weight_sln_prob"].shape == (4, 3, 2) and grid["misplaced"] == 0
    assert grid["sum_weight_sln_prob_sigma"].shape == (4, 3, 2) and grid["n_eff"].shape == (4, 3)
    assert np.all(grid["sum_weight_sln_prob_sigma"] > 0) and np.all((grid["n_eff"] > 1) & (grid["n_eff"] <= N))
    assert set(grid["replicates"]) == {"R", "flux", "totals", "n_g", "a_g", "f_inx"} and grid["replicates"]["a_g"].sum() == r["f_inx"]
    assert (d["f_inx"], d["n_rows"]) == (r["f_inx"], r["n_rows"])
    rows, dr = r["rows_raw"], d["rows_raw"]
    other = [c for c in range(rows.shape[1]) if c != 7]
    assert np.array_equal(dr[:, other], rows[:, other], equal_nan=True)  # the same events, forests and rows but column 7
    # β per event, and per row the power at each coupling as the grid forms it (the base pipeline's own factors;
    # the couplings of _factors are another list, so the scan is made here once more for these four)
    eng = _eng()[0]
    parts = _pipe(0, N)
    sc = eng.event_reweight(*parts, g, mc_nodes=5, return_weights=True, nbins=NBINS)
    _, hs, prow, fin = _factors()
    assert np.array_equal(prow, rows, equal_nan=True)
    W, B, ratio = sc["weights"].cpu().numpy(), sc["back"].cpu().numpy(), hs["ratio"].cpu().numpy()
    ev, sp = rows[:, 0].astype(np.int64) - 1, rows[:, 1].astype(np.int64)
    v = parts[0]["vifty"].cpu().numpy().reshape(3, N) * C_KM
    be = beta(np.sqrt((v * v).sum(axis=0)), (base.v0, base.v_ns), (h.v0, h.v_ns), base.vp())
    assert be.max() < 1e-12
    fb = T.hist_bins(rows[:, 3], NBINS)
    lab, k = sp * NBINS + fb, fb >= 0
    cnt = _counts(rows, 8)
    own, raw = d["coupling_scan"]["raw"], grid["raw"]
    worst = 0.0
    for kg in range(4):
        p = ((W[kg, fin] * B[kg, ev]) * rows[:, 7]) * ratio[H, ev]
        db = be[ev] * p * (1.0 + be[ev])  # Σ β p, p the direct run's own within β
        worst = max(worst,
                    _within("direct_flux", raw["flux"][kg, H], own["flux"][kg], cnt["flux"],
                            np.bincount(lab[k], weights=db[k], minlength=2 * NBINS)),
                    _within("direct_totals", raw["totals"][kg, H, :2], own["totals"][kg, :2], cnt["totals"],
                            np.bincount(sp, weights=db, minlength=2)))
    rel = np.abs(raw["totals"][:, H, 1] / own["totals"][:, 1] - 1.0).max()
    # the limit: the crossing of column H against the direct run's own coupling_crossing
    col = grid["sum_weight_sln_prob"][:, H, 1]
    order = np.argsort(g)
    slope = np.diff(np.log(col[order])) / np.diff(np.log(np.asarray(g)[order]))
    assert np.all(slope >= 1.0), slope  # so the crossing moves by no more than the totals do
    power = float(np.sqrt(col[order][1] * col[order][2]))
    band = T.limit_band(grid, power)
    cross = T.coupling_crossing(d["coupling_scan"], power)
    assert not np.isnan(band["g"]).any() and band["groups_used"] == cross["groups_used"] == 8
    assert np.isclose(band["g"][H], cross["value"], rtol=1e-9, atol=0)
    assert g[1] < band["g"][H] < g[2] and np.isclose(band["sigma"][H], cross["sigma"], rtol=1e-6)
    assert band["lo"] <= band["g"][H] <= band["hi"] and band["ratio"] >= 1.0 and band["ratio_sigma"] >= 0
    # the models share every event: their limits move together
    corr = band["cov"][0, H] / (band["sigma"][0] * band["sigma"][H])
    assert corr > 0.0
    avg = T.limit_band(grid, power, average=[0, 1, 2])
    assert band["lo"] <= avg["g_avg"] <= band["hi"] and avg["sigma_avg"] > 0
    _report("direct_run", model=[h.v0, list(h.v_ns)], tables_over_bound=worst, photon_totals_rel=float(rel),
            slope_min=float(slope.min()), g_limit=float(band["g"][H]), g_direct=float(cross["value"]),
            g_rel=float(abs(band["g"][H] / cross["value"] - 1.0)), sigma=float(band["sigma"][H]), band=[band["lo"], band["hi"]],
            band_ratio=band["ratio"], band_ratio_sigma=band["ratio_sigma"], correlation_base_target=float(corr))


def test_main_runner_tree_returns_the_same_grid():
    import adiabatic_raytracer_amd as A
    base, models = _halos()
    g, r, _ = _runs()
    info = {}
    A.trees.main_runner_tree(_params("flat"), N + 1, device_events=True, halo=base, couplings=g, halos=models, grid=True,
                             replicates=8, errors=True, nbins=NBINS, run_info=info)
    assert set(info["grid"]) == set(r["grid"]) and info["f_inx"] == r["f_inx"] == info["grid"]["f_inx"]
    cnt = _counts(r["rows_raw"], 8)
    a = _first_moments_within("main_runner", info["grid"]["raw"], r["grid"]["raw"], cnt)
    b = _moments_within("main_runner_moments", info["grid"]["raw"]["moment_totals"], r["grid"]["raw"]["moment_totals"], r["rows_raw"])
    assert info["grid"]["raw"]["n_events"] == N and np.array_equal(info["grid"]["g"], r["grid"]["g"])
    assert np.allclose(info["grid"]["sum_weight_sln_prob"], r["grid"]["sum_weight_sln_prob"], rtol=1e-12, atol=0)
    _report("main_runner_tree", first_moments=a, moments=b)


# ---- 4. off by default

def test_off_by_default_and_chunked_run():
    base, models = _halos()
    eng = _eng()[0]
    g = _couplings()
    kw = dict(seed=SEED, chunk=96, halo=base, couplings=g, halos=models, replicates=R, errors=True, nbins=NBINS)
    plain = _np(eng.run_events(200, **kw))
    r = _np(eng.run_events(200, grid=True, **kw))
    assert set(r) - set(plain) == {"grid"} and "grid" not in plain
    for key in ("coupling_scan", "halo_scan"):
        assert set(r[key]) == set(plain[key]) and set(r[key]["raw"]) == set(plain[key]["raw"])
        assert not any(k in r[key]["raw"] for k in ("weights", "back", "back_prob", "ratio"))
    # the keys of a run with none of the keywords, as they were before the grid
    assert set(_np(eng.run_events(4, seed=SEED))) == {"rows", "flux", "f_inx", "sum_weight_sln_prob", "n_rows", "n_photon_rows",
                                                      "totals", "flux_raw", "rows_raw"}
    rows = r["rows_raw"]
    assert np.array_equal(plain["rows"], r["rows"], equal_nan=True) and plain["f_inx"] == r["f_inx"]
    cnt = _counts(rows, R)
    a = _within("off_flux", plain["flux_raw"], r["flux_raw"], cnt["flux"])
    # three chunks through run_events: the base column is the coupling scan of the same run (R is exactly 1 there)
    raw = r["grid"]["raw"]
    assert raw["n_events"] == 200 and raw["groups"][:, 0].sum() == 200 and raw["groups"][:, 1].sum() == r["f_inx"]
    own = r["coupling_scan"]["raw"]
    b = _within("base_column_flux", raw["flux"][:, 0], own["flux"], cnt["flux"])
    c = _within("base_column_totals", raw["totals"][:, 0, :2], own["totals"][:, :2], cnt["totals"])
    assert np.array_equal(raw["groups"], r["replicates"]["raw"]["groups"])
    _report("off_by_default", flux_with_vs_without=a, base_column_flux=b, base_column_totals=c)
