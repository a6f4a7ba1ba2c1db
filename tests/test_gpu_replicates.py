"""Jackknife replicates on the GPU (art_event_replicates_device, Engine.event_replicates, run_events(replicates=),
main_runner_tree(replicates=)) against trees.rows_replicates and np.bincount on the rows that Engine.event_rows
returns for the same forests.

Unit weights and integer powers: every table entry is an integer below 2^53, so the device tables are
np.array_equal to numpy's, whatever the order of the adds.

A weighted bin of one group is a sum of the same non-negative terms in another order: two such sums differ by at
most 2 (cnt + 1) u S with cnt its rows, S the bin and u = 2^-53 (tests/test_gpu_event_rows.py). The sum over the
groups of a bin adds one rounding per group that holds a row of it -- adding a zero is exact -- so at most cnt - 1
more, which the same bound with the bin's rows of all groups covers.

ART_PARITY_REPORT=path collects the JSON lines the tests print (profiles/replicates_parity.jsonl; DESIGN.md §3,
"Jackknife replicates")."""
import json
import os

import numpy as np
import pytest

from test_gpu_event_moments import SIZES, _synthetic_forest
from test_gpu_event_rows import SEED, U, _engine, _np, _params, _pipeline, _run, _unit

pytestmark = pytest.mark.gpu

N, R, NBINS = 600, 7, 50


def _report(what, **vals):
    line = json.dumps({"test": "replicates", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _sky():
    """6 x 11 x 4 with a Δω range that holds most of the run's rows and drops some"""
    lo, hi = np.quantile(_run("flat", N)["rows_raw"][:, 12], [0.02, 0.98])
    return dict(n_theta=6, n_phi=11, n_dw=4, dw_range=(float(lo), float(hi)))


def _attempts(n, **kw):
    return _engine().sample(n, seed=SEED, **kw)["attempts"].cpu().numpy()


def _counts(rows, groups, sky, lo=0):
    """the rows per (group, bin) of every table: rows_replicates of the same rows with unit powers"""
    from adiabatic_raytracer_amd import trees as T
    unit = np.array(rows, np.float64)
    unit[:, 7] = unit[:, 8] = 1.0
    return T.rows_replicates(unit, groups, NBINS, sky, None, lo, n_events=int(rows[:, 0].max()) - lo)


def _within(what, got, ref, cnt):
    """the module docstring's bound per entry; the largest measured / bound"""
    got, ref, cnt = (np.asarray(v, np.float64).reshape(-1) for v in (got, ref, cnt))
    assert got.shape == ref.shape == cnt.shape and np.all(ref >= 0) and np.all(got >= 0), what
    err, bound = np.abs(got - ref), 2 * (cnt + 1) * U * np.maximum(got, ref)
    f = (cnt > 0) & (bound > 0)
    ratio = float(np.max(err[f] / bound[f])) if f.any() else 0.0
    _report(what, bound_ratio_max=ratio, filled=int((cnt > 0).sum()))
    assert np.all(err <= bound), (what, ratio)
    assert np.all(got[cnt == 0] == 0) and np.all(ref[cnt == 0] == 0), what
    return ratio


def _tables_within(what, got, ref, cnt, k=0, kr=0):
    """set k of the raw dict `got` against set kr of `ref`, table by table"""
    for name in ("flux", "sky", "totals"):
        if ref.get(name) is not None:
            _within(f"{what}_{name}", got[name][k], ref[name][kr], cnt[name][0])


def _sum_within(what, raw, k, flux, sky, totals, cnt):
    """Σ_g of set k against the run's or the scan's own tables"""
    _within(f"{what}_flux", raw["flux"][k].sum(axis=0), flux, cnt["flux"][0].sum(axis=0))
    _within(f"{what}_totals", raw["totals"][k].sum(axis=0), totals, cnt["totals"][0].sum(axis=0))
    if sky is not None:
        _within(f"{what}_sky", raw["sky"][k].sum(axis=0), sky, cnt["sky"][0].sum(axis=0))


def _host(rep):
    from adiabatic_raytracer_amd import trees as T
    return T.replicates_raw(rep)


# ---- 1. the synthetic forest: exact

def _expected(rows, bins, att, groups, lo, sky_size):
    """the tables from rows and their device sky labels by np.bincount over (group, bin)"""
    from adiabatic_raytracer_amd import trees as T
    g = (rows[:, 0].astype(np.int64) - 1) % groups
    sp = rows[:, 1].astype(np.int64)
    p = rows[:, 8] * rows[:, 7]
    fb = T.hist_bins(rows[:, 3], NBINS)
    out = {}
    for name, lab, size in (("flux", np.where(fb >= 0, sp * NBINS + fb, -1), 2 * NBINS), ("sky", bins, sky_size), ("totals", sp, 2)):
        k = lab >= 0
        out[name] = np.bincount(g[k] * size + lab[k], weights=p[k], minlength=groups * size).reshape(groups, size)
    ev_g = (lo + np.arange(len(att))) % groups
    out["groups"] = np.stack([np.bincount(ev_g, minlength=groups),
                              np.bincount(ev_g, weights=att.astype(np.int64) - 1, minlength=groups)
                              + np.bincount(g[sp == 1], minlength=groups), np.zeros(groups)], axis=1)
    return out


@pytest.mark.parametrize("groups", [2, 5, 64])
def test_synthetic_forest_is_exact(groups):
    from adiabatic_raytracer_amd import trees as T
    lo, sky = 1003, dict(n_theta=2, n_phi=3, n_dw=1)
    eng = _engine()
    parts, nd, recs = _synthetic_forest()
    s, w5, back, fwd = parts
    att = s["attempts"].cpu().numpy()
    er = eng.event_rows(*parts, event_offset=lo, nbins=NBINS, sky=sky, return_bins=True)
    rows, bins = er["rows"].cpu().numpy(), er["bins"].cpu().numpy().astype(np.int64)
    pps = rows[:, 8] * rows[:, 7]
    assert len(rows) == (nd["is_final"] != 0).sum() and np.array_equal(pps, np.rint(pps)) and (bins < 0).any()
    got = _host(eng.event_replicates(*parts, groups, event_offset=lo, nbins=NBINS, sky=sky))
    want = _expected(rows, bins, att, groups, lo, 12)
    for name in ("flux", "sky", "totals"):
        assert np.array_equal(got[name][0].reshape(groups, -1), want[name]), name
        assert want[name].sum() > 0
    assert np.array_equal(got["groups"], want["groups"])
    assert got["groups"][:, 0].sum() == len(SIZES) and got["groups"][:, 1].sum() == er["totals"][4].item() + er["totals"][1].item()
    # rows_replicates says the same of the flux, the totals and the groups (its sky labels are numpy's own)
    ref = T.rows_replicates(rows, groups, NBINS, None, att, lo)
    for name in ("flux", "totals", "groups"):
        assert np.array_equal(got[name], ref[name]), name
    empty = want["groups"][:, 0] == 0
    assert empty.sum() == max(0, groups - len(SIZES))
    for name in ("flux", "sky", "totals"):
        assert not got[name][0][empty].any()
    # accumulated into: a second call doubles every table
    twice = eng.event_replicates(*parts, groups, event_offset=lo, nbins=NBINS, sky=sky)
    twice = _host(eng.event_replicates(*parts, groups, event_offset=lo, nbins=NBINS, sky=sky, rep=twice))
    for name in ("flux", "sky", "totals", "groups"):
        assert np.array_equal(twice[name], 2.0 * got[name]), name
    # a final record of tree 3 inside the range of tree 7: counted for the group of the tree it names, and skipped
    start = np.r_[0, np.cumsum(SIZES)]
    fin = np.flatnonzero(nd["is_final"] != 0)
    q = fin[(fin >= start[7] + 100)][0]
    bad = nd.copy()
    bad["tree"][q] = 3
    got_bad = _host(eng.event_replicates(s, w5, back, dict(fwd, nodes=recs(bad)), groups, event_offset=lo, nbins=NBINS, sky=sky))
    keep = np.arange(len(rows)) != np.searchsorted(fin, q)
    want_bad = _expected(rows[keep], bins[keep], att, groups, lo, 12)
    want_bad["groups"][(lo + 3) % groups, 2] = 1.0
    for name in ("flux", "sky", "totals"):
        assert np.array_equal(got_bad[name][0].reshape(groups, -1), want_bad[name]), name
    assert np.array_equal(got_bad["groups"], want_bad["groups"]) and not np.array_equal(got_bad["totals"], got["totals"])
    assert T.replicates_result(got_bad, 1)["misplaced"] == 1


# ---- 2. the run's tables at 600 flat events

def test_unit_weights_are_the_bincount_of_the_labels():
    sky = _sky()
    eng = _engine()
    parts = _unit(_pipeline("flat", 0, N))
    assert parts[3]["n_nodes"] > 1024  # several blocks, trees across wave and block boundaries
    er = eng.event_rows(*parts, nbins=NBINS, sky=sky, return_bins=True)
    rows, bins = er["rows"].cpu().numpy(), er["bins"].cpu().numpy().astype(np.int64)
    assert np.array_equal(rows[:, 8] * rows[:, 7], np.ones(len(rows))) and (bins < 0).any() and (bins >= 0).sum() > 500
    got = _host(eng.event_replicates(*parts, R, nbins=NBINS, sky=sky))
    want = _expected(rows, bins, parts[0]["attempts"].cpu().numpy(), R, 0, 2 * 6 * 11 * 4)
    for name in ("flux", "sky", "totals"):
        assert np.array_equal(got[name][0].reshape(R, -1), want[name]), name
    assert np.array_equal(got["groups"], want["groups"]) and want["groups"][:, 0].min() >= N // R
    assert np.array_equal(got["sky"][0].sum(axis=0), er["sky_hist"].cpu().numpy())  # the same bins as the run's map
    _report("unit_600", nodes=int(parts[3]["n_nodes"]), rows=int(len(rows)))


def test_run_events_tables_chunks_and_no_rows():
    from adiabatic_raytracer_amd import trees as T
    sky = _sky()
    kw = dict(replicates=R, nbins=NBINS, sky_map=sky)
    r = _run("flat", N, chunk=250, **kw)
    rep = r["replicates"]
    raw = rep["raw"]
    assert rep["R"] == R and rep["kind"] == "run" and rep["misplaced"] == 0 and rep["f_inx"] == r["f_inx"]
    assert raw["flux"].shape == (1, R, 2 * NBINS) and raw["sky"].shape == (1, R, 2, 6, 11, 4) and raw["totals"].shape == (1, R, 2)
    assert rep["a_g"].sum() == r["f_inx"] and rep["n_g"].sum() == N and rep["n_g"].min() >= N // R
    rows = r["rows_raw"]
    ref = T.rows_replicates(rows, R, NBINS, sky, _attempts(N), 0)
    cnt = _counts(rows, R, sky)
    assert np.array_equal(raw["groups"], ref["groups"])
    _tables_within("run_vs_rows", raw, ref, cnt)
    _sum_within("run_sum", raw, 0, r["flux_raw"], r["sky_raw"], r["totals"][2:4], cnt)
    assert rep["flux"].shape == (2, NBINS) and rep["sky_map"].shape == (2, 6, 11, 4) and rep["sum_weight_sln_prob"].shape == (2,)
    one = _run("flat", N, **kw)["replicates"]["raw"]
    norows = _run("flat", N, chunk=250, rows=False, **kw)
    assert norows["rows"] is None
    for what, other in (("one_chunk", one), ("no_rows", norows["replicates"]["raw"])):
        assert np.array_equal(other["groups"], raw["groups"])
        _tables_within(what, other, raw, cnt)
    # needs no errors=True, and changes nothing else
    plain = _run("flat", N, chunk=250, nbins=NBINS, sky_map=sky)
    assert set(r) - set(plain) == {"replicates"} and np.array_equal(plain["rows"], r["rows"], equal_nan=True)


# ---- 3. the scans' tables, on 600 events drawn under the halo tests' base model

def test_scan_tables_against_numpy_and_the_run():
    from adiabatic_raytracer_amd import trees as T
    from adiabatic_raytracer_amd.engine import nodes_to_numpy
    from test_gpu_halo_scan import SKY, _eng, _halos, _pipe
    eng = _eng()[0]
    base, models = _halos()
    parts = _pipe(0, N)
    s, w5, back, fwd = parts
    g0 = eng.params.g_agg
    g = [g0, 2.0 * g0, 0.5 * g0]
    kw = dict(nbins=NBINS, sky=SKY)
    er = eng.event_rows(*parts, **kw)
    sc = eng.event_reweight(*parts, g, mc_nodes=5, return_weights=True, **kw)
    hs = eng.event_halo_scan(*parts, base, models, return_ratio=True, **kw)
    run = _host(eng.event_replicates(*parts, R, **kw))
    crep = _host(eng.event_replicates(*parts, R, kind="coupling", node_factor=sc["weights"], event_factor=sc["back"], **kw))
    hrep = _host(eng.event_replicates(*parts, R, kind="halo", event_factor=hs["ratio"], **kw))
    assert crep["flux"].shape == hrep["flux"].shape == (3, R, 2 * NBINS) and crep["sky"].shape == (3, R, 2, 6, 11, 4)
    assert np.array_equal(crep["groups"], run["groups"]) and np.array_equal(hrep["groups"], run["groups"])
    rows = er["rows"].cpu().numpy()
    nodes = nodes_to_numpy(fwd["nodes"])
    fin = np.flatnonzero(nodes["is_final"] != 0)
    ev = rows[:, 0].astype(np.int64) - 1
    assert len(fin) == len(rows) and np.array_equal(nodes["tree"][fin], ev)
    W, B, ratio = (v.cpu().numpy() for v in (sc["weights"], sc["back"], hs["ratio"]))
    cnt = _counts(rows, R, SKY)
    att = s["attempts"].cpu().numpy()
    scans = {k: {n: v.cpu().numpy() for n, v in d.items() if n in ("flux", "sky", "totals")} for k, d in (("coupling", sc), ("halo", hs))}
    for kind, rep, power in (("coupling", crep, lambda k: (W[k, fin] * B[k, ev]) * rows[:, 7]),
                             ("halo", hrep, lambda k: (rows[:, 8] * rows[:, 7]) * ratio[k, ev])):
        for k in range(3):
            mine = rows.copy()
            mine[:, 7], mine[:, 8] = power(k), 1.0  # (the powers of set k as the device forms them; 1.0 p = p)
            ref = T.rows_replicates(mine, R, NBINS, SKY, att, 0)
            assert np.array_equal(rep["groups"], ref["groups"])
            _tables_within(f"{kind}_{k}_vs_numpy", rep, ref, cnt, k=k)
            own = scans[kind]
            _sum_within(f"{kind}_{k}_sum", rep, k, own["flux"][k], own["sky"][k], own["totals"][k, :2], cnt)
    # g_k = g0 and the base model: the run's own replicates
    _tables_within("halo_base_vs_run", hrep, run, cnt, k=0)
    _tables_within("coupling_g0_vs_run", crep, run, cnt, k=0)


def test_run_events_scans_get_replicates():
    from test_gpu_halo_scan import SKY, _eng, _halos
    eng = _eng()[0]
    base, models = _halos()
    g0 = eng.params.g_agg
    g = [g0, 2.0 * g0, 0.5 * g0]
    r = _np(eng.run_events(200, seed=SEED, chunk=96, sky_map=SKY, halo=base, halos=models, couplings=g, replicates=R))
    plain = _np(eng.run_events(200, seed=SEED, chunk=96, sky_map=SKY, halo=base, halos=models, couplings=g))
    assert set(r) - set(plain) == {"replicates"}
    cnt = _counts(r["rows_raw"], R, SKY)
    for key in ("coupling_scan", "halo_scan"):
        assert set(r[key]) - set(plain[key]) == {"replicates"} and "weights" not in r[key]["raw"] and "ratio" not in r[key]["raw"]
        rep = r[key]["replicates"]
        assert rep["raw"]["flux"].shape == (3, R, 2 * NBINS) and rep["flux"].shape == (3, 2, NBINS) and rep["sky_map"].shape == (3, 2, 6, 11, 4)
        assert np.array_equal(rep["a_g"], r["replicates"]["a_g"]) and rep["a_g"].sum() == r["f_inx"]
        own = r[key]["raw"]
        for k in range(3):
            _sum_within(f"run_{key}_{k}_sum", rep["raw"], k, own["flux"][k], own["sky"][k], own["totals"][k, :2], cnt)
    # the worked example runs: a crossing inside the scanned couplings, with an error
    from adiabatic_raytracer_amd import trees as T
    curve = r["coupling_scan"]["sum_weight_sln_prob"][:, 1]
    out = T.coupling_crossing(r["coupling_scan"], float(np.sqrt(curve[0] * curve[1])))
    assert g0 < out["value"] < 2.0 * g0 and out["sigma"] > 0 and out["groups_used"] == R
    _report("coupling_crossing_200", g=float(out["value"]), sigma=float(out["sigma"]))


# ---- 4. cyclotron, 65 events

def test_cyclotron_65_sums_to_the_rows_tables():
    sky = dict(n_theta=3, n_phi=4, n_dw=1)
    r = _np(_engine().run_events(65, seed=SEED, cyclotron=True, saveMode=1, replicates=5, nbins=NBINS, sky_map=sky))
    rows = r["rows_raw"]
    assert (rows[:, 14] > 0).any()  # column 8 carries exp(-τ)
    raw = r["replicates"]["raw"]
    cnt = _counts(rows, 5, sky)
    _sum_within("cyclotron_65_sum", raw, 0, r["flux_raw"], r["sky_raw"], r["totals"][2:4], cnt)
    assert r["replicates"]["a_g"].sum() == r["f_inx"] and r["replicates"]["n_g"].sum() == 65


# ---- 5. main_runner_tree, 48 events

def test_main_runner_tree_paths():
    import adiabatic_raytracer_amd as A
    p = _params("flat")
    sky = dict(n_theta=4, n_phi=6, n_dw=1)
    info_d, info_h, info_0 = {}, {}, {}
    rows = A.trees.main_runner_tree(p, 49, device_events=True, replicates=4, sky_map=sky, run_info=info_d)
    A.trees.main_runner_tree(p, 49, device_trees=True, replicates=4, sky_map=sky, run_info=info_h)
    A.trees.main_runner_tree(p, 49, device_events=True, sky_map=sky, run_info=info_0)
    assert set(info_d) - set(info_0) == set(info_h) - set(info_0) == {"replicates"}
    run = _np(_engine().run_events(48, seed=SEED, replicates=4, nbins=NBINS, sky_map=sky))["replicates"]
    cnt = _counts(rows, 4, sky)  # (column 7 is divided by f_inx there: the counts do not read it)
    for what, info in (("main_runner_device", info_d), ("main_runner_host", info_h)):
        rep = info["replicates"]
        assert rep["f_inx"] == run["f_inx"] == info["f_inx"] and np.array_equal(rep["raw"]["groups"], run["raw"]["groups"])
        _tables_within(what, rep["raw"], run["raw"], cnt)


# ---- 6. off by default, and the cap

def test_off_by_default_and_the_cap(monkeypatch):
    from adiabatic_raytracer_amd.engine import Engine
    from test_gpu_halo_scan import _eng, _halos
    eng = _eng()[0]
    base, models = _halos()
    r = eng.run_events(20, seed=SEED, sky_map={}, halo=base, halos=models, couplings=[eng.params.g_agg], errors=True)
    assert "replicates" not in r and "replicates" not in r["coupling_scan"] and "replicates" not in r["halo_scan"]
    assert not any("replicates" in str(k) for d in (r, r["coupling_scan"], r["halo_scan"], r["coupling_scan"]["raw"]) for k in d)

    def no_launch(*a, **k):
        raise AssertionError("work was done before the cap was checked")

    monkeypatch.setattr(Engine, "sample", no_launch)
    big = dict(n_theta=64, n_phi=128, n_dw=16, dw_range=(-1.0, 1.0))
    with pytest.raises(ValueError, match="drop the sky map from the scan or lower R"):
        eng.run_events(10, couplings=[eng.params.g_agg] * 32, replicates=64, sky_map=big)
    with pytest.raises(ValueError, match="drop the sky map from the scan or lower R"):
        eng.run_events(10, halo=base, halos=[base] * 32, replicates=64, sky_map=big)
