"""Emission maps on the GPU (art_event_origin_device, Engine.event_origin, run_events(origin_map=),
main_runner_tree(origin_map=)) against np.bincount over the labels of Engine.event_rows (the observer bin) and
trees.origin_bins (the origin bin), and against trees.rows_origin on the rows the runs return.

Unit weights and integer powers: every table entry is an integer below 2^53, so the device tables are
np.array_equal to numpy's, whatever the order of the adds.

A weighted bin is a sum of the same non-negative terms in another order: two such sums differ by at most
2 (cnt + 1) u max(got, ref) with cnt the bin's rows and u = 2^-53 (tests/test_gpu_event_rows.py); an empty bin is 0.
The sum over the groups of a bin adds at most cnt - 1 roundings more, which the same bound with the bin's rows of
all groups covers (tests/test_gpu_replicates.py). The tables of two runs of the same events differ the same way,
since the order of the hardware adds is not fixed: "off by default" therefore holds the rows and the counts
bit-equal and the weighted tables of the two runs within the bound.

The device's acos and atan2 are within 1 ulp of numpy's (tests/test_gpu_event_rows.py), so a point's device label
is numpy's unless a coordinate lies within a few ulp of an edge: the labels are compared for every row whose numpy
coordinates lie more than 4 ulp from every edge, at most 2 rows may be excluded and more than 500 must be compared
(the chance that one row falls that close is about 1e-13; the cap keeps the test from hiding a wrong rule).

ART_PARITY_REPORT=path collects the JSON lines the tests print (profiles/origin_parity.jsonl; DESIGN.md §3,
"Emission maps")."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_event_moments import SIZES, _synthetic_forest
from test_gpu_event_rows import SEED, U, _engine, _np, _params, _pipeline, _run, _unit
from test_gpu_replicates import _within

pytestmark = pytest.mark.gpu

N, R, NBINS = 600, 7, 50
OBS = dict(n_theta=2, n_phi=3)


def _report(what, **vals):
    line = json.dumps({"test": "event_origin", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _spec(origin, observer=None, cfg="flat"):
    from adiabatic_raytracer_amd import trees as T
    return T.origin_spec(origin, observer, _params(cfg))


def _labels(rows, sky_bins, spec):
    """the flat table label of each row from its observer label (event_rows' sky bin at the observer's axes) and
    trees.origin_bins of its columns 9 to 11; -1: not counted"""
    from adiabatic_raytracer_amd import trees as T
    n_origin = spec["n_r"] * spec["n_theta"] * spec["n_phi"]
    ob = T.origin_bins(rows[:, 9], rows[:, 10], rows[:, 11], spec)
    return np.where((sky_bins >= 0) & (ob >= 0), sky_bins * n_origin + ob, -1)


def _bincount(labels, p, spec, g=None, groups=None):
    size = int(np.prod(spec["shape"]))
    k = labels >= 0
    if groups is None:
        return np.bincount(labels[k], weights=p[k], minlength=size).reshape(spec["shape"])
    return np.bincount(g[k] * size + labels[k], weights=p[k], minlength=groups * size).reshape((groups,) + spec["shape"])


def _unit_rows(rows):
    unit = np.array(rows, np.float64)
    unit[:, 7] = unit[:, 8] = 1.0
    return unit


# ---- 1. the synthetic forest: exact

def _planted_sample(parts, spec):
    """the synthetic forest's sample with its x overwritten: bin centres, and the planted points -- r on r_lo with
    z = 0, x = y = 0, r on r_hi, a NaN, r outside the range"""
    import torch
    s = parts[0]
    n = len(SIZES)
    centre = lambda r, c, ph: [r * np.sqrt(1 - c * c) * np.cos(ph), r * np.sqrt(1 - c * c) * np.sin(ph), r * c]  # noqa: E731
    pts = np.array([centre(11.25, 0.0, np.pi / 4), [3.0, 4.0, 0.0], [0.0, 0.0, 7.5], centre(23.75, -2.0 / 3.0, -0.75 * np.pi),
                    [10.0, 20.0, 20.0], [np.nan, 1.0, 1.0], centre(11.25, 2.0 / 3.0, 0.75 * np.pi),
                    centre(23.75, 2.0 / 3.0, -np.pi / 4), [1.0, 2.0, 2.0]])
    assert pts.shape == (n, 3)
    x = torch.from_numpy(np.ascontiguousarray(pts.T).reshape(-1)).to(s["x"].device)
    return (dict(s, x=x),) + tuple(parts[1:])


@pytest.mark.parametrize("frame", ["rotation", "magnetic"])
def test_synthetic_forest_is_exact(frame):
    lo = 1003
    eng = _engine()
    parts, nd, recs = _synthetic_forest()
    spec = _spec(dict(n_r=2, n_theta=3, n_phi=4, r_range=(5.0, 30.0), frame=frame), OBS)
    assert spec["shape"] == (2, 2, 3, 2, 3, 4)
    parts = _planted_sample(parts, spec)
    s, w5, back, fwd = parts
    er = eng.event_rows(*parts, event_offset=lo, nbins=NBINS, sky=dict(OBS, n_dw=1), return_bins=True)
    rows, sky_bins = er["rows"].cpu().numpy(), er["bins"].cpu().numpy().astype(np.int64)
    p = rows[:, 8] * rows[:, 7]
    fin = np.flatnonzero(nd["is_final"] != 0)
    assert len(rows) == len(fin) and np.array_equal(p, np.rint(p)) and (sky_bins < 0).any()
    labels = _labels(rows, sky_bins, spec)
    assert ((sky_bins >= 0) & (labels < 0)).any() and (labels >= 0).sum() > 100  # the NaN and the r outside drop rows
    if frame == "rotation":  # the planted points' bins: r_lo in the first r bin, r_hi in the last, x = y = 0 at the pole
        from adiabatic_raytracer_amd import trees as T
        x = s["x"].cpu().numpy().reshape(3, -1)
        assert T.origin_bins(*x, spec).tolist() == [(0 * 3 + 1) * 4 + 2, (0 * 3 + 1) * 4 + 2, (0 * 3 + 2) * 4 + 2,
                                                    (1 * 3 + 0) * 4 + 0, (1 * 3 + 2) * 4 + 2, -1, (0 * 3 + 2) * 4 + 3,
                                                    (1 * 3 + 2) * 4 + 1, -1]
    want = _bincount(labels, p, spec)
    assert want.sum() > 0
    got = {}
    for mode in (0, 1, 2):
        out = eng.event_origin(*parts, dict(spec, mode=mode), event_offset=lo, return_bins=True)
        got[mode] = out["hist"].cpu().numpy()
        assert got[mode].shape == spec["shape"] and np.array_equal(got[mode], want), mode
        assert out["misplaced"].item() == 0
        bins, power = out["bins"].cpu().numpy(), out["power"].cpu().numpy()
        full = np.full(len(nd), -1, np.int64)
        full[fin] = labels
        pw = np.zeros(len(nd))
        pw[fin] = p
        assert bins.dtype == np.int32 and np.array_equal(bins, full) and np.array_equal(power, pw), mode
    assert np.array_equal(got[1], got[2])
    # accumulated into: a second call doubles the table; a table of other axes is refused
    twice = eng.event_origin(*parts, spec, event_offset=lo)
    twice = eng.event_origin(*parts, spec, event_offset=lo, hist=twice)
    assert np.array_equal(twice["hist"].cpu().numpy(), 2.0 * want)
    with pytest.raises(ValueError, match="other axes or other groups"):
        eng.event_origin(*parts, dict(spec, n_phi=5, shape=(2, 2, 3, 2, 3, 5)), event_offset=lo, hist=twice)
    with pytest.raises(ValueError, match="other axes or other groups"):
        eng.event_origin(*parts, spec, event_offset=lo, hist=twice, groups=2)
    # a final record of tree 3 inside the range of tree 7: skipped and counted
    start = np.r_[0, np.cumsum(SIZES)]
    q = fin[(fin >= start[7] + 100) & (labels >= 0)][0]  # (one that the table counts)
    bad = nd.copy()
    bad["tree"][q] = 3
    got_bad = eng.event_origin(s, w5, back, dict(fwd, nodes=recs(bad)), spec, event_offset=lo, return_bins=True)
    keep = np.arange(len(rows)) != np.searchsorted(fin, q)
    assert got_bad["misplaced"].item() == 1 and got_bad["bins"][q].item() == -1 and got_bad["power"][q].item() == 0
    assert np.array_equal(got_bad["hist"].cpu().numpy(), _bincount(labels[keep], p[keep], spec))
    assert labels[~keep][0] >= 0 and not np.array_equal(got_bad["hist"].cpu().numpy(), want)
    # the groups: g = (event_offset + tree) mod R; R = 64 takes the table out of LDS
    g_rows = (rows[:, 0].astype(np.int64) - 1)
    for groups in (2, 5, 64):
        out = eng.event_origin(*parts, spec, groups=groups, event_offset=lo)
        tab = out["hist"].cpu().numpy()
        assert tab.shape == (groups,) + spec["shape"] and out["misplaced"].item() == 0
        assert np.array_equal(tab, _bincount(labels, p, spec, g_rows % groups, groups)), groups
        assert np.array_equal(tab.sum(axis=0), want)
        empty = np.bincount((lo + np.arange(len(SIZES))) % groups, minlength=groups) == 0
        assert empty.sum() == max(0, groups - len(SIZES)) and not tab[empty].any()
        for mode in (1, 2) if groups * want.size <= 8192 else (2,):
            assert np.array_equal(eng.event_origin(*parts, dict(spec, mode=mode), groups=groups, event_offset=lo)["hist"].cpu().numpy(), tab)
    with pytest.raises(Exception, match="LDS budget"):
        eng.event_origin(*parts, dict(spec, mode=1), groups=64, event_offset=lo)


# ---- 2. 600 flat events, unit weights

def _ulps_from_edges(v, edges):
    """the distance of each v from the nearest of `edges`, in units of the spacing of doubles there"""
    v = np.asarray(v, np.float64)[:, None]
    e = np.asarray(edges, np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        return np.min(np.abs(v - e) / np.spacing(np.maximum(np.abs(v), np.abs(e))), axis=1)


def test_unit_weights_labels_and_the_sky_map():
    from adiabatic_raytracer_amd import trees as T
    eng = _engine()
    parts = _unit(_pipeline("flat", 0, N))
    assert parts[3]["n_nodes"] > 1024  # several blocks, trees across wave and block boundaries
    obs = dict(n_theta=6, n_phi=11)
    er = eng.event_rows(*parts, nbins=NBINS, sky=dict(obs, n_dw=1), return_bins=True)
    rows, sky_bins = er["rows"].cpu().numpy(), er["bins"].cpu().numpy().astype(np.int64)
    assert np.array_equal(rows[:, 8] * rows[:, 7], np.ones(len(rows))) and len(rows) > 900
    from adiabatic_raytracer_amd.engine import nodes_to_numpy
    nodes_final = np.flatnonzero(nodes_to_numpy(parts[3]["nodes"])["is_final"] != 0)
    assert len(nodes_final) == len(rows)
    r_all = np.linalg.norm(rows[:, 9:12], axis=1)
    # (the rows of one event share its point, so a quantile of the rows' r is often some event's r itself: moved off it)
    r_range = tuple(float(v) * f for v, f in zip(np.quantile(r_all, [0.05, 0.9]), (1.0001, 0.9999)))
    for origin in (dict(n_r=2, n_theta=5, n_phi=7, theta_axis="theta", r_range=r_range), dict(n_r=3, n_theta=4, n_phi=9, r_range=r_range,
                                                                                                 frame="rotation"), {}):
        spec = _spec(origin, obs)
        n_origin = spec["n_r"] * spec["n_theta"] * spec["n_phi"]
        out = eng.event_origin(*parts, spec, return_bins=True)
        tab, dev = out["hist"].cpu().numpy(), out["bins"].cpu().numpy().astype(np.int64)[nodes_final]
        assert out["misplaced"].item() == 0
        # the table is the bincount of the labels the kernel handed out, and their observer part is the sky map's label
        assert np.array_equal(tab, _bincount(dev, np.ones(len(rows)), spec))
        assert np.array_equal(dev[dev >= 0] // n_origin, sky_bins[dev >= 0]) and not (dev[sky_bins < 0] >= 0).any()
        # the origin part against numpy's, away from the edges
        counted = sky_bins >= 0
        dev_ob = np.where(dev >= 0, dev % n_origin, -1)[counted]
        coords = T.origin_coordinates(rows[:, 9], rows[:, 10], rows[:, 11], spec)
        edges = T.origin_map_edges(spec)[2:]
        near = np.zeros(len(rows), bool)
        for v, e in zip(coords, edges):
            near |= _ulps_from_edges(v, e[np.isfinite(e)]) <= 4
        far = ~near[counted]
        ref_ob = T.origin_bins(rows[:, 9], rows[:, 10], rows[:, 11], spec)[counted]
        assert (~far).sum() <= 2 and far.sum() > 500
        assert np.array_equal(dev_ob[far], ref_ob[far])
        if spec["r_range"] is not None:
            assert (ref_ob < 0).sum() > 50  # the range drops rows
        _report("unit_600_labels", origin=str(origin), rows=int(len(rows)), compared=int(far.sum()), excluded=int((~far).sum()),
                dropped=int((ref_ob < 0).sum()), filled=int((tab > 0).sum()))
    # (the last spec: one r bin, no range) summed over its origin axes the table is the sky map of the observer's axes
    assert spec["n_r"] == 1 and spec["r_range"] is None
    sky = er["sky_hist"].cpu().numpy()
    assert np.array_equal(tab.sum(axis=(3, 4, 5)), sky[..., 0])
    assert np.array_equal(tab.sum(axis=(1, 2, 3, 4, 5)), er["totals"].cpu().numpy()[2:4])
    # and without observer axes the extents are 1 and the table is the joint one summed over them
    alone = eng.event_origin(*parts, _spec({}))["hist"].cpu().numpy()
    assert alone.shape == (2, 1, 1, 1, 16, 32) and np.array_equal(alone[:, 0, 0], tab.sum(axis=(1, 2)))


# ---- 3. run_events(600, origin_map=...)

def _origin_map():
    """2 x 5 x 7 over a range of r that holds most of the run's events and drops some, with an observer of 2 x 3"""
    rows = _run("flat", N)["rows_raw"]
    lo, hi = np.quantile(np.linalg.norm(rows[:, 9:12], axis=1), [0.05, 0.9])
    return dict(n_r=2, n_theta=5, n_phi=7, r_range=(float(lo), float(hi)), observer=dict(OBS))


def test_run_events_chunks_no_rows_and_replicates():
    from adiabatic_raytracer_amd import trees as T
    om = _origin_map()
    r = _run("flat", N, chunk=250, origin_map=om)
    o = r["origin"]
    spec = o["spec"]
    assert set(o) == {"map", "raw", "edges", "spec", "misplaced"} and o["misplaced"] == 0
    assert o["raw"].shape == o["map"].shape == spec["shape"] == (2, 2, 3, 2, 5, 7) and len(o["edges"]) == 5
    assert np.array_equal(o["map"], o["raw"] / float(r["f_inx"]))
    rows = r["rows_raw"]
    ref, cnt = T.rows_origin(rows, spec), T.rows_origin(_unit_rows(rows), spec)
    assert 0 < cnt.sum() < len(rows) and cnt.max() > 3
    ratios = {"run_vs_rows": _within("origin_run_vs_rows", o["raw"], ref, cnt)}
    one = _run("flat", N, origin_map=om)["origin"]["raw"]
    norows = _run("flat", N, chunk=250, rows=False, origin_map=om)
    assert norows["rows"] is None
    ratios["one_chunk"] = _within("origin_one_chunk", one, o["raw"], cnt)
    ratios["no_rows"] = _within("origin_no_rows", norows["origin"]["raw"], o["raw"], cnt)
    # replicates=7: the group tables, and their sum against the run's table
    r7 = _run("flat", N, chunk=250, origin_map=om, replicates=R)
    rep = r7["origin"]["replicates"]
    assert rep["raw"].shape == (R,) + spec["shape"] and rep["R"] == R and rep["f_inx"] == r7["f_inx"] == r["f_inx"]
    assert np.array_equal(rep["n_g"], r7["replicates"]["n_g"]) and np.array_equal(rep["a_g"], r7["replicates"]["a_g"])
    ratios["groups_vs_rows"] = _within("origin_groups_vs_rows", rep["raw"], T.rows_origin(rows, spec, R=R),
                                       T.rows_origin(_unit_rows(rows), spec, R=R))
    ratios["groups_sum"] = _within("origin_groups_sum", rep["raw"].sum(axis=0), r7["origin"]["raw"], cnt)
    jk = T.origin_jackknife(r7["origin"], lambda m: T.emission_profile(m, spec)[0].sum(axis=1))
    assert jk["groups_used"] == R and jk["value"].shape == (5,) and np.all(jk["sigma"][jk["value"] > 0] > 0)
    _report("origin_600", bound_ratio_max=max(ratios.values()), **ratios, rows=int(len(rows)), counted=int(cnt.sum()))
    # off by default: one more key, and nothing else changes (the order of the adds aside; module docstring)
    plain = _run("flat", N, chunk=250)
    assert set(r) - set(plain) == {"origin"}
    assert np.array_equal(plain["rows"], r["rows"], equal_nan=True) and np.array_equal(plain["rows_raw"], rows, equal_nan=True)
    assert plain["f_inx"] == r["f_inx"] and plain["n_rows"] == r["n_rows"] and plain["n_photon_rows"] == r["n_photon_rows"]
    assert np.array_equal(plain["totals"][[0, 1, 4, 5]], r["totals"][[0, 1, 4, 5]])
    fb = T.hist_bins(rows[:, 3], NBINS)
    fcnt = np.bincount(((rows[:, 1] != 0) * NBINS + fb)[fb >= 0], minlength=2 * NBINS)
    _within("origin_off_flux", r["flux_raw"].reshape(-1), plain["flux_raw"].reshape(-1), fcnt)
    _within("origin_off_totals", r["totals"][2:4], plain["totals"][2:4], np.array([(rows[:, 1] == 0).sum(), (rows[:, 1] == 1).sum()]))


def test_run_events_exact_is_the_fraction_sum():
    from adiabatic_raytracer_amd import trees as T
    om = dict(n_r=1, n_theta=3, n_phi=4, observer=dict(OBS))
    eng = _engine()
    runs = {c: eng.run_events(200, seed=SEED, chunk=c, origin_map=om, exact=True) for c in (250, None, 96)}
    r = runs[250]
    x = r["exact"]
    spec = r["origin"]["spec"]
    raw = x["origin_raw"].cpu().numpy()
    assert raw.shape == spec["shape"] and tuple(x["acc"]["origin"].shape) == (1,) + spec["shape"] + (66,)
    rows = r["rows_raw"].cpu().numpy()
    sb = T.sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], n_dw=1, **OBS)
    labels = _labels(rows, sb, spec)
    p = rows[:, 8] * rows[:, 7]
    want = np.zeros(raw.size)
    for b in range(raw.size):
        want[b] = float(sum((Fraction(float(v)) for v in p[labels == b]), Fraction(0)))
    assert (labels >= 0).sum() > 300 and np.array_equal(raw.reshape(-1), want)
    assert np.array_equal(x["origin_map"].cpu().numpy(), raw / float(max(r["f_inx"], 1)))
    for c in (None, 96):
        assert np.array_equal(runs[c]["exact"]["origin_raw"].cpu().numpy(), raw), c
        assert np.array_equal(runs[c]["exact"]["acc"]["origin"].cpu().numpy(), x["acc"]["origin"].cpu().numpy()), c
    # the float table is within the order bound of the exact one
    _within("origin_exact_vs_float", r["origin"]["raw"], raw, T.rows_origin(_unit_rows(rows), spec))
    # exact_merge carries the origin accumulators: two halves of the run add up to the whole
    a = eng.run_events(100, seed=SEED, origin_map=om, exact=True)["exact"]["acc"]
    b = eng.run_events(100, seed=SEED, event_offset=100, origin_map=om, exact=True)["exact"]["acc"]
    assert np.array_equal(T.exact_finish(T.exact_merge([a, b]))["origin_raw"], raw)
    plain = eng.run_events(200, seed=SEED, exact=True)
    assert "origin_raw" not in plain["exact"] and plain["exact"]["acc"].get("origin") is None
    # off by default, held exactly: the origin launches leave every other table's exact sums bit for bit what they are
    for c in (250, None, 96):
        for name in ("flux_raw", "totals_raw"):
            assert np.array_equal(runs[c]["exact"][name].cpu().numpy(), plain["exact"][name].cpu().numpy()), (c, name)
        assert np.array_equal(runs[c]["rows_raw"].cpu().numpy(), plain["rows_raw"].cpu().numpy(), equal_nan=True), c


# ---- 4. cyclotron, 65 events

def test_cyclotron_65_sums_to_the_rows_powers():
    from adiabatic_raytracer_amd import trees as T
    om = dict(n_r=1, n_theta=3, n_phi=4, observer=dict(n_theta=3, n_phi=4))
    r = _np(_engine().run_events(65, seed=SEED, cyclotron=True, saveMode=1, origin_map=om))
    rows = r["rows_raw"]
    assert (rows[:, 14] > 0).any()  # column 8 carries exp(-τ)
    spec = r["origin"]["spec"]
    cnt = T.rows_origin(_unit_rows(rows), spec)
    _within("origin_cyclotron_65", r["origin"]["raw"], T.rows_origin(rows, spec), cnt)
    # summed over its origin axes it is the run's sky map of the same axes, and over everything the species' totals
    sky = _np(_engine().run_events(65, seed=SEED, cyclotron=True, saveMode=1, sky_map=dict(n_theta=3, n_phi=4, n_dw=1)))["sky_raw"]
    _within("origin_cyclotron_65_sky", r["origin"]["raw"].sum(axis=(3, 4, 5)), sky[..., 0], cnt.sum(axis=(3, 4, 5)))
    _within("origin_cyclotron_65_totals", r["origin"]["raw"].sum(axis=(1, 2, 3, 4, 5)), r["totals"][2:4], cnt.sum(axis=(1, 2, 3, 4, 5)))


# ---- 5. main_runner_tree, 300 events

def test_main_runner_tree_paths(monkeypatch):
    import adiabatic_raytracer_amd as A
    T = A.trees
    p = _params("flat")
    om = dict(n_r=1, n_theta=4, n_phi=6, observer=dict(OBS))
    seen = []
    real = T.rank_vector

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append((len(out[0]), len(out[1]), k.get("origin") is not None))
        return out

    monkeypatch.setattr(T, "rank_vector", spy)
    info_0 = {}
    T.main_runner_tree(p, 301, device_events=True, run_info=info_0)
    old = seen[-1]
    assert old == (2 * NBINS + 4, 1, False) and "origin" not in info_0  # pack_totals' vector alone, as before
    for what, kw in (("host", {}), ("device_trees", dict(device_trees=True)), ("device_events", dict(device_events=True))):
        info = {}
        rows = T.main_runner_tree(p, 301, origin_map=om, run_info=info, **kw)
        o = info["origin"]
        spec = o["spec"]
        assert set(info) - set(info_0) == {"origin"} and o["raw"].shape == spec["shape"] == (2, 2, 3, 1, 4, 6)
        assert seen[-1] == (old[0] + o["raw"].size, 2, True)
        assert np.array_equal(o["map"], o["raw"] / float(info["f_inx"]))
        raw_rows = np.array(rows)
        raw_rows[:, 7] = rows[:, 7] * float(info["f_inx"])  # (column 7 comes back divided by f_inx)
        _within(f"origin_main_runner_{what}", o["raw"], T.rows_origin(raw_rows, spec), T.rows_origin(_unit_rows(rows), spec))
