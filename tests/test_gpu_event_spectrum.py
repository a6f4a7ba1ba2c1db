"""The event power spectrum on the GPU (art_event_spectrum_device, Engine.event_spectrum, run_events(spectrum=),
main_runner_tree(spectrum=)) against trees.rows_spectrum and numpy on the rows that Engine.event_rows returns for the
same forests.

Integer powers: every X, every X² and every table entry is an integer below 2^53, so the device tables are
np.array_equal to numpy's, whatever the order of the adds, and the lists are equal bit for bit.

A real run. X of an event is formed by the same adds in the same order on the device (node order) and in numpy (row
order: the rows are the final nodes in node order), so it is expected to be the same double; the tests allow 4 ulp and
report whether it is bit-equal. An event whose X lies within 4 ulp of a bin edge may then fall on either side: such
events are left out of the comparison of `count` and must be at most 0.1 % of the positive events (the edges are 2^49
ulp apart: the expected number is 0). A bin's sum and sum_sq, and the totals S and Q, are sums of the same non-negative
terms in another order: two such sums differ by at most 2 (n + 1) u of the larger, with n the terms and u = 2^-53
(tests/test_gpu_event_rows.py).

ART_PARITY_REPORT=path collects the JSON lines the tests print (profiles/event_spectrum_parity.jsonl; DESIGN.md §3,
"Event power spectrum")."""
import json
import os

import numpy as np
import pytest

from test_gpu_event_moments import SIZES
from test_gpu_event_rows import SEED, U, _engine, _np, _params, _run

pytestmark = pytest.mark.gpu

N = 600
LO = 1003
TABLES = ("count", "sum", "sum_sq", "totals")
RUN_KEYS = {"rows", "flux", "f_inx", "sum_weight_sln_prob", "n_rows", "n_photon_rows", "totals", "flux_raw", "rows_raw"}

_cache = {}


def _report(what, **vals):
    line = json.dumps({"test": "event_spectrum", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _raw(spec):
    from adiabatic_raytracer_amd import trees as T
    return T.spectrum_raw(spec)


def _ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


# ---- the forests built here, after test_gpu_event_moments._synthetic_forest

def _build(sizes, weight=None, final=None, species=None, sln=None):
    """(sample, weight5, back, forward) uploaded from numpy records, the forward records, the uploader of records and
    sln_prob per event. Defaults: integer weights 1 .. 19 and sln_prob 1 .. 3, half of the records final, both species."""
    import torch
    from adiabatic_raytracer_amd.trees import NODE_DTYPE
    eng = _engine()
    rng = np.random.default_rng(1769)
    sizes = np.asarray(sizes, np.int64)
    n, nn = len(sizes), int(sizes.sum())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    nd = np.zeros(nn, NODE_DTYPE)
    nd["tree"] = np.repeat(np.arange(n), sizes)
    nd["is_final"] = rng.random(nn) < 0.5 if final is None else final
    nd["species"] = rng.integers(0, 2, nn) if species is None else species
    nd["weight"] = rng.integers(1, 20, nn) if weight is None else weight
    nd["k_end"] = rng.normal(size=(nn, 3)) * 1e-5
    nd["x_end"] = rng.normal(size=(nn, 3)) * 100.0
    nd["u7_end"] = rng.normal(size=nn) * 1e-11
    bk = np.zeros(n, NODE_DTYPE)
    bk["tree"], bk["prob"], bk["weight"] = np.arange(n), 1.0, 1.0
    w5 = np.zeros((5, n))
    w5[0], w5[2] = rng.uniform(-1, 1, n), rng.integers(1, 4, n) if sln is None else sln  # cos_w, sln_prob
    sample = {"x": up(rng.normal(size=3 * n) * 30.0), "k_init": up(rng.normal(size=3 * n) * 1e-5),
              "erg": up(np.full(n, 1e-5)), "attempts": up(rng.integers(1, 6, n).astype(np.int32))}
    recs = lambda a: up(a.view(np.uint8).reshape(len(a), NODE_DTYPE.itemsize))  # noqa: E731
    back = {"nodes": recs(bk), "counts": up(np.ones(n, np.int32)), "n_nodes": n}
    fwd = {"nodes": recs(nd), "node_start": up(np.r_[0, np.cumsum(sizes)].astype(np.int64)),
           "counts": up(sizes.astype(np.int32)), "infos": up(np.zeros(n, np.int32)), "n_nodes": nn}
    return (sample, up(w5), back, fwd), nd, recs, w5[2].copy()


def _forest603():
    """603 trees whose sizes cycle through SIZES, with the rows of event_rows (event_offset = LO)"""
    if "f603" not in _cache:
        sizes = [SIZES[e % len(SIZES)] for e in range(603)]
        parts, nd, recs, sln = _build(sizes)
        rows = _engine().event_rows(*parts, event_offset=LO, nbins=50)["rows"].cpu().numpy()
        rows.setflags(write=False)
        _cache["f603"] = (parts, nd, recs, sln, np.asarray(sizes), rows)
    return _cache["f603"]


# ---- 1. the synthetic forest: exact

def test_synthetic_forest_input():
    from adiabatic_raytracer_amd import trees as T
    parts, nd, recs, sln, sizes, rows = _forest603()
    pps = rows[:, 8] * rows[:, 7]
    assert len(rows) == (nd["is_final"] != 0).sum() and np.array_equal(pps, np.rint(pps)) and set(rows[:, 1]) == {0.0, 1.0}
    X = T.rows_spectrum(rows, 0, 0, event_lo=LO, n_events=603)
    ph = np.bincount(rows[rows[:, 1] == 1, 0].astype(np.int64) - 1 - LO, weights=pps[rows[:, 1] == 1], minlength=603)
    assert X["totals"][0, 1, 1] == np.count_nonzero(ph > 0) > 256  # more events than the longest list
    assert len(np.unique(ph[ph > 0])) < np.count_nonzero(ph > 0)  # at least two events share a photon power exactly
    has_row = np.bincount(rows[:, 0].astype(np.int64) - 1 - LO, minlength=603) > 0
    assert np.count_nonzero(~has_row) >= 2  # trees without a final row (the empty ones among them)
    assert ph.max() ** 2 * 603 < 2.0 ** 53


@pytest.mark.parametrize("top", [1, 5, 256])
@pytest.mark.parametrize("sub_bits", [0, 3, 4])
def test_synthetic_forest_is_exact(sub_bits, top):
    from adiabatic_raytracer_amd import trees as T
    eng = _engine()
    parts, nd, recs, sln, sizes, rows = _forest603()
    s, w5, back, fwd = parts
    got = _raw(eng.event_spectrum(*parts, sub_bits=sub_bits, top=top, event_offset=LO))
    want = T.rows_spectrum(rows, sub_bits, top, event_lo=LO, n_events=603)
    assert got["kind"] == "run" and got["sub_bits"] == sub_bits and got["top"] == top
    for k in TABLES:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["top_event"], want["top_event"]) and got["top_event"].dtype == np.int64
    assert np.array_equal(got["top_power"].view(np.int64), want["top_power"].view(np.int64))
    assert np.all(got["totals"][0, :, 0] == 603) and np.all(got["totals"][0, :, 2] >= 2) and np.all(got["totals"][0, :, 6:] == 0)
    assert (got["top_event"][0, 1] >= LO).sum() == min(top, int(got["totals"][0, 1, 1]))
    # accumulated into: a second call doubles the tables, and the list is that of the doubled multiset
    twice = eng.event_spectrum(*parts, sub_bits=sub_bits, top=top, event_offset=LO)
    twice = _raw(eng.event_spectrum(*parts, sub_bits=sub_bits, top=top, event_offset=LO, spec=twice))
    both = T.spectrum_merge([want, want])
    for k in TABLES:
        assert np.array_equal(twice[k], 2.0 * got[k]), k
    assert np.array_equal(twice["top_event"], both["top_event"]) and np.array_equal(twice["top_power"], both["top_power"])
    # a final record of tree 3 inside the range of tree 7: skipped, and counted in totals[6] of the first entry
    start = np.r_[0, np.cumsum(sizes)]
    fin = np.flatnonzero(nd["is_final"] != 0)
    q = fin[(fin >= start[7] + 100)][0]
    bad = nd.copy()
    bad["tree"][q] = 3
    got_bad = _raw(eng.event_spectrum(s, w5, back, dict(fwd, nodes=recs(bad)), sub_bits=sub_bits, top=top, event_offset=LO))
    keep = np.arange(len(rows)) != np.searchsorted(fin, q)
    want_bad = T.rows_spectrum(rows[keep], sub_bits, top, event_lo=LO, n_events=603)
    want_bad["totals"][0, 0, 6] = 1.0
    for k in TABLES + ("top_power", "top_event"):
        assert np.array_equal(got_bad[k], want_bad[k]), k
    assert not np.array_equal(got_bad["sum"], got["sum"]) and T.spectrum_result(got_bad, 1)["misplaced"] == 1


# ---- 2. extremes and bad values

@pytest.mark.parametrize("sub_bits", [0, 3, 4])
def test_extremes_and_bad_values(sub_bits):
    from adiabatic_raytracer_amd import trees as T
    w = np.array([5e-324, 2.2250738585072014e-308, 1.0, 1.7976931348623157e308, 0.0, -3.0, np.nan, np.inf])
    parts, nd, recs, sln = _build(np.ones(8, np.int64), weight=w, final=np.ones(8, bool), species=np.ones(8, np.int64),
                                  sln=np.ones(8))
    m = sub_bits
    got = _raw(_engine().event_spectrum(*parts, sub_bits=m, top=6, event_offset=40))
    ph = got["count"][0, 1]
    want_bins = [0, 1 << m, 1023 << m, (2047 << m) - 1]
    assert np.array_equal(np.flatnonzero(ph), want_bins) and np.all(ph[want_bins] == 1)
    assert np.array_equal(got["sum"][0, 1, want_bins], w[:4])
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(got["sum_sq"][0, 1, want_bins], w[:4] * w[:4])
    t = got["totals"][0, 1]
    assert (t[0], t[1], t[2], t[3]) == (8, 4, 1, 3) and t[4] == w[:4].sum() and np.isinf(t[5]) and t[6] == t[7] == 0
    assert np.array_equal(got["top_event"][0, 1], [43, 42, 41, 40, -1, -1])
    assert np.array_equal(got["top_power"][0, 1].view(np.int64), np.r_[w[3::-1], 0.0, 0.0].view(np.int64))
    # the axions: eight events without a row
    assert not got["count"][0, 0].any() and np.array_equal(got["totals"][0, 0], [8, 0, 8, 0, 0, 0, 0, 0])
    assert np.all(got["top_event"][0, 0] == -1) and not got["top_power"][0, 0].any()
    res = T.spectrum_result(got, 1)
    assert res["zeros"][1] == 1 and res["bad"][1] == 3 and res["positive"][1] == 4 and res["bins"] == (0, (2047 << m) - 1)


# ---- 3. sets

def _set_powers(nd, sizes, power_of):
    """X (K, 2, n) in numpy: per set the final records' powers added per (tree, species) in node order"""
    fin = np.flatnonzero(nd["is_final"] != 0)
    ev, sp = nd["tree"][fin], nd["species"][fin] != 0
    X = []
    for k in range(power_of.K):
        p = power_of(k, fin, ev)
        X.append([np.bincount(ev[w], weights=p[w], minlength=len(sizes)) for w in (~sp, sp)])
    return np.array(X)


@pytest.mark.parametrize("kind", ["halo", "coupling"])
def test_sets_against_numpy(kind):
    import torch
    from adiabatic_raytracer_amd import trees as T
    eng = _engine()
    parts, nd, recs, sln, sizes, rows = _forest603()
    n, nn = len(sizes), len(nd)
    rng = np.random.default_rng(17)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(eng.device)  # noqa: E731
    if kind == "halo":
        R = rng.integers(0, 4, (32, n)).astype(np.float64)
        pr = np.zeros(nn)
        pr[nd["is_final"] != 0] = rows[:, 8] * rows[:, 7]
        power_of = lambda k, fin, ev: pr[fin] * R[k, ev]  # noqa: E731
        power_of.K = 32
        kw = dict(kind="halo", event_factor=up(R))
        assert (R == 0).any()
    else:
        W, B = rng.integers(0, 5, (3, nn)).astype(np.float64), rng.integers(1, 4, (3, n)).astype(np.float64)
        power_of = lambda k, fin, ev: (W[k, fin] * B[k, ev]) * sln[ev]  # noqa: E731
        power_of.K = 3
        kw = dict(kind="coupling", node_factor=up(W), event_factor=up(B))
    X = _set_powers(nd, sizes, power_of)
    m, top = 3, 64
    want = T._spectrum_tables(X, np.arange(LO, LO + n, dtype=np.int64), m, top)
    got = _raw(eng.event_spectrum(*parts, sub_bits=m, top=top, event_offset=LO, **kw))
    assert got["kind"] == kind and got["count"].shape == (power_of.K, 2, 2047 << m)
    for k in range(power_of.K):
        for name in TABLES + ("top_event",):
            assert np.array_equal(got[name][k], want[name][k]), (name, k)
        assert np.array_equal(got["top_power"][k].view(np.int64), want["top_power"][k].view(np.int64)), k
    assert len({got["totals"][k, 1, 4] for k in range(power_of.K)}) > 1 and want["totals"][:, 1, 1].min() > 64
    res = T.spectrum_result(got, 10)
    assert res["n_eff"].shape == (power_of.K, 2) and res["top_share"].shape == (power_of.K, 2, top)
    with pytest.raises(ValueError, match="needs its factor arrays"):
        eng.event_spectrum(*parts, kind=kind)
    with pytest.raises(ValueError, match="was made for"):
        eng.event_spectrum(*parts, spec=eng._zero_spectrum("run", 1, 3, 64), **kw)
    # a factor array the kernel would misread: another dtype, host memory, another shape, not a tensor
    ef = kw["event_factor"]
    for wrong in (ef.float(), ef.cpu(), ef[:, :-1], ef.t().contiguous().t(), ef.cpu().numpy()):
        with pytest.raises(ValueError, match="event_factor must be a contiguous float64"):
            eng.event_spectrum(*parts, **dict(kw, event_factor=wrong))
    if kind == "coupling":
        for wrong in (kw["node_factor"].float(), kw["node_factor"].cpu(), kw["node_factor"][:, 1:]):
            with pytest.raises(ValueError, match="node_factor must be a contiguous float64"):
                eng.event_spectrum(*parts, **dict(kw, node_factor=wrong))


# ---- 4. - 6. a real run of 600 flat events against its rows, its chunking and the replay of its top event

def _real():
    return _run("flat", N, rows=True, errors=True, spectrum=dict(sub_bits=3, top=64))


def _sum_bound(what, got, ref, n):
    got, ref, n = (np.asarray(v, np.float64).reshape(-1) for v in (got, ref, n))
    err, bound = np.abs(got - ref), 2 * (n + 1) * U * np.maximum(np.abs(got), np.abs(ref))
    f = bound > 0
    ratio = float(np.max(err[f] / bound[f])) if f.any() else 0.0
    _report(what, bound_ratio_max=ratio, entries=int(f.sum()))
    assert np.all(err <= bound), (what, ratio)
    assert np.all(got[n == 0] == 0) and np.all(ref[n == 0] == 0), what


def test_real_run_against_its_rows():
    from adiabatic_raytracer_amd import trees as T
    r = _real()
    spec = r["spectrum"]
    raw, rows = spec["raw"], r["rows_raw"]
    ref = T.rows_spectrum(rows, 3, 64, n_events=N)
    assert spec["misplaced"] == 0 and spec["f_inx"] == r["f_inx"] and spec["kind"] == "run" and raw["count"].shape == (1, 2, 2047 << 3)
    assert np.array_equal(raw["top_event"], ref["top_event"])
    ulp = _ulps(raw["top_power"], ref["top_power"])
    _report("real_600_top_power", ulp_max=int(ulp.max()), bit_equal=bool(ulp.max() == 0))
    assert ulp.max() <= 4
    assert np.array_equal(raw["totals"][..., :4], ref["totals"][..., :4])
    # count, without the events within 4 ulp of a bin edge
    gid = rows[:, 0].astype(np.int64) - 1
    pps = rows[:, 8] * rows[:, 7]
    for s in range(2):
        w = (rows[:, 1] != 0) == bool(s)
        X = np.bincount(gid[w], weights=pps[w], minlength=N)
        X = X[X > 0]
        b = T.spectrum_bin(X, 3)
        near = (T.spectrum_bin(X * (1 - 8 * U), 3) != b) | (T.spectrum_bin(X * (1 + 8 * U), 3) != b)
        assert near.sum() <= 1e-3 * len(X)
        inside = np.bincount(b[~near], minlength=2047 << 3)
        slack = sum(np.bincount(np.clip(b[near] + d, 0, (2047 << 3) - 1), minlength=2047 << 3) for d in (-1, 0, 1))
        got = raw["count"][0, s]
        assert np.all(inside <= got) and np.all(got <= inside + slack)
        _report("real_600_count", species=s, positive=int(len(X)), left_out=int(near.sum()), bins=int((got > 0).sum()))
    for k in ("sum", "sum_sq"):
        _sum_bound(f"real_600_{k}", raw[k], ref[k], ref["count"])
    n_rows = np.array([(rows[:, 1] == 0).sum(), (rows[:, 1] != 0).sum()])
    _sum_bound("real_600_S_vs_event_rows", raw["totals"][0, :, 4], r["totals"][2:4], n_rows)
    _sum_bound("real_600_Q_vs_moments", raw["totals"][0, :, 5], r["moments"]["totals"].cpu().numpy()[3:5], raw["totals"][0, :, 1])
    _report("real_600", alpha=float(spec["alpha"][1]), alpha_sigma=float(spec["alpha_sigma"][1]), n_eff=float(spec["n_eff"][1]),
            max_share=float(spec["max_share"][1]), positive=float(spec["positive"][1]))
    assert np.isfinite(spec["alpha"][1]) and 1 < spec["n_eff"][1] <= N and 0 < spec["max_share"][1] <= 1
    assert np.all(np.diff(spec["top_share"][1]) >= 0) and spec["top_share"][1, -1] <= 1 + 64 * U
    plain = _run("flat", N, rows=True, errors=True)
    assert set(r) - set(plain) == {"spectrum"} and np.array_equal(plain["rows"], r["rows"], equal_nan=True)


def test_chunking():
    one = _real()["spectrum"]["raw"]
    many = _run("flat", N, rows=False, chunk=97, spectrum=dict(sub_bits=3, top=64))["spectrum"]["raw"]
    assert np.array_equal(many["count"], one["count"]) and np.array_equal(many["totals"][..., :4], one["totals"][..., :4])
    assert np.array_equal(many["top_event"], one["top_event"])
    assert np.array_equal(many["top_power"].view(np.int64), one["top_power"].view(np.int64))
    for k in ("sum", "sum_sq"):
        _sum_bound(f"chunk_97_{k}", many[k], one[k], one["count"])
    _sum_bound("chunk_97_S_Q", many["totals"][..., 4:6], one["totals"][..., 4:6], np.repeat(one["totals"][..., 1:2], 2, axis=-1))


def test_replay_of_the_top_event():
    spec = _real()["spectrum"]
    eid = int(spec["top_event"][1, 0])
    assert eid >= 0
    one = _np(_engine().run_events(1, seed=SEED, event_offset=eid, rows=True))
    rows = one["rows_raw"]
    ph = rows[rows[:, 1] != 0]
    assert len(ph) and np.all(ph[:, 0] == eid + 1)
    x = 0.0
    for p in ph[:, 8] * ph[:, 7]:
        x += p
    assert np.float64(x).view(np.int64) == spec["top_power_raw"][1, 0].view(np.int64)
    _report("replay", event=eid, rows=int(len(ph)), power=float(x))


# ---- 7. the scans

def test_scans():
    from test_gpu_halo_scan import _eng, _halos
    eng = _eng()[0]
    base, models = _halos()
    g0 = eng.params.g_agg
    r = eng.run_events(N, seed=SEED, rows=False, couplings=[0.5 * g0, g0, 2.0 * g0], halo=base, halos=[base, models[1]],
                       spectrum={}, errors=True)
    plain_keys = set(eng.run_events(8, seed=SEED, rows=False, couplings=[g0], halo=base, halos=[base], errors=True)["halo_scan"])
    run, cs, hs = r["spectrum"], r["coupling_scan"]["spectrum"], r["halo_scan"]["spectrum"]
    assert set(r["halo_scan"]) - plain_keys == {"spectrum"} and "ratio" not in r["halo_scan"]["raw"]
    assert "weights" not in r["coupling_scan"]["raw"] and r["rows"] is None
    assert cs["kind"] == "coupling" and hs["kind"] == "halo" and cs["sub_bits"] == 3 and cs["top"] == 64
    assert cs["raw"]["count"].shape == (3, 2, 2047 << 3) and hs["raw"]["count"].shape == (2, 2, 2047 << 3)
    assert cs["n_eff"].shape == (3, 2) and hs["top_event"].shape == (2, 2, 64) and run["n_eff"].shape == (2,)
    for what, scan, k in (("coupling_g0", cs, 1), ("halo_base", hs, 0)):
        assert np.array_equal(scan["raw"]["count"][k], run["raw"]["count"][0]), what
        assert np.array_equal(scan["top_event"][k], run["top_event"]), what
        rel = np.abs(scan["n_eff"][k] / run["n_eff"] - 1)
        _report(f"scan_{what}", n_eff_rel=float(rel.max()), n_eff=float(run["n_eff"][1]))
        assert np.all(rel <= 1e-12), (what, rel)
    rel = np.abs(hs["n_eff"][:, 1] / r["halo_scan"]["n_eff"] - 1)
    _report("scan_halo_n_eff", rel=float(rel.max()), n_eff=[float(v) for v in hs["n_eff"][:, 1]])
    assert np.all(rel <= 1e-12)
    # the variance grows with the distance from the base coupling: the scan now says by how much
    _report("scan_coupling_n_eff", n_eff=[float(v) for v in cs["n_eff"][:, 1]], alpha=[float(v) for v in cs["alpha"][:, 1]])
    assert cs["misplaced"] == 0 and hs["misplaced"] == 0


# ---- 8. main_runner_tree, 48 events

def test_main_runner_tree_paths():
    import adiabatic_raytracer_amd as A
    p = _params("flat")
    info_d, info_h, info_0 = {}, {}, {}
    A.trees.main_runner_tree(p, 49, device_events=True, spectrum={}, run_info=info_d)
    A.trees.main_runner_tree(p, 49, device_trees=True, spectrum={}, run_info=info_h)
    A.trees.main_runner_tree(p, 49, device_events=True, run_info=info_0)
    assert set(info_d) - set(info_0) == set(info_h) - set(info_0) == {"spectrum"}
    run = _np(_engine().run_events(48, seed=SEED, spectrum={}))["spectrum"]
    d, h = info_d["spectrum"], info_h["spectrum"]
    assert d["f_inx"] == run["f_inx"] == info_d["f_inx"] and d["sub_bits"] == 3 and d["top"] == 64
    for k in ("count", "top_event", "top_power"):
        assert np.array_equal(d["raw"][k], run["raw"][k]), k
    assert np.array_equal(d["raw"]["totals"][..., :4], run["raw"]["totals"][..., :4])
    for k in ("sum", "sum_sq"):
        _sum_bound(f"main_runner_device_{k}", d["raw"][k], run["raw"][k], run["raw"]["count"])
    assert np.array_equal(d["n_eff"] > 0, run["n_eff"] > 0) and np.allclose(d["n_eff"], run["n_eff"], rtol=1e-12, equal_nan=True)
    assert np.array_equal(h["raw"]["count"], run["raw"]["count"]) and np.array_equal(h["top_event"], run["top_event"])


# ---- 9. off by default

def test_off_by_default():
    eng = _engine()
    r = eng.run_events(20, seed=SEED)
    assert set(r) == RUN_KEYS
    with pytest.raises(ValueError, match="spectrum: unknown keys"):
        eng.run_events(20, seed=SEED, spectrum=dict(bins=3))
    with pytest.raises(ValueError, match="spectrum: top"):
        eng.run_events(20, seed=SEED, spectrum=dict(top=257))
    empty = eng.run_events(0, spectrum=dict(sub_bits=1, top=3))["spectrum"]
    assert empty["bins"] is None and not empty["raw"]["count"].any() and np.all(empty["top_event"] == -1)
