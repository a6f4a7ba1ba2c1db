"""Event rows on the GPU (art_event_rows_device, Engine.event_rows, Engine.run_events,
main_runner_tree(device_events=True)) against the host assembly of main_runner_tree(device_trees=True),
which grows the same device forests and builds the rows in numpy, and against numpy on the forests'
own nodes.

Column rules: the shape and column 1 are identical; columns 2-5 (acos, atan2 of the device against
numpy's) within 4 ulp; every other column, column 7 after its division by f_inx included, bit-equal
(NaN equal to NaN); the order is the host's, tree[tree["is_final"] != 0].

Counts (unit weights) are exact in every accumulation mode. A weighted bin is a sum of the same terms
in another order: two such sums differ by at most 2 (terms + 1) u Σ|w| with u = 2^-53 (Higham §4.2,
the bound of tests/test_gpu_skymap.py).

ART_PARITY_REPORT=path collects the JSON lines the tests print. Measured on an MI355X
(profiles/event_rows_parity.jsonl; DESIGN.md §3, "Event rows on the device"): angle columns at most
1 ulp from numpy's in every comparison (bound 4), every other column bit-equal; 1100 events give 3737
nodes and 1927 rows; over two sessions weighted sky bins at most 0.26 of the bound, flux bins 0.11,
chunked against one chunk 0.22 (sky) and 0.10 (flux), flux against the summed sky map and the host's
flux 1.4e-4; 0 of 1927 rows within 4 ulp of a bin edge; cyclotron column 8 within 1 ulp of
col13 * exp(-col14) (bound 3), 55 photon rows with τ > 0, 14 root photons with the host call's τ bit
for bit; GR: 16 of the 44 events with rows have grouped backtrace crossings."""
import json
import math
import os

import numpy as np
import pytest

from conftest import CONFIGS
from test_event_rows import _numpy_rows, _ulps

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
AXION, PHOTON = 0, 1
ANGLES = (2, 3, 4, 5)
SEED = 1769

_cache = {}


def _report(what, **vals):
    line = json.dumps({"test": "event_rows", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _params(cfg):
    import adiabatic_raytracer_amd as A
    return A.Params(**CONFIGS[cfg])


def _engine(cfg="flat"):
    from adiabatic_raytracer_amd.engine import Engine
    if ("eng", cfg) not in _cache:
        _cache[("eng", cfg)] = Engine(_params(cfg))
    return _cache[("eng", cfg)]


def _host(cfg, n, saveMode, **kw):
    """main_runner_tree(device_trees=True): (rows, run_info), computed once and left unchanged"""
    import adiabatic_raytracer_amd as A
    key = ("host", cfg, n, saveMode, tuple(sorted(kw.items())))
    if key not in _cache:
        info = {}
        rows = A.trees.main_runner_tree(_params(cfg), n + 1, saveMode=saveMode, run_info=info, device_trees=True, **kw)
        rows.setflags(write=False)
        _cache[key] = (rows, info)
    return _cache[key]


def _np(r):
    """run_events' dict with its tensors on the host"""
    import torch
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _run(cfg, n, **kw):
    key = ("run", cfg, n, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = _np(_engine(cfg).run_events(n, seed=SEED, **kw))
    return _cache[key]


def _check_rows(what, got, ref):
    """The column rules of the module docstring; returns the largest angle difference in ulp"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got[:, 1], ref[:, 1])
    worst = 0.0
    for c in range(ref.shape[1]):
        if c in ANGLES:
            u = _ulps(got[:, c], ref[:, c])
            worst = max(worst, float(u.max()) if u.size else 0.0)
            assert np.all(u <= 4), (what, c, float(u.max()))
        else:
            assert np.array_equal(got[:, c], ref[:, c], equal_nan=True), (what, c)
    _report(what, rows=int(len(ref)), ncols=int(ref.shape[1]), angle_ulp_max=worst)
    return worst


def _pipeline(cfg, lo, c):
    """The steps of run_events for events [lo, lo + c), device-resident: (sample, weight5, back, forward)"""
    from dataclasses import replace
    from adiabatic_raytracer_amd.engine import Engine
    key = ("pipe", cfg, lo, c)
    if key not in _cache:
        eng = _engine(cfg)
        if ("back", cfg) not in _cache:
            _cache[("back", cfg)] = Engine(replace(eng.params, B0=-eng.params.B0))
        s = eng.sample(c, seed=SEED, ray_offset=lo)
        w5 = eng.event_weight(s)
        back = _cache[("back", cfg)].grow_trees(s["x"], -s["k_init"], s["erg"], AXION, num_cutoff=0, splittings_cutoff=100000,
                                                crossing_cap=256, seed=SEED, tree_offset=lo)
        fwd = eng.grow_trees(s["x"], s["k_init"], s["erg"], PHOTON, seed=SEED, tree_offset=lo)
        _cache[key] = (s, w5, back, fwd)
    return _cache[key]


def _unit(parts):
    """The same events with every row's column 8 * column 7 equal to 1: sln_prob, the backtrace's prob and
    weight and the forward nodes' weights set to 1 in copies"""
    import torch
    s, w5, back, fwd = parts
    w5 = w5.clone()
    w5[2] = 1.0
    out = []
    for forest in (back, fwd):
        f = dict(forest)
        nodes = forest["nodes"].clone()
        d = nodes.view(-1).view(torch.float64).view(nodes.shape[0], -1)
        d[:, 3] = 1.0  # weight (art_tree_node: six int32, then weight, prob, ...)
        if forest is back:
            d[:, 4] = 1.0  # prob
        f["nodes"] = nodes
        out.append(f)
    return s, w5, out[0], out[1]


def _evd(parts):
    """tests/test_event_rows.py's per-event table from the device-resident parts, and the forward nodes"""
    from adiabatic_raytracer_amd.engine import nodes_to_numpy
    s, w5, back, fwd = parts
    n = s["erg"].numel()
    w = w5.cpu().numpy()
    bn = nodes_to_numpy(back["nodes"])
    assert len(bn) == n and np.array_equal(bn["tree"], np.arange(n))
    ev = np.zeros((n, 14))
    ev[:, 0:3] = s["x"].cpu().numpy().reshape(3, n).T
    ev[:, 3:6] = s["k_init"].cpu().numpy().reshape(3, n).T
    ev[:, 6], ev[:, 7], ev[:, 8] = w[2], w[4], w[0]
    ev[:, 9], ev[:, 10] = bn["prob"], bn["weight"]
    ev[:, 11] = back["counts"].cpu().numpy()
    ev[:, 12], ev[:, 13] = fwd["counts"].cpu().numpy(), fwd["infos"].cpu().numpy()
    return ev, nodes_to_numpy(fwd["nodes"])


def _divide(raw, f_inx):
    rows = raw.copy()
    rows[:, 7] /= float(f_inx)
    return rows


# ---- 1. rows equal the host assembly, 48 events (the project's smallest run)

@pytest.mark.parametrize("saveMode", [0, 1])
def test_rows_equal_host_assembly_48(saveMode):
    ref, info = _host("flat", 48, saveMode)
    r = _run("flat", 48, saveMode=saveMode)
    assert r["rows"].shape[1] == (29 if saveMode else 13) and len(ref) > 24
    _check_rows(f"rows48_saveMode{saveMode}", r["rows"], ref)
    assert r["f_inx"] == info["f_inx"] and r["n_rows"] == info["rows"] == len(ref)
    assert np.array_equal(r["rows"][:, 0], ref[:, 0])  # the host's order


# ---- 2. more than one block and a grid-stride pass: 1100 events

def test_compaction_1100_against_host_and_numpy():
    n = 1100
    ref, info = _host("flat", n, 1)
    r = _run("flat", n, saveMode=1)
    _check_rows("rows1100_host", r["rows"], ref)
    assert r["f_inx"] == info["f_inx"]
    # the rows in numpy from Engine.grow_trees' own nodes, pulled to the host
    parts = _pipeline("flat", 0, n)
    ev, nodes = _evd(parts)
    fin = nodes[nodes["is_final"] != 0]
    derived, _ = _numpy_rows(fin, ev, 0, _params("flat").mass_a)
    got = _engine().event_rows(*parts, saveMode=1)
    tot = got["totals"].cpu().numpy()
    n_rows, n_nodes = got["n_rows"], parts[3]["n_nodes"]
    assert n_nodes > 2048 and 0 < n_rows < n_nodes and n_rows == len(fin) == int(tot[0])
    assert int(tot[1]) == int((fin["species"] == PHOTON).sum())
    assert int(tot[4]) == int((parts[0]["attempts"].cpu().numpy().astype(np.int64) - 1).sum()) and tot[5] == 0
    _check_rows("rows1100_numpy", got["rows"].cpu().numpy(), derived)
    f_inx = int(tot[4] + tot[1])
    assert f_inx == r["f_inx"]
    _check_rows("rows1100_numpy_vs_run", r["rows"], _divide(derived, f_inx))
    _report("compaction", n_nodes=int(n_nodes), n_rows=int(n_rows))


# ---- 3. chunk invariance

def _bound_check(what, a, b, cnt):
    """|a - b| <= 2 (terms + 1) u Σ|w| per bin (non-negative weights: Σ|w| is the bin itself)"""
    a, b, cnt = (np.asarray(v, np.float64).reshape(-1) for v in (a, b, cnt))
    assert np.all(b >= 0)
    err, bound = np.abs(a - b), 2 * (cnt + 1) * U * np.maximum(a, b)
    ratio = float(np.max(err[cnt > 0] / bound[cnt > 0])) if (cnt > 0).any() else 0.0
    _report(what, bound_ratio_max=ratio, bins_filled=int((cnt > 0).sum()))
    assert np.all(err <= bound), (what, ratio)
    return ratio


def test_chunk_invariance_1100():
    n = 1100
    sky = dict(n_theta=6, n_phi=11, n_dw=5, dw_range=_dw_range(n))
    one = _run("flat", n, saveMode=1, sky_map=sky)
    ch = _run("flat", n, saveMode=1, sky_map=sky, chunk=400)  # 400, 400, 300
    assert one["rows"].tobytes() == ch["rows"].tobytes()
    for k in ("f_inx", "n_rows", "n_photon_rows"):
        assert one[k] == ch[k], k
    # unit weights: the chunks' tables are the one chunk's, identically
    eng = _engine()
    whole = eng.event_rows(*_unit(_pipeline("flat", 0, n)), sky=sky, rows=False)
    acc = dict(flux=None, sky_hist=None, totals=None)
    for lo, c in ((0, 400), (400, 400), (800, 300)):
        r = eng.event_rows(*_unit(_pipeline("flat", lo, c)), event_offset=lo, sky=sky, rows=False, **acc)
        acc = {k: r[k] for k in acc}
    import torch
    for k in acc:
        assert torch.equal(acc[k], whole[k]), k
    assert whole["totals"][0].item() == one["n_rows"] and whole["flux"].sum().item() == one["n_rows"]
    # weighted: the same terms in another order
    _bound_check("chunk_flux", ch["flux_raw"], one["flux_raw"], whole["flux"].cpu().numpy())
    _bound_check("chunk_sky", ch["sky_raw"], one["sky_raw"], whole["sky_hist"].cpu().numpy())
    assert abs(ch["totals"][3] - one["totals"][3]) <= 2 * (one["n_rows"] + 1) * U * one["totals"][3]


# ---- 4. tables are the bincount of their labels

def _dw_range(n):
    ref, _ = _host("flat", n, 1)
    return tuple(float(v) for v in np.quantile(ref[:, 12], [0.02, 0.98]))


@pytest.mark.parametrize("theta_axis", ["cos", "theta"])
@pytest.mark.parametrize("mode", [1, 2])
def test_tables_are_the_bincount_of_their_labels(theta_axis, mode):
    n = 1100
    shape = (6, 11, 5)
    eng = _engine()
    parts = _pipeline("flat", 0, n)
    sky = dict(n_theta=6, n_phi=11, n_dw=5, theta_axis=theta_axis, dw_range=_dw_range(n), mode=mode)
    size = 2 * int(np.prod(shape))
    u = eng.event_rows(*_unit(parts), sky=sky, rows=False, return_bins=True)
    labels = u["bins"].cpu().numpy()
    assert len(labels) == u["n_rows"] and (labels >= 0).sum() > 0.5 * len(labels) and (labels < 0).any()
    cnt = np.bincount(labels[labels >= 0], minlength=size)
    assert np.array_equal(u["sky_hist"].cpu().numpy().reshape(-1), cnt)
    w = eng.event_rows(*parts, sky=sky, saveMode=1, return_bins=True)
    assert np.array_equal(w["bins"].cpu().numpy(), labels)
    rows = w["rows"].cpu().numpy()
    pps = rows[:, 8] * rows[:, 7]
    refw = np.bincount(labels[labels >= 0], weights=pps[labels >= 0], minlength=size)
    _bound_check(f"sky_{theta_axis}_mode{mode}", w["sky_hist"].cpu().numpy(), refw, cnt)
    # the flux table: np.histogram's bins of column 3, both species
    for s in (0, 1):
        m = rows[:, 1] == s
        fc, _ = np.histogram(rows[m, 3], 50, range=(-np.pi, np.pi))
        fw, _ = np.histogram(rows[m, 3], 50, range=(-np.pi, np.pi), weights=pps[m])
        assert np.array_equal(u["flux"].cpu().numpy().reshape(2, 50)[s], fc)
        _bound_check(f"flux_{theta_axis}_mode{mode}_s{s}", w["flux"].cpu().numpy().reshape(2, 50)[s], fw, fc)
    if theta_axis != "cos":
        return
    # the labels are numpy's bins of kz / |k|, φf and Δω recomputed from the nodes
    ev, nodes = _evd(parts)
    fin = nodes[nodes["is_final"] != 0]
    derived, ct = _numpy_rows(fin, ev, 0, _params("flat").mass_a)
    ranges = ((-1.0, 1.0), (-np.pi, np.pi), sky["dw_range"])
    _, edges = np.histogramdd(np.zeros((1, 3)), bins=shape, range=ranges)
    idx, near = [], np.zeros(len(fin), bool)
    for v, e in zip((ct, derived[:, 3], derived[:, 12]), edges):
        i = np.searchsorted(e, v, side="right") - 1
        i[v == e[-1]] -= 1
        idx.append(np.where((i >= 0) & (i < e.size - 1) & np.isfinite(v), i, -1))
        gap = np.abs(v[:, None] - e[None, :])
        near |= np.any(gap <= 4 * np.spacing(np.maximum(np.abs(v[:, None]), np.abs(e[None, :]))), axis=1)
    sp = (fin["species"] != AXION).astype(int)
    ok = (idx[0] >= 0) & (idx[1] >= 0) & (idx[2] >= 0)
    ref = np.where(ok, ((sp * shape[0] + idx[0]) * shape[1] + idx[1]) * shape[2] + idx[2], -1)
    _report(f"labels_mode{mode}", rows=int(len(fin)), near_edge=int(near.sum()), counted=int((ref >= 0).sum()))
    assert near.sum() <= max(1, 1e-3 * len(fin))
    assert np.array_equal(labels[~near], ref[~near]), np.flatnonzero((labels != ref) & ~near)[:10]


def test_flux_is_the_sky_map_summed_and_the_hosts_flux():
    n = 1100
    ref, info = _host("flat", n, 1)
    r = _run("flat", n, saveMode=1, sky_map=dict(n_theta=6, n_phi=50, n_dw=1))
    w = ref[:, 8] * ref[:, 7]  # weight * sln_prob / f_inx
    terms = len(ref) + 6 + 2  # the rows of a bin, the n_theta n_dw bins numpy adds up, the divisions by f_inx
    worst = 0.0
    for s in (0, 1):
        bound = 2 * terms * U * np.abs(w[ref[:, 1] == s]).sum()
        d_sky = np.abs(r["sky_map"][s].sum(axis=(0, 2)) - r["flux"][s])
        d_host = np.abs(r["flux"][s] - info["flux"][s])
        worst = max(worst, float(d_sky.max() / bound), float(d_host.max() / bound))
        assert np.all(d_sky <= bound) and np.all(d_host <= bound), s
        assert abs(r["sum_weight_sln_prob"][s] - info["sum_weight_sln_prob"][s]) <= bound
    assert r["flux"][1].sum() > 0 and r["sky_map"].shape == (2, 6, 50, 1)
    _report("flux_vs_sky_and_host", bound_ratio_max=worst)


# ---- 5. main_runner_tree(device_events=True), 48 events

def test_main_runner_tree_device_events(tmp_path):
    import adiabatic_raytracer_amd as A
    p = _params("flat")
    sky = dict(n_theta=8, n_phi=50, n_dw=3, dw_range=_dw_range(48))
    info_h, info_d = {}, {}
    ref = A.trees.main_runner_tree(p, 49, saveMode=1, run_info=info_h, sky_map=sky, dir_tag=str(tmp_path / "h"), file_tag="s",
                                   device_trees=True)
    rows = A.trees.main_runner_tree(p, 49, saveMode=1, run_info=info_d, sky_map=sky, dir_tag=str(tmp_path / "d"), file_tag="s",
                                    device_events=True)
    _check_rows("main_runner_device_events", rows, ref)
    assert set(info_d) == set(info_h)
    for k in ("f_inx", "rows", "events", "n_events"):
        assert info_d[k] == info_h[k], k
    terms = len(ref) + 8 * 3 + 2
    w = ref[:, 8] * ref[:, 7]
    for s in (0, 1):
        bound = 2 * terms * U * np.abs(w[ref[:, 1] == s]).sum()
        assert np.all(np.abs(info_d["flux"][s] - info_h["flux"][s]) <= bound), s
        assert np.all(np.abs(info_d["sky_map"][s] - info_h["sky_map"][s]) <= bound), s
        assert abs(info_d["sum_weight_sln_prob"][s] - info_h["sum_weight_sln_prob"][s]) <= bound
    for a, b in zip(info_d["sky_map_edges"], info_h["sky_map_edges"]):
        assert np.array_equal(a, b)
    names = lambda d: sorted(f.name for f in (tmp_path / d / "npy").iterdir())  # noqa: E731
    assert names("d") == names("h") and len(names("d")) == 2
    npy = [f for f in (tmp_path / "d" / "npy").iterdir() if f.suffix == ".npy"][0]
    assert np.load(npy).tobytes() == rows.tobytes()
    with pytest.raises(ValueError, match="device_events"):
        A.trees.main_runner_tree(p, 49, saveMode=2, dir_tag=str(tmp_path / "x"), device_events=True)


# ---- 6. cyclotron, 65 events

def test_cyclotron_65():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd.engine import nodes_to_numpy
    n = 65
    plain = _run("flat", n, saveMode=1)
    cyc = _run("flat", n, saveMode=1, cyclotron=True)
    a, b = cyc["rows"], plain["rows"]
    assert a.shape == b.shape
    differ = [c for c in range(29) if not np.array_equal(a[:, c], b[:, c], equal_nan=True)]
    assert differ == [8, 14], differ
    assert cyc["totals"][5] == 0 and cyc["f_inx"] == plain["f_inx"]
    ph = a[:, 1] == 1
    assert np.all(a[~ph, 14] == 0) and (a[ph, 14] > 0).any() and np.all(a[:, 14] >= 0)
    u = _ulps(a[:, 8], a[:, 13] * np.exp(-a[:, 14]))
    _report("cyclotron_weight", rows=int(len(a)), photons_with_tau=int((a[ph, 14] > 0).sum()), ulp_max=float(u.max()))
    assert np.all(u <= 3)
    # final photon nodes that are roots: τ is the host call's on the same segment, bit for bit
    parts = _pipeline("flat", 0, n)
    r = _engine().event_rows(*parts, saveMode=1, cyclotron=True)
    rows = r["rows"].cpu().numpy()
    assert np.array_equal(_divide(rows, cyc["f_inx"]), a, equal_nan=True) and r["totals"][5].item() == 0
    nodes = nodes_to_numpy(parts[3]["nodes"])
    fin = nodes[nodes["is_final"] != 0]
    sel = np.flatnonzero((fin["species"] == PHOTON) & (fin["t0"] == 0))
    assert sel.size > 0
    f = fin[sel]
    erg = parts[0]["erg"].cpu().numpy()[f["tree"]]
    ln_t0 = math.log(math.exp(-30.0))  # the forest's root value
    assert ln_t0 == -30.0
    res = A.propagate_batch(_params("flat"), f["x0"].T, f["k0"].T, erg, f["dw0"], np.full(sel.size, ln_t0),
                            np.full(sel.size, PHOTON, np.int8), max_crossings=-1, cyclotron=True)
    assert np.array_equal(res["cyc_tau"], rows[sel, 14])
    _report("cyclotron_roots", roots=int(sel.size), with_tau=int((res["cyc_tau"] > 0).sum()))


# ---- 7. GR, 48 events

def test_gr_48():
    ref, info = _host("gr", 48, 1)
    r = _run("gr", 48, saveMode=1)
    _check_rows("rows48_gr", r["rows"], ref)
    assert r["f_inx"] == info["f_inx"]
    # Grouped crossings feed column 25. Column 27 cannot show them: it is the backtrace tree's get_tree
    # count, 1 for every event in the backtrace form (only the root is processed), in the host's rows
    # too. The crossings of a backtrace are its node's n_cross: some event with rows has two or more,
    # and its column 25 is that node's prob * weight, the weight a product over the group.
    from adiabatic_raytracer_amd.engine import nodes_to_numpy
    bn = nodes_to_numpy(_pipeline("gr", 0, 48)[2]["nodes"])
    ev = r["rows"][:, 0].astype(np.int64) - 1
    assert np.all(r["rows"][:, 27] == 1)
    assert (bn["n_cross"][ev] >= 2).any()
    assert np.array_equal(r["rows"][:, 25], (bn["prob"] * bn["weight"])[ev])
    _report("gr_backtrace", events_with_rows=int(np.unique(ev).size), grouped=int((bn["n_cross"][np.unique(ev)] >= 2).sum()))


# ---- 8. edges

def test_edges():
    import torch
    eng = _engine()
    # no events: no rows, zero tables, f_inx = 0
    r0 = eng.run_events(0, saveMode=1, sky_map={})
    assert r0["rows"].shape == (0, 29) and r0["f_inx"] == 0 and r0["n_rows"] == 0
    assert not r0["flux"].any() and not r0["sky_map"].any() and r0["flux"].shape == (2, 50)
    # one event
    ref, info = _host("flat", 1, 1)
    r1 = _np(eng.run_events(1, seed=SEED, saveMode=1))
    _check_rows("rows1", r1["rows"], ref)
    assert r1["f_inx"] == info["f_inx"]
    # rows=False: no rows; under unit weights the tables and totals are those of the run with rows
    parts = _unit(_pipeline("flat", 0, 48))
    sky = dict(n_theta=6, n_phi=11, n_dw=1)
    with_rows = eng.event_rows(*parts, sky=sky, saveMode=1)
    without = eng.event_rows(*parts, sky=sky, saveMode=1, rows=False)
    assert without["rows"] is None and without["n_rows"] is None and len(with_rows["rows"]) == with_rows["n_rows"] > 0
    for k in ("flux", "sky_hist", "totals"):
        assert torch.equal(with_rows[k], without[k]), k
    nr = _np(eng.run_events(48, seed=SEED, rows=False))
    assert nr["rows"] is None and nr["n_rows"] == _run("flat", 48, saveMode=0)["n_rows"]
    assert nr["f_inx"] == _run("flat", 48, saveMode=0)["f_inx"]
    # a stream of the caller's
    base = _run("flat", 48, saveMode=1)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = eng.run_events(48, seed=SEED, saveMode=1)
    side.synchronize()
    assert r["rows"].cpu().numpy().tobytes() == base["rows"].tobytes() and r["f_inx"] == base["f_inx"]
    # a sky map over Δω needs its range
    with pytest.raises(ValueError, match="dw_range"):
        eng.run_events(4, sky_map=dict(n_dw=3))
