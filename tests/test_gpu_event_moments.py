"""Event moments on the GPU (art_event_moments_device, Engine.event_moments, run_events(errors=True),
main_runner_tree(errors=True)) against trees.event_moments / trees.moments_sigma in numpy on the rows and
sky labels that Engine.event_rows returns for the same forests.

Unit weights and integer powers: every X, X² and X a_e is an integer below 2^53, so the device tables are
np.array_equal to numpy's, whatever the order of the adds.

Weighted tables are sums of non-negative terms in another order. Per bin b with E_b events and at most m_b
rows of one event: each X is within (m_b - 1) u of the other order's, squaring doubles the relative error and
adds one rounding, a_e is an exact integer, then come E_b terms: |a - b| <= 2 (E_b + 2 m_b + 2) u max(a, b),
u = 2^-53.

σ follows from V = Q - 2 F C + F² A2, F = S / f, which cancels; so σ is compared through V. With the bounds
bQ, bC above and bS = 2 (rows_b + 1) u S_b (tests/test_gpu_event_rows.py) for the tables of either side:
|ΔV| <= bQ + 2 F bC + (2 C + 2 F A2) bS / f + 8 u (Q + 2 F C + F² A2), the last term for the roundings of the
expression itself and of σ² (n - 1) / n f² back from σ; twice that between two device results.

ART_PARITY_REPORT=path collects the JSON lines the tests print. Measured on an MI355X
(profiles/event_moments_parity.jsonl; DESIGN.md §3, "Monte-Carlo errors"): 1100 events give 3737 nodes and
1927 rows, at most 4 rows of one event in a bin of the coarse map; unit weights and the synthetic forest
exact; weighted bins at most 0.14 of the bound (coarse 0.09), chunked against one chunk 0.14, cyclotron at 65
events 0.11; σ of run_events against numpy on the rows at most 0.22 of the bound on V (flux 0.12, totals
0.002), with against without rows 0.11; main_runner_tree's two paths 0.05; the photon flux bins' relative σ
at 1100 events 0.21-0.27 at the smallest and the median."""
import json
import os

import numpy as np
import pytest

from test_gpu_event_rows import SEED, U, _dw_range, _engine, _np, _params, _pipeline, _unit

pytestmark = pytest.mark.gpu

N = 1100
NBINS = 50
COARSE = dict(n_theta=1, n_phi=2, n_dw=1)


def _fine():
    return dict(n_theta=6, n_phi=11, n_dw=5, dw_range=_dw_range(N))


def _size(sky):
    return 2 * sky["n_theta"] * sky["n_phi"] * sky["n_dw"]


def _report(what, **vals):
    line = json.dumps({"test": "event_moments", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _groups(ev, labels, size):
    """per bin: E, the events with a row in it, m, the most rows one event has in it, and its rows"""
    keep = labels >= 0
    g, cnt = np.unique(ev[keep] * size + labels[keep], return_counts=True)
    E, m = np.bincount(g % size, minlength=size), np.zeros(size, np.int64)
    np.maximum.at(m, g % size, cnt)
    return E, m, np.bincount(labels[keep], minlength=size)


def _reference(rows, labels, attempts, lo, sky):
    """numpy's tables from rows (column 7 raw) and their sky labels: per table (S, Q, C) and (E, m, rows)"""
    from adiabatic_raytracer_amd import trees as T
    n = len(attempts)
    ev = rows[:, 0].astype(np.int64) - 1 - lo
    sp = rows[:, 1].astype(np.int64)
    a = attempts.astype(np.int64) - 1 + np.bincount(ev[sp == 1], minlength=n)
    pps = rows[:, 8] * rows[:, 7]
    fb = T.hist_bins(rows[:, 3], NBINS)
    fl = np.where(fb >= 0, sp * NBINS + fb, -1)
    for s in (0, 1):  # hist_bins is np.histogram's rule on these values
        assert np.array_equal(np.bincount(fb[(sp == s) & (fb >= 0)], minlength=NBINS),
                              np.histogram(rows[sp == s, 3], NBINS, range=(-np.pi, np.pi))[0])
    ref = {"a": a, "n": n,
           "flux": T.event_moments(ev, fl, pps, 2 * NBINS, a), "flux_g": _groups(ev, fl, 2 * NBINS),
           "tot": T.event_moments(ev, sp, pps, 2, a), "tot_g": _groups(ev, sp, 2)}
    if sky is not None:
        ref.update(sky=T.event_moments(ev, labels, pps, _size(sky), a), sky_g=_groups(ev, labels, _size(sky)))
    return ref


def _totals_ref(ref):
    a, (_, tq, tc) = ref["a"], ref["tot"]
    return np.r_[float(ref["n"]), a.sum(), (a * a).sum(), tq, tc, 0.0]


def _host(mo):
    return {k: (None if v is None else v.cpu().numpy().reshape(-1)) for k, v in mo.items()}


def _bound(a, b, groups):
    E, m, _ = groups
    return 2 * (E + 2 * m + 2) * U * np.maximum(a, b)


def _check_weighted(what, got, ref, tables):
    """the device tables against numpy's within the module docstring's bound; the largest ratio to it"""
    worst = 0.0
    for name in tables:
        _, Q, Cc = ref[name]
        g = ref[name + "_g"]
        pairs = ((got[name + "_sq"], Q), (got[name + "_xa"], Cc)) if name != "tot" else \
            ((got["totals"][3:5], Q), (got["totals"][5:7], Cc))
        for a, b in pairs:
            assert np.all(b >= 0) and np.all(a[g[0] == 0] == 0)
            err, bound = np.abs(a - b), _bound(a, b, g)
            f = (g[0] > 0) & (bound > 0)
            ratio = float(np.max(err[f] / bound[f])) if f.any() else 0.0
            worst = max(worst, ratio)
            assert np.all(err <= bound), (what, name, ratio)
    _report(what, bound_ratio_max=worst)
    return worst


def _rows_and_moments(parts, sky, lo=0, **kw):
    eng = _engine()
    er = eng.event_rows(*parts, event_offset=lo, sky=sky, return_bins=True, **kw)
    mo = eng.event_moments(*parts, event_offset=lo, nbins=NBINS, sky=sky, cyclotron_rerun=er["cyclotron_rerun"])
    att = parts[0]["attempts"].cpu().numpy()
    ref = _reference(er["rows"].cpu().numpy(), er["bins"].cpu().numpy().astype(np.int64), att, lo, sky)
    return er, _host(mo), ref


# ---- 1. exact, unit weights: 1100 events, 3737 nodes

@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_unit_weights_are_exact(which):
    sky = COARSE if which == "coarse" else _fine()
    parts = _unit(_pipeline("flat", 0, N))
    assert parts[3]["n_nodes"] > 2048  # several blocks, trees across wave and block boundaries
    er, got, ref = _rows_and_moments(parts, sky)
    for name in ("sky", "flux"):
        S, Q, Cc = ref[name]
        assert np.array_equal(got[name + "_sq"], Q) and np.array_equal(got[name + "_xa"], Cc), name
        assert Q.sum() > 0 and Cc.sum() > 0
    S, Q, _ = ref["sky"]
    assert np.array_equal(er["sky_hist"].cpu().numpy().reshape(-1), S)  # the same bins as the first moments
    if which == "coarse":
        assert np.all(ref["sky_g"][1] >= 2) and np.all(Q > S)  # events with several rows in one bin
    t, te = got["totals"], er["totals"].cpu().numpy()
    assert t[0] == N and t[1] == te[4] + te[1] and t[7] == 0
    assert np.array_equal(t, _totals_ref(ref))
    _report(f"unit_{which}", nodes=int(parts[3]["n_nodes"]), rows=int(te[0]), most_rows_of_an_event_in_a_bin=int(ref["sky_g"][1].max()))


# ---- 2. weighted, the same events

@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_weighted_within_the_bound(which):
    sky = COARSE if which == "coarse" else _fine()
    er, got, ref = _rows_and_moments(_pipeline("flat", 0, N), sky)
    _check_weighted(f"weighted_{which}", got, ref, ("sky", "flux", "tot"))
    assert np.array_equal(got["totals"][[0, 1, 2, 7]], _totals_ref(ref)[[0, 1, 2, 7]])


# ---- 3. chunks 400 / 400 / 300 accumulated against one chunk

def test_chunks_accumulate():
    import torch
    eng, sky = _engine(), _fine()
    for unit in (True, False):
        prep = _unit if unit else (lambda p: p)
        whole = eng.event_moments(*prep(_pipeline("flat", 0, N)), nbins=NBINS, sky=sky)
        acc = None
        for lo, c in ((0, 400), (400, 400), (800, 300)):
            acc = eng.event_moments(*prep(_pipeline("flat", lo, c)), event_offset=lo, nbins=NBINS, sky=sky, moments=acc)
        if unit:
            for k in whole:
                assert torch.equal(acc[k], whole[k]), k
            continue
        _, _, ref = _rows_and_moments(_pipeline("flat", 0, N), sky)
        a, w = _host(acc), _host(whole)
        worst = 0.0
        for name in ("sky", "flux"):
            for k in ("_sq", "_xa"):
                err, bound = np.abs(a[name + k] - w[name + k]), _bound(a[name + k], w[name + k], ref[name + "_g"])
                assert np.all(err <= bound), (name, k)
                worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        for q in (3, 4, 5, 6):
            g = tuple(v[(q - 3) % 2] for v in ref["tot_g"])
            assert abs(a["totals"][q] - w["totals"][q]) <= _bound(a["totals"][q], w["totals"][q], g), q
        assert np.array_equal(a["totals"][[0, 1, 2, 7]], w["totals"][[0, 1, 2, 7]])
        _report("chunks_weighted", bound_ratio_max=worst)


# ---- 4. a synthetic forest: tree sizes around the wave size, empty trees, a long tree

SIZES = (0, 1, 2, 63, 64, 65, 0, 300, 1)


def _synthetic_forest():
    """(sample, weight5, back, forward) uploaded from numpy records, with integer-valued powers; and the
    forward records"""
    import torch
    from adiabatic_raytracer_amd.trees import NODE_DTYPE
    eng = _engine()
    rng = np.random.default_rng(1769)
    n, nn = len(SIZES), sum(SIZES)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    nd = np.zeros(nn, NODE_DTYPE)
    nd["tree"] = np.repeat(np.arange(n), SIZES)
    nd["is_final"] = rng.random(nn) < 0.5
    nd["is_final"][[0, 1]] = 1  # the tree of one record has a row
    nd["species"] = rng.integers(0, 2, nn)
    nd["weight"] = rng.integers(1, 20, nn)
    nd["k_end"] = rng.normal(size=(nn, 3)) * 1e-5
    nd["k_end"][rng.random(nn) < 0.1] = np.nan  # rows no table counts: the species' totals still do
    nd["x_end"] = rng.normal(size=(nn, 3)) * 100.0
    nd["u7_end"] = rng.normal(size=nn) * 1e-11
    bk = np.zeros(n, NODE_DTYPE)
    bk["tree"], bk["prob"], bk["weight"] = np.arange(n), 1.0, 1.0
    w5 = np.zeros((5, n))
    w5[0], w5[2] = rng.uniform(-1, 1, n), rng.integers(1, 4, n)  # cos_w, sln_prob
    sample = {"x": up(rng.normal(size=3 * n) * 30.0), "k_init": up(rng.normal(size=3 * n) * 1e-5),
              "erg": up(np.full(n, 1e-5)), "attempts": up(rng.integers(1, 6, n).astype(np.int32))}
    recs = lambda a: up(a.view(np.uint8).reshape(len(a), NODE_DTYPE.itemsize))  # noqa: E731
    ones = up(np.ones(n, np.int32))
    back = {"nodes": recs(bk), "counts": ones, "n_nodes": n}
    fwd = {"nodes": recs(nd), "node_start": up(np.r_[0, np.cumsum(SIZES)].astype(np.int64)),
           "counts": up(np.asarray(SIZES, np.int32)), "infos": up(np.zeros(n, np.int32)), "n_nodes": nn}
    return (sample, up(w5), back, fwd), nd, recs


def test_synthetic_forest_sizes_and_a_misplaced_record():
    sky = dict(n_theta=2, n_phi=3, n_dw=1)  # coarse: a tree of 300 has many rows in a bin
    parts, nd, recs = _synthetic_forest()
    er, got, ref = _rows_and_moments(parts, sky)
    rows = er["rows"].cpu().numpy()
    pps = rows[:, 8] * rows[:, 7]
    assert len(rows) == (nd["is_final"] != 0).sum() and np.array_equal(pps, np.rint(pps)) and set(rows[:, 1]) == {0.0, 1.0}
    labels = er["bins"].cpu().numpy()
    assert (labels < 0).any() and ref["sky_g"][1].max() > 8
    for name in ("sky", "flux"):
        _, Q, Cc = ref[name]
        assert np.array_equal(got[name + "_sq"], Q) and np.array_equal(got[name + "_xa"], Cc), name
    assert np.array_equal(got["totals"], _totals_ref(ref))
    # a final record of tree 3 inside the range of tree 7: counted in totals[7] and skipped
    start = np.r_[0, np.cumsum(SIZES)]
    fin = np.flatnonzero(nd["is_final"] != 0)
    q = fin[(fin >= start[7] + 100)][0]
    bad = nd.copy()
    bad["tree"][q] = 3
    s, w5, back, fwd = parts
    got_bad = _host(_engine().event_moments(s, w5, back, dict(fwd, nodes=recs(bad)), nbins=NBINS, sky=sky))
    keep = np.arange(len(rows)) != np.searchsorted(fin, q)
    ref_bad = _reference(rows[keep], labels[keep].astype(np.int64), s["attempts"].cpu().numpy(), 0, sky)
    assert got_bad["totals"][7] == 1
    want = _totals_ref(ref_bad)
    want[7] = 1
    assert np.array_equal(got_bad["totals"], want) and not np.array_equal(got_bad["totals"][3:7], got["totals"][3:7])
    for name in ("sky", "flux"):
        _, Q, Cc = ref_bad[name]
        assert np.array_equal(got_bad[name + "_sq"], Q) and np.array_equal(got_bad[name + "_xa"], Cc), name


# ---- 5. run_events(errors=True): σ with and without rows, against numpy on the returned rows

def _var_check(what, sig_a, sig_b, S, Q, Cc, g, f, A2, n, sides=1):
    """two σ arrays of the same tables through V (module docstring)"""
    sig_a, sig_b, S, Q, Cc = (np.asarray(v, np.float64).reshape(-1) for v in (sig_a, sig_b, S, Q, Cc))
    E, m, cnt = g
    F = S / f
    bQ, bC, bS = _bound(Q, Q, g), _bound(Cc, Cc, g), 2 * (cnt + 1) * U * S
    dV = sides * (bQ + 2 * F * bC + (2 * Cc + 2 * F * A2) * bS / f + 8 * U * (Q + 2 * F * Cc + F * F * A2))
    Va, Vb = ((s * f) ** 2 * (n - 1) / n for s in (sig_a, sig_b))
    assert np.all(np.isfinite(sig_a)) and np.all(np.isfinite(sig_b))
    err = np.abs(Va - Vb)
    ratio = float(np.max(err[dV > 0] / dV[dV > 0])) if (dV > 0).any() else 0.0
    _report(what, bound_ratio_max=ratio)
    assert np.all(err <= dV), (what, ratio)


def test_run_events_sigma_with_and_without_rows():
    from adiabatic_raytracer_amd import trees as T
    eng, sky = _engine(), dict(n_theta=6, n_phi=11, n_dw=1)
    r = _np(eng.run_events(N, seed=SEED, sky_map=sky, errors=True))
    q = _np(eng.run_events(N, seed=SEED, sky_map=sky, errors=True, rows=False, chunk=400))
    assert q["rows"] is None and r["f_inx"] == q["f_inx"]
    assert set(r) - set(_np(eng.run_events(4, seed=SEED, sky_map=sky))) == {"flux_sigma", "sky_map_sigma",
                                                                           "sum_weight_sln_prob_sigma", "moments"}
    rows = r["rows_raw"]
    att = eng.sample(N, seed=SEED)["attempts"].cpu().numpy()
    ref = _reference(rows, T.sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **sky), att, 0, sky)
    mt = _totals_ref(ref)
    f, A2 = float(r["f_inx"]), mt[2]
    assert mt[1] == f and r["moments"]["totals"].cpu().numpy()[0] == N
    for name, key, shape in (("flux", "flux_sigma", (2, NBINS)), ("sky", "sky_map_sigma", (2, 6, 11, 1))):
        S, Q, Cc = ref[name]
        want = T.moments_sigma(S, Q, Cc, f, A2, N)
        assert r[key].shape == q[key].shape == shape and (want[ref[name + "_g"][0] > 0] > 0).all()
        _var_check(f"run_{name}_rows", r[key], want, S, Q, Cc, ref[name + "_g"], f, A2, N)
        _var_check(f"run_{name}_norows", q[key], want, S, Q, Cc, ref[name + "_g"], f, A2, N)
        _var_check(f"run_{name}_rows_vs_norows", r[key], q[key], S, Q, Cc, ref[name + "_g"], f, A2, N, sides=2)
    S, Q, Cc = ref["tot"]
    want = T.moments_sigma(S, Q, Cc, f, A2, N)
    for res, tag in ((r, "rows"), (q, "norows")):
        _var_check(f"run_tot_{tag}", res["sum_weight_sln_prob_sigma"], want, S, Q, Cc, ref["tot_g"], f, A2, N)
    # a σ is in its estimate's units, and a relative error below 1 somewhere shows it is not a blow-up
    rel = r["flux_sigma"][1][r["flux"][1] > 0] / r["flux"][1][r["flux"][1] > 0]
    _report("run_flux_relative_sigma", smallest=float(rel.min()), median=float(np.median(rel)))
    assert rel.min() < 1.0


# ---- 6. cyclotron, 65 events

def test_cyclotron_65_reuses_the_rerun(monkeypatch):
    eng, sky = _engine(), dict(n_theta=3, n_phi=4, n_dw=1)
    parts = _pipeline("flat", 0, 65)
    er, got, ref = _rows_and_moments(parts, sky, saveMode=1, cyclotron=True)
    rows = er["rows"].cpu().numpy()
    assert (rows[:, 14] > 0).any() and er["totals"][5].item() == 0  # column 8 carries exp(-τ)
    _check_weighted("cyclotron_65", got, ref, ("sky", "flux", "tot"))
    _, plain, _ = _rows_and_moments(parts, sky)
    assert plain["totals"][4] > got["totals"][4]  # the absorbed photons' second moment is smaller
    calls = []
    orig = type(eng).propagate

    def counting(self, *a, **kw):
        calls.append(bool(kw.get("cyclotron")))
        return orig(self, *a, **kw)

    monkeypatch.setattr(type(eng), "propagate", counting)
    r = _np(eng.run_events(65, seed=SEED, cyclotron=True, errors=True, sky_map=sky))
    assert calls == [True]  # one chunk: one cyclotron propagation, event_rows', and none by event_moments
    run = _host(r["moments"])
    for k in ("flux_sq", "flux_xa", "sky_sq", "sky_xa"):
        g = ref[k[:-3] + "_g"]
        assert np.all(np.abs(run[k] - got[k]) <= _bound(run[k], got[k], g)), k
    assert np.array_equal(run["totals"][[0, 1, 2, 7]], got["totals"][[0, 1, 2, 7]])


# ---- 7. main_runner_tree(errors=True), 48 events

def test_main_runner_tree_errors(tmp_path):
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import trees as T
    p = _params("flat")
    sky = dict(n_theta=4, n_phi=6, n_dw=1)
    info_h, info_d, info_0, info_1 = {}, {}, {}, {}
    kw = dict(run_info=info_h, sky_map=sky, file_tag="s")
    rows = A.trees.main_runner_tree(p, 49, dir_tag=str(tmp_path / "h"), device_trees=True, errors=True, **kw)
    A.trees.main_runner_tree(p, 49, dir_tag=str(tmp_path / "d"), device_events=True, errors=True, **dict(kw, run_info=info_d))
    A.trees.main_runner_tree(p, 49, dir_tag=str(tmp_path / "0"), device_events=True, **dict(kw, run_info=info_0))
    A.trees.main_runner_tree(p, 49, device_trees=True, **dict(kw, run_info=info_1))
    today = {"f_inx", "flux", "sum_weight_sln_prob", "rows", "events", "n_events", "sky_map", "sky_map_edges"}
    new = {"flux_sigma", "sky_map_sigma", "sum_weight_sln_prob_sigma"}
    assert set(info_0) == set(info_1) == today and set(info_h) == set(info_d) == today | new
    npz = lambda d: np.load([f for f in (tmp_path / d / "npy").iterdir() if f.suffix == ".npz"][0])  # noqa: E731
    names = {"sky_map", "theta_edges", "phi_edges", "dw_edges", "theta_axis", "f_inx"}
    assert set(npz("0").files) == names and set(npz("h").files) == set(npz("d").files) == names | {"sky_map_sigma"}
    assert np.array_equal(npz("d")["sky_map_sigma"], info_d["sky_map_sigma"], equal_nan=True)
    for k in ("f_inx", "rows"):
        assert info_h[k] == info_d[k] == info_0[k]
    # the bound's tables from the returned rows (column 7 is divided by f_inx there: magnitudes only)
    f, n = float(info_h["f_inx"]), 48
    raw = rows.copy()
    raw[:, 7] *= f
    att = _engine().sample(n, seed=SEED)["attempts"].cpu().numpy()  # (main_runner_tree's default seed)
    ref = _reference(raw, T.sky_bins(raw[:, 2], raw[:, 3], raw[:, 12], raw[:, 1], **sky), att, 0, sky)
    A2 = _totals_ref(ref)[2]
    assert _totals_ref(ref)[1] == f
    for name, key in (("flux", "flux_sigma"), ("sky", "sky_map_sigma"), ("tot", "sum_weight_sln_prob_sigma")):
        S, Q, Cc = ref[name]
        assert np.shape(info_h[key]) == np.shape(info_d[key]) and np.nansum(info_h[key]) > 0
        _var_check(f"main_runner_{name}", info_d[key], info_h[key], S, Q, Cc, ref[name + "_g"], f, A2, n, sides=2)


# ---- 8. edges: no events, one event

def test_edges_no_events_and_one_event():
    eng = _engine()
    r0 = _np(eng.run_events(0, errors=True, sky_map={}))
    assert r0["flux_sigma"].shape == (2, 50) and np.isnan(r0["flux_sigma"]).all()
    assert r0["sky_map_sigma"].shape == (2, 32, 64, 1) and np.isnan(r0["sky_map_sigma"]).all()
    assert np.isnan(r0["sum_weight_sln_prob_sigma"]).all()
    assert all(v is not None and not v.any() for v in _host(r0["moments"]).values())
    r1 = _np(eng.run_events(1, seed=SEED, errors=True, sky_map={}))
    m1 = _host(r1["moments"])
    f = float(r1["f_inx"])
    assert np.array_equal(m1["totals"][[0, 1, 2, 7]], [1.0, f, f * f, 0.0])
    assert np.isnan(r1["flux_sigma"]).all() and np.isnan(r1["sky_map_sigma"]).all()
    # one event: Q = S², C = S a, the event's bin contents summed in another order (at most n_rows rows in a bin)
    nr = r1["n_rows"]
    for S, name in ((r1["flux_raw"], "flux"), (r1["sky_raw"].reshape(-1), "sky")):
        tol = 2 * (2 * nr + 3) * U
        assert np.all(np.abs(m1[name + "_sq"] - S * S) <= tol * S * S) and np.all(np.abs(m1[name + "_xa"] - S * f) <= tol * S * f)
    assert (m1["flux_sq"].sum() > 0) == (r1["flux_raw"].sum() > 0)
