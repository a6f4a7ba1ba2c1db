"""The halo scan on the GPU (art_event_halo_scan_device, Engine.event_halo_scan, run_events(halos=),
main_runner_tree(device_events=True, halos=)): 600 events of the flat configuration sampled and weighted under
the base Halo(260, (0, 230, 0)) -- more than two 256-lane blocks of events, a ragged last block, several
blocks of node records -- reweighted to [the base itself, Halo(220, (0, 230, 0)), Halo(260, (100, 180, -60))]
and held against trees.halo_ratio, numpy binning of the device's own rows, and direct runs under the targets.

Bounds, u = 2^-53, for an event of speed s = |vifty| c and a target h seen from the base b, vp the proposal:
  t = s²/vp²,  Q_x = (s + |v_x|)²/v0_x²
  ρ = (8 (Q_b + Q_h) + 8) u             relative: R on the device against numpy
  β = 8 (2t + 2 Q_b + 2 Q_h + 3) u      relative: column 7 of the base run times R against the direct run's
  adds  a table bin is a sum of the same terms in another order: 2 (cnt + 1) u S per bin of cnt rows
        (tests/test_gpu_event_rows.py); where the terms differ, their own bounds are added (Σ β p).
ρ and β are ceilings on the roundings of the squares, the difference of the exponents, two exponentials within
an ulp of libm and the prefactor; they stay below 1e-12 here. ART_PARITY_REPORT=path collects the JSON lines
the tests print (measured ÷ bound). Measured on an MI355X (profiles/halo_scan_parity.jsonl; DESIGN.md §3, "Halo
scan"): speeds up to 896 km/s, R from 1.1e-3 to 9.6, bit-equal to numpy's on 95 % of the values and at most 0.07
of ρ elsewhere; identity tables 0.23 of the add-order bound, tables against numpy 0.24; against the two direct
runs 1102 rows bit-equal but column 7, column 7 at most 0.09 of β, tables 0.09 of their bound; chunks 0.13;
σ per model at most 0.27 of the bound on V; n_eff 176 (the base), 137 and 169 of 600 events."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest

from test_gpu_event_moments import _bound as _moment_bound
from test_gpu_event_moments import _groups, _var_check
from test_gpu_event_rows import SEED, U, _np, _params

pytestmark = pytest.mark.gpu

AXION, PHOTON = 0, 1
N, NBINS = 600, 50
C_KM = 2.99792e5
SKY = dict(n_theta=6, n_phi=11, n_dw=4, dw_range=(-1 - 1e-6, -1 + 3e-6))
SKY_SIZE = 2 * 6 * 11 * 4

_cache = {}


def _report(what, **vals):
    line = json.dumps({"test": "halo_scan", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _halos():
    import adiabatic_raytracer_amd as A
    base = A.Halo(260.0, (0.0, 230.0, 0.0))
    return base, [base, A.Halo(220.0, (0.0, 230.0, 0.0)), A.Halo(260.0, (100.0, 180.0, -60.0))]


def _eng():
    from adiabatic_raytracer_amd.engine import Engine
    if "eng" not in _cache:
        p = _params("flat")
        _cache["eng"] = (Engine(p), Engine(replace(p, B0=-p.B0)))
    return _cache["eng"]


def _pipe(lo, c):
    """run_events' steps for events [lo, lo + c) under the base halo: (sample, weight5, back, forward)"""
    if ("pipe", lo, c) not in _cache:
        eng, beng = _eng()
        base, _ = _halos()
        s = eng.sample(c, seed=SEED, ray_offset=lo, halo=base)
        w5 = eng.event_weight(s, halo=base)
        back = beng.grow_trees(s["x"], -s["k_init"], s["erg"], AXION, num_cutoff=0, splittings_cutoff=100000,
                               crossing_cap=256, seed=SEED, tree_offset=lo)
        fwd = eng.grow_trees(s["x"], s["k_init"], s["erg"], PHOTON, seed=SEED, tree_offset=lo)
        _cache[("pipe", lo, c)] = (s, w5, back, fwd)
    return _cache[("pipe", lo, c)]


def _host(scan):
    import torch
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in scan.items()}


def _scan(lo=0, c=N, **kw):
    base, models = _halos()
    return _eng()[0].event_halo_scan(*_pipe(lo, c), base, models, event_offset=lo, nbins=NBINS, sky=SKY, **kw)


def _whole():
    """the scan of all N events in one call, with the ratios, and event_rows' own rows and tables"""
    if "whole" not in _cache:
        er = _eng()[0].event_rows(*_pipe(0, N), nbins=NBINS, sky=SKY, return_bins=True)
        _cache["whole"] = (_host(_scan(return_ratio=True)), {k: er[k].cpu().numpy() for k in ("rows", "flux", "sky_hist", "totals", "bins")})
    return _cache["whole"]


def _speed():
    """s = |vifty| c per event, from the sample"""
    v = _pipe(0, N)[0]["vifty"].cpu().numpy().reshape(3, N) * C_KM
    return np.sqrt((v * v).sum(axis=0))


def _Q(s, h):
    return (s + np.linalg.norm(h.v_ns)) ** 2 / h.v0 ** 2


def _rho(s, b, h):
    return (8.0 * (_Q(s, b) + _Q(s, h)) + 8.0) * U


def _beta(s, b, h):
    return 8.0 * (2.0 * s * s / b.vp() ** 2 + 2.0 * _Q(s, b) + 2.0 * _Q(s, h) + 3.0) * U


def _labels(rows):
    """name -> (label per row, table size) of the three tables, by numpy's rules"""
    from adiabatic_raytracer_amd import trees as T
    sp = rows[:, 1].astype(np.int64)
    fb = T.hist_bins(rows[:, 3], NBINS)
    return {"flux": (np.where(fb >= 0, sp * NBINS + fb, -1), 2 * NBINS),
            "sky": (T.sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **SKY), SKY_SIZE), "totals": (sp, 2)}


def _binned(lab, size, w):
    k = lab >= 0
    return np.bincount(lab[k], minlength=size), np.bincount(lab[k], weights=w[k], minlength=size)


def _tables(sc, k):
    return {"flux": sc["flux"][k], "sky": sc["sky"][k].reshape(-1), "totals": sc["totals"][k, :2]}


def _within(what, got, ref, tol, cnt):
    e = np.abs(got - ref)
    worst = float((e[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    assert np.all(e <= tol), (what, worst)
    assert np.all(got[cnt == 0] == 0) and np.all(ref[cnt == 0] == 0), what
    return worst


# ---- 1. the ratios against numpy

def test_ratio_against_numpy():
    from adiabatic_raytracer_amd import trees as T
    base, models = _halos()
    sc, _ = _whole()
    R = sc["ratio"]
    assert R.shape == (3, N) and np.all(np.isfinite(R)) and np.all(R > 0)
    Rn = T.halo_ratio(_pipe(0, N)[0]["vifty"].cpu().numpy(), base, models)
    s = _speed()
    worst = []
    for k, h in enumerate(models):
        tol = _rho(s, base, h)
        assert tol.max() < 1e-12
        rel = np.abs(R[k] - Rn[k]) / Rn[k]
        worst.append(float((rel / tol).max()))
        assert np.all(rel <= tol), (k, worst[-1])
    _report("ratio_numpy", worst_over_bound=worst, bit_equal_share=float(np.mean(R == Rn)), s_max=float(s.max()),
            ratio_min=float(R.min()), ratio_max=float(R.max()))


# ---- 2. identity: the base among the models

def test_identity_at_the_base():
    sc, er = _whole()
    assert np.array_equal(sc["ratio"][0], np.ones(N))
    rows = er["rows"]
    p = rows[:, 8] * rows[:, 7]
    own = {"flux": er["flux"], "sky": er["sky_hist"].reshape(-1), "totals": er["totals"][2:4]}
    lab = _labels(rows)
    assert np.array_equal(lab["sky"][0], er["bins"].astype(np.int64))  # numpy's sky labels are the device's
    worst = 0.0
    for name, (lb, size) in lab.items():
        cnt, S = _binned(lb, size, p)
        assert S.sum() > 0
        worst = max(worst, _within(name, _tables(sc, 0)[name], own[name], 2 * (cnt + 1) * U * S, cnt))
    assert (lab["sky"][0] >= 0).sum() > 100 and len(set(lab["sky"][0][lab["sky"][0] >= 0] % 4)) > 1  # several Δω bins are filled
    _report("identity_tables", worst_over_bound=worst, rows=int(len(rows)))


# ---- 3. the tables against numpy binning of the device's own rows and ratios

def test_tables_against_numpy():
    from adiabatic_raytracer_amd import trees as T
    sc, er = _whole()
    rows, R = er["rows"], sc["ratio"]
    assert _pipe(0, N)[3]["n_nodes"] > 3 * 256  # several blocks of node records
    ref = T.halo_scan_tables(rows, R, NBINS, SKY)
    ev = rows[:, 0].astype(np.int64) - 1
    p = rows[:, 8] * rows[:, 7]
    worst = 0.0
    for k in range(3):
        for name, (lb, size) in _labels(rows).items():
            cnt, S = _binned(lb, size, p * R[k, ev])
            worst = max(worst, _within((name, k), _tables(sc, k)[name], ref[name][k].reshape(-1), 2 * (cnt + 1) * U * S, cnt))
        for col, want in ((2, R[k].sum()), (3, (R[k] * R[k]).sum())):
            assert abs(sc["totals"][k, col] - want) <= 2 * (N + 1) * U * want, (k, col)
    assert np.all(sc["totals"][:, 4] == 0)  # misplaced
    assert sc["totals"][0, 2] == N and sc["totals"][0, 3] == N
    _report("tables_numpy", worst_over_bound=worst, ratio_sum=[float(v) for v in sc["totals"][:, 2]],
            ratio_sq=[float(v) for v in sc["totals"][:, 3]])


# ---- 4. against direct runs under the target models, drawn with the base's proposal

def _run(halo, **kw):
    key = ("run", halo.v0, tuple(halo.v_ns), halo.v_prop, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = _np(_eng()[0].run_events(N, seed=SEED, halo=halo, **kw))
    return _cache[key]


def test_against_direct_runs():
    import adiabatic_raytracer_amd as A
    base, models = _halos()
    sc, _ = _whole()
    b = _run(base, saveMode=1, nbins=NBINS, sky_map=SKY)
    rows = b["rows_raw"]
    ev = rows[:, 0].astype(np.int64) - 1
    s = _speed()
    lab = _labels(rows)
    other = [c for c in range(rows.shape[1]) if c != 7]
    for k in (1, 2):
        h = models[k]
        d = _run(A.Halo(h.v0, h.v_ns, v_prop=base.vp()), saveMode=1, nbins=NBINS, sky_map=SKY)
        assert (d["f_inx"], d["n_rows"], d["n_photon_rows"]) == (b["f_inx"], b["n_rows"], b["n_photon_rows"])
        dr = d["rows_raw"]
        assert dr.shape == rows.shape and np.array_equal(dr[:, other], rows[:, other], equal_nan=True)  # bit-equal but column 7
        be = _beta(s, base, h)
        assert be.max() < 1e-12
        mine = rows[:, 7] * sc["ratio"][k, ev]
        rel = np.abs(dr[:, 7] - mine) / dr[:, 7]
        w7 = float((rel / be[ev]).max())
        assert np.all(rel <= be[ev]), w7
        # the tables: the direct run's own against the scan's, add order plus Σ β p
        p = dr[:, 8] * dr[:, 7]
        worst = 0.0
        for name, (lb, size) in lab.items():
            cnt, S = _binned(lb, size, p)
            _, dS = _binned(lb, size, be[ev] * p)
            ref = {"flux": d["flux_raw"], "sky": d["sky_raw"].reshape(-1), "totals": d["totals"][2:4]}[name]
            worst = max(worst, _within((name, k), _tables(sc, k)[name], ref, 2 * (cnt + 1) * U * S + dS, cnt))
        _report("direct", model=[h.v0, list(h.v_ns)], rows=int(len(rows)), column7_over_beta=w7, tables_over_bound=worst)


# ---- 5. chunks

def test_chunks_256_256_88_against_one_chunk():
    whole, er = _whole()
    acc, Rs = None, []
    for lo, c in ((0, 256), (256, 256), (512, 88)):
        acc = _scan(lo, c, scan=acc, return_ratio=True)
        Rs.append(acc["ratio"].cpu().numpy())
    assert np.array_equal(np.concatenate(Rs, axis=1), whole["ratio"])  # bit-identical
    a = _host(acc)
    assert a["n_events"] == N and np.all(a["totals"][:, 4] == 0)
    rows = er["rows"]
    ev = rows[:, 0].astype(np.int64) - 1
    p = rows[:, 8] * rows[:, 7]
    worst = 0.0
    for k in range(3):
        for name, (lb, size) in _labels(rows).items():
            cnt, S = _binned(lb, size, p * whole["ratio"][k, ev])
            worst = max(worst, _within((name, k), _tables(a, k)[name], _tables(whole, k)[name], 2 * 2 * (cnt + 1) * U * S, cnt))
        for col in (2, 3):
            assert abs(a["totals"][k, col] - whole["totals"][k, col]) <= 2 * 2 * (N + 1) * U * whole["totals"][k, col]
    _report("chunks", worst_over_bound=worst)
    with pytest.raises(ValueError, match="scan"):  # a scan made for other models is refused
        _eng()[0].event_halo_scan(*_pipe(0, 256), _halos()[0], _halos()[1][:2], nbins=NBINS, sky=SKY, scan=acc)


# ---- 6. errors

def test_errors_per_model():
    from adiabatic_raytracer_amd import trees as T
    base, models = _halos()
    r = _run(base, nbins=NBINS, sky_map=SKY, errors=True, halos=models)
    hs = r["halo_scan"]
    assert hs["flux_sigma"].shape == (3, 2, NBINS) and hs["sky_map_sigma"].shape == (3, 2, 6, 11, 4)
    assert hs["sum_weight_sln_prob_sigma"].shape == (3, 2) and hs["n_eff"].shape == (3,) and hs["misplaced"] == 0
    assert hs["flux"].shape == (3, 2, NBINS) and hs["sky_map"].shape == (3, 2, 6, 11, 4) and hs["sum_weight_sln_prob"].shape == (3, 2)
    assert [(m[0], tuple(m[1])) for m in hs["models"]] == [(h.v0, tuple(h.v_ns)) for h in models]
    R = _whole()[0]["ratio"]
    rows = r["rows_raw"]
    ev, sp = rows[:, 0].astype(np.int64) - 1, rows[:, 1].astype(np.int64)
    att = _pipe(0, N)[0]["attempts"].cpu().numpy()
    a = att.astype(np.int64) - 1 + np.bincount(ev[sp == 1], minlength=N)
    f, A2 = float(r["f_inx"]), float((a * a).sum())
    lab = _labels(rows)
    keys = (("flux", "flux_sigma"), ("sky", "sky_map_sigma"), ("totals", "sum_weight_sln_prob_sigma"))
    for k in range(3):
        p = (rows[:, 8] * rows[:, 7]) * R[k, ev]
        for name, key in keys:
            lb, size = lab[name]
            S, Q, Cc = T.event_moments(ev, lb, p, size, a)
            _var_check(f"halo_sigma_{name}_{k}", hs[key][k], T.moments_sigma(S, Q, Cc, f, A2, N), S, Q, Cc, _groups(ev, lb, size),
                       f, A2, N)
    # at the base the scan's σ are the run's own (two device results: both sides of the bound)
    p = rows[:, 8] * rows[:, 7]
    for name, key in keys:
        lb, size = lab[name]
        S, Q, Cc = T.event_moments(ev, lb, p, size, a)
        _var_check(f"halo_sigma_{name}_base", hs[key][0], np.asarray(r[key], np.float64), S, Q, Cc, _groups(ev, lb, size), f, A2, N,
                   sides=2)
    # n_eff of the base: S² / Q of the run's own photon total, each within its add-order bound
    S, Q = r["totals"][3], r["moments"]["totals"].cpu().numpy()[4]
    g = _groups(ev, sp, 2)
    cnt = g[2][1]
    rel = 2 * 2 * 2 * (cnt + 1) * U + 2 * _moment_bound(Q, Q, (g[0][1], g[1][1], cnt)) / Q + 8 * U
    assert abs(hs["n_eff"][0] - S * S / Q) <= rel * (S * S / Q)
    assert np.all(hs["n_eff"] > 0) and np.all(hs["n_eff"] <= N)
    _report("n_eff", n_eff=[float(v) for v in hs["n_eff"]], events=N)


# ---- 7. off: halos=None is the parent's result, key for key

def _close(x, y, n_terms):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and np.all(np.abs(x - y) <= 2 * 2 * (n_terms + 1) * U * np.maximum(np.abs(x), np.abs(y)))


def test_off_by_default_and_main_runner_tree():
    import adiabatic_raytracer_amd as A
    import torch
    eng = _eng()[0]
    base, models = _halos()
    a = eng.run_events(200, seed=SEED, sky_map=SKY, halo=base)
    b = eng.run_events(200, seed=SEED, sky_map=SKY, halo=base, halos=models)
    assert set(b) - set(a) == {"halo_scan"}
    assert set(a) == {"rows", "flux", "f_inx", "sum_weight_sln_prob", "n_rows", "n_photon_rows", "totals", "flux_raw",
                      "rows_raw", "sky_map", "sky_raw", "sky_map_edges"}
    for k in ("rows", "rows_raw"):
        assert torch.equal(a[k], b[k])  # the scan does not touch the run's own rows
    assert a["f_inx"] == b["f_inx"] and a["n_rows"] == b["n_rows"]
    hb = b["halo_scan"]
    assert set(hb) == {"models", "flux", "sky_map", "sum_weight_sln_prob", "ratio_sum", "ratio_sq", "misplaced", "f_inx", "raw"}
    nr = a["n_rows"]
    assert _close(hb["flux"][0], a["flux"].cpu().numpy(), nr) and _close(hb["sky_map"][0], a["sky_map"].cpu().numpy(), nr)
    assert hb["ratio_sum"][0] == 200 and hb["misplaced"] == 0
    # rows=False: the large-run mode
    c = eng.run_events(200, seed=SEED, sky_map=SKY, halo=base, halos=models, rows=False, chunk=96)
    assert c["rows"] is None
    for k in ("flux", "sky_map", "sum_weight_sln_prob", "ratio_sum", "ratio_sq"):
        assert _close(c["halo_scan"][k], hb[k], nr), k
    # refused before any work: no base, an empty list, too many, a model wider than the base's proposal
    for halo, bad in ((None, models), (base, []), (base, [base] * 33), (base, [A.Halo(400.0)])):
        with pytest.raises(ValueError, match="halos: "):
            eng.run_events(0, halo=halo, halos=bad)
    # main_runner_tree(device_events=True)
    p = _params("flat")
    i0, i1 = {}, {}
    r0 = A.trees.main_runner_tree(p, 201, seed=SEED, device_events=True, run_info=i0, sky_map=SKY, halo=base)
    r1 = A.trees.main_runner_tree(p, 201, seed=SEED, device_events=True, run_info=i1, sky_map=SKY, halo=base, halos=models)
    assert set(i1) - set(i0) == {"halo_scan"} and np.array_equal(r0, r1, equal_nan=True)
    assert set(i0) == {"f_inx", "flux", "sum_weight_sln_prob", "rows", "events", "n_events", "sky_map", "sky_map_edges"}
    assert np.array_equal(r0, b["rows"].cpu().numpy(), equal_nan=True)
    hm = i1["halo_scan"]
    for k in ("flux", "sky_map", "sum_weight_sln_prob", "ratio_sum", "ratio_sq"):
        assert _close(hm[k], hb[k], nr), k
    assert hm["models"] == hb["models"] and hm["misplaced"] == 0
    for kw in ({}, {"device_trees": True}):
        with pytest.raises(ValueError, match="device_events"):
            A.trees.main_runner_tree(p, 5, halo=base, halos=models, **kw)
    # both scans in one run: each is the one of the run with it alone
    g = [p.g_agg / 2, 3 * p.g_agg]
    both = eng.run_events(200, seed=SEED, sky_map=SKY, halo=base, halos=models, couplings=g)
    only = eng.run_events(200, seed=SEED, sky_map=SKY, halo=base, couplings=g)
    assert set(both) - set(a) == {"halo_scan", "coupling_scan"}
    for k in ("flux", "sky_map", "sum_weight_sln_prob", "ratio_sum", "ratio_sq"):
        assert _close(both["halo_scan"][k], hb[k], nr), k
    for k in ("flux", "sky_map", "sum_weight_sln_prob", "coverage"):
        assert _close(both["coupling_scan"][k], only["coupling_scan"][k], nr + 200), k
    assert both["coupling_scan"]["unlinked"] == 0
    # trees.line_profile and pulse_profile take sky_map[k] as they take the run's own
    prof, centres = A.trees.line_profile(hb["sky_map"][1], 1.0, SKY["dw_range"])
    assert prof.shape == centres.shape == (4,) and np.all(prof >= 0)
    assert A.trees.pulse_profile(hb["sky_map"][2], 1.0)[0].shape == (11,)


# ---- 8. the line position per model: report only (heavy-tailed weights: 600 events do not order it)

def test_report_line_position():
    _, models = _halos()
    sc, er = _whole()
    rows = er["rows"]
    ev = rows[:, 0].astype(np.int64) - 1
    ph = rows[:, 1] == 1
    v = _pipe(0, N)[0]["vifty"].cpu().numpy().reshape(3, N)
    vel = (v * v).sum(axis=0) / 2.0
    p = rows[:, 8] * rows[:, 7]
    out = []
    for k in range(3):
        w = (p * sc["ratio"][k, ev])[ph]
        out.append(float((w * vel[ev][ph]).sum() / w.sum()))
    _report("line_position", models=[[h.v0, list(h.v_ns)] for h in models], mean_vel_eng=out)
