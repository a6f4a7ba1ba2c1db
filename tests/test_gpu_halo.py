"""The halo velocity model on the GPU (include/art.h art_halo; sample_kernel's HALO builds,
event_weight_halo_kernel, the halo= keyword of the sampler, the event weight, Engine.run_events and
main_runner_tree) against numpy's restatement of its three formulas on the sampler's own outputs,
and against the oracle for everything the model leaves alone.

The uniforms of sample i's accepted attempt come from the oracle (oracle_attempt_uniforms(seed,
ray_offset + i, attempts[i] - 1)), so the speed is checked against the draw itself. The conversion
point is checked by a bracket: the oracle's condition at the point's own energy changes sign (or is
0) between x - h va and x + h va along the attempt's line, h = 1e-9 max|x| -- the bound
tests/test_gpu_sampler_prob.py holds the sampler's roots to.

Row rules are those of tests/test_gpu_event_rows.py: the angle columns 2-5 within 4 ulp, every other
column bit-equal; a weighted bin within 2 (terms + 1) u Σ|w| of numpy's sum of the same terms.

ART_PARITY_REPORT=path collects the JSON lines the tests print. Measured on an MI355X
(profiles/halo_parity.jsonl; DESIGN.md §3, "Halo velocity model"), largest relative errors, flat
(4096 samples) / gr_oblique (1024): speed against the draw 1.4e-15 / 8.9e-16 (bound 1e-12); erg
against today's expression of |vifty| 0 / 0 (1e-14); vifty against numpy's asymptote 1.4e-15 /
1.1e-15 (1e-9); the oracle's condition at the points at most 4.8e-15 / 2.7e-15 in value, every
bracket of 1e-9 max|x| holding its root; weight rows 0, 1, 3 against the oracle 8.0e-12 / 1.2e-12
(1e-9), sln_prob against the oracle's times numpy's F 8.0e-12 / 1.2e-12 (1e-9; F from 3.4e-6 to 5.4),
with Halo(220, 0) against the oracle's own 8.0e-12 / 1.2e-12; vel_eng 2 ulp from |vifty|²/2 (4).
600 flat events give 1092 rows: the angle columns 1 ulp from the host assembly's (4), the rest
bit-equal on all three paths; column 12 - u7_end/m_a recovers |vifty|²/2 to 0.083 of its rounding
bound; the (4, 8, 6) sky map's weighted bins at most 0.21 of the bound from np.histogramdd's."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from conftest import CONFIGS
from test_event_rows import _ulps

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
C_KM = 2.99792e5
GNEW = 132712000000.0
AXION, PHOTON = 0, 1
ANGLES = (2, 3, 4, 5)
SEED = 1769
OFFSET = 1000
HALO = dict(v0=200.0, v_ns=(150.0, -60.0, 90.0))
SHAPES = {"flat": 4096, "gr_oblique": 1024}

_cache = {}


def _report(what, **vals):
    line = json.dumps({"test": "halo", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _A():
    import adiabatic_raytracer_amd as A
    return A


def _halo(**kw):
    return _A().Halo(**(kw or HALO))


def _params(cfg):
    return _A().Params(**CONFIGS[cfg])


def _engine(cfg="flat"):
    from adiabatic_raytracer_amd.engine import Engine
    if ("eng", cfg) not in _cache:
        _cache[("eng", cfg)] = Engine(_params(cfg))
    return _cache[("eng", cfg)]


def _samples(cfg):
    """the halo samples of a configuration, drawn once and left unchanged"""
    if ("s", cfg) not in _cache:
        s = _A().sample_conversion_points(_params(cfg), SHAPES[cfg], seed=SEED, ray_offset=OFFSET, halo=_halo())
        for v in s.values():
            v.setflags(write=False)
        _cache[("s", cfg)] = s
    return _cache[("s", cfg)]


def _uniforms(oracle_lib, attempts, n):
    U = np.zeros((n, 10))
    fn = oracle_lib.lib().oracle_attempt_uniforms
    for i in range(n):
        fn(SEED, OFFSET + i, int(attempts[i]) - 1, U[i].ctypes.data_as(C.POINTER(C.c_double)))
    return U


def np_asymptote(x, d, s, GM):
    """the issue's formula as written: u = [s² v + s (GM/r) r̂ - s v_r v] / [s² + GM/r - s v_r]"""
    r = np.linalg.norm(x, axis=1)
    rh = x / r[:, None]
    v = d * np.sqrt(s * s + 2.0 * GM / r)[:, None]
    vr = np.sum(v * rh, axis=1)
    num = (s * s)[:, None] * v + (s * GM / r)[:, None] * rh - (s * vr)[:, None] * v
    return num / (s * s + GM / r - s * vr)[:, None]


def np_factor(u, s, v0, v_ns, vp):
    w = u + np.asarray(v_ns)
    return (220.0 / v0) * (vp / v0) ** 2 * np.exp(s * s / (vp * vp) - np.sum(w * w, axis=1) / (v0 * v0))


def _erg(mass_a, vm):
    """today's expression of |vifty| (MainRunner.jl:514-526)"""
    gA = 1.0 / np.sqrt(1.0 - vm * vm)
    return mass_a * np.sqrt(1.0 + (vm * gA) * (vm * gA))


# ---- 1. off is off

@pytest.mark.parametrize("cfg,n", [("flat", 2048), ("gr", 512)])
def test_null_halo_is_the_old_entry_points(cfg, n):
    import torch
    A = _A()
    p = _params(cfg)
    lib = A._lib.load()
    max_r = p.max_r()
    old = A.sample_conversion_points(p, n, seed=SEED, ray_offset=OFFSET)
    keys = ("x", "k_init", "erg", "vifty", "weights", "attempts")
    new = {k: np.zeros_like(v) for k, v in old.items()}
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    A._lib.check(lib.art_sample_conversion_points_halo_host(C.byref(p.to_c()), None, float(max_r), SEED, OFFSET, n,
                                                            *[ptr(new[k]) for k in keys]))
    for k in keys:
        assert old[k].tobytes() == new[k].tobytes(), k
    w_old = A.raytracer.event_weight(p, old["x"], old["k_init"], old["vifty"])
    out = np.zeros(5 * n)
    A._lib.check(lib.art_event_weight_halo_host(C.byref(p.to_c()), None, float(max_r), 0.45, 6.0, n, ptr(old["x"]),
                                                ptr(old["k_init"]), ptr(old["vifty"]), ptr(out)))
    for i, k in enumerate(A.raytracer.EVENT_FIELDS):
        assert out.reshape(5, n)[i].tobytes() == w_old[k].tobytes(), k
    # the device entry points
    eng = _engine(cfg)
    d_old = eng.sample(n, seed=SEED, ray_offset=OFFSET)
    d_new = {k: torch.zeros_like(v) for k, v in d_old.items()}
    tp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    A._lib.check(lib.art_sample_conversion_points_halo_device(C.byref(eng.cp), None, float(max_r), SEED, OFFSET, n,
                                                              *[tp(d_new[k]) for k in keys], stream))
    for k in keys:
        assert torch.equal(d_old[k], d_new[k]), k
        assert d_old[k].cpu().numpy().tobytes() == old[k].tobytes(), k
    w5 = eng.event_weight(d_old)
    w5n = torch.zeros(5 * n, dtype=torch.float64, device=w5.device)
    A._lib.check(lib.art_event_weight_halo_device(C.byref(eng.cp), None, float(max_r), 0.45, 6.0, n, tp(d_old["x"]),
                                                  tp(d_old["k_init"]), tp(d_old["vifty"]), tp(w5n), stream))
    assert torch.equal(w5.reshape(-1), w5n)


# ---- 2. the sampler, sample by sample

@pytest.mark.parametrize("cfg", sorted(SHAPES))
def test_sampler_per_sample(cfg, oracle_lib):
    kw = CONFIGS[cfg]
    n = SHAPES[cfg]
    s = _samples(cfg)
    H = _halo()
    vp = H.vp()
    assert math.isclose(vp, math.sqrt(200.0 ** 2 + 150.0 ** 2 + 60.0 ** 2 + 90.0 ** 2), rel_tol=1e-15)
    x = s["x"].reshape(3, n).T
    k = s["k_init"].reshape(3, n).T
    vif = s["vifty"].reshape(3, n).T
    assert np.all(np.isfinite(x)) and np.all(s["attempts"] >= 1) and np.all(s["weights"] >= 1)
    Us = _uniforms(oracle_lib, s["attempts"], n)
    # the speed is the draw
    sp = vp * np.sqrt(-np.log(1.0 - Us[:, 6]))
    vm = np.linalg.norm(vif, axis=1)
    e_speed = np.abs(vm * C_KM / sp - 1.0)
    assert e_speed.max() <= 1e-12, e_speed.max()
    assert np.unique(sp).size == n  # (a speed per event)
    # erg: today's expression of |vifty|
    e_erg = np.abs(s["erg"] / _erg(kw["mass_a"], vm) - 1.0)
    assert e_erg.max() <= 1e-14, e_erg.max()
    # vifty is the incoming asymptote through (x, k_init / |k_init|) at that speed
    d = k / np.linalg.norm(k, axis=1)[:, None]
    GM = GNEW * kw.get("mass_ns", 1.0)
    u = np_asymptote(x, d, sp, GM)
    e_asym = np.linalg.norm(vif * C_KM - u, axis=1) / np.linalg.norm(u, axis=1)
    assert e_asym.max() <= 1e-9, e_asym.max()
    # the point is on the conversion surface at its own energy: the root along the attempt's line
    # (direction va of U[0], U[1]) lies within h = 1e-9 max|x| of it
    r = np.linalg.norm(x, axis=1)
    assert np.all(r > kw.get("rNS", 10.0))
    po = oracle_lib.make_params(**kw)
    ct = 1.0 - 2.0 * Us[:, 0]
    st = np.sqrt((1.0 - ct) * (1.0 + ct))
    va = np.stack([st * np.cos(2.0 * np.pi * Us[:, 1]), st * np.sin(2.0 * np.pi * Us[:, 1]), ct], axis=1)
    vloc = d * (np.sqrt(sp * sp + 2.0 * GM / r) / C_KM)[:, None]
    h = 1e-9 * np.abs(x).max()
    worst_c = 0.0
    for i in range(n):
        c0 = oracle_lib.sampler_condition(po, x[i], vloc[i], float(s["erg"][i]))
        worst_c = max(worst_c, abs(c0))
        if c0 == 0.0:
            continue
        ca = oracle_lib.sampler_condition(po, x[i] - h * va[i], vloc[i], float(s["erg"][i]))
        cb = oracle_lib.sampler_condition(po, x[i] + h * va[i], vloc[i], float(s["erg"][i]))
        assert ca * cb <= 0.0, (i, ca, c0, cb)
    _report(f"sampler_{cfg}", n=n, speed_rel_max=float(e_speed.max()), erg_rel_max=float(e_erg.max()),
            asymptote_rel_max=float(e_asym.max()), condition_abs_max=float(worst_c),
            speed_kms_min=float(sp.min()), speed_kms_max=float(sp.max()))


# ---- 3. invariance

def _same(a, b, sl=slice(None)):
    for k in ("x", "k_init", "erg", "vifty", "weights", "attempts"):
        va, vb = a[k], b[k]
        if va.size != a["erg"].size:
            va = va.reshape(3, -1)[:, sl]
            vb = vb.reshape(3, -1)
        else:
            va = va[sl]
        assert np.ascontiguousarray(va).tobytes() == np.ascontiguousarray(vb).tobytes(), k


def test_halves_equal_the_whole():
    A = _A()
    p, H = _params("flat"), _halo()
    whole = _samples("flat")
    n = SHAPES["flat"]
    cut = 1531
    a = A.sample_conversion_points(p, cut, seed=SEED, ray_offset=OFFSET, halo=H)
    b = A.sample_conversion_points(p, n - cut, seed=SEED, ray_offset=OFFSET + cut, halo=H)
    _same(whole, a, slice(0, cut))
    _same(whole, b, slice(cut, n))


def _device_sample(eng, n, H, max_r=None):
    return {k: v.cpu().numpy() for k, v in eng.sample(n, seed=SEED, ray_offset=OFFSET, max_r=max_r, halo=H).items()}


def test_wave_settings_agree():
    from adiabatic_raytracer_amd.engine import Engine
    H = _halo()
    eng = _engine("flat")
    big = Engine(_A().Params(theta_m=0.0, mass_a=1e-6))  # maxR > 60 km: the blocks-of-steps builds
    assert big.params.max_r() > 60.0 >= eng.params.max_r()
    try:
        eng.set_sampler_waves(2)
        a2 = _device_sample(eng, SHAPES["flat"], H)
        b2 = _device_sample(big, 512, H)
        eng.set_sampler_waves(3)
        a3 = _device_sample(eng, SHAPES["flat"], H)
        b3 = _device_sample(big, 512, H)
    finally:
        eng.set_sampler_waves(0)
    _same(a2, a3)
    _same(b2, b3)
    _same(_samples("flat"), a2)  # the host call's samples, too
    assert np.all(np.isfinite(b2["x"])) and np.unique(np.linalg.norm(b2["vifty"].reshape(3, -1), axis=0)).size == 512


# ---- 4. the weight

@pytest.mark.parametrize("cfg", sorted(SHAPES))
def test_weight(cfg, oracle_lib):
    A = _A()
    kw = CONFIGS[cfg]
    n = SHAPES[cfg]
    p, po = _params(cfg), oracle_lib.make_params(**kw)
    s = _samples(cfg)
    H = _halo()
    max_r = p.max_r()
    g = A.raytracer.event_weight(p, s["x"], s["k_init"], s["vifty"], max_r=max_r, halo=H)
    o = oracle_lib.event_weight(po, s["x"], s["k_init"], s["vifty"], oracle_lib.find_conversion_surface(po))
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))  # noqa: E731
    errs = {k: rel(g[k], o[k]) for k in ("cos_w", "jacobian_GR", "erg_inf_ini")}
    for k, e in errs.items():
        assert e <= 1e-9, (k, e)
    vif = s["vifty"].reshape(3, n).T
    u = vif * C_KM
    F = np_factor(u, np.linalg.norm(u, axis=1), H.v0, H.v_ns, H.vp())
    e_w = rel(g["sln_prob"], o["sln_prob"] * F)
    assert e_w <= 1e-9, e_w
    assert F.max() / F.min() > 10.0  # (the factor is at work)
    ve = np.sum(vif * vif, axis=1) / 2.0
    ulp = _ulps(g["vel_eng"], ve)
    assert np.all(ulp <= 4), float(ulp.max())
    # the reference's halo: the oracle's sln_prob itself
    g1 = A.raytracer.event_weight(p, s["x"], s["k_init"], s["vifty"], max_r=max_r, halo=A.Halo(220.0, (0.0, 0.0, 0.0)))
    e_1 = rel(g1["sln_prob"], o["sln_prob"])
    assert e_1 <= 1e-9, e_1
    _report(f"weight_{cfg}", n=n, rows013_rel_max=max(errs.values()), sln_prob_rel_max=e_w, vel_eng_ulp_max=float(ulp.max()),
            reference_halo_rel_max=e_1, factor_min=float(F.min()), factor_max=float(F.max()))


# ---- 5. end to end, 600 flat events

N_EV = 600
H_E2E = dict(v0=220.0, v_ns=(0.0, 230.0, 0.0))


def _check_rows(what, got, ref):
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


def _host_rows():
    """main_runner_tree(device_trees=True, halo=H): the host assembly, once"""
    if "host" not in _cache:
        info = {}
        rows = _A().trees.main_runner_tree(_params("flat"), N_EV + 1, saveMode=1, run_info=info, device_trees=True,
                                           halo=_halo(**H_E2E))
        rows.setflags(write=False)
        _cache["host"] = (rows, info)
    return _cache["host"]


def _dw_range():
    return tuple(float(v) for v in np.quantile(_host_rows()[0][:, 12], [0.02, 0.98]))


def _np(r):
    import torch
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _run(**kw):
    key = ("run", tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = _np(_engine().run_events(N_EV, seed=SEED, saveMode=1, halo=_halo(**H_E2E), **kw))
    return _cache[key]


def test_rows_of_the_three_paths():
    A = _A()
    ref, info = _host_rows()
    assert ref.shape[1] == 29 and len(ref) > N_EV // 2
    r = _run()
    _check_rows("run_events", r["rows"], ref)
    assert r["f_inx"] == info["f_inx"]
    dev = A.trees.main_runner_tree(_params("flat"), N_EV + 1, saveMode=1, device_events=True, halo=_halo(**H_E2E))
    _check_rows("device_events", dev, ref)
    # and the halo changes them: the same run without it
    plain = _np(_engine().run_events(N_EV, seed=SEED, saveMode=1))
    assert plain["rows"].shape != r["rows"].shape or not np.array_equal(plain["rows"][:, 12], r["rows"][:, 12])
    ch = _run(chunk=128)
    assert ch["rows"].tobytes() == r["rows"].tobytes() and ch["f_inx"] == r["f_inx"]


def test_column_12_is_the_line_position():
    from dataclasses import replace
    from adiabatic_raytracer_amd.engine import Engine, nodes_to_numpy
    eng, H = _engine(), _halo(**H_E2E)
    p = eng.params
    s = eng.sample(N_EV, seed=SEED, ray_offset=0, halo=H)
    w5 = eng.event_weight(s, halo=H)
    back = Engine(replace(p, B0=-p.B0)).grow_trees(s["x"], -s["k_init"], s["erg"], AXION, num_cutoff=0,
                                                   splittings_cutoff=100000, crossing_cap=256, seed=SEED, tree_offset=0)
    fwd = eng.grow_trees(s["x"], s["k_init"], s["erg"], PHOTON, seed=SEED, tree_offset=0)
    rows = eng.event_rows(s, w5, back, fwd, saveMode=1)["rows"].cpu().numpy()
    nodes = nodes_to_numpy(fwd["nodes"])
    fin = nodes[nodes["is_final"] != 0]
    assert len(fin) == len(rows) and np.array_equal(rows[:, 0], fin["tree"] + 1.0)
    assert np.array_equal(rows[:, 12], _run()["rows"][:, 12])  # the rows of run_events
    vif = s["vifty"].cpu().numpy().reshape(3, N_EV).T
    ve = (np.sum(vif * vif, axis=1) / 2.0)[fin["tree"]]
    a = fin["u7_end"] / p.mass_a
    # column 12 is fl(a + vel_eng): vel_eng within 4 ulp = 8 u of |vifty|²/2, a one rounded division (u |a|),
    # the sum's rounding (u |col 12|) and this subtraction's (u |col 12 - a|): 11 u of the largest at most
    tol = 12 * U53 * np.maximum(np.maximum(np.abs(a), np.abs(ve)), np.abs(rows[:, 12]))
    err = np.abs((rows[:, 12] - a) - ve)
    assert np.all(err <= tol), float(np.max(err / tol))
    # the intrinsic line: v∞²/2 of order v0²/2c² = 2.7e-7, a value per event
    assert 1e-8 < np.median(ve) < 3e-6 and np.unique(ve).size == np.unique(fin["tree"]).size
    root = (fin["species"] == PHOTON) & (fin["t0"] == 0)
    assert root.sum() > 10 and np.unique(rows[root, 12]).size > 1
    assert np.unique(rows[root, 12] - a[root]).size > 1
    _report("column12", rows=int(len(rows)), root_photons=int(root.sum()), err_over_tol_max=float(np.max(err / tol)),
            vel_eng_median=float(np.median(ve)), dw_plus_1_abs_median=float(np.median(np.abs(rows[:, 12] + 1.0))),
            u7_over_ma_plus_1_median=float(np.median(a + 1.0)), dw_min=float(rows[:, 12].min()), dw_max=float(rows[:, 12].max()))


def test_sky_map_is_histogramdd_of_the_rows():
    shape = (4, 8, 6)
    dw_range = _dw_range()
    sky = dict(n_theta=4, n_phi=8, n_dw=6, dw_range=dw_range)
    r = _run(sky_map=sky)
    rows = r["rows_raw"]
    assert len(rows) > N_EV // 2 and np.array_equal(rows[:, 12], _run()["rows_raw"][:, 12])
    pps = rows[:, 8] * rows[:, 7]
    ranges = ((-1.0, 1.0), (-np.pi, np.pi), dw_range)
    worst = 0.0
    for sp in (AXION, PHOTON):
        m = rows[:, 1] == sp
        pts = np.stack([np.cos(rows[m, 2]), rows[m, 3], rows[m, 12]], axis=1)
        cnt, _ = np.histogramdd(pts, bins=shape, range=ranges)
        ref, _ = np.histogramdd(pts, bins=shape, range=ranges, weights=pps[m])
        got = r["sky_raw"][sp]
        assert got.shape == shape
        err, bound = np.abs(got - ref), 2 * (cnt + 1) * U53 * np.maximum(got, ref)
        assert np.all(err <= bound), (sp, float(np.max(err[cnt > 0] / bound[cnt > 0])))
        if (cnt > 0).any():
            worst = max(worst, float(np.max(err[cnt > 0] / bound[cnt > 0])))
        assert np.array_equal(got > 0, ref > 0)
    assert (r["sky_raw"][PHOTON].sum(axis=(0, 1)) > 0).sum() >= 3  # the line spreads over Δω bins
    # the line profile of the map, the README's use
    prof, centres = _A().trees.line_profile(r["sky_map"], math.pi / 3, dw_range)
    assert prof.shape == (6,) and np.all(prof >= 0) and prof.sum() > 0 and dw_range[0] < centres[0] < centres[-1] < dw_range[1]
    _report("sky_map", bound_ratio_max=worst, dw_range=list(dw_range), bins_filled=int((r["sky_raw"] > 0).sum()))


# ---- 6. validation

@pytest.mark.parametrize("kw,msg", [
    (dict(v0=0.0), "v0"), (dict(v0=-1.0), "v0"), (dict(v0=float("nan")), "v0"), (dict(v0=float("inf")), "v0"),
    (dict(v_ns=(0.0, float("nan"), 0.0)), "v_ns"), (dict(v_ns=(float("inf"), 0.0, 0.0)), "v_ns"),
    (dict(v0=220.0, v_prop=219.0), "v_prop"), (dict(v_prop=3000.5), "v_prop"),
    (dict(v0=220.0, v_ns=(3000.0, 0.0, 0.0)), "v_prop"),
])
def test_invalid_halo(kw, msg):
    A = _A()
    p = _params("flat")
    H = A.Halo(**kw)
    lib = A._lib.load()
    x = np.array([20.0, 0.0, 0.0])
    with pytest.raises(A.ArtError, match=msg):
        A.sample_conversion_points(p, 4, halo=H)
    with pytest.raises(A.ArtError, match=msg):
        A.raytracer.event_weight(p, x, x, x * 1e-4, halo=H)
    out = np.zeros(5)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.art_event_weight_halo_host(C.byref(p.to_c()), C.byref(H.to_c()), 40.0, 0.45, 6.0, 1, ptr(x), ptr(x), ptr(x),
                                        ptr(out))
    assert rc == -1 and msg in lib.art_last_error().decode()  # ART_E_INVALID
    with pytest.raises(A.ArtError, match=msg):
        _engine().sample(4, halo=H)


def test_valid_edges_of_the_halo():
    """v_prop = v0 and v_prop = 3000 are allowed; v_prop <= 0 is the default scale"""
    A = _A()
    p = _params("flat")
    for H in (A.Halo(220.0, (0.0, 0.0, 0.0), 220.0), A.Halo(220.0, (0.0, 0.0, 0.0), 3000.0), A.Halo(220.0, (0.0, 0.0, 0.0), 0.0)):
        s = A.sample_conversion_points(p, 8, seed=SEED, halo=H)
        assert np.all(np.isfinite(s["vifty"])) and np.all(np.linalg.norm(s["vifty"].reshape(3, 8), axis=0) < 0.07)
