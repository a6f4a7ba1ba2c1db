"""Emission maps without a GPU: trees.origin_bins / rows_origin against np.histogramdd, the origin binning of
art_event_origin.h in a host build (tools/eventorigin.py) against trees.origin_bins, the read-offs
(emission_profile, observer_view, origin_jackknife) against numbers worked out here, the argument checks of
art_event_origin_device, which come before any device is touched, and the Python surface.

A weighted bin of np.histogramdd and of np.bincount is a sum of the same non-negative terms in another order: two
such sums differ by at most 2 (cnt + 1) u max(a, b) with cnt the bin's rows and u = 2^-53
(tests/test_gpu_event_rows.py)."""
import ctypes as C
import inspect
import math
from dataclasses import replace

import numpy as np
import pytest

INVALID = -1  # ART_E_INVALID
U = 2.0 ** -53
THETA_M = 0.2


def _params():
    import adiabatic_raytracer_amd as A
    return replace(A.Params(), theta_m=THETA_M)


def _synthetic_rows(n=2000, seed=7):
    """rows with the columns rows_origin reads: event id, species, θf, φf, sln_prob, weight, the sampled x, Δω"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 13))
    rows[:, 0] = rng.integers(1, 400, n)
    rows[:, 1] = rng.integers(0, 2, n)
    rows[:, 2] = np.arccos(rng.uniform(-1, 1, n))
    rows[:, 3] = rng.uniform(-np.pi, np.pi, n)
    rows[:, 7] = rng.uniform(0.1, 2.0, n)
    rows[:, 8] = rng.uniform(0.1, 2.0, n)
    d = rng.normal(size=(n, 3))
    rows[:, 9:12] = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(8.0, 42.0, n)[:, None]
    rows[:, 12] = rng.normal(size=n) * 1e-6
    return rows


# ---- 1. origin_bins / rows_origin against np.histogramdd

@pytest.mark.parametrize("frame", ["magnetic", "rotation"])
@pytest.mark.parametrize("axis", ["cos", "theta"])
def test_rows_origin_is_histogramdd(frame, axis):
    from adiabatic_raytracer_amd import trees as T
    rows = _synthetic_rows()
    spec = T.origin_spec(dict(n_r=2, n_theta=5, n_phi=7, theta_axis=axis, r_range=(10.0, 40.0), frame=frame),
                         dict(n_theta=2, n_phi=3, theta_axis=axis), _params())
    assert spec["shape"] == (2, 2, 3, 2, 5, 7)
    assert (spec["cm"], spec["sm"]) == ((math.cos(THETA_M), math.sin(THETA_M)) if frame == "magnetic" else (1.0, 0.0))
    x, y, z = rows[:, 9], rows[:, 10], rows[:, 11]
    r, a, ph = T.origin_coordinates(x, y, z, spec)
    if frame == "rotation":  # v = (x, y, z), bit for bit
        assert np.array_equal(r, np.sqrt((x * x + y * y) + z * z)) and np.array_equal(ph, np.arctan2(y, x))
    else:
        assert np.array_equal(ph, np.arctan2(y, x * spec["cm"] - z * spec["sm"]))
    ob = T.origin_bins(x, y, z, spec)
    dropped = (r < 10.0) | (r > 40.0)
    assert dropped.sum() > 20 and np.array_equal(ob < 0, dropped)
    oa = np.cos(rows[:, 2]) if axis == "cos" else rows[:, 2]
    coords = np.stack([oa, rows[:, 3], r, a, ph], axis=1)
    edges = T.origin_map_edges(spec)
    assert [len(e) for e in edges] == [3, 4, 3, 6, 8]
    rng = [(e[0], e[-1]) for e in edges]
    unit = rows.copy()
    unit[:, 7] = unit[:, 8] = 1.0
    cnt, got = T.rows_origin(unit, spec), T.rows_origin(rows, spec)
    for sp in (0, 1):
        k = rows[:, 1] == sp
        ref_cnt, _ = np.histogramdd(coords[k], bins=(2, 3, 2, 5, 7), range=rng)
        assert np.array_equal(cnt[sp], ref_cnt)
        ref, _ = np.histogramdd(coords[k], bins=(2, 3, 2, 5, 7), range=rng, weights=(rows[:, 8] * rows[:, 7])[k])
        assert np.all(np.abs(got[sp] - ref) <= 2 * (cnt[sp] + 1) * U * np.maximum(got[sp], ref))
    assert cnt.sum() == (~dropped).sum() and cnt.max() > 1
    # the groups: (column 0 - 1) mod R, and their sum is the table
    grp = T.rows_origin(unit, spec, R=7)
    assert grp.shape == (7,) + spec["shape"] and np.array_equal(grp.sum(axis=0), cnt)
    g3 = (rows[:, 0].astype(np.int64) - 1) % 7 == 3
    assert np.array_equal(grp[3], T.rows_origin(unit[g3], spec))
    # one r bin without a range: every row
    every = T.origin_spec(dict(n_theta=5, n_phi=7, theta_axis=axis, frame=frame), None, _params())
    assert every["shape"] == (2, 1, 1, 1, 5, 7) and T.rows_origin(unit, every).sum() == len(rows)
    assert np.array_equal(T.origin_map_edges(every)[2], [0.0, np.inf])


def test_origin_spec_defaults_and_errors():
    from adiabatic_raytracer_amd import trees as T
    spec = T.origin_spec({}, None, _params())
    assert (spec["n_r"], spec["n_theta"], spec["n_phi"], spec["theta_axis"], spec["frame"]) == (1, 16, 32, "cos", "magnetic")
    assert spec["shape"] == (2, 1, 1, 1, 16, 32) and spec["observer"] is None and T.origin_spec(spec) is spec
    assert T.origin_spec({"mode": "lds"}, None, _params())["mode"] == 1
    # a completed spec is checked again: its shape must follow from its axes, its mode be a number, no observer= beside it
    assert T.origin_spec(dict(spec, mode=2))["mode"] == 2
    for changed in (dict(spec, n_phi=5), dict(spec, mode="lds"), dict(spec, n_r=0, shape=(2, 1, 1, 0, 16, 32))):
        with pytest.raises(ValueError, match="changed after origin_spec"):
            T.origin_spec(changed)
    with pytest.raises(ValueError, match="observer= beside it"):
        T.origin_spec(spec, dict(n_theta=2, n_phi=3))
    for bad in (dict(n_r=2), dict(colour=1), dict(n_phi=0), dict(theta_axis="sin"), dict(frame="lab"), dict(mode=3),
                dict(n_r=2, r_range=(3.0, 3.0)), dict(r_range=(0.0, np.inf))):
        with pytest.raises(ValueError):
            T.origin_spec(bad, None, _params())
    for bad in (dict(n_dw=2), dict(n_theta=0), dict(theta_axis="x")):
        with pytest.raises(ValueError):
            T.origin_spec({}, bad, _params())
    with pytest.raises(ValueError, match="needs the run's params"):
        T.origin_spec({})


# ---- 2. the host build of art_event_origin.h

def _points(n=10000, seed=3):
    """random points, then the planted ones: z = 0, x = y = 0, r on r_lo and on r_hi, a NaN, r outside the range"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(3, n)) * 12.0
    planted = np.array([[3.0, 4.0, 0.0], [-6.0, 8.0, 0.0], [0.0, 0.0, 7.5], [0.0, 0.0, -7.5], [5.0, 0.0, 0.0], [0.0, 3.0, 4.0],
                        [30.0, 0.0, 0.0], [0.0, 18.0, 24.0], [np.nan, 1.0, 1.0], [1.0, 1.0, np.nan], [1.0, 2.0, 2.0],
                        [40.0, 30.0, 0.0]]).T
    return np.concatenate([p, planted], axis=1), n


@pytest.mark.parametrize("axis", ["cos", "theta"])
def test_host_build_labels_equal_origin_bins(axis):
    from adiabatic_raytracer_amd import trees as T
    from tools import eventorigin
    p, n = _points()
    kw = dict(n_r=3, n_theta=4, n_phi=6, theta_axis=axis, r_range=(5.0, 30.0))
    rot = T.origin_spec(dict(kw, frame="rotation"))
    got = eventorigin.bins(*p, rot)
    assert got.dtype == np.int32 and np.array_equal(got, T.origin_bins(*p, rot))
    assert (got >= 0).sum() > 5000 and (got < 0).sum() > 100 and len(set(got)) == 3 * 4 * 6 + 1
    if axis == "cos":
        # the planted points in the rotation frame: cos θ = 0 is the interior edge of n_theta = 4 and belongs to the
        # bin on its right; x = y = 0 has φ = 0, an edge of n_phi = 6; r_lo and r_hi lie in the first and last bin
        lab = lambda ir, ia, ib: (ir * 4 + ia) * 6 + ib  # noqa: E731
        want = [lab(0, 2, 3), lab(0, 2, 5), lab(0, 3, 3), lab(0, 0, 3), lab(0, 2, 3), lab(0, 3, 4), lab(2, 2, 3), lab(2, 3, 4),
                -1, -1, -1, -1]
        assert list(got[n:]) == want
    # the magnetic frame, and the same labels from (cm, sm) = (1, 0) applied to points turned beforehand
    mag = T.origin_spec(dict(kw, frame="magnetic"), None, _params())
    got_m = eventorigin.bins(*p, mag)
    assert np.array_equal(got_m, T.origin_bins(*p, mag)) and not np.array_equal(got_m, got)
    cm, sm = mag["cm"], mag["sm"]
    turned = np.stack([p[0] * cm - p[2] * sm, p[1], p[0] * sm + p[2] * cm])
    assert np.array_equal(eventorigin.bins(*turned, rot), got_m)
    # one r bin for every finite r
    every = T.origin_spec(dict(n_theta=4, n_phi=6, theta_axis=axis, frame="rotation"))
    got_e = eventorigin.bins(*p, every)
    assert np.array_equal(got_e, T.origin_bins(*p, every)) and (got_e < 0).sum() == 2


# ---- 3. the read-offs on a hand-made table

def test_profile_view_and_jackknife_by_hand():
    from adiabatic_raytracer_amd import trees as T
    spec = T.origin_spec(dict(n_r=1, n_theta=2, n_phi=2, frame="rotation"), dict(n_theta=2, n_phi=3))
    assert spec["shape"] == (2, 2, 3, 1, 2, 2)
    m = np.arange(48, dtype=np.float64).reshape(spec["shape"])
    # emission_profile: photons, summed over the 6 observer bins and r, per steradian of a (2 / 2)(2π / 2) bin
    prof, tc, pc = T.emission_profile(m, spec)
    ph = m[1].reshape(6, 4)  # [observer bin][origin bin]
    assert np.allclose(prof.reshape(-1), ph.sum(axis=0) / math.pi, rtol=1e-15)
    assert ph.sum(axis=0).tolist() == [204.0, 210.0, 216.0, 222.0]  # 24 + 4 j + i over j = 0 .. 5
    assert tc.tolist() == [-0.5, 0.5] and np.allclose(pc, [-math.pi / 2, math.pi / 2])
    ax, _, _ = T.emission_profile(m, spec, species=0)
    assert np.allclose(ax.reshape(-1), np.array([60.0, 66.0, 72.0, 78.0]) / math.pi, rtol=1e-15)
    # observer_view: θ_obs = 1.0 has cos θ = 0.54, the second row; its ring is 2π (1 - 0) sr, one φ bin a third
    view = T.observer_view(m, spec, 1.0)
    assert view.shape == (1, 2, 2)
    rows3 = ph[3:6]  # the observer row 1: bins (1, 0), (1, 1), (1, 2)
    assert np.allclose(view.reshape(-1), rows3.sum(axis=0) / (2 * math.pi), rtol=1e-15)
    assert rows3.sum(axis=0).tolist() == [120.0, 123.0, 126.0, 129.0]
    at = T.observer_view(m, spec, 1.0, phase=0.0)  # φ = 0 lies in the middle bin of three
    assert np.allclose(at.reshape(-1), ph[4] / (2 * math.pi / 3), rtol=1e-15) and ph[4].tolist() == [40.0, 41.0, 42.0, 43.0]
    low = T.observer_view(m, spec, 2.0, phase=-3.0, species=0)  # cos 2.0 < 0: the first row; φ = -3: the first bin
    assert np.allclose(low.reshape(-1), np.arange(4.0) / (2 * math.pi / 3), rtol=1e-15)
    with pytest.raises(ValueError, match="no observer axes"):
        T.observer_view(m[:, :1, :1], T.origin_spec(dict(n_theta=2, n_phi=2, frame="rotation")), 1.0)
    with pytest.raises(ValueError, match="outside"):
        T.observer_view(m, spec, 1.0, phase=4.0)
    # origin_jackknife: all groups equal gives σ = 0 and the value of the whole
    R = 4
    origin = {"raw": R * m, "spec": spec, "replicates": {"raw": np.stack([m] * R), "n_g": np.full(R, 5.0), "a_g": np.full(R, 10.0),
                                                           "R": R, "f_inx": 40}}
    fn = lambda t: T.emission_profile(t, spec)[0]  # noqa: E731
    jk = T.origin_jackknife(origin, fn, cov=True)
    assert jk["groups_used"] == R and jk["value"].shape == (2, 2) and np.allclose(jk["value"], prof * R / 40.0, rtol=1e-15)
    assert np.array_equal(jk["sigma"], np.zeros((2, 2))) and not jk["cov"].any()
    # one group twice as bright: the leave-one-out values (3m / 30 three times, 4m / 30... ) worked out for a total
    tot = lambda t: t[1].sum()  # noqa: E731
    bright = np.stack([m, m, m, 2 * m])
    origin["replicates"]["raw"] = bright
    jk = T.origin_jackknife(origin, tot)
    s = m[1].sum()
    theta = np.array([4 * s / 30, 4 * s / 30, 4 * s / 30, 3 * s / 30])
    want = math.sqrt(3.0 / 4.0 * ((theta - theta.mean()) ** 2).sum())
    assert math.isclose(jk["value"], 5 * s / 40, rel_tol=1e-15) and math.isclose(jk["sigma"], want, rel_tol=1e-12)
    with pytest.raises(ValueError, match="no replicates"):
        T.origin_jackknife({"raw": m, "spec": spec}, tot)


# ---- 4. the C boundary: every ART_E_INVALID comes before any device is touched

def _structs():
    from adiabatic_raytracer_amd._lib import EventOriginOut, EventRowsIn, OriginSpec
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    og = OriginSpec(2, 4, 6, 1, 0, 5.0, 30.0, math.cos(THETA_M), math.sin(THETA_M))
    oo = EventOriginOut(C.pointer(og), None, 0, a, None, None, a)
    return d, ein, oo, og


def _call(lib, cp, ein, start, oo):
    ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731
    return lib.art_event_origin_device(ref(cp), ref(ein), start, ref(oo), None)


def test_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import SkySpec
    lib = A.load_library()
    cp = A.Params().to_c()
    d, ein, oo, og = _structs()
    start = C.c_void_p(C.addressof(d))
    err = lib.art_last_error
    assert _call(lib, None, ein, start, oo) == INVALID and b"params" in err()
    assert _call(lib, cp, None, start, oo) == INVALID and b"NULL in, out or origin" in err()
    assert _call(lib, cp, ein, start, None) == INVALID and b"NULL in, out or origin" in err()

    def bad(msg, start=start, observer=None, **kw):
        _, i, o, g = _structs()
        for k, v in kw.items():
            setattr(i if hasattr(i, k) else (o if hasattr(o, k) else g), k, v)
        if observer is not None:
            sk = SkySpec(**observer)
            o.observer = C.pointer(sk)
        assert _call(lib, cp, i, start, o) == INVALID, msg
        assert msg.encode() in err(), (msg, err())

    bad("NULL in, out or origin", origin=None)
    for k in ("n_r", "n_theta", "n_phi"):
        for v in (0, -3):
            bad("origin bin counts must be >= 1", **{k: v})
    for v in (-1, 2):
        bad("theta_axis must be", theta_axis=v)
    for v in (-1, 3, 7):
        bad("origin mode must be", mode=v)
    bad("LDS budget of 8192 doubles", mode=1, n_theta=64, n_phi=64)           # 2 * 2 * 64 * 64 = 16384
    bad("LDS budget of 8192 doubles", mode=1, groups=64, n_theta=8, n_phi=8)  # 64 * 2 * 2 * 8 * 8 = 16384
    bad("LDS budget of 8192 doubles", mode=1, observer=dict(n_theta=8, n_phi=16, n_dw=1, theta_axis=1))
    for lo, hi in ((30.0, 5.0), (5.0, 5.0), (0.0, 0.0)):  # (n_r = 2: (0, 0) is no "every finite r" there)
        bad("needs r_lo < r_hi", r_lo=lo, r_hi=hi)
    bad("needs r_lo < r_hi", n_r=1, r_lo=3.0, r_hi=3.0)
    for k in ("cm", "sm", "r_lo", "r_hi"):
        for v in (float("nan"), float("inf")):
            bad("must be finite", **{k: v})
    good = dict(n_theta=2, n_phi=3, n_dw=1, theta_axis=1, mode=0, dw_lo=0.0, dw_hi=0.0)
    bad("observer axes need n_dw == 1", observer=dict(good, n_dw=2, dw_lo=-1.0, dw_hi=1.0))
    bad("bin counts", observer=dict(good, n_phi=0))
    bad("theta_axis", observer=dict(good, theta_axis=2))
    for R in (-1, 1, 65, 1000):
        bad("groups must be 0 (one table) or in [2, 64]", groups=R)
    bad("2^31 doubles or more", n_r=1024, n_theta=1024, n_phi=1024, r_lo=1.0, r_hi=2.0)
    bad("2^31 doubles or more", n_theta=4096, n_phi=4096, observer=dict(good, n_theta=8, n_phi=8))
    bad("2^31 doubles or more", groups=64, n_theta=2048, n_phi=4096)
    bad("hist or misplaced is NULL", hist=None)
    bad("hist or misplaced is NULL", misplaced=None)
    # art_event_replicates_device's faults on in and node_start
    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    bad("node_start is NULL", start=None)
    bad("NULL input buffer", weight5=None)
    bad("NULL input buffer", x=None)
    # no events: ART_OK after the checks, nothing touched (no device is reached: there is none here); one r bin for
    # every finite r, an observer whose mode is not looked at
    for groups in (0, 2, 64):
        _, i, o, g = _structs()
        i.n_events = i.n_nodes = 0
        i.x = i.weight5 = i.nodes = None
        g.n_r, g.r_lo, g.r_hi = 1, 0.0, 0.0
        sk = SkySpec(**dict(good, mode=7))
        o.observer, o.groups = C.pointer(sk), groups
        assert _call(lib, cp, i, None, o) == 0, err()


# ---- 5. the symbol, the structs and the Python surface

def test_symbol_structs_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib, trees
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    assert "art_event_origin_device" in _lib.SIGNATURES and hasattr(lib, "art_event_origin_device")
    assert C.sizeof(_lib.OriginSpec) == 5 * 4 + 4 + 4 * 8 and C.sizeof(_lib.EventOriginOut) == 2 * 8 + 4 + 4 + 4 * 8
    assert _lib.ORIGIN_MODES == {"auto": 0, "lds": 1, "global": 2} and Engine.ORIGIN_MAX_BYTES == 1 << 30
    for fn in (Engine.run_events, trees.main_runner_tree):
        par = inspect.signature(fn).parameters["origin_map"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    for fn in (trees.rank_vector, trees._finish_run):
        par = inspect.signature(fn).parameters["origin"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    eo = inspect.signature(Engine.event_origin).parameters
    assert list(eo)[:6] == ["self", "sample", "weight5", "back", "forward", "origin"]
    for k, v in dict(observer=None, groups=None, event_offset=0, hist=None, cyclotron_rerun=None, return_bins=False).items():
        assert eo[k].kind is inspect.Parameter.KEYWORD_ONLY and eo[k].default == v, k
    for name in ("origin_spec", "origin_map_edges", "origin_bins", "rows_origin", "emission_profile", "observer_view",
                 "origin_jackknife"):
        assert callable(getattr(trees, name)), name
    # the caps, before any work is done (nothing of the engine is touched)
    eng = Engine.__new__(Engine)
    eng.params = A.Params()
    with pytest.raises(ValueError, match="origin_map: unknown keys"):
        Engine.run_events(eng, 0, origin_map={"colour": 1})
    with pytest.raises(ValueError, match="more than 1073741824"):
        Engine.run_events(eng, 10, origin_map=dict(n_theta=512, n_phi=1024, observer=dict(n_theta=16, n_phi=16)))
    with pytest.raises(ValueError, match="lower R"):
        Engine.run_events(eng, 10, replicates=64, origin_map=dict(n_theta=64, n_phi=128, observer=dict(n_theta=16, n_phi=16)))
    with pytest.raises(ValueError, match="exact accumulators"):
        Engine.run_events(eng, 10, exact=True, origin_map=dict(n_theta=64, n_phi=128, observer=dict(n_theta=16, n_phi=16)))
    with pytest.raises(ValueError, match="n_r > 1 needs an r_range"):
        Engine.run_events(eng, 10, origin_map=dict(n_r=2))


def test_exact_keys_and_pack_without_an_origin_table():
    from adiabatic_raytracer_amd import _lib, trees
    assert trees.EXACT_KEYS[-1] == "origin" and trees.EXACT_KEYS[:3] == ("flux", "sky", "totals")
    rng = np.random.default_rng(5)
    p = rng.uniform(0.0, 3.0, 200)
    acc = {"kind": "run", "flux": trees.exact_add(p, rng.integers(0, 8, 200), 8)[0][None],
           "sky": None, "totals": trees.exact_add(p, rng.integers(0, 2, 200), 2)[0][None],
           "nonfinite": np.zeros(1), "misplaced": np.zeros(1)}
    vec = trees.exact_pack(acc)
    # a dict without an origin table: the vector of the three tables alone, as before
    old = np.concatenate([acc["flux"].reshape(-1).astype(np.float64), acc["totals"].reshape(-1).astype(np.float64),
                          acc["nonfinite"], acc["misplaced"]])
    assert vec.tobytes() == old.tobytes() and trees.exact_pack(dict(acc, origin=None)).tobytes() == old.tobytes()
    back = trees.exact_unpack(2.0 * vec, acc)
    assert back["origin"] is None and np.array_equal(trees.exact_round(back["flux"]), 2.0 * trees.exact_round(acc["flux"]))
    # with one: its limbs follow the totals', and merge, finish and result carry it
    lab = rng.integers(0, 12, 200).astype(np.int32)
    og = dict(acc, origin=trees.exact_add(p, lab, 12)[0].reshape(1, 2, 1, 1, 1, 2, 3, _lib.EXACT_LIMBS))
    v2 = trees.exact_pack(og)
    assert len(v2) == len(vec) + 12 * _lib.EXACT_LIMBS and v2[:len(old) - 2].tobytes() == old[:-2].tobytes()
    un = trees.exact_unpack(v2, og)
    assert np.array_equal(un["origin"], og["origin"])
    merged = trees.exact_merge([og, og])
    fin = trees.exact_result(merged, 4)
    want = np.array([math.fsum(2.0 * p[lab == b]) for b in range(12)]).reshape(2, 1, 1, 1, 2, 3)
    assert np.array_equal(fin["origin_raw"], want) and np.array_equal(fin["origin_map"], want / 4.0)
    assert "origin_raw" not in trees.exact_result(trees.exact_merge([acc, acc]), 4)
    with pytest.raises(ValueError, match="other tables"):
        trees.exact_merge([og, acc])


def test_rank_vector_appends_the_origin_last():
    from adiabatic_raytracer_amd import shard, trees
    tot = trees.pack_totals(np.arange(100.0), 7, 1.0, 2.0, 5)
    assert trees.rank_vector(tot)[0] is tot and trees.rank_vector(tot, origin=None)[0] is tot
    m = np.arange(24.0).reshape(2, 1, 1, 1, 3, 4)
    vec, ends = trees.rank_vector(tot, origin=m)
    assert len(vec) == len(tot) + 24 and vec[:len(tot)].tobytes() == tot.tobytes() and vec[len(tot):].tolist() == m.reshape(-1).tolist()
    assert list(ends) == [len(tot), len(tot) + 24]
