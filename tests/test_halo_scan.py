"""The halo scan without a GPU: art_halo.h's halo_ratio through a host compile (tools/haloscan) against
trees.halo_ratio and a numpy.longdouble evaluation, its identity, its algebra against halo_factor
(tools/halocheck), its normalisation, art_event_halo_scan_device's argument checks, and the numpy helpers
(trees.halo_scan_tables, the pack / unpack round trip, halo_scan_result, the ValueErrors).

Bounds, u = 2^-53, for an event of speed s and a target h seen from the base b under the proposal vp:
  t = s²/vp²,  Q_x = (s + |v_x|)²/v0_x²  (a ceiling on q_x = |u + v_x|²/v0_x²)
  ρ = (8 (Q_b + Q_h) + 8) u             relative, two evaluations of R
  β = 8 (2t + 2 Q_b + 2 Q_h + 3) u      relative, F_b R against F_h
ceilings on the roundings of the squares, the difference of the exponents (an absolute error of the
exponent is a relative one of the exponential), two exponentials within an ulp of libm and the prefactor.
At vp ≈ 350 they stay below 1e-12."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import halocheck  # noqa: E402
import haloscan  # noqa: E402

U = 2.0 ** -53
INVALID = -1
C_KM = 2.99792e5
BASE = (260.0, (0.0, 230.0, 0.0))
TARGETS = [(220.0, (0.0, 230.0, 0.0)), (260.0, (100.0, 180.0, -60.0)), (180.0, (0.0, 0.0, 0.0))]


def _vp(h):
    return float(np.sqrt(h[0] ** 2 + sum(c * c for c in h[1])))


def _Q(s, h):
    return (s + np.linalg.norm(h[1])) ** 2 / h[0] ** 2


def rho(s, b, h):
    return (8.0 * (_Q(s, b) + _Q(s, h)) + 8.0) * U


def beta(s, b, h, vp):
    return 8.0 * (2.0 * s * s / (vp * vp) + 2.0 * _Q(s, b) + 2.0 * _Q(s, h) + 3.0) * U


def unit(rng, n):
    c = rng.uniform(-1.0, 1.0, n)
    p = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - c * c)
    return np.stack([s * np.cos(p), s * np.sin(p), c], axis=1)


@pytest.fixture(scope="module")
def draws():
    """10^4 events as the sampler makes them: s from halo_speed under the base's proposal, isotropic
    directions, stored as vifty = u / c; (vifty (3n, SoA), u = vifty c (n, 3), s = |u|)"""
    rng = np.random.default_rng(20251)
    n = 10 ** 4
    s = halocheck.speed(rng.uniform(0.0, 1.0, n), _vp(BASE))
    vifty = (unit(rng, n) * s[:, None] / C_KM).T.reshape(-1)
    u = (vifty.reshape(3, n) * C_KM).T.copy()
    return vifty, u, np.linalg.norm(u, axis=1)


def _long(u, b, h):
    L = np.longdouble
    ul = u.astype(L)

    def q(m):
        w = ul + np.array(m[1], L)
        return (w * w).sum(axis=1) / (L(m[0]) * L(m[0]))

    return (L(b[0]) / L(h[0])) ** 3 * np.exp(q(b) - q(h))


def test_ratio_against_numpy_and_longdouble(draws):
    from adiabatic_raytracer_amd import trees
    vifty, u, s = draws
    Rn = trees.halo_ratio(vifty, BASE, TARGETS)
    assert Rn.shape == (3, len(s)) and np.all(np.isfinite(Rn)) and np.all(Rn > 0)
    worst = 0.0
    for k, h in enumerate(TARGETS):
        Rt = haloscan.ratio(u, BASE, h)
        Rl = _long(u, BASE, h)
        tol = rho(s, BASE, h)
        assert tol.max() < 1e-12
        for what, a, b in (("tool-numpy", Rt, Rn[k]), ("tool-long", Rt, Rl), ("numpy-long", Rn[k], Rl)):
            rel = np.abs((a - b) / Rl).astype(np.float64)
            worst = max(worst, float((rel / tol).max()))
            assert np.all(rel <= tol), (what, k, float((rel / tol).max()))
    print("halo_ratio: worst measured / rho =", worst)
    # the Halo objects of the package and plain pairs are the same models
    import adiabatic_raytracer_amd as A
    assert np.array_equal(trees.halo_ratio(vifty, A.Halo(*BASE), [A.Halo(*h) for h in TARGETS]), Rn)


def test_identity_is_exactly_one(draws):
    from adiabatic_raytracer_amd import trees
    vifty, u, _ = draws
    for b in [BASE] + TARGETS:
        assert np.array_equal(haloscan.ratio(u, b, b), np.ones(len(u)))
        assert np.array_equal(trees.halo_ratio(vifty, b, [b])[0], np.ones(len(u)))
    # ... whatever the proposal of either: v_prop plays no part
    import adiabatic_raytracer_amd as A
    assert np.array_equal(trees.halo_ratio(vifty, A.Halo(*BASE, v_prop=900.0), [A.Halo(*BASE, v_prop=400.0)])[0], np.ones(len(u)))


def test_factor_times_ratio_is_the_targets_factor(draws):
    _, u, s = draws
    vp = _vp(BASE)
    worst = 0.0
    for h in TARGETS:
        Fb = halocheck.factor(u, s, BASE[0], BASE[1], vp)
        Fh = halocheck.factor(u, s, h[0], h[1], vp)
        R = haloscan.ratio(u, BASE, h)
        tol = beta(s, BASE, h, vp)
        assert tol.max() < 1e-12
        rel = np.abs(Fb * R - Fh) / Fh
        worst = max(worst, float((rel / tol).max()))
        assert np.all(rel <= tol), float((rel / tol).max())
    print("F_b R against F_h: worst measured / beta =", worst)


def test_normalisation_pins_the_prefactor():
    """E_b[R_h] = ∫ f_h = 1 for u drawn from the base's own Maxwellian: a wrong power of v0_b/v0_h misses by
    (260/220)^±1 = 18 % or more, hundreds of standard errors here"""
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(20251)
    n = 4 * 10 ** 5
    u = rng.normal(size=(n, 3)) * (BASE[0] / np.sqrt(2.0)) - np.array(BASE[1])
    R = trees.halo_ratio((u / C_KM).T.reshape(-1), BASE, TARGETS)
    for k, h in enumerate(TARGETS):
        z = (R[k].mean() - 1.0) / (R[k].std(ddof=1) / np.sqrt(n))
        print("normalisation", h, "mean", R[k].mean(), "z", z)
        assert abs(z) <= 5.0, (h, z)
        Rt = haloscan.ratio((u / C_KM) * C_KM, BASE, h)  # the header's own, on the same u as numpy formed
        assert abs((Rt.mean() - 1.0) / (Rt.std(ddof=1) / np.sqrt(n))) <= 5.0


# ---------------------------------------------------------------------------------------------------
# the C boundary
def _structs():
    from adiabatic_raytracer_amd._lib import ArtHalo, EventHaloScanOut, EventRowsIn
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    ho = EventHaloScanOut(a, 50, 0, a, None, None, a, None, None, None, None, None, None)
    base = ArtHalo(260.0, (C.c_double * 3)(0.0, 230.0, 0.0), -1.0)
    return d, ein, ho, base


def _models(ms):
    from adiabatic_raytracer_amd._lib import ArtHalo
    return (ArtHalo * max(len(ms), 1))(*[ArtHalo(v0, (C.c_double * 3)(*v), vp) for v0, v, vp in ms])


GOOD = [(260.0, (0.0, 230.0, 0.0), -1.0), (220.0, (0.0, 230.0, 0.0), -1.0)]


def _call(lib, cp, ein, start, base, ms, ho, n=None):
    ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731
    arr = _models(ms) if ms is not None else None
    return lib.art_event_halo_scan_device(ref(cp), ref(ein), start, ref(base), len(ms) if n is None else n, arr, ref(ho), None)


def test_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import ArtHalo, SkySpec
    lib = A.load_library()
    cp = A.Params().to_c()
    d, ein, ho, base = _structs()
    start = C.c_void_p(C.addressof(d))
    err = lib.art_last_error
    assert _call(lib, None, ein, start, base, GOOD, ho) == INVALID and b"params" in err()
    assert _call(lib, cp, None, start, base, GOOD, ho) == INVALID and b"NULL in or out" in err()
    assert _call(lib, cp, ein, start, base, GOOD, None) == INVALID and b"NULL in or out" in err()
    assert _call(lib, cp, ein, start, None, GOOD, ho) == INVALID and b"NULL base or models" in err()
    assert _call(lib, cp, ein, start, base, None, ho, n=2) == INVALID and b"NULL base or models" in err()
    assert _call(lib, cp, ein, start, base, GOOD, ho, n=0) == INVALID and b"n_models" in err()
    assert _call(lib, cp, ein, start, base, [GOOD[0]] * 33, ho) == INVALID and b"n_models" in err()
    _, none, _, _ = _structs()  # (a call that passes every check has no events: it must not reach a device)
    none.n_events = none.n_nodes = 0
    assert _call(lib, cp, none, start, base, [GOOD[0]] * 32, ho) == 0
    # an invalid base: halo_of's faults
    for bad in (ArtHalo(0.0, (C.c_double * 3)(0, 0, 0), -1.0), ArtHalo(float("nan"), (C.c_double * 3)(0, 0, 0), -1.0),
                ArtHalo(220.0, (C.c_double * 3)(0, float("inf"), 0), -1.0), ArtHalo(220.0, (C.c_double * 3)(0, 0, 0), 100.0),
                ArtHalo(220.0, (C.c_double * 3)(0, 0, 0), 4000.0)):
        assert _call(lib, cp, ein, start, bad, GOOD, ho) == INVALID and b"halo: " in err()
    # the models: v0 finite and positive, v_ns finite, v0 at most the base's resolved v_prop
    for v0 in (0.0, -220.0, float("nan"), float("inf")):
        assert _call(lib, cp, ein, start, base, [GOOD[0], (v0, (0.0, 0.0, 0.0), -1.0)], ho) == INVALID and b"model's v0 must be finite" in err()
    for v in (float("nan"), float("inf")):
        assert _call(lib, cp, ein, start, base, [GOOD[0], (220.0, (0.0, v, 0.0), -1.0)], ho) == INVALID and b"v_ns must be finite" in err()
    vp = float(np.sqrt(260.0 ** 2 + 230.0 ** 2))
    assert _call(lib, cp, ein, start, base, [(np.nextafter(vp, 1e9), (0.0, 0.0, 0.0), -1.0)], ho) == INVALID and b"base's v_prop" in err()
    wide = ArtHalo(260.0, (C.c_double * 3)(0.0, 230.0, 0.0), 500.0)  # the base's own v_prop is what counts ...
    assert _call(lib, cp, ein, start, wide, [(501.0, (0.0, 0.0, 0.0), -1.0)], ho) == INVALID and b"base's v_prop" in err()
    # ... and a model's own v_prop is ignored, whatever it holds
    assert _call(lib, cp, none, start, wide, [(500.0, (0.0, 0.0, 0.0), 1.0), (220.0, (0.0, 0.0, 0.0), float("nan"))], ho) == 0

    def bad(msg, start=start, **kw):
        _, i, o, _ = _structs()
        for k, v in kw.items():
            setattr(i if hasattr(i, k) else o, k, v)
        assert _call(lib, cp, i, start, base, GOOD, o) == INVALID, msg
        assert msg.encode() in err(), (msg, err())

    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    bad("nbins must be", nbins=4097)
    bad("nbins must be", nbins=-1)
    bad("reserved must be 0", reserved=1)
    bad("node_start is NULL", start=None)
    bad("vifty is NULL", vifty=None)
    bad("totals is NULL", totals=None)
    bad("flux is NULL", flux=None)
    bad("NULL input buffer", weight5=None)
    bad("flux_sq or flux_xa", moment_totals=C.addressof(d))
    good = dict(n_theta=4, n_phi=8, n_dw=3, theta_axis=1, mode=0, dw_lo=-1e-6, dw_hi=1e-6)
    for msg, kw in {"bin counts": dict(good, n_theta=0), "theta_axis": dict(good, theta_axis=2), "ranges": dict(good, dw_hi=-1.0),
                    "sky_hist is NULL": good}.items():
        spec = SkySpec(**kw)
        bad(msg, sky=C.pointer(spec))
    spec = SkySpec(**good)
    bad("sky_sq or sky_xa", sky=C.pointer(spec), sky_hist=C.addressof(d), moment_totals=C.addressof(d), flux_sq=C.addressof(d),
        flux_xa=C.addressof(d))
    # no events: ART_OK after the checks, nothing touched
    _, i, o, _ = _structs()
    i.n_events = i.n_nodes = 0
    o.flux = o.totals = o.vifty = None
    assert _call(lib, cp, i, None, base, GOOD, o) == 0


def test_symbol_struct_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib, trees
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    assert "art_event_halo_scan_device" in _lib.SIGNATURES and hasattr(lib, "art_event_halo_scan_device")
    assert C.sizeof(_lib.EventHaloScanOut) == 2 * 4 + 11 * 8
    assert len(_lib.HALO_SCAN_TOTALS) == 5 and _lib.HALO_SCAN_MAX_MODELS == 32 and lib.art_abi_version() == 1
    run = inspect.signature(Engine.run_events).parameters
    assert run["halos"].kind is inspect.Parameter.KEYWORD_ONLY and run["halos"].default is None
    assert inspect.signature(trees.main_runner_tree).parameters["halos"].default is None
    hs = inspect.signature(Engine.event_halo_scan).parameters
    assert list(hs)[:7] == ["self", "sample", "weight5", "back", "forward", "base", "halos"]
    for k, v in dict(event_offset=0, nbins=50, sky=None, scan=None, errors=False, return_ratio=False, cyclotron_rerun=None).items():
        assert hs[k].kind is inspect.Parameter.KEYWORD_ONLY and hs[k].default == v, k


def test_python_value_errors():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import trees
    from adiabatic_raytracer_amd.engine import Engine
    base = A.Halo(*BASE)
    vp = base.vp()
    cases = {"needs halo=": (None, [base]), "1 to 32": (base, []), "1 to 32 models, not 33": (base, [base] * 33),
             "exceeds the base's proposal": (base, [A.Halo(np.nextafter(vp, 1e9))]), "finite": (base, [A.Halo(float("nan"))]),
             "finite v0": (base, [A.Halo(220.0, (0.0, float("inf"), 0.0))]), "v0 > 0": (base, [A.Halo(-1.0)])}
    for msg, (b, hs) in cases.items():
        with pytest.raises(ValueError, match="halos: "):
            trees.halo_scan_models(b, hs)
        # run_events refuses the list before any work is done (nothing of the engine is touched: no GPU here)
        with pytest.raises(ValueError, match="halos: "):
            Engine.run_events(None, 0, halo=b, halos=hs)
        with pytest.raises(ValueError, match="halos: "):
            trees.main_runner_tree(A.Params(), 3, device_events=True, halo=b, halos=hs)
    assert trees.halo_scan_models(A.Halo(*BASE, v_prop=500.0), [A.Halo(500.0)]) == [(500.0, (0.0, 0.0, 0.0))]
    assert trees.halo_scan_models(base, [base] * 32)[31] == BASE
    # the host paths hold no run in HBM to reweight
    for kw in ({}, {"device_trees": True}):
        with pytest.raises(ValueError, match="device_events"):
            trees.main_runner_tree(A.Params(), 3, halo=base, halos=[base], **kw)


# ---------------------------------------------------------------------------------------------------
# the numpy helpers on synthetic rows
def _rows(rng, n_events, n_rows):
    rows = np.zeros((n_rows, 13))
    rows[:, 0] = np.sort(rng.integers(0, n_events, n_rows)) + 1.0 + 7  # (event_lo = 7)
    rows[:, 1] = rng.integers(0, 2, n_rows)
    rows[:, 2] = np.arccos(rng.uniform(-1, 1, n_rows))
    rows[:, 3] = rng.uniform(-np.pi, np.pi, n_rows)
    rows[:4, 3] = [-np.pi, np.pi, 0.0, np.nan]  # the edges, and a row no table counts
    rows[:, 7] = rng.uniform(0.5, 2.0, n_rows)
    rows[:, 8] = rng.uniform(0.0, 1.0, n_rows)
    rows[:, 12] = -1.0 + rng.uniform(-2e-6, 4e-6, n_rows)
    return rows


def test_halo_scan_tables_bins_p_times_r():
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(5)
    n_events, n_rows, K, nbins = 40, 300, 3, 10
    rows = _rows(rng, n_events, n_rows)
    R = rng.uniform(0.2, 3.0, (K, n_events))
    R[0] = 1.0
    sky = dict(n_theta=3, n_phi=5, n_dw=4, theta_axis="cos", dw_range=(-1 - 1e-6, -1 + 3e-6))
    got = trees.halo_scan_tables(rows, R, nbins, sky, event_lo=7)
    ev = rows[:, 0].astype(np.int64) - 8
    sp = rows[:, 1].astype(np.int64)
    p = rows[:, 8] * rows[:, 7]
    ok = np.isfinite(rows[:, 3])
    lab = trees.sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **sky)
    assert (lab >= 0).sum() > 50 and (lab < 0).sum() > 50
    for k in range(K):
        w = p * R[k, ev]
        for s_ in (0, 1):
            h, _ = np.histogram(rows[ok & (sp == s_), 3], bins=nbins, range=(-np.pi, np.pi), weights=w[ok & (sp == s_)])
            assert np.allclose(got["flux"][k, s_ * nbins:(s_ + 1) * nbins], h, rtol=1e-13, atol=0)
            assert got["totals"][k, s_] == pytest.approx(w[sp == s_].sum(), rel=1e-13)
        assert np.array_equal(got["sky"][k], np.bincount(lab[lab >= 0], weights=w[lab >= 0], minlength=2 * 3 * 5 * 4))
    # R = 1 is the run's own tables, and without a sky spec there is no sky table
    own = trees.halo_scan_tables(rows, np.ones((1, n_events)), nbins, None, event_lo=7)
    assert own["sky"] is None and np.array_equal(own["flux"][0], got["flux"][0])


def test_pack_round_trip_and_result():
    from adiabatic_raytracer_amd import trees
    K, nbins = 3, 4
    rng = np.random.default_rng(2)
    models = [BASE] + TARGETS[:2]
    tot = np.array([[1.0, 2.0, 10.0, 10.0, 0], [2.0, 4.0, 9.0, 12.0, 0], [3.0, 8.0, 11.0, 30.0, 0]])
    raw = {"models": models, "n_events": 10, "flux": rng.random((K, 2 * nbins)), "sky": rng.random((K, 2, 2, 3, 1)), "totals": tot}
    res = trees.halo_scan_result(raw, 20)
    assert res["models"] == models and res["misplaced"] == 0 and res["f_inx"] == 20
    assert np.array_equal(res["flux"], (raw["flux"] / 20.0).reshape(K, 2, nbins)) and np.array_equal(res["sky_map"], raw["sky"] / 20.0)
    assert np.array_equal(res["sum_weight_sln_prob"], tot[:, :2] / 20.0)
    assert np.array_equal(res["ratio_sum"], [10.0, 9.0, 11.0]) and np.array_equal(res["ratio_sq"], [10.0, 12.0, 30.0])
    assert "n_eff" not in res and "flux_sigma" not in res
    back = trees.halo_scan_unpack(trees.halo_scan_pack(raw), raw)
    assert back["models"] == models and back["n_events"] == 10 and "g" not in back
    for k in ("flux", "sky", "totals"):
        assert np.array_equal(back[k], raw[k]) and back[k].shape == raw[k].shape
    # with moments: σ per model by moments_sigma, n_eff = S_photon² / Q_photon, and the sum over two ranks
    mt = np.tile(np.array([10.0, 20.0, 50.0, 0.3, 0.9, 0.5, 1.5, 0.0]), (K, 1))
    raw.update(flux_sq=rng.random((K, 2 * nbins)), flux_xa=rng.random((K, 2 * nbins)), sky_sq=rng.random((K, 2, 2, 3, 1)),
               sky_xa=rng.random((K, 2, 2, 3, 1)), moment_totals=mt)
    res = trees.halo_scan_result(raw, 20)
    for k in range(K):
        ref = trees.moments_sigma(raw["flux"][k], raw["flux_sq"][k], raw["flux_xa"][k], 20, 50.0, 10.0)
        assert np.array_equal(res["flux_sigma"][k].reshape(-1), ref, equal_nan=True)
    assert res["sky_map_sigma"].shape == (K, 2, 2, 3, 1) and res["sum_weight_sln_prob_sigma"].shape == (K, 2)
    assert np.array_equal(res["n_eff"], tot[:, 1] ** 2 / 0.9)
    two = trees.halo_scan_unpack(2.0 * trees.halo_scan_pack(raw), raw)
    assert two["n_events"] == 20 and np.array_equal(two["moment_totals"], 2.0 * mt) and np.array_equal(two["sky_xa"], 2.0 * raw["sky_xa"])
    # a misplaced record shows in the result
    tot[:, 4] = 2.0
    assert trees.halo_scan_result(raw, 20)["misplaced"] == 2


def _same(a, b):
    """deep equality of scan results: dicts by key order, arrays bit for bit (NaN equal to NaN)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_rank_vector_layout_and_finish(monkeypatch):
    """The reduced vector of a run with a sky map, errors, two couplings and two halo models is
    [pack_totals | coupling scan | halo scan], and the finish both drivers share turns its sum over two ranks into
    the run_info that scan_result and halo_scan_result give for the doubled tables."""
    from adiabatic_raytracer_amd import shard, trees
    K, nbins, shape = 2, 4, (2, 2, 3, 1)
    rng = np.random.default_rng(11)
    tab = lambda *s: rng.random(s) + 0.5  # noqa: E731
    mom = {"flux_sq": tab(2 * nbins), "flux_xa": tab(2 * nbins), "sky_sq": tab(*shape), "sky_xa": tab(*shape),
           "totals": np.array([6.0, 30.0, 170.0, 0.4, 0.8, 1.5, 2.5, 0.0])}
    flux, sky, f_inx = tab(2 * nbins), tab(*shape), 30
    tot = trees.pack_totals(flux, f_inx, 1.25, 2.5, 7, sky, mom)

    def scan_tables(width):
        t = {"flux": tab(K, 2 * nbins), "sky": tab(K, *shape), "totals": tab(K, width), "flux_sq": tab(K, 2 * nbins),
             "flux_xa": tab(K, 2 * nbins), "sky_sq": tab(K, *shape), "sky_xa": tab(K, *shape),
             "moment_totals": np.tile(mom["totals"], (K, 1)), "n_events": 6}
        t["totals"][:, 3:] = 0.0  # (the counters: saturated, unlinked, ... and misplaced)
        return t

    craw = trees.scan_raw({"g": [1e-12, 3e-12], **scan_tables(6)})
    hraw = trees.halo_scan_raw({"models": [BASE, TARGETS[0]], **scan_tables(5)})
    vec, ends = trees.rank_vector(tot, craw, hraw)
    want = np.concatenate([tot, trees.scan_pack(craw), trees.halo_scan_pack(hraw)])
    assert vec.dtype == np.float64 and vec.tobytes() == want.tobytes()
    assert list(ends) == [len(tot), len(tot) + len(trees.scan_pack(craw)), len(want)]
    # without the scans the vector is the totals' own, and one scan alone follows them directly
    assert trees.rank_vector(tot)[0] is tot
    assert trees.rank_vector(tot, None, hraw)[0].tobytes() == np.concatenate([tot, trees.halo_scan_pack(hraw)]).tobytes()

    monkeypatch.setattr(shard, "allreduce_sum", lambda v: 2.0 * v)  # two ranks with the same tables
    sky_kw = {"n_theta": 2, "n_phi": 3, "n_dw": 1, "theta_axis": "cos", "dw_range": None}
    rows0 = tab(3, 13)
    info = {}
    rows = trees._finish_run(rows0.copy(), tot, craw, hraw, nbins=nbins, sky_kw=sky_kw, errors=True, world=2, run_info=info,
                             events=(0, 6), n_events=12, g0=1e-12, path=None)
    assert np.array_equal(rows[:, 7], rows0[:, 7] / 60.0) and np.array_equal(np.delete(rows, 7, 1), np.delete(rows0, 7, 1))
    assert list(info) == ["f_inx", "flux", "sum_weight_sln_prob", "rows", "events", "n_events", "sky_map", "sky_map_edges",
                          "flux_sigma", "sum_weight_sln_prob_sigma", "sky_map_sigma", "coupling_scan", "halo_scan"]
    assert info["f_inx"] == 60 and info["rows"] == 14 and info["events"] == (0, 6) and info["n_events"] == 12
    assert np.array_equal(info["flux"], (2.0 * flux / 60.0).reshape(2, nbins)) and np.array_equal(info["sky_map"], 2.0 * sky / 60.0)
    assert info["sum_weight_sln_prob"] == (2.5 / 60.0, 5.0 / 60.0)
    assert np.array_equal(info["flux_sigma"].reshape(-1),
                          trees.moments_sigma(2.0 * flux, 2.0 * mom["flux_sq"], 2.0 * mom["flux_xa"], 60, 340.0, 12.0))

    def doubled(raw):
        return {k: (2 * v if k == "n_events" else 2.0 * v if isinstance(v, np.ndarray) else v) for k, v in raw.items()}

    assert _same(info["coupling_scan"], trees.scan_result(trees.scan_unpack(trees.scan_pack(doubled(craw)), craw), 1e-12, 60))
    assert _same(info["halo_scan"], trees.halo_scan_result(trees.halo_scan_unpack(trees.halo_scan_pack(doubled(hraw)), hraw), 60))
    assert _same(info["coupling_scan"]["raw"]["sky_xa"], 2.0 * craw["sky_xa"]) and info["halo_scan"]["raw"]["n_events"] == 12
    assert info["halo_scan"]["n_eff"].shape == (K,) and info["coupling_scan"]["unlinked"] == 0
