"""Event moments without a GPU: the argument checks of art_event_moments_device, which come before any
device is touched; the Python surface (Engine.event_moments, run_events(errors=), main_runner_tree(errors=),
pack_totals(moments=)); trees.event_moments and trees.moments_sigma against their definitions written as
plain loops; and the per-tree group-by of art_event_moments.h in a host build (tools/eventmoments.py)
against trees.event_moments.

Integer powers make every sum exact, so those comparisons are equalities. moments_sigma against the direct
form Σ_e (X_e - F a_e)²: the expansion Q - 2 F C + F² A2 cancels, so the variances are compared against the
size of the terms, |Δvar| <= 8 (n + 4) u (Q + 2 |F C| + F² A2) with u = 2^-53 (each of the three tables is a
sum of n non-negative terms, Higham §4.2)."""
import ctypes as C
import inspect

import numpy as np
import pytest

INVALID = -1  # ART_E_INVALID
U = 2.0 ** -53


def _structs():
    from adiabatic_raytracer_amd._lib import EventMomentsOut, EventRowsIn
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    mo = EventMomentsOut(50, 0, a, a, None, None, None, a)
    return d, ein, mo


def _call(lib, cp, ein, start, mo):
    return lib.art_event_moments_device(C.byref(cp) if cp is not None else None, C.byref(ein) if ein is not None else None,
                                        start, C.byref(mo) if mo is not None else None, None)


def test_event_moments_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import SkySpec
    lib = A.load_library()
    cp = A.Params().to_c()
    d, ein, mo = _structs()
    start = C.c_void_p(C.addressof(d))
    assert _call(lib, None, ein, start, mo) == INVALID and b"params" in lib.art_last_error()
    assert _call(lib, cp, None, start, mo) == INVALID and b"NULL in or out" in lib.art_last_error()
    assert _call(lib, cp, ein, start, None) == INVALID and b"NULL in or out" in lib.art_last_error()

    def bad(msg, start=start, **kw):
        _, i, o = _structs()
        for k, v in kw.items():
            setattr(i if hasattr(i, k) else o, k, v)
        assert _call(lib, cp, i, start, o) == INVALID, msg
        assert msg.encode() in lib.art_last_error(), (msg, lib.art_last_error())

    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    bad("nbins must be", nbins=-1)
    bad("nbins must be", nbins=4097)
    bad("reserved must be 0", reserved=1)
    bad("node_start is NULL", start=None)
    bad("totals is NULL", totals=None)
    bad("flux_sq or flux_xa", flux_sq=None)
    bad("flux_sq or flux_xa", flux_xa=None)
    bad("NULL input buffer", weight5=None)
    bad("cyc_slot needs", cyc_slot=C.addressof(d), cyc_n=3)
    good = dict(n_theta=4, n_phi=8, n_dw=3, theta_axis=1, mode=0, dw_lo=-1e-6, dw_hi=1e-6)
    sky_cases = {
        "bin counts": dict(good, n_theta=0),
        "finite lo < hi": dict(good, dw_hi=-1e-6),
        "theta_axis": dict(good, theta_axis=2),
        "2^26": dict(good, n_theta=8192, n_phi=8192),
        "sky_sq or sky_xa": good,  # a good spec without its tables
    }
    for msg, kw in sky_cases.items():
        spec = SkySpec(**kw)
        bad(msg, sky=C.pointer(spec))
    spec = SkySpec(**good)
    bad("sky_sq or sky_xa", sky=C.pointer(spec), sky_sq=C.addressof(d))
    # no tables asked for and no flux bins: only the totals are needed, and that is checked too
    bad("totals is NULL", nbins=0, flux_sq=None, flux_xa=None, totals=None)
    # no events: ART_OK after the checks, nothing touched (NULL buffers, NULL node_start)
    _, i, o = _structs()
    i.n_events = i.n_nodes = 0
    o.flux_sq = o.flux_xa = o.totals = None
    assert _call(lib, cp, i, None, o) == 0
    spec = SkySpec(**dict(good, n_dw=1, mode=7, dw_lo=float("nan"), dw_hi=float("nan")))  # mode and, with n_dw = 1,
    o.sky = C.pointer(spec)  # the range are not looked at
    assert _call(lib, cp, i, None, o) == 0


def test_symbol_struct_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    assert "art_event_moments_device" in _lib.SIGNATURES and hasattr(lib, "art_event_moments_device")
    assert C.sizeof(_lib.EventMomentsOut) == 2 * 4 + 6 * 8
    assert len(_lib.MOMENT_TOTALS) == 8
    # the structs of art_event_rows_device are as they were
    assert C.sizeof(_lib.EventRowsIn) == 16 * 8 and C.sizeof(_lib.EventRowsOut) == 2 * 4 + 7 * 8 and len(_lib.EVENT_TOTALS) == 6
    run = inspect.signature(Engine.run_events).parameters
    assert run["errors"].kind is inspect.Parameter.KEYWORD_ONLY and run["errors"].default is False
    assert inspect.signature(A.trees.main_runner_tree).parameters["errors"].default is False
    em = inspect.signature(Engine.event_moments).parameters
    assert list(em)[:5] == ["self", "sample", "weight5", "back", "forward"]
    for k, v in dict(event_offset=0, nbins=50, sky=None, moments=None, cyclotron_rerun=None).items():
        assert em[k].kind is inspect.Parameter.KEYWORD_ONLY and em[k].default == v, k
    from tools import eventmoments
    assert eventmoments.lib().em_entry_bytes() == 16


# ---- trees.event_moments and trees.moments_sigma against plain loops

N_EV, N_ROWS, SIZE = 37, 400, 12


def _synthetic_rows(integer=True):
    """N_ROWS rows of N_EV events (some events without rows), labels in a table of SIZE bins coarse enough that
    an event has several rows in a bin, about a tenth of the labels -1; trials per event"""
    rng = np.random.default_rng(1769)
    event = np.sort(rng.choice(np.setdiff1d(np.arange(N_EV), [0, 5, 36]), N_ROWS))
    bins = rng.integers(0, SIZE, N_ROWS)
    bins[rng.random(N_ROWS) < 0.1] = -1
    power = rng.integers(1, 1000, N_ROWS).astype(float) if integer else rng.lognormal(0.0, 1.5, N_ROWS)
    trials = rng.integers(1, 9, N_EV)
    return event, bins, power, trials


def _loops(event, bins, power, trials):
    S, Q, Cc = np.zeros(SIZE), np.zeros(SIZE), np.zeros(SIZE)
    X = np.zeros((N_EV, SIZE))
    for e in range(N_EV):
        for b in range(SIZE):
            for r in np.flatnonzero((event == e) & (bins == b)):
                X[e, b] += power[r]
            S[b] += X[e, b]
            Q[b] += X[e, b] ** 2
            Cc[b] += X[e, b] * trials[e]
    return S, Q, Cc, X


def test_event_moments_equal_the_double_loop():
    from adiabatic_raytracer_amd.trees import event_moments
    event, bins, power, trials = _synthetic_rows()
    S, Q, Cc, X = _loops(event, bins, power, trials)
    assert (np.count_nonzero(X, axis=None) < (bins >= 0).sum()) and (bins < 0).any()  # several rows in a group
    got = event_moments(event, bins, power, SIZE, trials)
    for g, r in zip(got, (S, Q, Cc)):
        assert g.shape == (SIZE,) and np.array_equal(g, r)
    # Q is not the rows' Σ p²: the group-by matters
    assert not np.array_equal(Q, np.bincount(bins[bins >= 0], weights=power[bins >= 0] ** 2, minlength=SIZE))
    S2, Q2, C2 = event_moments(event, bins, power, SIZE, None)
    assert np.array_equal(S2, S) and np.array_equal(Q2, Q) and C2 is None
    # global event ids index trials as well; rows in any order give the same integers
    perm = np.random.default_rng(5).permutation(N_ROWS)
    got = event_moments(event[perm], bins[perm], power[perm], SIZE, trials)
    assert all(np.array_equal(g, r) for g, r in zip(got, (S, Q, Cc)))
    z = event_moments(np.zeros(0, int), np.zeros(0, int), np.zeros(0), SIZE, trials)
    assert all(np.array_equal(v, np.zeros(SIZE)) for v in z)
    with pytest.raises(ValueError):
        event_moments(event, bins + SIZE, power, SIZE, trials)


def test_moments_sigma_against_the_direct_and_the_textbook_form():
    from adiabatic_raytracer_amd.trees import event_moments, moments_sigma
    event, bins, power, trials = _synthetic_rows(integer=False)
    S, Q, Cc, X = _loops(event, bins, power, trials)
    n, f, A2 = N_EV, float(trials.sum()), float((trials ** 2).sum())
    got = moments_sigma(*event_moments(event, bins, power, SIZE, trials), f, A2, n)
    F = S / f
    direct_var = ((X - F[None, :] * trials[:, None]) ** 2).sum(axis=0)
    got_var = (got * f) ** 2 * (n - 1) / n
    bound = 8 * (n + 4) * U * (Q + 2 * np.abs(F * Cc) + F * F * A2)
    assert np.all(np.abs(got_var - direct_var) <= bound), np.max(np.abs(got_var - direct_var) / bound)
    assert np.all(got > 0) and got.shape == (SIZE,)
    # constant a_e: the textbook n / (n - 1) (Q - S² / n) / f², from the full form and from the C = None form
    a = np.full(N_EV, 3)
    f, A2 = 3.0 * n, 9.0 * n
    S, Q, Cc = event_moments(event, bins, power, SIZE, a)
    text = np.sqrt(n / (n - 1) * (Q - S * S / n)) / f
    full = moments_sigma(S, Q, Cc, f, A2, n)
    assert np.allclose(full, text, rtol=1e-12, atol=0) and np.array_equal(moments_sigma(S, Q, None, f, None, n), text)
    # below two events, or without trials, there is no error estimate
    assert np.isnan(moments_sigma(S, Q, Cc, f, A2, 1)).all() and np.isnan(moments_sigma(S, Q, Cc, f, A2, 0)).all()
    assert np.isnan(moments_sigma(S, Q, Cc, 0, A2, n)).all()
    assert moments_sigma(S.reshape(2, 6), Q.reshape(2, 6), Cc.reshape(2, 6), f, A2, n).shape == (2, 6)
    # a variance that cancels to a negative rounding residue is 0, not NaN
    assert moments_sigma(np.array([3.0]), np.array([9.0 * (1 - 1e-16) / 2]), None, 2.0, None, 2)[0] == 0.0


def test_hist_and_sky_bins_are_numpys():
    from adiabatic_raytracer_amd.trees import hist_bins, sky_bins
    rng = np.random.default_rng(2)
    x = np.r_[rng.uniform(-4, 4, 500), np.linspace(-np.pi, np.pi, 51), np.nan, np.inf, -np.pi, np.pi]
    b = hist_bins(x, 50)
    ok = b >= 0
    assert np.array_equal(np.bincount(b[ok], minlength=50), np.histogram(x[np.isfinite(x)], 50, range=(-np.pi, np.pi))[0])
    assert b[-1] == 49 and b[-2] == 0 and b[-3] == -1 and b[-4] == -1
    th, ph, dw = rng.uniform(0, np.pi, 300), rng.uniform(-np.pi, np.pi, 300), rng.normal(size=300)
    dw[:5] = np.nan
    sp = rng.integers(0, 2, 300)
    kw = dict(n_theta=3, n_phi=4, n_dw=5, theta_axis="cos", dw_range=(-1.0, 1.0))
    lab = sky_bins(th, ph, dw, sp, **kw)
    for s in (0, 1):
        m = sp == s
        ref, _ = np.histogramdd(np.stack([np.cos(th[m]), ph[m], dw[m]], axis=1)[np.isfinite(dw[m])], bins=(3, 4, 5),
                                range=((-1, 1), (-np.pi, np.pi), (-1, 1)))
        got = np.bincount(lab[m & (lab >= 0)] - s * 60, minlength=60).reshape(3, 4, 5)
        assert np.array_equal(got, ref)
    one = sky_bins(th, ph, dw, sp, n_theta=3, n_phi=4)
    assert ((one >= 0) == np.isfinite(dw)).all()


def test_pack_totals_round_trip_with_and_without_moments():
    from adiabatic_raytracer_amd.trees import pack_totals, unpack_totals
    rng = np.random.default_rng(3)
    nbins, shape = 7, (2, 3, 4, 2)
    flux, sky = rng.random(2 * nbins), rng.random(shape)
    mo = {"flux_sq": rng.random(2 * nbins), "flux_xa": rng.random(2 * nbins), "sky_sq": rng.random(shape),
          "sky_xa": rng.random(shape), "totals": rng.random(8)}
    # without the new part: the vector is today's, byte for byte
    old = np.concatenate([flux, [11.0, 0.5, 0.25, 9.0]])
    assert pack_totals(flux, 11, 0.5, 0.25, 9).tobytes() == old.tobytes()
    assert pack_totals(flux, 11, 0.5, 0.25, 9, sky).tobytes() == np.concatenate([old, sky.reshape(-1)]).tobytes()
    assert "moments" not in unpack_totals(pack_totals(flux, 11, 0.5, 0.25, 9, sky), nbins, shape)
    for with_sky in (True, False):
        v = pack_totals(flux, 11, 0.5, 0.25, 9, sky if with_sky else None, mo)
        head = pack_totals(flux, 11, 0.5, 0.25, 9, sky if with_sky else None)
        assert v[:head.size].tobytes() == head.tobytes()
        assert v.size == head.size + 4 * nbins + (2 * sky.size if with_sky else 0) + 8
        tt = unpack_totals(v, nbins, shape if with_sky else None, moments=True)
        assert tt["f_inx"] == 11 and tt["rows"] == 9 and np.array_equal(tt["flux"], flux)
        for k in ("flux_sq", "flux_xa", "totals"):
            assert np.array_equal(tt["moments"][k], mo[k]), k
        for k in ("sky_sq", "sky_xa"):
            assert np.array_equal(tt["moments"][k], mo[k]) if with_sky else tt["moments"][k] is None
        assert np.array_equal(tt["sky"], sky) if with_sky else "sky" not in tt
        assert np.array_equal(unpack_totals(v + v, nbins, shape if with_sky else None, moments=True)["moments"]["totals"],
                              2 * mo["totals"])  # the parts add over ranks


# ---- the host build of the per-tree group-by

TREE_SIZES = (0, 1, 2, 64, 65, 300)


def test_group_by_host_build_equals_numpy():
    from adiabatic_raytracer_amd.trees import event_moments
    from tools import eventmoments as EM
    rng = np.random.default_rng(11)
    nbins, sky_size = 3, 10  # few keys: they repeat inside a tree
    start = np.r_[0, np.cumsum(TREE_SIZES)]
    n = int(start[-1])
    tree = np.repeat(np.arange(len(TREE_SIZES)), TREE_SIZES)
    final = rng.random(n) < 0.6
    final[0] = final[1] = True  # the tree of one record has a row, the first of the tree of two as well
    sp = rng.integers(0, 2, n)
    fb = np.where(rng.random(n) < 0.85, rng.integers(0, nbins, n), -1)  # flux bin, -1 outside the range
    sky = np.where(rng.random(n) < 0.85, sp * (sky_size // 2) + rng.integers(0, sky_size // 2, n), -1)
    flux = np.where(fb >= 0, sp * nbins + fb, np.where(sp == 1, EM.PHOTON, EM.AXION))
    flux, sky = np.where(final, flux, EM.NONE), np.where(final, sky, -1)
    power = rng.integers(1, 100, n).astype(float)
    att1 = rng.integers(0, 5, len(TREE_SIZES))
    got = EM.forest(start, flux, sky, power, att1, nbins, sky_size)
    a = att1 + np.bincount(tree[final & (sp == 1)], minlength=len(TREE_SIZES))
    f = final
    _, fq, fc = event_moments(tree[f], np.where(fb >= 0, sp * nbins + fb, -1)[f], power[f], 2 * nbins, a)
    _, sq, sc = event_moments(tree[f], sky[f], power[f], sky_size, a)
    _, tq, tc = event_moments(tree[f], sp[f], power[f], 2, a)
    assert np.array_equal(got["flux_sq"], fq) and np.array_equal(got["flux_xa"], fc)
    assert np.array_equal(got["sky_sq"], sq) and np.array_equal(got["sky_xa"], sc)
    assert np.array_equal(got["totals"], np.r_[len(TREE_SIZES), a.sum(), (a * a).sum(), tq, tc, 0.0])
    assert fq.min() > 0 and (fb[f] < 0).any() and (sky[f] < 0).any()
    # the rows' Σ p² would be another table: keys do repeat inside these trees
    assert not np.array_equal(sq, np.bincount(sky[f & (sky >= 0)], weights=power[f & (sky >= 0)] ** 2, minlength=sky_size))
    # nbins = 0: no flux table, the species still come from the encoded field
    got0 = EM.forest(start, np.where(final, np.where(sp == 1, EM.PHOTON, EM.AXION), EM.NONE), sky, power, att1, 0, sky_size)
    assert np.array_equal(got0["totals"], got["totals"]) and np.array_equal(got0["sky_sq"], sq)
