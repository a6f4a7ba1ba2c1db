"""Jackknife replicates without a GPU ("Jackknife replicates"): the C boundary's argument checks,
trees.rows_replicates against a brute-force loop, trees.jackknife against closed forms, trees.coupling_crossing,
and the packing into the run's one reduced vector.

Tolerances. The synthetic powers are integers, so every table, every sum S over the groups and every S - T_g is
exact, and the closed forms are evaluated in exact rational arithmetic (fractions.Fraction). What is left is the
rounding of jackknife itself, with u = 2^-53 and R' groups:
  θ_g = (S - T_g) / (f - a_g f / Σa): the divisor takes three roundings, the quotient one: relative 4 u;
  mean θ: R' - 1 adds and a division: relative R' u; so d_g = θ_g - mean is within δ = (R' + 6) u max|θ| of exact;
  Σ d_g²: each square 2 |d_g| δ + u d_g², the sum (R' - 1) u, the factor (R' - 1) / R' two more; sqrt and the test's
  own squaring of σ three more: |Δσ²| <= c (2 δ Σ|d_g| + (R' + 8) u Σ d_g²), c = (R' - 1) / R'.
"""
import ctypes as C
import inspect
from fractions import Fraction

import numpy as np
import pytest

U = 2.0 ** -53
INVALID = -1


# ---------------------------------------------------------------------------------------------------
# the C boundary
def _structs():
    from adiabatic_raytracer_amd._lib import EventReplicatesOut, EventRowsIn
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    ro = EventReplicatesOut(8, 0, 1, 50, None, None, a, None, None, a, a)
    return d, ein, ro


def _call(lib, cp, ein, start, ro):
    ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731
    return lib.art_event_replicates_device(ref(cp), ref(ein), start, ref(ro), None)


def test_symbol_struct_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib, trees
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    assert "art_event_replicates_device" in _lib.SIGNATURES and hasattr(lib, "art_event_replicates_device")
    assert C.sizeof(_lib.EventReplicatesOut) == 4 * 4 + 7 * 8 and lib.art_abi_version() == 1
    assert _lib.REPLICATE_GROUPS == ("events", "a", "misplaced") and _lib.REPLICATE_KINDS == {"run": 0, "coupling": 1, "halo": 2}
    for fn in (Engine.run_events, trees.main_runner_tree):
        par = inspect.signature(fn).parameters["replicates"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    er = inspect.signature(Engine.event_replicates).parameters
    assert list(er)[:6] == ["self", "sample", "weight5", "back", "forward", "R"]
    for k, v in dict(event_offset=0, nbins=50, sky=None, cyclotron_rerun=None, rep=None, kind="run", node_factor=None,
                     event_factor=None).items():
        assert er[k].kind is inspect.Parameter.KEYWORD_ONLY and er[k].default == v, k
    for fn in (trees.rank_vector, trees._finish_run):
        par = inspect.signature(fn).parameters["replicates"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    assert Engine.REPLICATES_MAX_BYTES == 1 << 30


def test_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import SkySpec
    lib = A.load_library()
    cp = A.Params().to_c()
    d, ein, ro = _structs()
    start = C.c_void_p(C.addressof(d))
    err = lib.art_last_error
    assert _call(lib, None, ein, start, ro) == INVALID and b"params" in err()
    assert _call(lib, cp, None, start, ro) == INVALID and b"NULL in or out" in err()
    assert _call(lib, cp, ein, start, None) == INVALID and b"NULL in or out" in err()

    def bad(msg, start=start, **kw):
        _, i, o = _structs()
        for k, v in kw.items():
            setattr(i if hasattr(i, k) else o, k, v)
        assert _call(lib, cp, i, start, o) == INVALID, msg
        assert msg.encode() in err(), (msg, err())

    a = C.addressof(d)
    for R in (-1, 0, 1, 65, 1000):
        bad("n_groups must be in [2, 64]", n_groups=R)
    for kind in (-1, 3):
        bad("kind must be", kind=kind)
    for K in (0, -1, 33):
        bad("n_sets must be in [1, 32]", kind=2, n_sets=K, event_factor=a)
    bad("n_sets must be 1 with kind 0", n_sets=2)
    bad("node_factor is NULL", kind=1, n_sets=3, event_factor=a)
    bad("event_factor is NULL", kind=1, n_sets=3, node_factor=a)
    bad("event_factor is NULL", kind=2, n_sets=3)
    # the moments call's faults on the sizes, nbins, the sky spec and node_start
    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    bad("nbins must be", nbins=4097)
    bad("nbins must be", nbins=-1)
    bad("node_start is NULL", start=None)
    good = dict(n_theta=4, n_phi=8, n_dw=3, theta_axis=1, mode=0, dw_lo=-1e-6, dw_hi=1e-6)
    for msg, kw in {"bin counts": dict(good, n_theta=0), "theta_axis": dict(good, theta_axis=2), "ranges": dict(good, dw_hi=-1.0),
                    "sky_hist is NULL": good}.items():
        spec = SkySpec(**kw)
        bad(msg, sky=C.pointer(spec))
    # a NULL table that the call needs, a NULL input buffer
    bad("totals or groups is NULL", totals=None)
    bad("totals or groups is NULL", groups=None)
    bad("flux is NULL", flux=None)
    bad("NULL input buffer", weight5=None)
    # no events: ART_OK after the checks, nothing touched (no device is reached: there is none here)
    for kind, K, nf, ef in ((0, 1, None, None), (1, 32, a, a), (2, 5, None, a)):
        _, i, o = _structs()
        i.n_events = i.n_nodes = 0
        o.kind, o.n_sets, o.node_factor, o.event_factor = kind, K, nf, ef
        o.flux = o.totals = o.groups = None
        assert _call(lib, cp, i, None, o) == 0


def test_python_value_errors():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import trees
    from adiabatic_raytracer_amd.engine import Engine
    for R in (0, 1, 65, 2.5):
        with pytest.raises(ValueError, match="replicates: 2 to 64 groups"):
            Engine.run_events(None, 0, replicates=R)  # (before any work is done: nothing of the engine is touched)
    for R in (1, 65):
        with pytest.raises(ValueError, match="replicates: 2 to 64 groups"):
            trees.main_runner_tree(A.Params(), 3, replicates=R)
        with pytest.raises(ValueError, match="replicates: 2 to 64 groups"):
            trees.rows_replicates(np.zeros((0, 13)), R, 10)
    # the 1 GiB cap: 32 sets x 64 groups of a 64 x 128 x 16 map; the run's own 64 groups of it fit
    shape = (2, 64, 128, 16)
    Engine._replicates_fit("the run", 1, 64, 50, shape)
    with pytest.raises(ValueError, match="drop the sky map from the scan or lower R"):
        Engine._replicates_fit("the coupling scan", 32, 64, 50, shape)
    Engine._replicates_fit("the coupling scan", 32, 64, 50, None)
    assert 8 * 32 * 64 * (100 + 2 * 64 * 128 * 16 + 2) > Engine.REPLICATES_MAX_BYTES


# ---------------------------------------------------------------------------------------------------
# rows_replicates on synthetic rows with integer powers
EVENT_LO = 1003


def _rows(rng, n_events, n_rows, lo=EVENT_LO):
    """rows of the events lo .. lo + n_events (some of them without a row), with integer powers"""
    rows = np.zeros((n_rows, 13))
    have = rng.choice(n_events, size=max(1, (2 * n_events) // 3), replace=False)
    rows[:, 0] = np.sort(rng.choice(have, n_rows)) + 1.0 + lo
    rows[:, 1] = rng.integers(0, 2, n_rows)
    rows[:, 2] = np.arccos(rng.uniform(-1, 1, n_rows))
    rows[:, 3] = rng.uniform(-np.pi, np.pi, n_rows)
    rows[:4, 3] = [-np.pi, np.pi, 0.0, np.nan][:min(4, n_rows)]  # the edges, and a row no table counts
    rows[:, 7] = rng.integers(1, 4, n_rows)
    rows[:, 8] = rng.integers(1, 20, n_rows)
    rows[:, 12] = -1.0 + rng.uniform(-2e-6, 4e-6, n_rows)
    return rows


SKY = dict(n_theta=3, n_phi=5, n_dw=4, theta_axis="cos", dw_range=(-1 - 1e-6, -1 + 3e-6))


@pytest.mark.parametrize("R,n_events,n_rows", [(5, 40, 300), (7, 41, 250), (64, 9, 30), (2, 1, 3)])
def test_rows_replicates_against_a_loop(R, n_events, n_rows):
    from adiabatic_raytracer_amd import trees
    assert EVENT_LO % R != 0
    rng = np.random.default_rng(100 * R + n_events)
    rows = _rows(rng, n_events, n_rows)
    att = rng.integers(1, 6, n_events).astype(np.int32)
    nbins = 10
    got = trees.rows_replicates(rows, R, nbins, SKY, att, EVENT_LO)
    assert got["kind"] == "run" and got["R"] == R
    assert got["flux"].shape == (1, R, 2 * nbins) and got["sky"].shape == (1, R, 2, 3, 5, 4) and got["totals"].shape == (1, R, 2)
    fb = trees.hist_bins(rows[:, 3], nbins)
    sb = trees.sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **SKY)
    flux, sky, tot, grp = np.zeros((R, 2 * nbins)), np.zeros((R, 2 * 3 * 5 * 4)), np.zeros((R, 2)), np.zeros((R, 3))
    for e in range(n_events):
        grp[(EVENT_LO + e) % R, 0] += 1
        grp[(EVENT_LO + e) % R, 1] += int(att[e]) - 1
    for i, row in enumerate(rows):
        g, sp, p = (int(row[0]) - 1) % R, int(row[1]), row[8] * row[7]
        tot[g, sp] += p
        grp[g, 1] += sp
        if fb[i] >= 0:
            flux[g, sp * nbins + fb[i]] += p
        if sb[i] >= 0:
            sky[g, sb[i]] += p
    assert np.array_equal(got["flux"][0], flux) and np.array_equal(got["sky"][0].reshape(R, -1), sky)
    assert np.array_equal(got["totals"][0], tot) and np.array_equal(got["groups"], grp)
    if n_events < R:
        assert (grp[:, 0] == 0).sum() == R - n_events and not got["flux"][0][grp[:, 0] == 0].any()
    # the sum over the groups is the run's own tables, and Σ a_g its f_inx
    p = rows[:, 8] * rows[:, 7]
    ok = fb >= 0
    for s_ in (0, 1):
        h, _ = np.histogram(rows[ok & (rows[:, 1] == s_), 3], bins=nbins, range=(-np.pi, np.pi), weights=p[ok & (rows[:, 1] == s_)])
        assert np.array_equal(got["flux"][0].sum(axis=0)[s_ * nbins:(s_ + 1) * nbins], h)
    assert np.array_equal(got["sky"][0].sum(axis=0).reshape(-1), np.bincount(sb[sb >= 0], weights=p[sb >= 0], minlength=120))
    f_inx = int((att.astype(np.int64) - 1).sum() + (rows[:, 1] == 1).sum())
    assert got["groups"][:, 1].sum() == f_inx and got["groups"][:, 0].sum() == n_events
    # without attempts: a_e constant, the events counted up to n_events (or to the last one that has a row)
    const = trees.rows_replicates(rows, R, nbins, None, None, EVENT_LO, n_events=n_events)
    assert const["sky"] is None and np.array_equal(const["groups"][:, 1], const["groups"][:, 0])
    assert np.array_equal(const["groups"][:, 0], grp[:, 0]) and np.array_equal(const["flux"], got["flux"])
    last = int(rows[:, 0].max()) - EVENT_LO
    assert trees.rows_replicates(rows, R, nbins, None, None, EVENT_LO)["groups"][:, 0].sum() == last
    res = trees.replicates_result(got, f_inx)
    assert res["misplaced"] == 0 and res["flux"].shape == (2, nbins) and res["sky_map"].shape == (2, 3, 5, 4)
    assert np.array_equal(res["flux"].reshape(-1), got["flux"][0].sum(axis=0) / f_inx)
    assert np.array_equal(res["sum_weight_sln_prob"], tot.sum(axis=0) / f_inx) and np.array_equal(res["a_g"], grp[:, 1])


# ---------------------------------------------------------------------------------------------------
# jackknife against closed forms
def _exact_sigma2(T, a, f):
    """the jackknife variance of S / f per column, in exact rational arithmetic: T (R', m) integers, a (R') the
    groups' parts of f (Fractions); and Σ|d|, Σ d², max|θ| as floats for the tolerance"""
    Rp, m = len(T), len(T[0])
    var, sd, sdd, tmax = [], [], [], []
    for j in range(m):
        S = sum(Fraction(int(T[g][j])) for g in range(Rp))
        th = [(S - Fraction(int(T[g][j]))) / (f - a[g]) for g in range(Rp)]
        mean = sum(th) / Rp
        d = [t - mean for t in th]
        var.append(Fraction(Rp - 1, Rp) * sum(x * x for x in d))
        sd.append(float(sum(abs(x) for x in d)))
        sdd.append(float(sum(x * x for x in d)))
        tmax.append(float(max(abs(t) for t in th)))
    return var, np.array(sd), np.array(sdd), np.array(tmax)


def _tolerance(Rp, sd, sdd, tmax):
    """the module docstring's bound on |Δσ²|"""
    c = (Rp - 1.0) / Rp
    return c * (2.0 * (Rp + 6) * U * tmax * sd + (Rp + 8) * U * sdd)


@pytest.mark.parametrize("R", [2, 5, 64])
def test_jackknife_linear_is_batch_means(R):
    """constant a_e and equal groups: σ² of a linear φ is R / ((R - 1) f²) Σ_g (T_g - mean T)²"""
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(R)
    n_events, nbins, f_inx = 3 * R, 6, 977
    rows = _rows(rng, n_events, 40 * R, lo=0)
    rep = trees.replicates_result(trees.rows_replicates(rows, R, nbins, None, None, 0, n_events=n_events), f_inx)
    assert np.array_equal(rep["n_g"], np.full(R, 3.0))
    out = trees.jackknife(rep, lambda t: np.concatenate([t["flux"].reshape(-1), t["sum_weight_sln_prob"]]))
    T = np.concatenate([rep["raw"]["flux"][0], rep["raw"]["totals"][0]], axis=1)
    assert out["groups_used"] == R and out["value"].shape == out["sigma"].shape == (2 * nbins + 2,)
    assert np.array_equal(out["value"], T.sum(axis=0) / f_inx)
    f = Fraction(f_inx)
    for j in range(T.shape[1]):
        S = sum(Fraction(int(v)) for v in T[:, j])
        want = Fraction(R, R - 1) / (f * f) * sum((Fraction(int(v)) - S / R) ** 2 for v in T[:, j])
        _, sd, sdd, tmax = _exact_sigma2(T[:, j:j + 1], [f / R] * R, f)
        tol = _tolerance(R, sd, sdd, tmax)[0] + 3 * U * float(want)
        assert abs(out["sigma"][j] ** 2 - float(want)) <= tol, (j, out["sigma"][j] ** 2, float(want), tol)
    assert out["sigma"][-1] > 0


@pytest.mark.parametrize("n", [2, 7, 64])
def test_jackknife_one_event_per_group_is_the_textbook_error(n):
    """n = R: the jackknife of S / f is moments_sigma's trials=None form n / (n - 1) (Q - S² / n) / f²"""
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(n)
    rows = _rows(rng, n, 6 * n, lo=0)
    nbins, f_inx = 4, 53 * n
    rep = trees.replicates_result(trees.rows_replicates(rows, n, nbins, None, None, 0, n_events=n), f_inx)
    assert np.array_equal(rep["n_g"], np.ones(n))
    out = trees.jackknife(rep, lambda t: np.concatenate([t["flux"].reshape(-1), t["sum_weight_sln_prob"]]))
    T = np.concatenate([rep["raw"]["flux"][0], rep["raw"]["totals"][0]], axis=1)  # one event per group: T_g is X_e
    S, Q = T.sum(axis=0), (T * T).sum(axis=0)
    ref = trees.moments_sigma(S, Q, None, f_inx, None, n)
    f = Fraction(f_inx)
    var, sd, sdd, tmax = _exact_sigma2(T, [f / n] * n, f)
    for j in range(T.shape[1]):
        want = Fraction(n, n - 1) * (Fraction(int(Q[j])) - Fraction(int(S[j])) ** 2 / n) / (f * f)
        assert var[j] == want  # the two forms are one in exact arithmetic
        tol = _tolerance(n, sd, sdd, tmax)[j] + 3 * U * float(want)
        assert abs(out["sigma"][j] ** 2 - float(want)) <= tol, j
        # moments_sigma's own rounding: S² / n rounds once (u S² / n), then three more operations
        ref_tol = (U * float(S[j]) ** 2 / n + 3 * U * abs(float(Q[j]) - float(S[j]) ** 2 / n)) * n / ((n - 1.0) * f_inx ** 2) \
            + 3 * U * float(want)
        assert abs(out["sigma"][j] ** 2 - ref[j] ** 2) <= tol + ref_tol, j


def test_jackknife_empty_groups_nan_and_cov():
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(3)
    R, n_events, nbins = 16, 5, 4  # events 1003 .. 1007: five groups hold one event each, eleven are empty
    rows = _rows(rng, n_events, 40)
    att = rng.integers(2, 6, n_events).astype(np.int32)
    raw = trees.rows_replicates(rows, R, nbins, None, att, EVENT_LO)
    f_inx = int(raw["groups"][:, 1].sum())
    rep = trees.replicates_result(raw, f_inx)
    used = np.flatnonzero(rep["n_g"] > 0)
    assert len(used) == 5
    out = trees.jackknife(rep, lambda t: t["sum_weight_sln_prob"], cov=True)
    assert out["groups_used"] == 5 and out["cov"].shape == (2, 2)
    T, a = raw["totals"][0][used], [Fraction(int(v)) for v in raw["groups"][used, 1]]
    var, sd, sdd, tmax = _exact_sigma2(T, a, Fraction(f_inx))
    tol = _tolerance(5, sd, sdd, tmax)
    for j in range(2):
        assert abs(out["sigma"][j] ** 2 - float(var[j])) <= tol[j] + 3 * U * float(var[j])
        assert abs(out["cov"][j, j] - out["sigma"][j] ** 2) <= 4 * U * out["cov"][j, j]  # the diagonal is σ²
    assert out["cov"][0, 1] == out["cov"][1, 0]
    # the same events in sixteen or in 64 groups: the empty ones change nothing
    out64 = trees.jackknife(trees.replicates_result(trees.rows_replicates(rows, 64, nbins, None, att, EVENT_LO), f_inx),
                            lambda t: t["sum_weight_sln_prob"])
    assert out64["groups_used"] == 5 and np.allclose(out64["sigma"], out["sigma"], rtol=64 * U, atol=0)
    # one group with events: NaN; a leave-out divisor of 0: NaN
    one = trees.rows_replicates(rows[rows[:, 0] == rows[0, 0]], 4, nbins, None, att[:1], int(rows[0, 0]) - 1)
    res = trees.jackknife(trees.replicates_result(one, int(one["groups"][:, 1].sum())), lambda t: t["flux"], cov=True)
    assert res["groups_used"] == 1 and np.isnan(res["sigma"]).all() and res["sigma"].shape == (2, nbins) and np.isnan(res["cov"]).all()
    assert np.isfinite(res["value"]).all()
    two = trees.rows_replicates(rows[:0], 2, nbins, None, np.array([4, 1], np.int32), 0)  # a_g = (3, 0): leaving group 0 out leaves f = 0
    res = trees.jackknife(trees.replicates_result(two, 3), lambda t: t["sum_weight_sln_prob"])
    assert res["groups_used"] == 2 and np.isnan(res["sigma"]).all()
    # a nonlinear function of a scan's tables is handed the leading axis
    scan = {k: (np.repeat(v, 3, axis=0) if k in ("flux", "totals") else v) for k, v in raw.items()}
    scan["kind"] = "coupling"
    res = trees.jackknife(trees.replicates_result(scan, f_inx), lambda t: t["sum_weight_sln_prob"][2, 1] / t["sum_weight_sln_prob"][0, 1])
    assert res["value"] == 1.0 and res["sigma"] == 0.0


def test_coupling_crossing_on_a_quadratic_scan():
    """totals exactly ∝ g² in every group: the crossing of `power` is g = sqrt(power f / c) for the c of all groups,
    and its leave-one-out values the same with c and f of the groups left in"""
    from adiabatic_raytracer_amd import trees
    R, g = 6, np.array([1e-12, 2e-12, 4e-12, 8e-12])
    c_g = np.array([3.0, 5.0, 2.0, 7.0, 0.0, 4.0])  # photon power / (g / 1e-12)² per group
    a_g, n_g = np.array([10.0, 12.0, 9.0, 11.0, 8.0, 10.0]), np.full(R, 5.0)
    s = (g / 1e-12) ** 2  # 1, 4, 16, 64: every product below is exact
    totals = np.zeros((len(g), R, 2))
    totals[:, :, 1] = s[:, None] * c_g[None, :]
    totals[:, :, 0] = 1.0
    raw = {"kind": "coupling", "R": R, "flux": np.zeros((len(g), R, 0)), "sky": None, "totals": totals,
           "groups": np.stack([n_g, a_g, np.zeros(R)], axis=1)}
    f = int(a_g.sum())
    scan = {"g": g, "replicates": trees.replicates_result(raw, f)}
    assert scan["replicates"]["sum_weight_sln_prob"].shape == (4, 2)
    power = 2.0  # c / f = 21 / 60: the crossing lies between g = 2e-12 and 4e-12
    out = trees.coupling_crossing(scan, power)
    crossing = lambda c, ff: 1e-12 * np.sqrt(power * ff / c)  # noqa: E731
    # log g = -27.6 rounds by 27.6 u, the interpolated sum as much again, exp turns that into a relative error:
    # (2 |log g| + 8) u of the crossing with the other operations, 63 u
    rel = (2 * abs(np.log(1e-12)) + 8) * U
    assert out["groups_used"] == R and out["value"] == pytest.approx(crossing(c_g.sum(), f), rel=rel)
    assert 2e-12 < out["value"] < 4e-12
    th = crossing(c_g.sum() - c_g, f - a_g)
    want = np.sqrt((R - 1.0) / R * ((th - th.mean()) ** 2).sum())
    # each θ_g within rel θ_g of the closed form: σ, a norm of the θ's deviations, within sqrt(R) rel max θ
    assert out["sigma"] == pytest.approx(want, abs=np.sqrt(R) * rel * th.max()) and out["sigma"] > 0
    assert np.isnan(trees.coupling_crossing(scan, 1e6)["value"])  # the curve does not reach it
    ax = trees.coupling_crossing(scan, 1.0 / 60.0 * 1.0, species=0)  # the axion total does not depend on g: no crossing
    assert np.isnan(ax["value"])
    with pytest.raises(ValueError, match="no replicates"):
        trees.coupling_crossing({"g": g}, power)
    with pytest.raises(ValueError, match="power"):
        trees.coupling_crossing(scan, 0.0)


# ---------------------------------------------------------------------------------------------------
# packing
def test_pack_round_trip_and_rank_vector(monkeypatch):
    from adiabatic_raytracer_amd import shard, trees
    rng = np.random.default_rng(8)
    R, nbins, n_events = 5, 6, 30
    rows = _rows(rng, n_events, 200, lo=0)
    att = rng.integers(1, 6, n_events).astype(np.int32)
    sky_kw = dict(SKY)
    whole = trees.rows_replicates(rows, R, nbins, sky_kw, att, 0)
    back = trees.replicates_unpack(trees.replicates_pack(whole), whole)
    assert back["kind"] == "run" and back["R"] == R
    for k in trees.REPLICATE_KEYS:
        assert np.array_equal(back[k], whole[k]) and back[k].shape == whole[k].shape
    nosky = trees.rows_replicates(rows, R, nbins, None, att, 0)
    assert len(trees.replicates_pack(nosky)) == R * (2 * nbins + 2 + 3) and trees.replicates_unpack(trees.replicates_pack(nosky), nosky)["sky"] is None
    # two disjoint event ranges' vectors add to the whole range's (integer powers: exactly)
    cut = 13
    first, second = rows[rows[:, 0] <= cut], rows[rows[:, 0] > cut]
    va = trees.replicates_pack(trees.rows_replicates(first, R, nbins, sky_kw, att[:cut], 0))
    vb = trees.replicates_pack(trees.rows_replicates(second, R, nbins, sky_kw, att[cut:], cut))
    assert np.array_equal(va + vb, trees.replicates_pack(whole))
    # rank_vector: without replicates the vector and its ends are today's; with them they come last
    tot = trees.pack_totals(rng.random(2 * nbins), 40, 1.0, 2.0, 7)
    assert trees.rank_vector(tot)[0] is tot and trees.rank_vector(tot, replicates=None)[0] is tot
    assert list(trees.rank_vector(tot)[1]) == [len(tot)] and list(trees.rank_vector(tot, replicates={})[1]) == [len(tot)]
    K = 2
    scan = {"kind": "coupling", "R": R, "flux": rng.random((K, R, 2 * nbins)), "sky": None, "totals": rng.random((K, R, 2)),
            "groups": whole["groups"]}
    hscan = dict(scan, kind="halo", flux=rng.random((K, R, 2 * nbins)))
    craw = {"g": [1e-12, 2e-12], "n_events": n_events, "flux": rng.random((K, 2 * nbins)), "sky": None,
            "totals": np.concatenate([rng.random((K, 3)), np.zeros((K, 3))], axis=1)}
    hraw = {"models": [(220.0, (0.0, 0.0, 0.0))] * K, "n_events": n_events, "flux": rng.random((K, 2 * nbins)), "sky": None,
            "totals": np.concatenate([rng.random((K, 4)), np.zeros((K, 1))], axis=1)}
    reps = {"halo": hscan, "run": nosky, "coupling": scan}  # (any order of the keys: the vector's is run, coupling, halo)
    vec, ends = trees.rank_vector(tot, craw, hraw, replicates=reps)
    old, old_ends = trees.rank_vector(tot, craw, hraw)
    want = np.concatenate([old, trees.replicates_pack(nosky), trees.replicates_pack(scan), trees.replicates_pack(hscan)])
    assert vec.tobytes() == want.tobytes() and list(ends[:3]) == list(old_ends) and ends[-1] == len(want) and len(ends) == 6
    # _finish_run over two ranks with the same tables: every part comes back doubled, the halo scan's too
    monkeypatch.setattr(shard, "allreduce_sum", lambda v: 2.0 * v)
    info, plain = {}, {}
    kw = dict(nbins=nbins, sky_kw=None, errors=False, world=2, events=(0, n_events), n_events=2 * n_events, g0=1e-12, path=None)
    trees._finish_run(np.zeros((0, 13)), tot, craw, hraw, run_info=info, replicates=reps, **kw)
    trees._finish_run(np.zeros((0, 13)), tot, craw, hraw, run_info=plain, **kw)
    assert list(info) == list(plain) + ["replicates"] and "replicates" not in plain["coupling_scan"]
    assert np.array_equal(info["halo_scan"]["raw"]["flux"], 2.0 * hraw["flux"]) and np.array_equal(info["halo_scan"]["flux"], plain["halo_scan"]["flux"])
    assert np.array_equal(info["coupling_scan"]["flux"], plain["coupling_scan"]["flux"])
    assert info["replicates"]["f_inx"] == 80 and np.array_equal(info["replicates"]["raw"]["flux"], 2.0 * nosky["flux"])
    assert np.array_equal(info["coupling_scan"]["replicates"]["raw"]["totals"], 2.0 * scan["totals"])
    assert np.array_equal(info["halo_scan"]["replicates"]["raw"]["flux"], 2.0 * hscan["flux"])
    assert info["halo_scan"]["replicates"]["kind"] == "halo" and info["coupling_scan"]["replicates"]["sum_weight_sln_prob"].shape == (K, 2)
    # the run's replicates alone, with no scan
    only = {}
    trees._finish_run(np.zeros((0, 13)), tot, run_info=only, replicates={"run": nosky}, **kw)
    assert np.array_equal(only["replicates"]["raw"]["groups"], 2.0 * nosky["groups"]) and "coupling_scan" not in only
