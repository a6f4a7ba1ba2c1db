"""The coupling x halo grid without a GPU ("Coupling x halo grid"): the C boundary's struct and
argument checks, the header's per-record and per-event functions (tools/eventgrid, a host compile of
art_event_grid.h) against trees.grid_tables on hand-built records, the packing into the run's one reduced vector,
and the read-off, trees.grid_jackknife and trees.limit_band, against closed forms.

Tolerances. The hand-built factors and powers are small integers, so every table entry, group table and moment
total is an integer below 2^53 and the two sides are np.array_equal, whatever the order of the adds. limit_band on
P[kg, kh] = c_h g_kg⁴ interpolates a straight line in log-log: the crossing is exp(x_i + (y0 - y_i) / (y_j - y_i)
(x_j - x_i)) with every log and exp within an ulp and |x| <= 28, |y| <= 120: the cancellation in y0 - y_i loses at
most 120 u absolute of a slope-4 line, so 1e-13 relative on g covers it with room. The batch-means identity takes
tests/test_replicates.py's bound on jackknife's own roundings."""
import ctypes as C
import inspect
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

from test_replicates import _exact_sigma2, _tolerance

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

U = 2.0 ** -53
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------
# the C boundary
def _structs():
    from adiabatic_raytracer_amd._lib import EventGridOut, EventRowsIn
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    go = EventGridOut(3, 2, 50, 8, a, a, a, a, a, a, a, a, None)
    return d, ein, go


def _call(lib, cp, ein, start, go):
    ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731
    return lib.art_event_grid_device(ref(cp), ref(ein), start, ref(go), None)


def test_symbol_struct_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib, trees
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    assert "art_event_grid_device" in _lib.SIGNATURES and hasattr(lib, "art_event_grid_device")
    assert lib.art_abi_version() == 1
    # the ctypes struct field by field against the header's
    text = open(os.path.join(ROOT, "include", "art.h")).read()
    body = re.search(r"typedef struct art_event_grid_out \{(.*?)\} art_event_grid_out;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w \*]+?)\s*\b(\w+);", body)]
    kinds = {"int32_t": C.c_int32, "const double*": C.c_void_p, "double*": C.c_void_p}
    assert [(n, kinds[t]) for t, n in fields] == list(_lib.EventGridOut._fields_)
    assert C.sizeof(_lib.EventGridOut) == 4 * 4 + 9 * 8
    assert re.search(r"int art_event_grid_device\(const art_params\* p, const art_event_rows_in\* in, const int64_t\* "
                     r"node_start,\s*const art_event_grid_out\* out, void\* stream\);", text)
    assert _lib.GRID_TOTALS == ("sum_axion", "sum_photon", "misplaced")
    assert (_lib.GRID_MAX_COUPLINGS, _lib.GRID_MAX_MODELS) == (32, 32)
    import eventgrid
    assert eventgrid.limits()[:3] == (_lib.GRID_MAX_COUPLINGS, _lib.GRID_MAX_MODELS, len(_lib.GRID_TOTALS))
    for fn in (Engine.run_events, trees.main_runner_tree):
        par = inspect.signature(fn).parameters["grid"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    for fn in (trees.rank_vector, trees._finish_run):
        par = inspect.signature(fn).parameters["grid"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    eg = inspect.signature(Engine.event_grid).parameters
    assert list(eg)[:5] == ["self", "sample", "weight5", "back", "forward"]
    for k in ("weights", "back_factor", "ratio", "g", "models", "base"):
        assert eg[k].kind is inspect.Parameter.KEYWORD_ONLY and eg[k].default is inspect.Parameter.empty, k
    for k, v in dict(event_offset=0, nbins=50, replicates=None, errors=False, cyclotron_rerun=None, grid=None).items():
        assert eg[k].kind is inspect.Parameter.KEYWORD_ONLY and eg[k].default == v, k
    for name in ("grid_raw", "grid_pack", "grid_unpack", "grid_result", "grid_tables", "grid_jackknife", "limit_band"):
        assert callable(getattr(trees, name)), name


def test_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    lib = A.load_library()
    cp = A.Params().to_c()
    d, ein, go = _structs()
    start = C.c_void_p(C.addressof(d))
    err = lib.art_last_error
    assert _call(lib, None, ein, start, go) == INVALID and b"params" in err()
    assert _call(lib, cp, None, start, go) == INVALID and b"NULL in or out" in err()
    assert _call(lib, cp, ein, start, None) == INVALID and b"NULL in or out" in err()

    def bad(msg, start=start, **kw):
        _, i, o = _structs()
        for k, v in kw.items():
            setattr(o if hasattr(o, k) else i, k, v)  # (`back` names a field of both: the grid's is meant)
        assert _call(lib, cp, i, start, o) == INVALID, msg
        assert msg.encode() in err(), (msg, err())

    for K in (0, -1, 33):
        bad("n_couplings must be in [1, 32]", n_couplings=K)
        bad("n_models must be in [1, 32]", n_models=K)
    for R in (-1, 1, 65, 1000):
        bad("n_groups must be 0", n_groups=R)
    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    bad("nbins must be", nbins=4097)  # the moments call's faults on nbins
    bad("nbins must be", nbins=-1)
    bad("node_factor is NULL", node_factor=None)
    bad("back or ratio is NULL", back=None)
    bad("back or ratio is NULL", ratio=None)
    bad("back or ratio is NULL", ratio=None, n_nodes=0)  # events alone need their factors too
    bad("node_start is NULL", start=None)
    bad("totals is NULL", totals=None)
    bad("flux is NULL", flux=None)
    bad("totals_rep or groups is NULL", totals_rep=None)
    bad("totals_rep or groups is NULL", groups=None)
    bad("flux_rep is NULL", flux_rep=None)
    bad("NULL input buffer", weight5=None)
    # no events: ART_OK after the range checks, nothing touched (no device is reached: there is none here)
    for R in (0, 2, 64):
        _, i, o = _structs()
        i.n_events = i.n_nodes = 0
        o.n_groups = R
        o.node_factor = o.back = o.ratio = o.flux = o.totals = o.flux_rep = o.totals_rep = o.groups = None
        assert _call(lib, cp, i, None, o) == 0


def test_python_value_errors():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import trees
    from adiabatic_raytracer_amd.engine import Engine
    base = A.Halo(260.0, (0.0, 230.0, 0.0))
    g = [1e-12, 2e-12]
    # (before any work is done: nothing of the engine is touched)
    for kw in (dict(couplings=g, halos=[base]), dict(couplings=g, halo=base), dict(halos=[base], halo=base), {}):
        with pytest.raises(ValueError, match="grid: the coupling x halo grid needs couplings=, halos= and halo="):
            Engine.run_events(None, 0, grid=True, **kw)
        with pytest.raises(ValueError, match="grid: the coupling x halo grid needs couplings=, halos= and halo="):
            trees.main_runner_tree(A.Params(), 3, device_events=True, grid=True, **kw)
    for kw in (dict(device_trees=True), {}):
        with pytest.raises(ValueError, match="grid: .* needs device_events=True"):
            trees.main_runner_tree(A.Params(), 3, grid=True, couplings=g, halos=[base], halo=base, **kw)
    # the cap: 32 x 32 cells with 64 groups fit at 50 bins and do not at 4096
    Engine._grid_fit(32, 32, 64, 50, True)
    with pytest.raises(ValueError, match="grid: the tables of 32 x 32 cells and 64 groups"):
        Engine._grid_fit(32, 32, 64, 4096, True)
    assert 8 * 1024 * 65 * 8192 > Engine.REPLICATES_MAX_BYTES
    grid = _synthetic_grid([1.0, 2.0], 4, 3)
    plain = dict(grid)
    del plain["replicates"]
    for fn in (lambda: trees.limit_band(plain, 1.0), lambda: trees.grid_jackknife(plain, lambda t: 0.0)):
        with pytest.raises(ValueError, match="the grid has no replicates"):
            fn()
    for power in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="power must be finite and > 0"):
            trees.limit_band(grid, power)
    for average in ([], [2], [-1], [0.5, 0.5, 0.5], [0.0, 0.0], [1.0, -1.0]):
        with pytest.raises(ValueError, match="limit_band: "):
            trees.limit_band(grid, 1.0, average=average)


# ---------------------------------------------------------------------------------------------------
# the header's functions (tools/eventgrid) against trees.grid_tables on hand-built records
SIZES = (0, 1, 2, 63, 64, 65, 0, 300, 1)
EVENT_LO = 1003


def _forest(rng, Kg, Kh):
    """records of trees of SIZES records with integer factors, W in 0..3 and B, R in 1..3"""
    n, nn = len(SIZES), sum(SIZES)
    start = np.r_[0, np.cumsum(SIZES)].astype(np.int64)
    f = dict(start=start, tree=np.repeat(np.arange(n), SIZES).astype(np.int64), fin=(rng.random(nn) < 0.5).astype(np.int32),
             species=rng.integers(0, 2, nn).astype(np.int32), tau=np.zeros(nn), sln=rng.integers(1, 4, n).astype(np.float64),
             a=rng.integers(0, 5, n).astype(np.int64), W=rng.integers(0, 4, (Kg, nn)).astype(np.float64),
             B=rng.integers(1, 4, (Kg, n)).astype(np.float64), R=rng.integers(1, 4, (Kh, n)).astype(np.float64))
    f["fin"][[0, 1]] = 1
    phi = rng.uniform(-np.pi, np.pi, nn)
    phi[rng.random(nn) < 0.1] = np.nan  # rows the flux table does not count: the totals still do
    phi[3:6] = [-np.pi, np.pi, 0.0]
    f["phi"] = phi
    return f


def _rows_of(f, keep=None):
    """the 13-column rows of the final records (keep: a mask over the records) and their record indices"""
    idx = np.flatnonzero((f["fin"] != 0) if keep is None else ((f["fin"] != 0) & keep))
    rows = np.zeros((len(idx), 13))
    rows[:, 0] = f["tree"][idx] + 1.0 + EVENT_LO
    rows[:, 1] = f["species"][idx]
    rows[:, 3] = f["phi"][idx]
    rows[:, 7] = f["sln"][f["tree"][idx]]
    return rows, idx


def _public(cm, Kg, Kh, R):
    """the tool's cell-minor tables as trees.grid_raw lays them out"""
    from adiabatic_raytracer_amd import trees
    return trees.grid_raw(dict(cm, g=[1.0] * Kg, models=[(1.0, (0.0, 0.0, 0.0))] * Kh, base=None, R=R, n_events=len(SIZES)))


@pytest.mark.parametrize("Kg,Kh", [(1, 1), (3, 2), (5, 13)])
@pytest.mark.parametrize("R", [None, 2, 64])
@pytest.mark.parametrize("nbins", [0, 10])
def test_header_functions_against_grid_tables(Kg, Kh, R, nbins):
    import eventgrid
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(1000 * Kg + 10 * Kh + (R or 0) + nbins)
    f = _forest(rng, Kg, Kh)
    fb = trees.hist_bins(f["phi"], nbins) if nbins else np.full(len(f["phi"]), -1)
    args = [f[k] for k in ("start", "tree", "fin", "species")] + [fb] + [f[k] for k in ("tau", "sln", "a", "W", "B", "R")]
    got = _public(eventgrid.forest(*args, nbins, n_groups=R or 0, event_offset=EVENT_LO), Kg, Kh, R)
    rows, idx = _rows_of(f)
    ref = trees.grid_tables(rows, f["W"], f["B"], f["R"], idx, nbins, R, f["a"] + 1, EVENT_LO)
    keys = ("flux", "totals", "moment_totals") + (("flux_rep", "totals_rep", "groups") if R else ())
    assert set(k for k in trees.GRID_KEYS if got.get(k) is not None) == set(keys) == set(ref)
    for k in keys:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert ref["totals"][..., :2].sum() > 0 and ref["moment_totals"][..., 3:7].min() >= 0
    assert ref["flux"].shape == (Kg, Kh, 2 * nbins) and ref["moment_totals"].shape == (Kg, Kh, 8)
    assert np.all(ref["moment_totals"][..., 0] == len(SIZES))
    if nbins:  # some rows are binned, some are not
        assert 0 < ref["flux"].sum() < ref["totals"][..., :2].sum()
    if R:
        assert np.array_equal(ref["flux_rep"].sum(axis=2), ref["flux"])
        assert np.array_equal(ref["totals_rep"].sum(axis=2), ref["totals"][..., :2])
        assert ref["groups"][:, 0].sum() == len(SIZES) and ref["groups"][:, 1].sum() == ref["moment_totals"][0, 0, 1]
    # accumulated into: a second call doubles every table
    twice = eventgrid.forest(*args, nbins, n_groups=R or 0, event_offset=EVENT_LO)
    twice = _public(eventgrid.forest(*args, nbins, n_groups=R or 0, event_offset=EVENT_LO, into=twice), Kg, Kh, R)
    for k in keys:
        assert np.array_equal(twice[k], 2.0 * ref[k]), k
    # a final record of tree 3 inside the range of tree 7: counted, for the group of the tree it names, and skipped
    q = np.flatnonzero((f["fin"] != 0) & (np.arange(len(f["fin"])) >= f["start"][7] + 100))[0]
    bad = dict(f, tree=f["tree"].copy())
    bad["tree"][q] = 3
    args[1] = bad["tree"]
    got_bad = _public(eventgrid.forest(*args, nbins, n_groups=R or 0, event_offset=EVENT_LO), Kg, Kh, R)
    rows_b, idx_b = _rows_of(f, np.arange(len(f["fin"])) != q)
    want = trees.grid_tables(rows_b, f["W"], f["B"], f["R"], idx_b, nbins, R, f["a"] + 1, EVENT_LO)
    want["totals"][0, 0, 2] = want["moment_totals"][0, 0, 7] = 1.0
    if R:
        want["groups"][(EVENT_LO + 3) % R, 2] = 1.0
    for k in keys:
        assert np.array_equal(got_bad[k], want[k]), k
    assert trees.grid_result(got_bad, 1)["misplaced"] == 1 and trees.grid_result(got, 1)["misplaced"] == 0


def test_grid_tables_without_attempts_and_with_tau():
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(5)
    f = _forest(rng, 2, 3)
    rows, idx = _rows_of(f)
    out = trees.grid_tables(rows, f["W"], f["B"], f["R"], idx, 10, 4, None, EVENT_LO)
    assert "moment_totals" not in out
    photons = np.bincount(f["tree"][idx][f["species"][idx] == 1], minlength=len(SIZES))
    assert out["groups"][:, 1].sum() == photons.sum()
    # 29 columns with τ in column 14: the coupling's power carries exp(-τ) before the ratio
    wide = np.zeros((len(rows), 29))
    wide[:, :13] = rows
    wide[:, 14] = np.log(2.0)
    half = trees.grid_tables(wide, f["W"], f["B"], f["R"], idx, 10, None, None, EVENT_LO)
    assert np.allclose(half["totals"][..., :2], 0.5 * out["totals"][..., :2], rtol=8 * U, atol=0)
    with pytest.raises(ValueError, match="grid_tables"):
        trees.grid_tables(rows, f["W"], f["B"][:1], f["R"], idx, 10)


# ---------------------------------------------------------------------------------------------------
# the packing
def _raw(Kg, Kh, R, nbins, errors, rng):
    from adiabatic_raytracer_amd import trees
    f = _forest(rng, Kg, Kh)
    rows, idx = _rows_of(f)
    out = trees.grid_tables(rows, f["W"], f["B"], f["R"], idx, nbins, R, (f["a"] + 1) if errors else None, EVENT_LO)
    out.update(g=[float(k + 1) for k in range(Kg)], models=[(200.0 + k, (0.0, 1.0 * k, 0.0)) for k in range(Kh)],
               base=(260.0, (0.0, 230.0, 0.0), 347.0), R=R, n_events=len(SIZES))
    return out


@pytest.mark.parametrize("R,errors", [(None, False), (5, False), (None, True), (64, True)])
def test_pack_unpack_round_trip(R, errors):
    from adiabatic_raytracer_amd import trees
    raw = _raw(3, 4, R, 6, errors, np.random.default_rng(11))
    vec = trees.grid_pack(raw)
    sizes = sum(raw[k].size for k in trees.GRID_KEYS if raw.get(k) is not None)
    assert vec.ndim == 1 and vec.size == sizes + 1 and vec[-1] == len(SIZES)
    back = trees.grid_unpack(vec, raw)
    assert set(back) == set(raw)
    for k in raw:
        if isinstance(raw[k], np.ndarray):
            assert back[k].shape == raw[k].shape and np.array_equal(back[k], raw[k]), k
        else:
            assert back[k] == raw[k], k
    # what adds over the ranks: twice the vector is twice every table
    both = trees.grid_unpack(2.0 * vec, raw)
    assert np.array_equal(both["flux"], 2.0 * raw["flux"]) and both["n_events"] == 2 * len(SIZES)
    res = trees.grid_result(back, 977)
    assert res["flux"].shape == (3, 4, 2, 6) and res["sum_weight_sln_prob"].shape == (3, 4, 2)
    assert np.array_equal(res["sum_weight_sln_prob"], raw["totals"][..., :2] / 977.0) and res["misplaced"] == 0
    assert ("replicates" in res) == (R is not None) and ("n_eff" in res) == errors == ("sum_weight_sln_prob_sigma" in res)
    if errors:
        mt, tot = raw["moment_totals"], raw["totals"]
        assert res["n_eff"].shape == (3, 4) and res["sum_weight_sln_prob_sigma"].shape == (3, 4, 2)
        want = trees.moments_sigma(tot[1, 2, :2], mt[1, 2, 3:5], mt[1, 2, 5:7], 977, mt[1, 2, 2], mt[1, 2, 0])
        assert np.array_equal(res["sum_weight_sln_prob_sigma"][1, 2], want)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(res["n_eff"], tot[..., 1] ** 2 / mt[..., 4], equal_nan=True)


def test_rank_vector_appends_the_grid_last():
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(3)
    totals = rng.random(104)
    rows = np.zeros((6, 13))
    rows[:, 0] = [1, 1, 2, 3, 3, 3]
    rows[:, 7] = rows[:, 8] = 1.0
    rep = {"run": trees.rows_replicates(rows, 2, 4, None, None, 0, n_events=3)}
    coupling = {"flux": rng.random((2, 8)), "sky": None, "totals": rng.random((2, 6)), "g": [1.0, 2.0], "n_events": 3}
    halo = {"flux": rng.random((3, 8)), "sky": None, "totals": rng.random((3, 5)), "models": [], "n_events": 3}
    grid = _raw(2, 3, 2, 4, True, rng)
    for args, kw in (((totals,), {}), ((totals, coupling, halo), {}), ((totals, coupling, halo), {"replicates": rep}),
                     ((totals, None, halo), {"replicates": rep})):
        v0, e0 = trees.rank_vector(*args, **kw)
        v1, e1 = trees.rank_vector(*args, grid=grid, **kw)
        assert len(e1) == len(e0) + 1 and np.array_equal(e1[:-1], e0)  # every earlier part ends where it did
        assert np.array_equal(v1[:len(v0)], v0) and np.array_equal(v1[len(v0):], trees.grid_pack(grid))
        assert e1[-1] == len(v1)
        back = trees.grid_unpack(v1[e1[-2]:e1[-1]], grid)
        assert np.array_equal(back["flux_rep"], grid["flux_rep"])
        vn, en = trees.rank_vector(*args, grid=None, **kw)
        assert np.array_equal(vn, v0) and np.array_equal(en, e0)


# ---------------------------------------------------------------------------------------------------
# the read-off
def _synthetic_grid(c, R, per_group, g=None, nbins=2, noise=None, f_inx=None):
    """a grid_result whose totals per group are P_g[kg, kh] = c_h g_kg⁴ (times 1 + noise[g]) for the photons and half
    that for the axions, with `per_group` events and a_g = per_group in every group"""
    from adiabatic_raytracer_amd import trees
    g = np.array([1e-13, 3e-13, 1e-12, 3e-12, 1e-11] if g is None else g, np.float64)
    c = np.asarray(c, np.float64)
    Kg, Kh = len(g), len(c)
    scale = np.ones(R) if noise is None else 1.0 + np.asarray(noise, np.float64)
    P = np.outer(g ** 4, c)[:, :, None] * scale[None, None, :]  # (Kg, Kh, R)
    totals_rep = np.stack([0.5 * P, P], axis=-1)
    flux_rep = np.repeat(totals_rep / nbins, nbins, axis=-1).reshape(Kg, Kh, R, 2 * nbins)  # (axion bins, photon bins)
    groups = np.stack([np.full(R, float(per_group)), np.full(R, float(per_group)), np.zeros(R)], axis=1)
    totals = np.concatenate([totals_rep.sum(axis=2), np.zeros((Kg, Kh, 1))], axis=-1)
    raw = {"flux": flux_rep.sum(axis=2), "totals": totals, "flux_rep": flux_rep, "totals_rep": totals_rep, "groups": groups,
           "g": list(g), "models": [(200.0 + k, (0.0, 0.0, 0.0)) for k in range(Kh)], "base": None, "R": R,
           "n_events": R * per_group}
    return trees.grid_result(raw, R * per_group if f_inx is None else f_inx)


def test_limit_band_on_power_laws():
    from adiabatic_raytracer_amd import trees
    c = np.array([3.0e30, 1.0e30, 8.0e30, 1.0e22])  # the last column stays below `power` everywhere
    R, per = 8, 5
    noise = np.linspace(-0.2, 0.2, R)
    grid = _synthetic_grid(c, R, per, noise=noise)
    f = R * per
    power = 1.0e-20 / f  # (the tables are divided by f_inx)
    out = trees.limit_band(grid, power)
    scale = (1.0 + noise).sum()
    want = (1.0e-20 / (c * scale)) ** 0.25
    assert out["g"].shape == out["sigma"].shape == (4,) and out["cov"].shape == (4, 4) and out["groups_used"] == R
    assert np.allclose(out["g"][:3], want[:3], rtol=1e-13, atol=0) and np.isnan(out["g"][3]) and np.isnan(out["sigma"][3])
    assert want[3] > grid["g"].max()
    cov = out["cov"][:3, :3]
    assert np.allclose(cov, cov.T, rtol=1e-14, atol=0) and np.allclose(np.diag(cov), out["sigma"][:3] ** 2, rtol=1e-12, atol=0)
    assert np.all(out["sigma"][:3] > 0)
    # one common factor per group moves every model's limit alike: the limits are fully correlated, the ratio is sharp
    corr = cov / np.outer(out["sigma"][:3], out["sigma"][:3])
    assert np.allclose(corr, 1.0, rtol=0, atol=1e-9)
    assert (out["lo_model"], out["hi_model"]) == (2, 1) and out["lo"] == out["g"][2] and out["hi"] == out["g"][1]
    assert np.isclose(out["lo_sigma"], out["sigma"][2], rtol=1e-12) and np.isclose(out["hi_sigma"], out["sigma"][1], rtol=1e-12)
    assert np.isclose(out["ratio"], 8.0 ** 0.25, rtol=1e-13) and out["ratio_sigma"] <= 1e-12 * out["ratio"]
    assert out["ratio_sigma"] < 1e-9 * np.hypot(out["lo_sigma"] / out["lo"], out["hi_sigma"] / out["hi"])
    # the leave-one-out limits in closed form: θ_g = (power (f - a_g) / (c (scale - scale_g)))^(1/4)
    th = ((1.0e-20 / f) * (f - per) / (c[0] * (scale - (1.0 + noise)))) ** 0.25
    sig = np.sqrt((R - 1.0) / R * ((th - th.mean()) ** 2).sum())
    assert np.isclose(out["sigma"][0], sig, rtol=1e-9)
    # the axions carry half the power: their limit is 2^(1/4) higher
    ax = trees.limit_band(grid, power, species=0)
    assert np.allclose(ax["g"][:3], want[:3] * 2.0 ** 0.25, rtol=1e-13, atol=0)
    # no column reaches it: NaN everywhere, no model
    none = trees.limit_band(grid, 1.0e40)
    assert np.isnan(none["g"]).all() and np.isnan(none["lo"]) and np.isnan(none["ratio"]) and none["lo_model"] == -1


def test_limit_band_average():
    from adiabatic_raytracer_amd import trees
    R, per = 6, 4
    noise = np.array([0.1, -0.1, 0.05, -0.05, 0.2, -0.2])
    same = _synthetic_grid([2.0e30, 2.0e30, 2.0e30], R, per, noise=noise)
    power = 1.0e-20 / (R * per)
    for average in ([0, 1, 2], [0, 2], [0.2, 0.3, 0.5], np.array([1.0, 0.0, 3.0])):
        out = trees.limit_band(same, power, average=average)
        assert np.isclose(out["g_avg"], out["g"][0], rtol=1e-13) and np.isclose(out["sigma_avg"], out["sigma"][0], rtol=1e-9)
        assert np.isclose(out["weights"].sum(), 1.0)
    # the tables are linear in the model: the average of c_h g⁴ columns is the column of the averaged c
    mixed = _synthetic_grid([1.0e30, 4.0e30, 7.0e30], R, per, noise=noise)
    out = trees.limit_band(mixed, power, average=[0.5, 0.0, 0.5])
    assert np.isclose(out["g_avg"], out["g"][1], rtol=1e-13)
    one = trees.limit_band(mixed, power, average=[2])
    assert one["g_avg"] == one["g"][2] and one["sigma_avg"] == one["sigma"][2]
    assert "g_avg" not in trees.limit_band(mixed, power)


@pytest.mark.parametrize("R", [2, 5, 64])
def test_grid_jackknife_linear_is_batch_means(R):
    """constant a_e and equal groups: σ² of a linear φ is R / ((R - 1) f²) Σ_g (T_g - mean T)², the identity of
    tests/test_replicates.py, cell by cell"""
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(R)
    Kg, Kh, nbins, f_inx = 2, 3, 3, 977
    f = _forest(rng, Kg, Kh)
    rows, idx = _rows_of(f)
    rows[:, 0] -= EVENT_LO
    n = R * (-(-len(SIZES) // R))  # equal groups: pad the events to a multiple of R
    pad = lambda a: np.concatenate([a, np.ones((a.shape[0], n - a.shape[1]))], axis=1)  # noqa: E731
    raw = trees.grid_tables(rows, f["W"], pad(f["B"]), pad(f["R"]), idx, nbins, R, None, 0)
    raw["groups"][:, 1] = raw["groups"][:, 0]  # a_e constant
    raw.update(g=[1.0, 2.0], models=[(1.0, (0.0, 0.0, 0.0))] * Kh, base=None, R=R, n_events=n)
    grid = trees.grid_result(raw, f_inx)
    assert np.array_equal(grid["replicates"]["n_g"], np.full(R, n / R))
    out = trees.grid_jackknife(grid, lambda t: np.concatenate([t["flux"].reshape(-1), t["sum_weight_sln_prob"].reshape(-1)]),
                               cov=True)
    T = np.concatenate([np.moveaxis(raw["flux_rep"], 2, 0).reshape(R, -1), np.moveaxis(raw["totals_rep"], 2, 0).reshape(R, -1)], axis=1)
    assert out["groups_used"] == R and out["value"].shape == out["sigma"].shape == (Kg * Kh * (2 * nbins + 2),)
    assert np.array_equal(out["value"], T.sum(axis=0) / f_inx) and out["cov"].shape == (T.shape[1],) * 2
    fr = Fraction(f_inx)
    for j in range(T.shape[1]):
        S = sum(Fraction(int(v)) for v in T[:, j])
        want = Fraction(R, R - 1) / (fr * fr) * sum((Fraction(int(v)) - S / R) ** 2 for v in T[:, j])
        _, sd, sdd, tmax = _exact_sigma2(T[:, j:j + 1], [fr / R] * R, fr)
        tol = _tolerance(R, sd, sdd, tmax)[0] + 3 * U * float(want)
        assert abs(out["sigma"][j] ** 2 - float(want)) <= tol, (j, out["sigma"][j] ** 2, float(want), tol)
    assert out["sigma"].max() > 0
    # the same NaN rules as jackknife: a lone group that holds events gives no error
    lone = dict(raw, groups=raw["groups"].copy())
    lone["groups"][1:, 0] = 0.0
    nan = trees.grid_jackknife(trees.grid_result(lone, f_inx), lambda t: t["sum_weight_sln_prob"])
    assert nan["groups_used"] == 1 and nan["sigma"].shape == (Kg, Kh, 2) and np.isnan(nan["sigma"]).all()
