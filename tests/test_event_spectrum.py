"""The event power spectrum without a GPU ("Event power spectrum"): the bin rule, the per-tree X and
the merge of the top lists of the host build of art_event_spectrum.h against numpy, trees.rows_spectrum against a
per-event loop, trees.tail_index on Pareto draws, the packing into the run's one reduced vector, and the C
boundary's argument checks.

Tolerances: none but the tail index's. Every table is compared with np.array_equal: the synthetic powers are
integers (their sums and squares are exact), and where they are not the comparison is of bit patterns formed by the
same adds in the same order. The tail index of 255 order statistics scatters by σ = α̂ / √k around α; the issue's
bound is 4 σ."""
import ctypes as C
import inspect
import itertools

import numpy as np
import pytest

INVALID = -1


# ---------------------------------------------------------------------------------------------------
# the bin rule
def _edge_cases(m):
    """EVERY bin edge of the table (the lower edges of bins 1 .. NB - 1), and each one ulp below and above"""
    from adiabatic_raytracer_amd import trees
    NB = 2047 << m
    edge = trees.spectrum_edges(1, NB - 1, m)
    assert len(edge) == NB - 1 and np.array_equal(edge.view(np.int64), np.arange(1, NB, dtype=np.int64) << (52 - m))
    return np.r_[edge, np.nextafter(edge, 0.0), np.nextafter(edge, np.inf)]


def test_bin_rule_host_build_equals_numpy():
    from adiabatic_raytracer_amd import trees
    from tools import eventspectrum
    rng = np.random.default_rng(1769)
    # random positive doubles over the whole range of patterns, and over the physical range
    x = np.r_[rng.integers(1, 0x7FEFFFFFFFFFFFFF, 50000, dtype=np.int64).view(np.float64),
              np.exp(rng.uniform(-700, 700, 50000))]
    tiny, big = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    special = np.array([5e-324, tiny, 1.0, np.nextafter(1.0, 0.0), np.nextafter(2.0, 0.0), big])
    none = np.array([0.0, -0.0, -1.0, -5e-324, -big, np.nan, np.inf, -np.inf])
    for m in range(5):
        edges = _edge_cases(m)
        NB = 2047 << m
        # an edge opens its bin, one ulp below it closes the bin before, one ulp above stays in its bin
        assert np.array_equal(eventspectrum.bins(edges, m), np.r_[np.arange(1, NB), np.arange(0, NB - 1), np.arange(1, NB)])
        v = np.r_[x, special, edges]
        assert np.all(np.isfinite(v) & (v > 0))
        want = v.view(np.int64) >> (52 - m)
        got = eventspectrum.bins(v, m)
        assert np.array_equal(got, want) and np.array_equal(trees.spectrum_bin(v, m), want), m
        assert want.min() >= 0 and want.max() < (2047 << m)
        # monotone, with edges whose low 52 - m mantissa bits are zero
        order = np.argsort(v)
        assert np.all(np.diff(want[order]) >= 0)
        assert np.array_equal(eventspectrum.bins(special, m), [0, 1 << m, 1023 << m, (1023 << m) - 1, (1024 << m) - 1,
                                                               (2047 << m) - 1])
        assert np.all(eventspectrum.bins(none, m) == -1) and np.all(trees.spectrum_bin(none, m) == -1)
        e = trees.spectrum_edges(0, 2047 << m, m)
        assert e[0] == 0.0 and np.isinf(e[-1]) and np.all(np.diff(e) > 0)
        assert np.array_equal(eventspectrum.bins(e[1:-1], m), np.arange(1, 2047 << m))
        assert np.all(e.view(np.int64) & ((1 << (52 - m)) - 1) == 0)
        assert trees.spectrum_bins(m) == 2047 << m


# ---------------------------------------------------------------------------------------------------
# rows_spectrum against a per-event loop
def _synthetic_rows(rng, n_events, lo):
    """rows (13 columns) of events lo .. lo + n_events: some without a row, some of one species only, duplicate powers"""
    rows = []
    for e in range(n_events):
        kind = e % 7
        n_ax, n_ph = ((0, 0), (1, 0), (0, 2), (3, 1), (2, 5), (1, 1), (0, 1))[kind]
        for sp, c in ((0, n_ax), (1, n_ph)):
            for _ in range(c):
                row = np.zeros(13)
                row[0], row[1] = lo + e + 1, sp
                row[7], row[8] = float(rng.integers(1, 4)), float(rng.integers(1, 6))  # (few values: many ties)
                rows.append(row)
    rows = np.array(rows)
    return rows[rng.permutation(len(rows))]  # (rows of an event need not be neighbours)


def _loop_spectrum(rows, m, T, lo, n):
    NB = 2047 << m
    out = {"count": np.zeros((1, 2, NB)), "sum": np.zeros((1, 2, NB)), "sum_sq": np.zeros((1, 2, NB)),
           "totals": np.zeros((1, 2, 8)), "top_power": np.zeros((1, 2, T)), "top_event": np.full((1, 2, T), -1, np.int64)}
    for s in range(2):
        pairs = []
        for e in range(lo, lo + n):
            X = 0.0
            for r in rows:
                if int(round(r[0])) - 1 == e and (r[1] != 0) == bool(s):
                    X += r[8] * r[7]
            t = out["totals"][0, s]
            t[0] += 1
            if X > 0 and np.isfinite(X):
                b = int(np.float64(X).view(np.int64)) >> (52 - m)
                out["count"][0, s, b] += 1
                out["sum"][0, s, b] += X
                out["sum_sq"][0, s, b] += X * X
                t[1] += 1
                t[4] += X
                t[5] += X * X
                pairs.append((-X, e))
            elif X == 0:
                t[2] += 1
            else:
                t[3] += 1
        for q, (negx, e) in enumerate(sorted(pairs)[:T]):
            out["top_power"][0, s, q], out["top_event"][0, s, q] = -negx, e
    return out


@pytest.mark.parametrize("m,T", [(0, 1), (3, 5), (4, 256)])
def test_rows_spectrum_against_a_loop(m, T):
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(7)
    lo, n = 1000, 83
    rows = _synthetic_rows(rng, n - 4, lo)  # (the last four events have no row at all)
    got = trees.rows_spectrum(rows, m, T, event_lo=lo, n_events=n)
    want = _loop_spectrum(rows, m, T, lo, n)
    assert got["kind"] == "run" and got["sub_bits"] == m and got["top"] == T
    for k, v in want.items():
        assert got[k].shape == v.shape and got[k].dtype == v.dtype and np.array_equal(got[k], v), k
    tot = got["totals"][0]
    assert np.all(tot[:, 0] == n) and np.all(tot[:, 2] > 4) and np.all(tot[:, 3] == 0) and np.all(tot[:, 6:] == 0)
    tp = got["top_power"][0, 1]
    assert T == 1 or np.any(tp[:-1][tp[:-1] > 0] == tp[1:][tp[:-1] > 0])  # (ties, broken by id)
    # n_events=None: up to the last event that has a row
    short = trees.rows_spectrum(rows, m, T, event_lo=lo)
    assert short["totals"][0, 0, 0] == int(rows[:, 0].max()) - lo
    with pytest.raises(ValueError, match="outside"):
        trees.rows_spectrum(rows, m, T, event_lo=lo + 2)
    for bad in (dict(sub_bits=5, top=4), dict(sub_bits=-1, top=4), dict(sub_bits=3, top=257), dict(sub_bits=3, top=-1)):
        with pytest.raises(ValueError, match="spectrum"):
            trees.rows_spectrum(rows, bad["sub_bits"], bad["top"])


def test_spectrum_result_of_rows():
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(11)
    rows = _synthetic_rows(rng, 60, 0)
    raw = trees.rows_spectrum(rows, 3, 16, n_events=64)
    res = trees.spectrum_result(raw, 200)
    S, Q = raw["totals"][0, :, 4], raw["totals"][0, :, 5]
    assert np.array_equal(res["n_eff"], S * S / Q) and res["misplaced"] == 0 and res["kind"] == "run"
    lo, hi = res["bins"]
    assert res["counts"].shape == (2, hi - lo + 1) and len(res["edges"]) == hi - lo + 2
    assert res["counts"].sum() == raw["totals"][0, :, 1].sum() and np.array_equal(res["power"], raw["sum"][0, :, lo:hi + 1] / 200)
    assert res["counts"][:, 0].sum() > 0 and res["counts"][:, -1].sum() > 0
    assert np.array_equal(res["top_power"], raw["top_power"][0] / 200) and np.array_equal(res["top_power_raw"], raw["top_power"][0])
    assert np.array_equal(res["top_share"], np.cumsum(raw["top_power"][0], axis=-1) / S[:, None])
    assert np.array_equal(res["max_share"], raw["top_power"][0, :, 0] / S)
    assert np.array_equal(res["events"], [64, 64]) and np.array_equal(res["zeros"] + res["positive"] + res["bad"], [64, 64])
    assert res["alpha"].shape == (2,) and res["hill"].shape == (2, 14)
    empty = trees.spectrum_result(trees.rows_spectrum(np.zeros((0, 13)), 3, 4), 0)
    assert empty["bins"] is None and np.all(np.isnan(empty["n_eff"])) and np.all(np.isnan(empty["alpha"]))


# ---------------------------------------------------------------------------------------------------
# the host build's per-tree X and merge
def test_host_group_by_equals_numpy():
    from tools import eventspectrum
    rng = np.random.default_rng(3)
    sizes = np.array([(0, 1, 2, 63, 64, 65, 0, 300, 1)[e % 9] for e in range(90)])
    start = np.r_[0, np.cumsum(sizes)]
    n = int(start[-1])
    species = rng.integers(-1, 2, n)
    power = rng.uniform(0.0, 1.0, n) * 10.0 ** rng.integers(-20, 20, n)  # (sums that round: the ORDER of the adds shows)
    X, differ = eventspectrum.forest(start, species, power)
    assert differ == 0  # the doubles of moment_group(..., MOMENT_KEY_SPECIES)
    tree = np.repeat(np.arange(90), sizes)
    for s in range(2):
        w = species == s
        want = np.bincount(tree[w], weights=power[w], minlength=90)  # (adds in record order, as the rows are)
        assert np.array_equal(X[s].view(np.int64), want.view(np.int64)), s
    assert np.count_nonzero(X == 0) >= 20  # (empty trees, trees without a final record of a species)


def _sorted_list(rng, n, T, id_lo=0):
    from adiabatic_raytracer_amd.trees import _spectrum_top
    X = rng.integers(1, 6, n).astype(np.float64)  # (few values: ties within and across the lists)
    ids = id_lo + rng.permutation(4 * n)[:n]
    return _spectrum_top(X, ids, T)


@pytest.mark.parametrize("T", [1, 5, 64, 256])
def test_merge_of_lists_in_every_order(T):
    from adiabatic_raytracer_amd import trees
    from tools import eventspectrum
    rng = np.random.default_rng(T)
    for n_lists in (2, 3, 8):
        lists = [_sorted_list(rng, int(rng.integers(0, 32)), T, id_lo=1000 * q) for q in range(n_lists)]
        allX = np.concatenate([p[i >= 0] for p, i in lists])
        allI = np.concatenate([i[i >= 0] for p, i in lists])
        want = trees._spectrum_top(allX, allI, T)
        assert T > len(allX) or T < 256  # (T = 256 is larger than all the entries)
        raws = [{"kind": "run", "sub_bits": 0, "top": T, "count": np.full((1, 2, 2047), float(q)), "sum": np.zeros((1, 2, 2047)),
                 "sum_sq": np.zeros((1, 2, 2047)), "totals": np.ones((1, 2, 8)), "top_power": np.stack([p, p])[None],
                 "top_event": np.stack([i, i])[None]} for q, (p, i) in enumerate(lists)]
        orders = list(itertools.permutations(range(n_lists))) if n_lists <= 3 else [rng.permutation(n_lists) for _ in range(6)]
        for order in orders:
            # the host build, folded pairwise in this order
            p, i = lists[order[0]]
            p, i = p[i >= 0], i[i >= 0]
            for step, q in enumerate(order[1:]):
                bp, bi = lists[q]
                p, i = eventspectrum.merge(p, i, bp[bi >= 0], bi[bi >= 0], T)
                if step < n_lists - 2:
                    p, i = p[i >= 0], i[i >= 0]
            assert np.array_equal(p, want[0]) and np.array_equal(i, want[1]), (n_lists, order)
            # trees.spectrum_merge: at once, and folded (associative)
            at_once = trees.spectrum_merge([raws[q] for q in order])
            folded = raws[order[0]]
            for q in order[1:]:
                folded = trees.spectrum_merge([folded, raws[q]])
            for got in (at_once, folded):
                for s in range(2):
                    assert np.array_equal(got["top_power"][0, s], want[0]) and np.array_equal(got["top_event"][0, s], want[1])
                assert np.all(got["count"] == sum(range(n_lists))) and np.all(got["totals"] == n_lists)
    with pytest.raises(ValueError, match="another kind"):
        trees.spectrum_merge([raws[0], dict(raws[1], top=T + 1)])


def test_merge_of_equal_entries_keeps_the_multiset():
    from tools import eventspectrum
    p, i = eventspectrum.merge([5.0, 3.0, 3.0], [7, 1, 2], [5.0, 3.0], [7, 1], 4)
    assert np.array_equal(p, [5.0, 5.0, 3.0, 3.0]) and np.array_equal(i, [7, 7, 1, 1])
    p, i = eventspectrum.merge([], [], [], [], 3)
    assert np.array_equal(p, [0.0, 0.0, 0.0]) and np.array_equal(i, [-1, -1, -1])


# ---------------------------------------------------------------------------------------------------
# the tail index
def _pareto_draws():
    """20 000 draws each for α = 1.5 and α = 3, one after the other from one generator"""
    rng = np.random.default_rng(1769)
    return {alpha: (1.0 - rng.random(20000)) ** (-1.0 / alpha) * 3e30 for alpha in (1.5, 3.0)}


@pytest.mark.parametrize("alpha,alpha_hat,sigma", [(1.5, 1.581, 0.099), (3.0, 2.760, 0.173)])
def test_tail_index_of_pareto_draws(alpha, alpha_hat, sigma):
    from adiabatic_raytracer_amd import trees
    x = _pareto_draws()[alpha]
    raw = trees.rows_spectrum(np.c_[np.arange(1, 20001), np.ones(20000), np.zeros((20000, 5)), np.ones(20000), x,
                                    np.zeros((20000, 4))], 3, 256)
    top = raw["top_power"][0, 1]
    assert np.array_equal(top, np.sort(x)[::-1][:256])
    t = trees.tail_index(top)
    print(f"alpha {alpha}: alpha_hat {t['alpha']:.4f} sigma {t['alpha_sigma']:.4f} k {t['k']}")
    assert t["k"] == 255 and len(t["hill"]) == 254 and t["hill"][-1] == t["alpha"]
    assert abs(t["alpha"] - alpha_hat) < 5e-4 and abs(t["alpha_sigma"] - sigma) < 5e-4  # (the figures checked by hand)
    assert abs(t["alpha"] - alpha) < 4 * t["alpha_sigma"]
    lg = np.log(top)
    assert t["alpha"] == pytest.approx(255 / np.sum(lg[:255] - lg[255]), rel=1e-12)
    t10 = trees.tail_index(top, k=10)
    assert t10["alpha"] == pytest.approx(10 / np.sum(lg[:10] - lg[10]), rel=1e-12) and t10["alpha_sigma"] == t10["alpha"] / np.sqrt(10)
    res = trees.spectrum_result(raw, 1)
    assert res["alpha"][1] == t["alpha"] and res["alpha_sigma"][1] == t["alpha_sigma"] and np.isnan(res["alpha"][0])


def test_tail_index_nan_cases():
    from adiabatic_raytracer_amd import trees
    for x in ([], [3.0], [3.0, 2.0], [3.0, 2.0, 0.0, 0.0], [0.0] * 8):
        t = trees.tail_index(x)
        assert np.isnan(t["alpha"]) and np.isnan(t["alpha_sigma"]) and len(t["hill"]) == 0, x
    t = trees.tail_index([4.0] * 9 + [0.0, 0.0])  # (all equal: the logs sum to 0)
    assert np.isnan(t["alpha"]) and np.isnan(t["alpha_sigma"]) and np.all(np.isnan(t["hill"])) and len(t["hill"]) == 7
    with pytest.raises(ValueError, match="k must be"):
        trees.tail_index([3.0, 2.0, 1.0], k=3)


# ---------------------------------------------------------------------------------------------------
# the run's one reduced vector
def test_rank_vector_round_trip_and_default_off():
    from adiabatic_raytracer_amd import trees
    rng = np.random.default_rng(5)
    nbins = 6
    flux = rng.uniform(size=2 * nbins)
    totals = trees.pack_totals(flux, 123, 4.0, 5.0, 77)
    plain, ends = trees.rank_vector(totals)
    assert plain is totals and list(ends) == [len(totals)]
    again, ends2 = trees.rank_vector(totals, spectrum=None)
    assert again is totals and list(ends2) == list(ends)
    world = 3
    raws = [trees.rows_spectrum(_synthetic_rows(rng, 20, 20 * r), 2, 8, event_lo=20 * r, n_events=20) for r in range(world)]
    vecs = []
    for r in range(world):
        v, e = trees.rank_vector(totals, spectrum={"run": raws[r]}, rank=r, world=world)
        NB, T = 2047 << 2, 8
        assert len(e) == 2 and e[0] == len(totals) and e[1] - e[0] == 3 * 2 * NB + 2 * 8 + 2 * world * 2 * T
        assert np.array_equal(v[:e[0]], totals)  # (the earlier part keeps its place and its content)
        vecs.append(v)
    red = np.sum(vecs, axis=0)
    tt = trees.unpack_totals(red[:e[0]], nbins)
    assert tt["f_inx"] == world * 123 and np.allclose(tt["flux"], world * flux)
    got = trees.spectrum_unpack(red[e[0]:e[1]], raws[0], world)
    want = trees.spectrum_merge(raws)
    for k in trees.SPECTRUM_TABLES + ("top_power", "top_event"):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    assert np.array_equal(want["totals"][0, :, 0], [60, 60])
    # a spectrum after a grid-less, replicate-less vector with scans absent: _finish_run's slices
    info = {}
    rows = np.zeros((0, 13))
    trees._finish_run(rows, trees.pack_totals(flux, 123, 4.0, 5.0, 0), nbins=nbins, sky_kw=None, errors=False, world=1,
                      run_info=info, events=(0, 20), n_events=20, g0=1e-12, path=None, spectrum={"run": raws[0]}, rank=0)
    assert np.array_equal(info["spectrum"]["raw"]["count"], raws[0]["count"])
    assert np.array_equal(info["spectrum"]["top_event"], raws[0]["top_event"][0]) and info["spectrum"]["f_inx"] == 123
    base = {}
    trees._finish_run(rows, trees.pack_totals(flux, 123, 4.0, 5.0, 0), nbins=nbins, sky_kw=None, errors=False, world=1,
                      run_info=base, events=(0, 20), n_events=20, g0=1e-12, path=None)
    assert "spectrum" not in base and set(info) - set(base) == {"spectrum"}
    with pytest.raises(ValueError, match="2\\^53"):
        trees.spectrum_pack(dict(raws[0], top_event=np.full((1, 2, 8), 2 ** 53)))


def test_keywords():
    from adiabatic_raytracer_amd import trees
    assert trees.spectrum_keywords({}) == (3, 64) and trees.spectrum_keywords(dict(sub_bits=0, top=0)) == (0, 0)
    for bad in (dict(bins=3), dict(sub_bits=5), dict(top=257), dict(sub_bits=1.5), dict(top=-1), True, 3, "top", [3, 64]):
        with pytest.raises(ValueError, match="spectrum"):
            trees.spectrum_keywords(bad)
    with pytest.raises(ValueError, match="spectrum"):
        trees.main_runner_tree(None, 10, spectrum=dict(nope=1))  # (before any work is done)


# ---------------------------------------------------------------------------------------------------
# the C boundary
def _structs():
    from adiabatic_raytracer_amd._lib import EventRowsIn, EventSpectrumOut
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    so = EventSpectrumOut(0, 1, 3, 64, None, None, a, a, a, a, a, a)
    return d, ein, so


def _call(lib, cp, ein, start, so):
    ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731
    return lib.art_event_spectrum_device(ref(cp), ref(ein), start, ref(so), None)


def test_symbol_struct_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib, trees
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    assert "art_event_spectrum_device" in _lib.SIGNATURES and hasattr(lib, "art_event_spectrum_device")
    assert C.sizeof(_lib.EventSpectrumOut) == 4 * 4 + 8 * 8 and lib.art_abi_version() == 1
    assert _lib.SPECTRUM_TOTALS == ("events", "positive", "zeros", "bad", "sum", "sum_sq", "misplaced", "reserved")
    for fn in (Engine.run_events, trees.main_runner_tree, trees.rank_vector, trees._finish_run):
        par = inspect.signature(fn).parameters["spectrum"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    es = inspect.signature(Engine.event_spectrum).parameters
    assert list(es)[:5] == ["self", "sample", "weight5", "back", "forward"]
    for k, v in dict(sub_bits=3, top=64, kind="run", node_factor=None, event_factor=None, event_offset=0,
                     cyclotron_rerun=None, spec=None).items():
        assert es[k].kind is inspect.Parameter.KEYWORD_ONLY and es[k].default == v, k
    assert hasattr(Engine, "_zero_spectrum") and Engine.SPECTRUM_MAX_BYTES == 64 << 20
    with pytest.raises(ValueError, match="spectrum"):
        Engine._spectrum_fit("the scan", 64, 4)
    Engine._spectrum_fit("the scan", 32, 4)


def test_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    lib = A.load_library()
    cp = A.Params().to_c()
    d, ein, so = _structs()
    start = C.c_void_p(C.addressof(d))
    err = lib.art_last_error
    assert _call(lib, None, ein, start, so) == INVALID and b"params" in err()
    assert _call(lib, cp, None, start, so) == INVALID and b"NULL in or out" in err()
    assert _call(lib, cp, ein, start, None) == INVALID and b"NULL in or out" in err()

    def bad(msg, start=start, **kw):
        _, i, o = _structs()
        for k, v in kw.items():
            setattr(i if hasattr(i, k) else o, k, v)
        assert _call(lib, cp, i, start, o) == INVALID, msg
        assert msg.encode() in err(), (msg, err())

    a = C.addressof(d)
    for kind in (-1, 3):
        bad("kind must be", kind=kind)
    for K in (0, -1, 33):
        bad("n_sets must be in [1, 32]", kind=2, n_sets=K, event_factor=a)
    bad("n_sets must be 1 with kind 0", n_sets=2)
    for m in (-1, 5):
        bad("sub_bits must be in [0, 4]", sub_bits=m)
    for T in (-1, 257):
        bad("top must be in [0, 256]", top=T)
    bad("node_factor is NULL", kind=1, n_sets=3, event_factor=a)
    bad("event_factor is NULL", kind=1, n_sets=3, node_factor=a)
    bad("event_factor is NULL", kind=2, n_sets=3)
    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    bad("node_start is NULL", start=None)
    for table in ("count", "sum", "sum_sq", "totals"):
        bad("count, sum, sum_sq or totals is NULL", **{table: None})
    bad("top_power or top_event is NULL", top_power=None)
    bad("top_power or top_event is NULL", top_event=None)
    bad("NULL input buffer", weight5=None)
    # top == 0 needs no list; no events: ART_OK after the checks, nothing touched (no device is reached)
    for kind, K, nf, ef in ((0, 1, None, None), (1, 32, a, a), (2, 5, None, a)):
        _, i, o = _structs()
        i.n_events, i.n_nodes = 0, 0
        o.kind, o.n_sets, o.node_factor, o.event_factor, o.top, o.top_power, o.top_event = kind, K, nf, ef, 0, None, None
        assert _call(lib, cp, i, None, o) == 0
    assert all(v == 0.0 for v in d)
