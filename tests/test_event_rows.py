"""Event rows without a GPU: the argument checks of art_event_rows_device and
art_event_gather_photons_device, which come before any device is touched; the Python surface
(Engine.event_rows, Engine.run_events, main_runner_tree(device_events=...)); and the row math of
art_event_rows.h in a host build (tools/eventrows.py) against the numpy expressions of
trees.main_runner_tree on synthetic final nodes.

Row math, measured on the host build (glibc's acos and atan2 against numpy's): copy, product, norm
and Δω columns bit-equal (NaN equal to NaN); angle columns 2-5 at most 1 ulp from numpy's (bound: 4);
cos θf bit-equal to kz / |k|."""
import ctypes as C
import inspect

import numpy as np
import pytest

INVALID = -1  # ART_E_INVALID


def _structs():
    from adiabatic_raytracer_amd._lib import EventRowsIn, EventRowsOut
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    eout = EventRowsOut(13, 50, a, 4, a, None, None, None, a)
    return d, ein, eout


def _call(lib, cp, ein, eout):
    return lib.art_event_rows_device(C.byref(cp) if cp is not None else None, C.byref(ein) if ein is not None else None,
                                     C.byref(eout) if eout is not None else None, None)


def test_event_rows_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import SkySpec
    lib = A.load_library()
    cp = A.Params().to_c()
    _, ein, eout = _structs()
    assert _call(lib, None, ein, eout) == INVALID and b"params" in lib.art_last_error()
    assert _call(lib, cp, None, eout) == INVALID and b"NULL in or out" in lib.art_last_error()
    assert _call(lib, cp, ein, None) == INVALID and b"NULL in or out" in lib.art_last_error()

    def bad(msg, **kw):
        _, i, o = _structs()
        for k, v in kw.items():
            setattr(i if hasattr(i, k) else o, k, v)
        assert _call(lib, cp, i, o) == INVALID, msg
        assert msg.encode() in lib.art_last_error(), (msg, lib.art_last_error())

    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    for ncols in (0, 12, 14, 28, 30):
        bad("ncols must be 13 or 29", ncols=ncols)
    bad("row_capacity", row_capacity=3)
    bad("nbins must be", nbins=-1)
    bad("nbins must be", nbins=4097)
    good = dict(n_theta=4, n_phi=8, n_dw=3, theta_axis=1, mode=0, dw_lo=-1e-6, dw_hi=1e-6)
    sky_cases = {
        "bin counts": dict(good, n_theta=0),
        "finite lo < hi": dict(good, dw_hi=-1e-6),
        "theta_axis": dict(good, theta_axis=2),
        "mode must be": dict(good, mode=7),
        "2^26": dict(good, n_theta=8192, n_phi=8192),
        "LDS budget": dict(good, n_theta=64, n_phi=128, n_dw=16, mode=1),
        # the sky table alone fits the budget, the flux table beside it does not
        "sky and flux tables": dict(good, n_theta=16, n_phi=32, n_dw=8, mode=1),
    }
    for msg, kw in sky_cases.items():
        spec = SkySpec(**kw)
        bad(msg, sky=C.pointer(spec))
    # a row buffer is not needed when neither rows nor bins are asked for; bins alone need the capacity
    d, i, o = _structs()
    o.rows, o.row_capacity, o.bin_out = None, 0, C.addressof(d)
    assert _call(lib, cp, i, o) == INVALID and b"row_capacity" in lib.art_last_error()
    # no events: ART_OK after the checks, nothing touched (NULL buffers)
    _, i, o = _structs()
    i.n_events = i.n_nodes = 0
    o.rows = o.flux = o.totals = None
    assert _call(lib, cp, i, o) == 0
    spec = SkySpec(**dict(good, n_dw=1, dw_lo=float("nan"), dw_hi=float("nan")))  # n_dw = 1: the range is not looked at
    o.sky = C.pointer(spec)
    assert _call(lib, cp, i, o) == 0


def test_gather_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    lib = A.load_library()
    cp = A.Params().to_c()
    d = (C.c_double * 64)()
    a = C.c_void_p(C.addressof(d))
    m = C.c_int64(7)

    def call(p=cp, n_events=4, n_nodes=4, capacity=4, n_out=m):
        return lib.art_event_gather_photons_device(C.byref(p) if p is not None else None, n_events, a, n_nodes, a, capacity,
                                                   a, a, a, a, a, a, a, C.byref(n_out) if n_out is not None else None, None)

    assert call(p=None) == INVALID and b"params" in lib.art_last_error()
    assert call(n_out=None) == INVALID and b"n_out" in lib.art_last_error()
    assert call(n_events=-1) == INVALID and b"n_events" in lib.art_last_error()
    assert call(n_nodes=-1) == INVALID and b"n_nodes" in lib.art_last_error()
    assert call(n_nodes=2 ** 31) == INVALID
    assert call(capacity=-1) == INVALID and b"capacity" in lib.art_last_error()
    assert call(n_nodes=0) == 0 and m.value == 0  # no nodes: no segments, nothing touched


def test_symbols_structs_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    for name in ("art_event_rows_device", "art_event_gather_photons_device"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(_lib.EventRowsIn) == 16 * 8 and C.sizeof(_lib.EventRowsOut) == 2 * 4 + 7 * 8
    assert len(_lib.EVENT_TOTALS) == 6
    run = inspect.signature(Engine.run_events).parameters
    want = dict(seed=1769, event_offset=0, chunk=None, saveMode=0, num_cutoff=5, MC_nodes=5, max_nodes=50, prob_cutoff=1e-10,
                backtrace_cap=256, rho_DM=0.45, n_maxSample=6, nbins=50, sky_map=None, cyclotron=False, rows=True)
    assert list(run)[:2] == ["self", "n_events"]
    for k, v in want.items():
        assert run[k].kind is inspect.Parameter.KEYWORD_ONLY and run[k].default == v, k
    ev = inspect.signature(Engine.event_rows).parameters
    assert list(ev)[:5] == ["self", "sample", "weight5", "back", "forward"]
    want = dict(event_offset=0, saveMode=0, nbins=50, flux=None, sky=None, sky_hist=None, totals=None, rows=True,
                cyclotron=False, return_bins=False)
    for k, v in want.items():
        assert ev[k].kind is inspect.Parameter.KEYWORD_ONLY and ev[k].default == v, k
    mrt = inspect.signature(A.trees.main_runner_tree).parameters
    assert mrt["device_events"].default is False
    with pytest.raises(ValueError, match="device_events"):
        A.trees.main_runner_tree(A.Params(), 9, device_events=True, saveMode=2, dir_tag="unused")


# ---- the row math


N_EV, N_NODES = 37, 400


def _synthetic():
    """N_NODES final nodes of N_EV events: random end states over many decades, then the special ones."""
    from adiabatic_raytracer_amd.trees import NODE_DTYPE
    rng = np.random.default_rng(1769)
    nd = np.zeros(N_NODES, NODE_DTYPE)
    nd["tree"] = np.sort(rng.integers(0, N_EV, N_NODES))
    nd["species"] = rng.integers(0, 2, N_NODES)
    nd["is_final"] = 1
    for f in ("weight", "prob", "prob_conv", "prob_conv0"):
        nd[f] = rng.lognormal(-3.0, 3.0, N_NODES)
    nd["x_end"] = rng.normal(size=(N_NODES, 3)) * 10.0 ** rng.uniform(1, 6, (N_NODES, 1))
    nd["k_end"] = rng.normal(size=(N_NODES, 3)) * 10.0 ** rng.uniform(-7, -4, (N_NODES, 1))
    nd["u7_end"] = rng.normal(size=N_NODES) * 1e-11
    q = 0
    nd["k_end"][q] = 0.0; q += 1  # NaN angles  # noqa: E702
    nd["k_end"][q] = (-0.0, 0.0, -0.0); q += 1  # noqa: E702
    nd["k_end"][q] = (0.0, -0.0, 1e-5); q += 1  # ±0 components: φ = atan2(-0, +0) = -0  # noqa: E702
    nd["k_end"][q] = (-0.0, -0.0, -1e-5); q += 1  # φ = -π, θ = π  # noqa: E702
    nd["k_end"][q] = (-1e-5, 0.0, 0.0); q += 1  # φ = π exactly: the last flux bin  # noqa: E702
    nd["k_end"][q] = (-1e-5, -0.0, 0.0); q += 1  # φ = -π  # noqa: E702
    for ax in range(3):  # x_end on an axis, both signs
        for sg in (1.0, -1.0):
            v = np.zeros(3)
            v[ax] = sg * 123.456
            nd["x_end"][q] = v
            q += 1
    nd["x_end"][q] = (0.0, -0.0, -0.0); q += 1  # noqa: E702
    nd["k_end"][q] = (np.nan, 1e-5, 1e-5); q += 1  # noqa: E702
    nd["k_end"][q] = (np.inf, 1e-5, 1e-5); q += 1  # noqa: E702
    for v in (np.nan, np.inf, -np.inf, 0.0, -0.0):  # non-finite u7_end
        nd["u7_end"][q] = v
        q += 1
    nd["k_end"][q] = (3e-160, 4e-160, 0.0); q += 1  # squares underflow, as numpy's do  # noqa: E702
    nd["species"][:q:2], nd["species"][1:q:2] = 0, 1  # both species among the special ones
    ev = np.zeros((N_EV, 14))
    ev[:, 0:3] = rng.normal(size=(N_EV, 3)) * 30.0
    ev[:, 3:6] = rng.normal(size=(N_EV, 3)) * 1e-5
    ev[:, 6] = rng.lognormal(20.0, 4.0, N_EV)  # sln_prob
    ev[:, 7] = rng.uniform(0.0, 1e-6, N_EV)  # vel_eng
    ev[:, 8] = rng.uniform(-1, 1, N_EV)  # cos_w
    ev[:, 9] = rng.uniform(0, 1, N_EV)  # back.prob
    ev[:, 10] = rng.uniform(0, 1, N_EV)  # back.weight
    ev[:, 11] = rng.integers(1, 4, N_EV)
    ev[:, 12] = rng.integers(1, 52, N_EV)
    ev[:, 13] = rng.integers(-4, 5, N_EV)
    return nd, ev


def _numpy_rows(fin, evd, lo, mass_a, tau=None, full=True):
    """trees.main_runner_tree's `cols` for final nodes fin, from the same per-event table"""
    from adiabatic_raytracer_amd.trees import AXION, _angles
    ev = fin["tree"]
    x, k = evd[:, 0:3], evd[:, 3:6]
    with np.errstate(all="ignore"):
        θf, ϕf, absf = _angles(fin["k_end"])
        θfX, ϕfX, absfX = _angles(fin["x_end"])
        samp_back_weight = evd[:, 9] * evd[:, 10]
        wgt = fin["weight"] * samp_back_weight[ev]
        wgt_tree = wgt
        ident = np.where(fin["species"] == AXION, 0.0, 1.0)
        tau_c = np.zeros_like(wgt)
        if tau is not None:
            tau_c = tau
            wgt = wgt * np.exp(-tau_c)
        dω = fin["u7_end"] / mass_a + evd[:, 7][ev]
        cos_t = fin["k_end"][:, 2] / absf
    cols = [lo + ev + 1.0, ident, θf, ϕf, θfX, ϕfX, absfX, evd[:, 6][ev], wgt, x[ev, 0], x[ev, 1], x[ev, 2], dω]
    if full:
        zero = np.zeros_like(wgt)
        cols += [wgt_tree, zero + tau_c, zero + 1.0, k[ev, 0], k[ev, 1], k[ev, 2], evd[:, 8][ev], evd[:, 12][ev],
                 evd[:, 13][ev], fin["prob"], fin["prob_conv"], fin["prob_conv0"], samp_back_weight[ev], absfX,
                 evd[:, 11][ev], evd[:, 9][ev]]
    return np.stack(cols, axis=1), cos_t


def _ulps(a, b):
    """|a - b| in units of b's spacing; 0 where both are NaN or equal (±0 included)"""
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.spacing(np.abs(b))
    d = np.where(both_nan | (a == b), 0.0, d)
    return np.where(np.isnan(d), np.inf, d)


ANGLES = (2, 3, 4, 5)


@pytest.mark.parametrize("ncols", [13, 29])
def test_row_math_equals_numpys(ncols):
    from tools import eventrows
    nd, ev = _synthetic()
    lo, mass_a = 1_000_003, 1e-5
    got, ct = eventrows.rows(nd, ev, event_offset=lo, mass_a=mass_a, ncols=ncols)
    ref, ct_ref = _numpy_rows(nd, ev, lo, mass_a, full=ncols == 29)
    assert got.shape == ref.shape == (N_NODES, ncols)
    # k_end = 0: θf = acos(0 / 0) is NaN (φf = atan2(0, 0) is 0)
    assert np.isnan(ref[0, 2]) and ref[0, 3] == 0 and np.isnan(ref[:, 12]).any() and np.isinf(ref[:, 12]).any()
    assert set(ref[:, 1]) == {0.0, 1.0}
    worst = 0.0
    for c in range(ncols):
        if c in ANGLES:
            u = _ulps(got[:, c], ref[:, c])
            worst = max(worst, float(u.max()))
            assert u.max() <= 4, (c, u.max(), int(u.argmax()))
            assert np.array_equal(np.isnan(got[:, c]), np.isnan(ref[:, c])), c
        else:
            assert got[:, c].tobytes() == ref[:, c].tobytes() or (
                np.array_equal(got[:, c], ref[:, c], equal_nan=True)
                and np.array_equal(np.signbit(got[:, c]), np.signbit(ref[:, c]))), c
    print(f"ncols {ncols}: angle columns within {worst:.3g} ulp of numpy's")
    assert np.array_equal(ct, ct_ref, equal_nan=True)


def test_row_math_cyclotron_columns():
    from tools import eventrows
    nd, ev = _synthetic()
    rng = np.random.default_rng(3)
    tau = np.where(nd["species"] == 1, rng.choice([0.0, 1e-3, 0.7, 30.0, 800.0, np.inf], N_NODES), 0.0)
    got, _ = eventrows.rows(nd, ev, mass_a=1e-5, tau=tau, ncols=29)
    ref, _ = _numpy_rows(nd, ev, 0, 1e-5, tau=tau)
    plain, _ = eventrows.rows(nd, ev, mass_a=1e-5, ncols=29)
    differ = [c for c in range(29) if not np.array_equal(got[:, c], plain[:, c], equal_nan=True)]
    assert differ == [8, 14]
    assert np.array_equal(got[:, 14], tau) and np.array_equal(got[:, 13], plain[:, 8], equal_nan=True)
    # exp(-0) is 1: a row without optical depth keeps its weight bit for bit
    assert np.array_equal(got[tau == 0, 8], plain[tau == 0, 8], equal_nan=True)
    # the product of column 13 and the library's exp, which is within 1 ulp of the true one, as numpy's is
    u = _ulps(got[:, 8], ref[:, 8])
    assert u.max() <= 3, u.max()
    assert (got[np.isinf(tau), 8] == 0).all()


def test_same_bits_or_both_nan():
    from tools import eventrows
    a = np.array([1.0, 0.0, -0.0, np.nan, np.nan, np.inf, 1.0, 0.0])
    b = np.array([1.0, 0.0, -0.0, np.nan, -np.nan, np.inf, np.nextafter(1.0, 2), -0.0])
    assert eventrows.same(a, b).tolist() == [True, True, True, True, True, True, False, False]
