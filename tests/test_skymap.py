"""Sky maps without a GPU: the pure-numpy end of adiabatic_raytracer_amd.trees (pulse_profile,
sky_map_edges, the packing of main_runner_tree's reduced vector) and the argument checks of the two
C entry points, which come before any device is touched."""
import ctypes as C

import numpy as np
import pytest

INVALID = -1  # ART_E_INVALID


def test_pulse_profile_rows_solid_angle_and_species():
    from adiabatic_raytracer_amd.trees import pulse_profile
    sky = np.arange(2 * 3 * 4 * 2, dtype=np.float64).reshape(2, 3, 4, 2) + 1.0
    centres = np.linspace(-np.pi, np.pi, 5)[:-1] + np.pi / 4
    # theta axis: three bins over [0, π]; an interior edge belongs to the bin on its right, π to the last
    for theta, row in ((0.0, 0), (0.5, 0), (np.linspace(0, np.pi, 4)[1], 1), (np.nextafter(np.linspace(0, np.pi, 4)[1], 0), 0),
                       (2.0, 1), (np.linspace(0, np.pi, 4)[2], 2), (np.pi, 2)):
        prof, phi = pulse_profile(sky, theta, "theta")
        assert np.array_equal(prof, sky[1, row].sum(-1)), theta
        assert np.allclose(phi, centres, rtol=0, atol=1e-15)
    # cos axis: three bins over [-1, 1] of cos θ (θ = 0 is the LAST row), per steradian
    omega = (2.0 / 3) * (2 * np.pi / 4)
    for theta, row in ((0.0, 2), (np.pi / 2, 1), (np.pi, 0), (np.arccos(0.5), 2), (np.arccos(-0.5), 0)):
        prof, _ = pulse_profile(sky, theta, "cos")
        assert np.array_equal(prof, sky[1, row].sum(-1) / omega), theta
    assert np.array_equal(pulse_profile(sky, 2.0, "theta", species=0)[0], sky[0, 1].sum(-1))
    # rows weighted by their solid angle give back the species' total
    tot = sum(pulse_profile(sky, np.arccos(c), "cos")[0].sum() * omega for c in (-2 / 3, 0.0, 2 / 3))
    assert tot == pytest.approx(sky[1].sum(), rel=1e-15)
    with pytest.raises(ValueError):
        pulse_profile(sky, 4.0, "theta")
    with pytest.raises(ValueError):
        pulse_profile(sky, 1.0, "sin")


@pytest.mark.parametrize("axis", ["cos", "theta"])
def test_sky_map_edges_are_histogramdd_edges(axis):
    from adiabatic_raytracer_amd.trees import sky_map_edges
    rng = np.random.default_rng(1)
    lo = -1.0 if axis == "cos" else 0.0
    hi = 1.0 if axis == "cos" else np.pi
    dw = (-3.1e-7, 4.7e-6)
    pts = np.stack([rng.uniform(lo, hi, 100), rng.uniform(-np.pi, np.pi, 100), rng.uniform(*dw, 100)], axis=1)
    _, ref = np.histogramdd(pts, bins=(7, 13, 5), range=((lo, hi), (-np.pi, np.pi), dw))
    got = sky_map_edges(7, 13, 5, axis, dw)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    te, pe, de = sky_map_edges(theta_axis=axis)
    assert te.shape == (33,) and pe.shape == (65,) and np.array_equal(de, [-np.inf, np.inf])
    with pytest.raises(ValueError):
        sky_map_edges(4, 4, 2, axis, None)


def test_totals_pack_round_trip_and_prefix():
    from adiabatic_raytracer_amd.trees import pack_totals, unpack_totals
    rng = np.random.default_rng(2)
    nbins = 50
    flux = rng.lognormal(size=2 * nbins)
    # the vector main_runner_tree reduced before sky maps existed
    old = np.concatenate([flux, [float(1234), float(0.25), float(7.5e-3), float(99)]])
    plain = pack_totals(flux, 1234, 0.25, 7.5e-3, 99)
    assert plain.tobytes() == old.tobytes()
    sky = rng.lognormal(size=(2, 3, 5, 2))
    tot = pack_totals(flux, 1234, 0.25, 7.5e-3, 99, sky)
    assert tot.size == old.size + sky.size and tot[:old.size].tobytes() == old.tobytes()
    u = unpack_totals(tot, nbins, sky.shape)
    assert np.array_equal(u["flux"], flux) and np.array_equal(u["sky"], sky)
    assert (u["f_inx"], u["sum_axion"], u["sum_photon"], u["rows"]) == (1234.0, 0.25, 7.5e-3, 99.0)
    assert "sky" not in unpack_totals(plain, nbins)
    # two ranks' vectors add part by part
    u2 = unpack_totals(tot + tot, nbins, sky.shape)
    assert np.array_equal(u2["sky"], 2 * sky) and u2["f_inx"] == 2468.0


def _h3(lib, n, nbins, lo, hi, mode, buf=True):
    d = (C.c_double * 8)() if buf else None
    return lib.art_histogram3_device(n, d, d, d, None, None, (C.c_int32 * 3)(*nbins), (C.c_double * 3)(*lo),
                                     (C.c_double * 3)(*hi), mode, d, None)


def test_histogram3_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    lib = A.load_library()
    lo, hi = (0.0, -1.0, 0.0), (1.0, 1.0, 2.0)
    cases = {
        "n must be": (-1, (3, 5, 2), lo, hi, 0),
        "bin counts": (4, (3, 0, 2), lo, hi, 0),
        "finite lo < hi": (4, (3, 5, 2), lo, (1.0, float("nan"), 2.0), 0),
        "mode must be": (4, (3, 5, 2), lo, hi, 3),
        "2^26": (4, (4096, 4096, 4), lo, hi, 0),
        "LDS budget": (4, (64, 128, 16), lo, hi, 1),
    }
    for msg, args in cases.items():
        assert _h3(lib, *args) == INVALID, msg
        assert msg.encode() in lib.art_last_error(), (msg, lib.art_last_error())
    for bad_hi in ((1.0, -1.0, 2.0), (1.0, -2.0, 2.0), (1.0, float("inf"), 2.0)):  # empty, reversed, infinite
        assert _h3(lib, 4, (3, 5, 2), lo, bad_hi, 0) == INVALID
        assert b"finite lo < hi" in lib.art_last_error()
    assert _h3(lib, 4, (3, 5, 2), (float("-inf"), -1.0, 0.0), hi, 0) == INVALID
    assert _h3(lib, 4, (-1, 5, 2), lo, hi, 0) == INVALID and _h3(lib, 4, (3, 5, 2), lo, hi, -1) == INVALID
    assert _h3(lib, 4, (2 ** 30, 2 ** 30, 2 ** 30), lo, hi, 0) == INVALID and b"2^26" in lib.art_last_error()
    # a table of exactly the LDS budget may be forced, one of exactly 2^26 doubles is allowed: n = 0 is
    # ART_OK after the checks and touches nothing
    assert _h3(lib, 0, (16, 32, 8), lo, hi, 1, buf=False) == 0
    assert _h3(lib, 0, (16, 32, 8 + 1), lo, hi, 1, buf=False) == INVALID
    assert _h3(lib, 0, (4096, 4096, 2), lo, hi, 0, buf=False) == 0


def test_sky_map_segments_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import SkySpec
    lib = A.load_library()
    cp = A.Params().to_c()
    d = (C.c_double * 16)()
    st = (C.c_int32 * 4)()

    def call(spec, n=4, p=cp):
        return lib.art_sky_map_segments_device(C.byref(p) if p is not None else None, C.byref(spec), n, d, d, d, st, None, None,
                                               None, d, None, None)

    good = dict(n_theta=4, n_phi=8, n_dw=3, theta_axis=1, mode=0, dw_lo=-1e-6, dw_hi=1e-6)
    cases = {
        "n must be": (dict(good), -1),
        "bin counts": (dict(good, n_theta=0), 4),
        "finite lo < hi": (dict(good, dw_hi=-1e-6), 4),
        "theta_axis": (dict(good, theta_axis=2), 4),
        "mode must be": (dict(good, mode=7), 4),
        "2^26": (dict(good, n_theta=8192, n_phi=8192), 4),
        "LDS budget": (dict(good, n_theta=64, n_phi=128, n_dw=16, mode=1), 4),
    }
    for msg, (kw, n) in cases.items():
        assert call(SkySpec(**kw), n) == INVALID, msg
        assert msg.encode() in lib.art_last_error(), (msg, lib.art_last_error())
    assert call(SkySpec(**dict(good, dw_lo=float("nan")))) == INVALID
    assert call(SkySpec(**dict(good, dw_lo=1e-6, dw_hi=1e-6))) == INVALID  # an empty range
    assert call(SkySpec(**good), p=None) == INVALID and b"params" in lib.art_last_error()
    # n = 0: ART_OK, nothing touched; with n_dw = 1 the Δω range is not looked at
    assert call(SkySpec(**good), n=0) == 0
    assert call(SkySpec(**dict(good, n_dw=1, dw_lo=float("nan"), dw_hi=float("nan"))), n=0) == 0


def test_sky_map_symbols_exported_and_bound():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib
    lib = A.load_library()
    for name in ("art_histogram3_device", "art_sky_map_segments_device"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(_lib.SkySpec) == 5 * 4 + 4 + 2 * 8  # art_sky_spec: five int32, padding, two doubles


def test_main_runner_tree_refuses_a_rank_dependent_range():
    import adiabatic_raytracer_amd as A
    with pytest.raises(ValueError, match="dw_range"):
        A.trees.main_runner_tree(A.Params(), 9, world=2, rank=0, sky_map={"n_dw": 4})
    with pytest.raises(ValueError, match="unknown keys"):
        A.trees.main_runner_tree(A.Params(), 9, sky_map={"n_thta": 4})
