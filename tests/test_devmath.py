"""The hand-written scalar functions of art_core.h against the TRUE value (mpmath at 256 bits,
tests/golden/devmath/*.npz from make_devmath_fixture.py), on the host compile of the header
(tools/corecheck): msincos, exp_fma, log_fma and the controller's exp_fma(log_fma(x) / 120), which
the host compiles from the same source as the device (but for log_fma's division, a Newton-refined
hardware reciprocal on the device). frcp and the min/max helpers are other code on the host (a
division, libm): tests/test_gpu_devmath.py holds the device to the same fixtures and bounds.

The bounds are on the true value and are not taken from any run of the code:
    msincos  2 ulp   1 ulp against glibc (test_corecheck.py) + glibc's documented 1 ulp
    exp_fma  1 ulp   art_core.h's statement
    log_fma  2 ulp   art_core.h's statement
    pow120   4 ulp   |ln EEst2| <= 92.2 on the set, so log_fma's 2 ulp are <= 2 2^-46; dividing by
                     120 and rounding the product leaves an argument error <= 2.9e-16, a relative
                     error <= 2.7 ulp of the result; exp_fma adds its 1 ulp
Measured on the host compile (x86-64, the maxima over each fixture; recorded results, not bounds):
    sin 1.249 (x = 138.74125174467332), cos 1.218 (x = 2.087845413262505),
    exp_fma 0.825 (x = -25.982465484032296), log_fma 1.714 (x = 1.0000004456889175),
    pow120 1.409 (x = 1.2242339508552513e-38)

The fixtures' error measure is in make_devmath_fixture.py: |(y - hi) / spacing(|hi|) - lo_ulp|."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import corecheck as cc  # noqa: E402

GOLD = os.path.join(HERE, "golden", "devmath")
BOUND = {"sincos": 2.0, "exp": 1.0, "log": 2.0, "rcp": 1.0, "pow120": 4.0}  # ulp of the true value
# the sets of make_devmath_fixture.py and their sizes, in the files' order
SETS = {
    "sincos": [("uniform_200", 2048), ("pi", 768), ("sampler_2pi", 384), ("uniform_1e6", 512), ("tiny", 64),
               ("k_half_pi", 300)],
    "exp": [("uniform_708", 1536), ("ln_t", 1536), ("small", 256), ("rint_ties", 750), ("zeros", 2)],
    "log": [("decades_300", 1280), ("half_to_2", 1024), ("one_1e-6", 512), ("one_1e-12", 256), ("eest2", 256),
            ("sqrt_half", 192), ("subnormal", 64), ("max", 1)],
    "rcp": [("mantissa_exponent", 2048), ("near_1_and_2", 384), ("mantissa_near_2", 512), ("powers_of_two", 1022)],
    "pow120": [("eest2", 2048)],
}
_cache = {}


def fixture(name):
    """the arrays of tests/golden/devmath/<name>.npz (read once, never written to)"""
    if name not in _cache:
        with np.load(os.path.join(GOLD, name + ".npz")) as z:
            _cache[name] = {k: z[k] for k in z.files}
        for a in _cache[name].values():
            a.setflags(write=False)
    return _cache[name]


def set_slice(name, set_name):
    names = [n for n, _ in SETS[name]]
    start = sum(s for _, s in SETS[name][:names.index(set_name)])
    return slice(start, start + SETS[name][names.index(set_name)][1])


def ulp_error(y, hi, lo_ulp):
    """|y - true value| in ulp of the true value (hi + lo_ulp spacing(|hi|)); inf where y is not finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs((y - hi) / np.spacing(np.abs(hi)) - lo_ulp.astype(np.float64))
    return np.where(np.isfinite(y), e, np.inf)


def report(label, x, err):
    """the measured maximum and the input that attains it; returns the maximum"""
    i = int(np.argmax(err))
    print(f"{label}: max error {err[i]:.3f} ulp at x = {float(x[i])!r} ({x.size} points)")
    return err[i]


@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_is_what_the_generator_states(name):
    f = fixture(name)
    x = f["x"]
    assert x.dtype == np.float64 and x.size <= 4096 and x.size == sum(s for _, s in SETS[name])
    assert os.path.getsize(os.path.join(GOLD, name + ".npz")) <= 128 * 1024
    assert [(str(n), int(s)) for n, s in zip(f["set_names"], f["set_sizes"])] == SETS[name]
    assert np.all(np.isfinite(x))
    for key in (("sin_", "cos_") if name == "sincos" else ("",)):
        hi, lo = f[key + "hi"], f[key + "lo_ulp"]
        assert hi.dtype == np.float64 and hi.shape == x.shape and lo.shape == x.shape
        # an ulp is taken of every hi
        assert np.all(np.isfinite(hi)) and np.all(hi != 0.0) and np.all(np.abs(lo) <= 0.5)


def test_fixture_sets_cover_the_stated_ranges():
    x = fixture("sincos")["x"]
    assert np.abs(x[set_slice("sincos", "uniform_200")]).max() <= 200.0
    assert np.abs(x[set_slice("sincos", "uniform_1e6")]).max() > 9e5
    assert 0.0 < np.abs(x[set_slice("sincos", "tiny")]).min() < 1e-250 and (x[set_slice("sincos", "tiny")] < 0).any()
    k = x[set_slice("sincos", "k_half_pi")].reshape(100, 3)
    assert np.array_equal(np.rint(k[:, 1] / (np.pi / 2)), np.arange(1, 101))
    assert np.array_equal(k[:, 0], np.nextafter(k[:, 1], -np.inf)) and np.array_equal(k[:, 2], np.nextafter(k[:, 1], np.inf))
    x = fixture("exp")["x"]
    assert np.abs(x).max() <= 708.0
    t = x[set_slice("exp", "rint_ties")].reshape(250, 3)[:, 1] / np.log(2.0)
    assert np.allclose(t - np.floor(t), 0.5, atol=1e-12) and np.floor(t).min() == -1000 and np.floor(t).max() == 1000
    z = x[set_slice("exp", "zeros")]
    assert np.all(z == 0.0) and list(np.signbit(z)) == [False, True]
    x = fixture("log")["x"]
    assert np.all(x > 0.0) and np.all(x != 1.0)
    assert np.abs(x[set_slice("log", "one_1e-12")] - 1.0).max() <= 1e-12
    sub = x[set_slice("log", "subnormal")]
    assert sub[0] == 5e-324 and np.all(sub < np.finfo(np.float64).tiny)
    assert x[-1] == np.finfo(np.float64).max
    x = fixture("rcp")["x"]
    assert np.abs(x).min() == 2.0 ** -1020 and np.abs(x).max() == 2.0 ** 1020
    for s, _ in SETS["rcp"]:
        assert (x[set_slice("rcp", s)] < 0).any() and (x[set_slice("rcp", s)] > 0).any()
    m, _ = np.frexp(np.abs(x[set_slice("rcp", "mantissa_near_2")]))
    assert np.all(2.0 * m >= 1.99) and np.all(2.0 * m < 2.0)
    m, _ = np.frexp(x[set_slice("rcp", "powers_of_two")])
    assert np.all(np.abs(m) == 0.5)
    x = fixture("pow120")["x"]
    assert 1e-40 <= x.min() and x.max() <= 1e10 and np.abs(np.log(x)).max() <= 92.2


def test_msincos_within_two_ulp_of_the_true_value():
    f = fixture("sincos")
    s, c = cc.sincos(f["x"])
    es = report("host msincos sin", f["x"], ulp_error(s, f["sin_hi"], f["sin_lo_ulp"]))
    ec = report("host msincos cos", f["x"], ulp_error(c, f["cos_hi"], f["cos_lo_ulp"]))
    for name, _ in SETS["sincos"]:
        sl = set_slice("sincos", name)
        report(f"  {name} sin", f["x"][sl], ulp_error(s[sl], f["sin_hi"][sl], f["sin_lo_ulp"][sl]))
    assert es <= BOUND["sincos"] and ec <= BOUND["sincos"]


def test_msincos_zero_and_parity():
    """sin(±0) = ±0 and cos(±0) = 1; sin odd and cos even bit for bit over the fixture"""
    z = np.array([0.0, -0.0])
    s, c = cc.sincos(z)
    assert np.array_equal(s.view(np.uint64), z.view(np.uint64)) and np.all(c == 1.0)
    x = fixture("sincos")["x"]
    s, c = cc.sincos(x)
    sn, cn = cc.sincos(-x)
    assert np.array_equal(sn.view(np.uint64), (-s).view(np.uint64)) and np.array_equal(cn.view(np.uint64), c.view(np.uint64))


def test_exp_fma_within_one_ulp_of_the_true_value():
    f = fixture("exp")
    e = report("host exp_fma", f["x"], ulp_error(cc.exp_fma(f["x"]), f["hi"], f["lo_ulp"]))
    assert e <= BOUND["exp"]


def test_log_fma_within_two_ulp_of_the_true_value():
    f = fixture("log")
    e = report("host log_fma", f["x"], ulp_error(cc.log_fma(f["x"]), f["hi"], f["lo_ulp"]))
    assert e <= BOUND["log"]


def test_pow120_within_four_ulp_of_the_true_value():
    f = fixture("pow120")
    e = report("host exp_fma(log_fma(x) / 120)", f["x"], ulp_error(cc.pow120(f["x"]), f["hi"], f["lo_ulp"]))
    assert e <= BOUND["pow120"]


# ---- the min/max helpers and the clamp: exact against numpy (the host compile is libm's fmax / fmin;
# the device's one-instruction forms are held to the same table in test_gpu_devmath.py)
SPECIAL = np.array([s * v for v in (0.0, 5e-324, 1.0, 1.5, 1e308, np.inf) for s in (1.0, -1.0)] + [np.nan])


def minmax_operands():
    """all ordered pairs of SPECIAL, then 1024 random pairs"""
    rng = np.random.default_rng(20260106)
    a, b = np.meshgrid(SPECIAL, SPECIAL, indexing="ij")
    ra = rng.standard_normal(1024) * 10.0 ** rng.uniform(-5.0, 5.0, 1024)
    rb = np.where(rng.random(1024) < 0.25, ra, rng.standard_normal(1024) * 10.0 ** rng.uniform(-5.0, 5.0, 1024))
    return np.concatenate([a.reshape(-1), ra]), np.concatenate([b.reshape(-1), rb])


def check_minmax(which, got, a, b):
    """got against numpy's fmax / fmin (a quiet NaN operand gives the other operand): equal values,
    NaN in the same places, and the sign of a zero result (MIN_Q / MAX_Q: except where the operands
    are zeros of opposite sign, which IEEE 754 leaves open; MAX_ABS: never negative)"""
    with np.errstate(invalid="ignore"):
        ref = {"MAX_ABS": np.fmax(np.abs(a), np.abs(b)), "MIN_Q": np.fmin(a, b), "MAX_Q": np.fmax(a, b),
               "RCLAMP": np.fmax(a, b)}[which]
    assert np.array_equal(np.isnan(got), np.isnan(ref)), which
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok], ref[ok]), which
    if which == "MAX_ABS":
        assert not np.signbit(got[ok]).any()
    else:
        open_case = (a == 0.0) & (b == 0.0) & (np.signbit(a) != np.signbit(b))
        m = ok & ~open_case
        assert np.array_equal(np.signbit(got[m]), np.signbit(ref[m])), which
    if which == "RCLAMP":  # a NaN radius gives rNS
        nan_r = np.isnan(a) & ~np.isnan(b)
        assert np.array_equal(got[nan_r], b[nan_r])


@pytest.mark.parametrize("which", ["MAX_ABS", "MIN_Q", "MAX_Q", "RCLAMP"])
def test_host_minmax_matches_numpy(which):
    a, b = minmax_operands()
    fn = {"MAX_ABS": cc.fmax_abs, "MIN_Q": cc.fmin_q, "MAX_Q": cc.fmax_q, "RCLAMP": cc.rclamp}[which]
    check_minmax(which, fn(a, b), a, b)
