"""The device's hand-written scalar functions (art_core.h: msincos, exp_fma, log_fma, frcp, the
one-instruction min/max, rclamp) through art_eval_math_device, which loads the operands, calls the
function itself and stores the result -- the __HIP_DEVICE_COMPILE__ branches that no host test
reaches (v_rndne / v_ldexp / v_frexp / v_rcp_f64, the inline-asm v_max_f64 / v_min_f64).

Accuracy is held against the TRUE value (tests/golden/devmath/*.npz, mpmath at 256 bits,
make_devmath_fixture.py) at bounds that are fixed by the functions' own statements and not taken
from a device run (test_devmath.BOUND and its docstring's derivations):

    msincos 2 ulp, exp_fma 1 ulp, log_fma 2 ulp, frcp 1 ulp for 2^-1020 <= |x| <= 2^1020,
    fexp(flog(x) * (1.0 / 120.0)) 4 ulp

Device maxima over the fixtures, measured on an MI355X (recorded results, not bounds; both
translation units give the same bits):

    msincos  sin 1.249 ulp at x = 138.74125174467332, cos 1.218 ulp at x = 2.087845413262505
             (the k π/2 set: 0.813 / 0.916; ±1e6: 1.168 / 0.977) -- the host compile's figures
    exp_fma  0.825 ulp at x = -25.982465484032296 (the rint ties: 0.782) -- the host compile's
    log_fma  1.902 ulp at x = 1.0000002345360504 (host compile, which divides: 1.714); away from
             1 ± 1e-6 at most 1.677 ([0.5, 2]); subnormals and the largest double below 0.5
    frcp     0.500 ulp: correctly rounded at every one of the 3966 points
    pow120   1.409 ulp at x = 1.2242339508552513e-38 -- the host compile's

What the tests found: msincos(-0) returned sin = +0 (the reduction's fma(+0, π/2, -0) is +0). The
function now reduces |x| and puts x's sign into sin's sign bit, which changes no other result.
"""
import numpy as np
import pytest

from test_devmath import BOUND, SETS, check_minmax, fixture, minmax_operands, report, set_slice, ulp_error

pytestmark = pytest.mark.gpu

ONE_OPERAND = ["SINCOS", "EXP", "LOG", "RCP", "POW120"]
TWO_OPERAND = ["MAX_ABS", "MIN_Q", "MAX_Q", "RCLAMP"]
FIXTURE_OF = {"SINCOS": "sincos", "EXP": "exp", "LOG": "log", "RCP": "rcp", "POW120": "pow120"}


@pytest.fixture(scope="module")
def eng():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    return Engine(A.Params(theta_m=0.2, B0=1e14, mass_a=1e-5, flat=True))


def run(eng, fn, a, b=None, tu=0):
    """fn at every element of a (and b) on the device: one array, or (sin, cos) for SINCOS"""
    import torch
    dev = lambda v: None if v is None else torch.as_tensor(np.array(v, np.float64), device=eng.device)  # noqa: E731
    out = eng.eval_math(fn, dev(a), dev(b), tu=tu)
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- accuracy against the true value
def test_msincos_within_two_ulp_of_the_true_value(eng):
    f = fixture("sincos")
    s, c = run(eng, "SINCOS", f["x"])
    es = report("device msincos sin", f["x"], ulp_error(s, f["sin_hi"], f["sin_lo_ulp"]))
    ec = report("device msincos cos", f["x"], ulp_error(c, f["cos_hi"], f["cos_lo_ulp"]))
    for name, _ in SETS["sincos"]:
        sl = set_slice("sincos", name)
        report(f"  {name} sin", f["x"][sl], ulp_error(s[sl], f["sin_hi"][sl], f["sin_lo_ulp"][sl]))
        report(f"  {name} cos", f["x"][sl], ulp_error(c[sl], f["cos_hi"][sl], f["cos_lo_ulp"][sl]))
    assert es <= BOUND["sincos"] and ec <= BOUND["sincos"]


@pytest.mark.parametrize("fn", ["EXP", "LOG", "POW120"])
def test_exp_log_pow120_within_their_bounds_of_the_true_value(eng, fn):
    name = FIXTURE_OF[fn]
    f = fixture(name)
    y = run(eng, fn, f["x"])
    err = ulp_error(y, f["hi"], f["lo_ulp"])
    for s, _ in SETS[name]:
        sl = set_slice(name, s)
        report(f"  {s}", f["x"][sl], err[sl])
    assert report(f"device {fn}", f["x"], err) <= BOUND[name]


def test_frcp_within_one_ulp_of_the_exact_quotient(eng):
    """2^-1020 <= |x| <= 2^1020 (the fixture's range): frcp's arguments are abstol + |u| reltol,
    controller factors and radii, and subnormal operands or results are not reached."""
    f = fixture("rcp")
    y = run(eng, "RCP", f["x"])
    err = ulp_error(y, f["hi"], f["lo_ulp"])
    for s, _ in SETS["rcp"]:
        sl = set_slice("rcp", s)
        report(f"  {s}", f["x"][sl], err[sl])
    assert report("device frcp", f["x"], err) <= BOUND["rcp"]


# ---- exact identities
def test_exact_identities(eng):
    z = np.array([0.0, -0.0])
    assert same_bits(run(eng, "EXP", z), [1.0, 1.0])
    assert same_bits(run(eng, "LOG", np.array([1.0])), [0.0])
    s, c = run(eng, "SINCOS", z)
    assert same_bits(s, z) and same_bits(c, [1.0, 1.0])


def test_sincos_parity_bit_for_bit(eng):
    x = fixture("sincos")["x"]
    s, c = run(eng, "SINCOS", x)
    sn, cn = run(eng, "SINCOS", -x)
    assert same_bits(sn, -s) and same_bits(cn, c)


def test_frcp_powers_of_two_and_oddness(eng):
    x = fixture("rcp")["x"]
    y = run(eng, "RCP", x)
    p2 = set_slice("rcp", "powers_of_two")
    m, e = np.frexp(x[p2])
    assert same_bits(y[p2], np.ldexp(m, 2 - e))  # ±2^(e-1) -> ±2^(1-e)
    assert same_bits(run(eng, "RCP", -x), -y)


# ---- documented edges, as art_core.h states them
def test_documented_edges(eng):
    assert np.isnan(run(eng, "RCP", np.array([0.0, -0.0, np.inf, -np.inf]))).all()
    nan = np.array([np.nan])
    for fn in ("EXP", "LOG", "RCP"):
        assert np.isnan(run(eng, fn, nan)).all(), fn
    s, c = run(eng, "SINCOS", nan)
    assert np.isnan(s).all() and np.isnan(c).all()
    y = run(eng, "EXP", np.array([710.0, -800.0]))
    assert y[0] == np.inf and y[1] == 0.0


# ---- min / max / clamp: exact against numpy
@pytest.mark.parametrize("fn", TWO_OPERAND)
def test_minmax_matches_numpy(eng, fn):
    """The NaN behaviour of the inline-asm v_max_f64 / v_min_f64 depends on the kernel's IEEE mode
    bit; the error norm relies on it: fmax_abs(u[i], y[i]) with a NaN y must not poison EEst2
    before the explicit finiteness check on y."""
    a, b = minmax_operands()
    check_minmax(fn, run(eng, fn, a, b), a, b)


# ---- the two translation units round alike (bulk, continuation and tail are bit-identical
# because these functions give the same bits wherever they are inlined)
@pytest.mark.parametrize("fn", ONE_OPERAND + TWO_OPERAND)
def test_translation_units_agree_bit_for_bit(eng, fn):
    if fn in TWO_OPERAND:
        a, b = minmax_operands()
    else:
        a, b = fixture(FIXTURE_OF[fn])["x"], None
    o0, o1 = run(eng, fn, a, b, tu=0), run(eng, fn, a, b, tu=1)
    if fn == "SINCOS":
        assert same_bits(o0[0], o1[0]) and same_bits(o0[1], o1[1])
    else:
        assert same_bits(o0, o1)


# ---- the interface
def test_unknown_fn_or_tu_is_invalid_and_empty_is_ok(eng):
    import torch
    from adiabatic_raytracer_amd._lib import ArtError
    a = torch.ones(4, dtype=torch.float64, device=eng.device)
    for fn, tu in ((-1, 0), (9, 0), (1000, 1), (0, 2), (0, -1)):
        with pytest.raises(ArtError, match="libart error -1"):
            eng.eval_math(fn, a, tu=tu)
    # n = 0: OK, and nothing is touched (NULL everywhere)
    assert eng.lib.art_eval_math_device(1, 0, 0, None, None, None, None, None) == 0
    assert eng.eval_math("EXP", a[:0]).numel() == 0
    # an unused output may be NULL
    out = torch.full((4,), -7.0, dtype=torch.float64, device=eng.device)
    import ctypes as C
    assert eng.lib.art_eval_math_device(0, 0, 4, C.c_void_p(a.data_ptr()), None, None, C.c_void_p(out.data_ptr()),
                                        None) == 0
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), run(eng, "SINCOS", np.ones(4))[1])
