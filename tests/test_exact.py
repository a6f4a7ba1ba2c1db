"""Exact tables without a GPU ("Exact tables"): the host twins of the accumulator (art_exact_add_host,
art_exact_normalize_host, art_exact_round_host: art_exact.h's functions, the ones the kernels run) and trees.rows_exact,
exact_merge, exact_finish and the rank vector's exact part, against the oracle float(sum(map(Fraction, values))), the
round-to-nearest-even of the infinitely precise sum (Fraction, not math.fsum, which raises on an intermediate overflow).
Every comparison is bit for bit: an exact sum has no tolerance."""
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest

from adiabatic_raytracer_amd import _lib, trees
from adiabatic_raytracer_amd.engine import Engine

LIMBS = 66
MASK = (1 << 32) - 1


def oracle(values):
    s = sum(map(Fraction, values))
    try:
        return float(s)  # (round-to-nearest-even of the exact rational)
    except OverflowError:
        return math.inf if s > 0 else -math.inf


def exact_sum(values):
    acc, bad = trees.exact_add(values)
    assert bad == 0
    return float(trees.exact_round(acc)[0]), acc


def same(a, b):
    """bit for bit, so that -0.0 is not +0.0"""
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def value_of(limbs):
    """the integer an accumulator holds, in units of 2^-1074"""
    return sum(int(v) << (32 * j) for j, v in enumerate(limbs))


def normalised(acc):
    acc = np.asarray(acc).reshape(-1, LIMBS)
    return bool(np.all((acc[:, :-1] >= 0) & (acc[:, :-1] <= MASK)))


def test_the_interface():
    lib = _lib.load()
    for name in ("art_exact_histogram_device", "art_exact_finish_device", "art_event_exact_device", "art_exact_add_host",
                 "art_exact_normalize_host", "art_exact_round_host"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.EXACT_LIMBS == LIMBS and Engine.EXACT_MAX_BYTES == 1 << 30
    for fn in (Engine.run_events, trees.main_runner_tree):
        par = inspect.signature(fn).parameters["exact"]
        assert par.default is False and par.kind is par.KEYWORD_ONLY
    for name in ("rows_exact", "exact_merge", "exact_finish", "exact_result", "exact_pack", "exact_unpack"):
        assert callable(getattr(trees, name))
    assert callable(Engine.event_exact) and callable(Engine.exact_finish)


def test_argument_checks_touch_no_device():
    import ctypes as C
    lib = _lib.load()
    z = np.zeros(LIMBS, np.int64)
    assert lib.art_exact_histogram_device(-1, None, None, 1, None, None, 0, None) == -1
    assert lib.art_exact_histogram_device(0, None, None, 0, None, None, 0, None) == -1
    assert lib.art_exact_histogram_device(0, None, None, 1, None, None, 3, None) == -1
    assert lib.art_exact_histogram_device(0, None, None, 125, None, None, 1, None) == -1 and b"124" in lib.art_last_error()
    assert lib.art_exact_histogram_device(0, None, None, 124, None, None, 1, None) == 0  # (n == 0: nothing touched)
    assert lib.art_exact_histogram_device(1, None, None, 1, z.ctypes.data, None, 0, None) == -1
    assert lib.art_exact_finish_device(-1, None, None, None) == -1 and lib.art_exact_finish_device(0, None, None, None) == 0
    assert lib.art_exact_finish_device(1, None, None, None) == -1
    assert lib.art_exact_add_host(1, None, None, 1, None, None) == -1 and lib.art_exact_round_host(1, None, None) == -1
    # the event call: the replicates call's rules, the mode and its LDS limit
    import adiabatic_raytracer_amd as A
    cp = A.Params().to_c()
    ein = _lib.EventRowsIn(0, 0, None, None, None, None, None, None, None, 0, None, None, None, 0, None, None)
    out = lambda **kw: _lib.EventExactOut(**{**dict(kind=0, n_sets=1, nbins=50, mode=0), **kw})  # noqa: E731
    call = lambda o: lib.art_event_exact_device(C.byref(cp), C.byref(ein), None, C.byref(o), None)  # noqa: E731
    assert call(out()) == 0  # (no events: nothing touched)
    assert lib.art_event_exact_device(None, C.byref(ein), None, C.byref(out()), None) == -1
    assert lib.art_event_exact_device(C.byref(cp), None, None, C.byref(out()), None) == -1
    assert lib.art_event_exact_device(C.byref(cp), C.byref(ein), None, None, None) == -1
    for bad in (dict(kind=3), dict(kind=-1), dict(n_sets=0), dict(n_sets=33), dict(n_sets=2), dict(kind=1, n_sets=2),
                dict(kind=2, n_sets=2), dict(mode=3), dict(mode=-1), dict(nbins=-1), dict(nbins=4097), dict(mode=1, nbins=57)):
        assert call(out(**bad)) == -1, bad
    assert call(out(mode=1, nbins=56)) == 0 and call(out(mode=2, nbins=4096)) == 0
    ein.n_events = 1
    assert call(out()) == -1  # (events and no tables)
    # the cap: a 64 x 128 x 16 map is 138 MB for the run and over the cap for a scan of 32
    shape = (2, 64, 128, 16)
    Engine._exact_fit("the run", 1, 50, shape)
    assert 8 * LIMBS * (100 + 2 * 64 * 128 * 16 + 2) == 138465888
    with pytest.raises(ValueError, match="exact: the accumulators of the coupling scan"):
        Engine._exact_fit("the coupling scan", 32, 50, shape)
    Engine._exact_fit("the coupling scan", 32, 50, None)
    with pytest.raises(ValueError, match="device_events=True"):
        trees.main_runner_tree(A.Params(), 3, exact=True)
    with pytest.raises(ValueError, match="device_events=True"):
        trees.main_runner_tree(A.Params(), 3, exact=True, device_trees=True)


def test_cancellation():
    got, _ = exact_sum([1e308, 1.0, -1e308])
    assert got == 1.0 == oracle([1e308, 1.0, -1e308]) and sum([1e308, 1.0, -1e308]) == 0.0  # (what float adds give)
    vals = [2.0 ** 53, 1.0, 1.0]
    want = oracle(vals)
    assert want == 2.0 ** 53 + 2
    first = None
    for perm in ([0, 1, 2], [1, 0, 2], [1, 2, 0], [2, 1, 0], [0, 2, 1], [2, 0, 1]):
        got, acc = exact_sum([vals[i] for i in perm])
        first = acc if first is None else first
        assert got == want and np.array_equal(acc, first), perm
    assert (2.0 ** 53 + 1.0) + 1.0 == 2.0 ** 53  # (the float sum in the stated order loses both)


def test_ties_to_even():
    assert exact_sum([2.0 ** 53, 1.0])[0] == 2.0 ** 53 == oracle([2.0 ** 53, 1.0])
    assert exact_sum([2.0 ** 53, 3.0])[0] == 2.0 ** 53 + 4 == oracle([2.0 ** 53, 3.0])
    assert exact_sum([2.0 ** 53, 1.0, 2.0 ** -1074])[0] == 2.0 ** 53 + 2  # (a sticky bit 2127 places down breaks the tie)
    assert exact_sum([-(2.0 ** 53), -1.0])[0] == -(2.0 ** 53) and exact_sum([-(2.0 ** 53), -3.0])[0] == -(2.0 ** 53) - 4
    # a carry out of the 53 bits: 2^54 - 1 rounds to 2^54
    vals = [2.0 ** 53, 2.0 ** 53 - 1.0]
    assert exact_sum(vals)[0] == 2.0 ** 54 == oracle(vals)


def test_subnormals():
    tiny = 5e-324
    assert exact_sum([tiny] * 3)[0] == 1.5e-323 == oracle([tiny] * 3)
    top = math.ldexp(1.0, -1022) - tiny  # the largest subnormal
    for vals in ([top, tiny], [top, top], [top, top, tiny], [math.ldexp(1.0, -1023)] * 3, [top, -tiny, -top]):
        assert same(exact_sum(vals)[0], oracle(vals)), vals
    assert exact_sum([top, tiny])[0] == math.ldexp(1.0, -1022)  # leaves the subnormal range, exactly


def test_overflow():
    assert exact_sum([1.7e308, 1.7e308])[0] == math.inf == oracle([1.7e308, 1.7e308])
    vals = [1.7e308, 1.7e308, -1.7e308]
    assert exact_sum(vals)[0] == 1.7e308 == oracle(vals)
    assert exact_sum([-1.7e308, -1.7e308])[0] == -math.inf
    big = float.fromhex("0x1.fffffffffffffp+1023")
    assert exact_sum([big, math.ldexp(1.0, 969)])[0] == big  # below the tie: stays finite
    assert exact_sum([big, math.ldexp(1.0, 970)])[0] == math.inf  # the tie rounds to even, 2^1024
    assert oracle([big, math.ldexp(1.0, 970)]) == math.inf


def test_signed_zero_sum():
    for vals in ([1.5, -1.5], [-1.5, 1.5], [-0.0], [-0.0, -0.0], [5e-324, -5e-324], [1e308, -1e308, 1e-308, -1e-308]):
        assert same(exact_sum(vals)[0], 0.0), vals
    assert same(float(trees.exact_round(np.zeros((1, LIMBS), np.int64))[0]), 0.0)


def test_nonfinite_values_are_counted_and_not_added():
    acc, bad = trees.exact_add([1.0, math.nan, math.inf, -math.inf, 2.0])
    assert bad == 3 and trees.exact_round(acc)[0] == 3.0
    acc2, bad2 = trees.exact_add([math.nan], acc=acc.copy())
    assert bad2 == 1 and np.array_equal(acc2, acc)
    # bins: -1 and out of range are skipped, whatever their value
    acc, bad = trees.exact_add([1.0, 2.0, math.nan, 4.0, 8.0], bins=[0, 2, -1, 3, 1], n_bins=3)
    assert bad == 0 and np.array_equal(trees.exact_round(acc), [1.0, 8.0, 2.0])


def test_bulk_three_shuffles():
    rng = np.random.default_rng(1769)
    vals = 10.0 ** rng.uniform(-300, 300, 10000) * rng.choice([-1.0, 1.0], 10000)
    want = oracle(vals.tolist())
    first = None
    for _ in range(3):
        v = rng.permutation(vals)
        got, acc = exact_sum(v)
        first = acc if first is None else first
        assert got == want and np.array_equal(acc, first) and normalised(acc)
    assert value_of(first[0]) * Fraction(1, 2 ** 1074) == sum(map(Fraction, vals.tolist()))
    assert float(np.sum(vals)) != want or float(np.sum(vals[::-1])) != want  # (the float sums do depend on the order)


def test_random_small_sums_round_correctly():
    """every path of exact_round: subnormal and normal results, the leading bit at every place of its limb, guard and
    sticky bits in the limb below and far below, negative sums"""
    rng = np.random.default_rng(7)
    for _ in range(4000):
        n = int(rng.integers(1, 6))
        ex = rng.choice([-1126, -1100, -1075, -1022, -970, -60, -53, -1, 0, 31, 32, 33, 64, 900, 938], n) + rng.integers(0, 33, n)
        vals = [math.ldexp(float(int(rng.integers(0, 1 << 53))) * float(rng.choice([-1, 1])), int(e)) for e in ex]
        assert all(math.isfinite(v) for v in vals)
        assert same(exact_sum(vals)[0], oracle(vals)), vals


def test_headroom():
    # 2^20 copies of the largest double below 2 through the host add
    x = float.fromhex("0x1.fffffffffffffp+0")
    acc, bad = trees.exact_add(np.full(1 << 20, x))
    want = oracle([x]) * 2.0 ** 20  # (a power of two times x: exact)
    assert bad == 0 and normalised(acc) and trees.exact_round(acc)[0] == want == float(Fraction(x) * (1 << 20))
    # the rule: every call leaves the accumulator normalised and adds at most 2^30 values between two normalisations,
    # so a limb holds at most its normalised content and 2^30 pieces below 2^32 in size. The extreme states of that
    # rule, of both signs, normalise to the same value with every low limb in [0, 2^32)
    hi = MASK + (1 << 30) * MASK
    assert hi < (1 << 63)
    rng = np.random.default_rng(3)
    for state in (np.full(LIMBS, hi), np.full(LIMBS, -(1 << 30) * MASK), np.where(rng.random(LIMBS) < 0.5, hi, -(1 << 30) * MASK),
                  rng.integers(-(1 << 30) * MASK, hi, LIMBS, endpoint=True)):
        state = state.astype(np.int64).reshape(1, LIMBS)
        state[0, -1] = int(rng.integers(-1000, 1000))  # the top limb: signed, the headroom
        before = value_of(state[0])
        after = trees.exact_normalize(state.copy())
        assert value_of(after[0]) == before and normalised(after)
        assert np.array_equal(trees.exact_normalize(after.copy()), after)  # (idempotent)
        # and the rounding does not need the normalised form
        assert same(trees.exact_round(state)[0], trees.exact_round(after)[0])
        frac = Fraction(before, 2 ** 1074)
        try:
            want = float(frac)
        except OverflowError:
            want = math.inf if frac > 0 else -math.inf
        assert same(trees.exact_round(after)[0], want)
    # one more normalised accumulator on top of an extreme one is still inside an int64
    assert hi + MASK < (1 << 63)


def _rows(n, rng, nbins):
    rows = np.zeros((n, 13))
    rows[:, 0] = rng.integers(1, 40, n)
    rows[:, 1] = rng.integers(0, 2, n)
    rows[:, 2] = rng.uniform(0, np.pi, n)
    rows[:, 3] = rng.uniform(-np.pi, np.pi, n)
    rows[:, 3][rng.random(n) < 0.05] = np.nan  # rows no flux bin counts: the totals still do
    rows[:, 7] = 10.0 ** rng.uniform(-12, 3, n)
    rows[:, 8] = 10.0 ** rng.uniform(-20, 8, n)
    rows[:, 12] = rng.uniform(-1.5e-6, 1.5e-6, n)
    return rows


SKY = dict(n_theta=3, n_phi=4, n_dw=2, theta_axis="theta", dw_range=(-1e-6, 1e-6))


def test_rows_exact_against_fraction():
    rng = np.random.default_rng(11)
    nbins = 7
    rows = _rows(3000, rng, nbins)
    rows[5, 8] = math.inf
    rows[9, 7] = math.nan
    got = trees.rows_exact(rows, nbins, SKY, f_inx=17, acc=True)
    assert got["nonfinite"] == 2
    p = rows[:, 8] * rows[:, 7]
    ok = np.isfinite(p)
    sp = (rows[:, 1] != 0).astype(int)
    fb = trees.hist_bins(rows[:, 3], nbins)
    sb = trees.sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **SKY)
    assert (fb < 0).any() and (sb < 0).any()
    for name, lab, shape in (("flux_raw", np.where(fb >= 0, sp * nbins + fb, -1), (2, nbins)), ("totals_raw", sp, (2,)),
                             ("sky_raw", sb, (2, 3, 4, 2))):
        want = np.array([oracle(p[ok & (lab == b)].tolist()) for b in range(int(np.prod(shape)))]).reshape(shape)
        assert got[name].shape == shape and np.array_equal(got[name], want), name
    assert np.array_equal(got["flux"], got["flux_raw"] / 17.0) and np.array_equal(got["sky_map"], got["sky_raw"] / 17.0)
    assert np.array_equal(got["sum_weight_sln_prob"], got["totals_raw"] / 17.0)
    # the accumulators of the same rows finish to the same tables
    fin = trees.exact_finish(got["acc"])
    for name in ("flux_raw", "sky_raw", "totals_raw"):
        assert np.array_equal(fin[name], got[name]), name
    res = trees.exact_result(got["acc"], 17)
    assert np.array_equal(res["flux"], got["flux"]) and res["nonfinite"] == 2
    # no rows, no map
    empty = trees.rows_exact(rows[:0], nbins)
    assert not empty["flux_raw"].any() and "sky_raw" not in empty and empty["nonfinite"] == 0


def test_exact_merge_of_two_halves_is_the_whole():
    rng = np.random.default_rng(12)
    nbins = 5
    rows = _rows(2000, rng, nbins)
    whole = trees.rows_exact(rows, nbins, SKY, acc=True)
    a = trees.rows_exact(rows[:700], nbins, SKY, acc=True)["acc"]
    b = trees.rows_exact(rows[700:], nbins, SKY, acc=True)["acc"]
    for order in ([a, b], [b, a]):
        m = trees.exact_merge(order)
        for k in ("flux", "sky", "totals"):
            assert np.array_equal(m[k], whole["acc"][k]) and normalised(m[k]), k
        fin = trees.exact_finish(m)
        for name in ("flux_raw", "sky_raw", "totals_raw"):
            assert np.array_equal(fin[name], whole[name]), name
    # the float sums of the halves' float tables do not all agree with the exact table
    with pytest.raises(ValueError, match="other sets or other tables"):
        trees.exact_merge([a, trees.rows_exact(rows, nbins + 1, SKY, acc=True)["acc"]])
    # the rank vector: without exact it is what it was; with it the limbs come last and sum exactly
    tot = np.arange(5.0)
    assert trees.rank_vector(tot)[0] is tot and trees.rank_vector(tot, exact=None)[0] is tot
    va, ends = trees.rank_vector(tot, exact={"run": a})
    vb, _ = trees.rank_vector(tot, exact={"run": b})
    assert list(ends) == [5, len(va)] and np.array_equal(va[:5], tot) and np.array_equal(va[5:], trees.exact_pack(a))
    back = trees.exact_unpack((va + vb)[5:], a)
    for k in ("flux", "sky", "totals"):
        assert np.array_equal(back[k], whole["acc"][k]), k
    assert back["kind"] == "run" and np.array_equal(back["nonfinite"], [0.0])


@pytest.mark.skipif(not __import__("os").path.exists("/opt/rocm/bin/hipcc") or __import__("shutil").which("make") is None,
                    reason="needs hipcc and make")
def test_the_header_is_sanitizer_clean():
    """tools/exactcheck.cpp, a stand-alone program on art_exact.h, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    import os
    import subprocess
    asan = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "asan")
    subprocess.run(["make", "-C", asan, "build/exact_asan"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(asan, "build", "exact_asan")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "exact OK" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr
