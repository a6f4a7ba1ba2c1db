"""The host paths' plan and copy lists (art_host_plan.h), through a host compile of the header
(tools/hostplancheck): the streamed call's upload units and block counts, and the row segments that
scatter a piece's output blob into the caller's arrays and gather the caller's inputs -- one
definition for the chunked pipeline and the streamed call. No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hostplancheck  # noqa: E402


def loop_units(n, first, step, ramp, lanes):
    """The loop the streamed call ran before its plan became a header (lanes: iblocks x 256)."""
    lanes = lanes if ramp else 0
    ulo, lo, sz = [0], 0, first
    while lo < n:
        lo = min(n, lo + sz)
        ulo.append(lo)
        if lo >= lanes:
            sz = min(step, 2 * sz) if (ramp and sz < step) else step
    return ulo


# worked out by hand from that loop
UNITS = [
    ((20011, 1024, 4096, True, 8192), list(range(0, 8193, 1024)) + [10240, 14336, 18432, 20011]),
    ((20011, 1024, 4096, False, 8192), [0, 1024, 5120, 9216, 13312, 17408, 20011]),
    ((777, 1024, 4096, True, 8192), [0, 777]),
    ((777, 1024, 4096, True, 0), [0, 777]),
    ((10 ** 7, 2 ** 16, 2 ** 18, True, 496 * 256),
     [0, 65536, 131072, 262144, 524288] + list(range(524288 + 2 ** 18, 10 ** 7, 2 ** 18)) + [10 ** 7]),
]


@pytest.mark.parametrize("args,want", UNITS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_upload_units(args, want):
    n = args[0]
    ok, got = hostplancheck.units(*args)  # (the tool itself checks that they span [0, n) and increase)
    assert ok, got
    assert got[0] == 0 and got[-1] == n and all(b > a for a, b in zip(got, got[1:]))
    assert got == want
    assert got == loop_units(*args)


def test_upload_units_first_case_has_12_units():
    ok, got = hostplancheck.units(20011, 1024, 4096, True, 8192)
    assert ok and len(got) - 1 == 12


@pytest.mark.parametrize("n,first,step,lanes", [(1250000, 2 ** 16, 2 ** 18, 496 * 256), (3001, 512, 1024, 700),
                                                (4096, 4096, 4096, 0), (1, 1, 1, 1), (100000, 3, 1000, 50)])
@pytest.mark.parametrize("ramp", [True, False])
def test_upload_units_equal_the_loop(n, first, step, lanes, ramp):
    ok, got = hostplancheck.units(n, first, step, ramp, lanes)
    assert ok, got
    assert got == loop_units(n, first, step, ramp, lanes)


def test_block_counts():
    assert hostplancheck.blocks(512, 2, 16, False) == (16, 496)
    assert hostplancheck.blocks(512, 1, 8, False) == (8, 496)  # a 1-wave/SIMD helper block holds two slots
    for hw, helpers in [(2, 16), (1, 8), (2, 1)]:
        assert hostplancheck.blocks(512, hw, helpers, True) == (helpers, 512)  # serial: every slot integrates
    assert hostplancheck.blocks(8, 2, 100, False) == (7, 1)  # helpers <= slots - 1
    assert hostplancheck.blocks(8, 2, 0, False) == (1, 7)  # ... and at least one


@pytest.mark.parametrize("cap", [0, 3])
def test_scatter_and_gather(cap):
    n, lo, m = 5000, 3000, 1000
    ok, text = hostplancheck.scatter(n, lo, m, cap)
    assert ok, text
    _, nseg, nbytes = text.split()
    # 8 double rows and 3 int32 rows; with crossings the counts and 9 cap double rows
    assert int(nseg) == 11 + (1 + 9 * cap if cap else 0)
    assert int(nbytes) == m * 76 + (m * 4 + cap * m * 72 if cap else 0)


@pytest.mark.parametrize("n,lo,m", [(777, 0, 777), (2049, 2048, 1), (4096, 1024, 3072)])
def test_scatter_and_gather_at_the_ends(n, lo, m):
    for cap in (0, 1):
        ok, text = hostplancheck.scatter(n, lo, m, cap)
        assert ok, text
