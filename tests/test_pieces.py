"""The streamed host pipeline's partition of a batch into output pieces (art_pieces.h), compiled
for the host (tools/piececheck): coarse pieces over the bulk of the batch and fine ones over its
last rays. For batch sizes from 1 ray to 2^31 - 1 and several (coarse, fine, region) settings the
pieces tile [0, n) without gap or overlap, number at most 64 (one flag, one counter and one
histogram lane each), agree with piece_of at both ends of every piece (64-bit and 32-bit ray
index), hold whole 1024-ray helper tiles, and have blobs that do not overlap. The header is the
one the host, the helpers and the integrator include."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import piececheck  # noqa: E402

SIZES = [1, 63, 64, 1023, 1024, 1025, 20011, 1_250_000, 10_000_000, 2**31 - 1]
# (coarse shift, fine shift, fine region in rays): the defaults' range for the 10^7-ray batch, the
# GPU tests' small pieces, one level (fine 0 / region 0 / fine >= coarse), a region beyond the batch
SETTINGS = [(18, 15, 1 << 20), (18, 14, 1 << 19), (18, 16, 1 << 20), (18, 14, 1 << 20), (16, 15, 156250),
            (12, 10, 7723), (12, 10, 100), (12, 10, 1 << 30), (11, 0, 0), (12, 10, 0), (12, 12, 5000), (12, 13, 5000),
            (10, 10, 1 << 20), (4, 3, 1000), (24, 10, 1 << 20)]


@pytest.mark.parametrize("n", SIZES)
def test_pieces_tile_the_batch(n):
    for shift, fine, region in SETTINGS:
        ok, text = piececheck.check(n, shift, fine, region)
        assert ok, (n, shift, fine, region, text)


def test_known_partitions():
    """The partitions the GPU tests and the 10^7-ray default rely on: (count, coarse pieces, coarse
    shift, fine shift, split)."""
    got = lambda *a: tuple(int(v) for v in piececheck.check(*a)[1].split()[1:])  # noqa: E731
    assert got(20011, 12, 10, 7723) == (11, 3, 12, 10, 12288)  # 3 coarse, 7 full fine pieces and a partial eighth
    assert got(20011, 12, 10, 0) == (5, 5, 12, 12, 20011)  # region 0: one level
    assert got(20011, 12, 10, 1 << 30) == (20, 0, 12, 10, 0)  # region >= n: every piece fine
    assert got(4096, 12, 10, 100) == (1, 1, 12, 12, 4096)  # split exactly at n: no fine piece
    assert got(20011, 11, 0, 0) == (10, 10, 11, 11, 20011)  # one level, as ART_HOST_PIECE_SHIFT alone
    assert got(10_000_000, 18, 15, 1 << 20) == (61, 35, 18, 15, 35 << 18)
    # too many fine pieces for the 64 flags: the fine pieces grow, the split stays
    assert got(10_000_000, 18, 14, 1 << 20) == (61, 35, 18, 15, 35 << 18)
    assert got(2**31 - 1, 18, 15, 1 << 20) == (64, 64, 25, 25, 2**31 - 1)
