"""GPU: the exclusive prefix scan (segalign_amd/csrc/scan.hip: reduce, one-workgroup scan of the tile sums, downsweep) alone, through the
test entry sa_scan_counts, against numpy.cumsum over uint64 with a leading 0.  Every stage reaches the scan only at the sizes and
pointer alignments its data happens to produce; here they are chosen:
  * the load path: the input lies `skew` words behind a 256-byte-aligned address -- skew 0 and 4 take the 16-byte loads (4: 16-byte but not
    32-byte aligned), 1, 2, 3 the scalar loads;
  * the tail tile: n on either side of 8 (a thread's items) and of 2048 (a tile);
  * the partials loop: 256 tiles (one trip), 257 (two), 513 tiles and 5 words (three);
  * wide sums: all 0xFFFFFFFF passes 2^32 at n = 2; the 64-bit form is exact, the 32-bit form is held to the sum modulo 2^32;
  * the total out[n], also for n = 0;
  * the scratch: exactly scan_temp_bytes(n) bytes, pre-filled with a non-zero pattern, a guard region directly behind it and behind the
    n + 1 outputs: every case asserts both guards intact and the input unchanged.
All comparisons are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 2048
PARTIALS = 256                                   # tile sums per trip of the partials loop
SMALL_N = (0, 1, 7, 8, 9, 2047, 2048, 2049)
LARGE_N = (524287, 524288, 524289, TILE * 513 + 5)
SKEWS = (0, 1, 2, 3, 4)
KINDS = ("zero", "one", "flags", "random", "max", "last-of-tile", "first-of-next-tile")


@pytest.fixture(scope="module")
def E(engine):
    engine.InitializeInterface(1)
    return engine


def counts_of(kind, n):
    c = np.zeros(n, dtype=np.uint32)
    if n == 0:
        return c
    if kind == "one":
        c[:] = 1
    elif kind == "flags":
        c[:] = np.random.default_rng(n).random(n) < 0.03
    elif kind == "random":
        c[:] = np.random.default_rng(n + 1).integers(0, 1 << 32, n, dtype=np.uint64)
    elif kind == "max":
        c[:] = 0xFFFFFFFF
    elif kind == "last-of-tile":     # the last element of the last full tile (of the only, partial tile when n < 2048)
        c[(n // TILE) * TILE - 1 if n >= TILE else n - 1] = 0xFFFFFFFE
    elif kind == "first-of-next-tile":  # the first element of the last tile that has one
        c[((n - 1) // TILE) * TILE] = 0xFFFFFFFE
    return c


def reference(c):
    """-> uint64[n + 1]: 0, c[0], c[0] + c[1], ..., the total; the total is checked in Python integers (the largest here,
    (2048 * 513 + 5) * (2^32 - 1), is a little above 2^52 and far inside uint64)"""
    want = np.zeros(c.size + 1, dtype=np.uint64)
    np.cumsum(c, dtype=np.uint64, out=want[1:])
    assert int(want[-1]) == sum(c.tolist())
    return want


def hold(E, c, want, skew, width, what):
    out, intact = E.ScanCounts(c, skew=skew, width=width)
    assert intact == dict(temp_guard=True, out_guard=True, input=True), (what, intact)
    assert out.dtype == (np.uint64 if width == 64 else np.uint32) and out.shape == want.shape, what
    exp = want if width == 64 else (want & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if not np.array_equal(out, exp):
        bad = np.flatnonzero(out != exp)
        raise AssertionError((what, "first differences at", bad[:4].tolist(), out[bad[:4]].tolist(), exp[bad[:4]].tolist()))
    assert int(out[-1]) == int(want[-1]) % (1 << width), what


def cross(E, n, skews):
    for kind in (KINDS if n else KINDS[:1]):
        c = counts_of(kind, n)
        want = reference(c)
        if kind == "one":
            assert np.array_equal(want, np.arange(n + 1, dtype=np.uint64))
        if kind == "max" and n >= 2:
            assert int(want[2]) >= 1 << 32 and int(want[-1]) < 1 << 53
        if kind in ("last-of-tile", "first-of-next-tile"):
            assert np.count_nonzero(c) == 1
        for skew in skews:
            for width in (32, 64):
                hold(E, c, want, skew, width, (n, kind, skew, width))


@pytest.mark.parametrize("n", SMALL_N + LARGE_N[:1])
def test_scan_at_every_skew(E, n):
    cross(E, n, SKEWS)


@pytest.mark.parametrize("n", LARGE_N[1:])
def test_scan_across_trips_of_the_partials_loop(E, n):
    tiles = (n + TILE - 1) // TILE
    assert (tiles + PARTIALS - 1) // PARTIALS == {524288: 1, 524289: 2, TILE * 513 + 5: 3}[n]
    cross(E, n, (0, 1))


def test_the_single_counts_sit_on_either_side_of_a_tile_boundary():
    for n in SMALL_N[1:] + LARGE_N:
        a, b = np.flatnonzero(counts_of("last-of-tile", n)), np.flatnonzero(counts_of("first-of-next-tile", n))
        assert a.size == 1 and b.size == 1
        if n > TILE:
            assert a[0] % TILE == TILE - 1 and b[0] % TILE == 0 and b[0] >= TILE
        if n == TILE * 513 + 5:
            assert a[0] // TILE == 512 and b[0] // TILE == 513  # in the third trip of the partials loop


def test_a_later_call_does_not_depend_on_an_earlier_ones_scratch(E):
    """a large call, then a small one, then n = 0, in one process and both widths: each gets its own answer"""
    big = counts_of("max", LARGE_N[-1])
    small = counts_of("random", 9)
    none = counts_of("zero", 0)
    for width in (64, 32):
        for c, skew in ((big, 0), (small, 3), (none, 1), (small, 0), (none, 0)):
            hold(E, c, reference(c), skew, width, (c.size, skew, width))


CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
E.ScanCounts(np.ones(10, dtype=np.uint32), skew=%d, width=%d)
print("returned")
"""


@pytest.mark.parametrize("skew,width", [(8, 32), (0, 16)])
def test_bad_arguments_end_with_a_message(skew, width):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, skew, width)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout, r.stderr
    assert b"sa_scan_counts" in r.stderr
