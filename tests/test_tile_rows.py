"""tests/tile_rows.py against a second formulation (strips dealt with counters, no modulo arithmetic), against the package's own
tiling.strip_rows and tiling.partition_rows, and its partition property: the sn * slots tiles of a range are pairwise disjoint and
their union is the range.  No GPU."""
import itertools

import numpy as np
import pytest

from ilgpu_raytracing_amd import tiling
from tests import tile_rows as TR

HEIGHTS = [1, 7, 8, 9, 21, 40, 125]
STRIPS = [1, 2, 3, 5]
SLOTS = [1, 2, 3]


def ranges(h):
    """Whole image, single rows at both ends, every begin 0..9 with a few ends, and ranges around multiples of 8."""
    out = {None, (0, 0), (0, h), (0, 1), (h - 1, h)}
    for rb in range(min(h, 10)):
        for re in (rb + 1, rb + 7, rb + 8, rb + 9, rb + 17, h - 1, h):
            if rb < re <= h:
                out.add((rb, re))
    for m in range(8, h, 8):
        for rb, re in ((m - 1, m), (m, m + 1), (m - 3, h), (3, m), (5, m + 5)):
            if 0 <= rb < re <= h:
                out.add((rb, re))
    return sorted(out, key=lambda r: (-1, -1) if r is None else r)


def dealt_with_counters(height, rows, strips, slots, slot):
    """The same ownership, restated as dealing: walk the rows of the range, open a new strip every 8 rows, hand the strips to the
    sn calls in turn, and each call's strips to its slots in turn."""
    rb, re = (0, height) if rows is None or tuple(rows) == (0, 0) else rows
    sn, si = (1, 0) if strips is None else strips
    call, turn, left = 0, [0] * sn, 0            # whose strip this is; per call: which slot is next; rows left in the open strip
    owner = None
    out = []
    for y in range(rb, re):
        if left == 0:
            owner = (call, turn[call])
            turn[call] += 1
            if turn[call] == slots:
                turn[call] = 0
            call += 1
            if call == sn:
                call = 0
            left = 8
        left -= 1
        if owner == (si, slot):
            out.append(y)
    return np.asarray(out, np.int64)


@pytest.mark.parametrize("h", HEIGHTS)
def test_equals_dealing_with_counters(h):
    n = 0
    for rows in ranges(h):
        S = TR.strip_count(h, rows)
        for sn in STRIPS + [S + 1]:
            for slots in SLOTS:
                for si, j in itertools.product(range(sn), range(slots)):
                    got = TR.owned_rows(h, rows, (sn, si), slots, j)
                    want = dealt_with_counters(h, rows, (sn, si), slots, j)
                    assert got.dtype == np.int64 and np.array_equal(got, want), (h, rows, sn, si, slots, j)
                    n += 1
    assert n > 100


@pytest.mark.parametrize("h", HEIGHTS)
def test_tiles_partition_the_range(h):
    for rows in ranges(h):
        rb, re = (0, h) if rows in (None, (0, 0)) else rows
        S = TR.strip_count(h, rows)
        for sn in STRIPS + [S + 1]:
            for slots in SLOTS:
                tiles = [TR.owned_rows(h, rows, (sn, si), slots, j) for si in range(sn) for j in range(slots)]
                allrows = np.concatenate(tiles)
                assert len(allrows) == re - rb, "tiles overlap or leave rows out: %s" % ((h, rows, sn, slots),)
                assert np.array_equal(np.sort(allrows), np.arange(rb, re)), (h, rows, sn, slots)
                for t in tiles:
                    assert np.array_equal(t, np.sort(t))
                for si in range(sn):               # the call's rows are the union of its slots', and do not depend on the slot count
                    call = TR.call_rows(h, rows, (sn, si), slots)
                    assert np.array_equal(call, np.sort(np.concatenate(tiles[si * slots:(si + 1) * slots])))
                    assert np.array_equal(call, TR.owned_rows(h, rows, (sn, si)))


@pytest.mark.parametrize("h", HEIGHTS)
def test_empty_tiles(h):
    """A tile is empty exactly when its first strip, si + sn * j, does not exist."""
    empties = 0
    for rows in ranges(h):
        S = TR.strip_count(h, rows)
        assert S == len(range(0, (h if rows in (None, (0, 0)) else rows[1] - rows[0]), 8))
        for sn in STRIPS + [S + 1]:
            for slots in SLOTS:
                for si, j in itertools.product(range(sn), range(slots)):
                    empty = len(TR.owned_rows(h, rows, (sn, si), slots, j)) == 0
                    assert empty == (si + sn * j >= S) == TR.owns_nothing(h, rows, (sn, si), slots, j), (h, rows, sn, si, slots, j)
                    empties += empty
        # S + 1 calls on one slot: S tiles of one strip each, and one empty tile
        sizes = [len(TR.owned_rows(h, rows, (S + 1, si))) for si in range(S + 1)]
        assert sizes[S] == 0 and all(0 < n <= 8 for n in sizes[:S]) and sizes[:S - 1] == [8] * (S - 1)
    assert empties > 0


def test_known_answers():
    assert TR.owned_rows(125, (13, 14), (3, 2)).tolist() == []
    assert TR.owned_rows(125, (13, 14), (3, 0)).tolist() == [13]
    assert TR.owned_rows(125, (3, 125), (3, 1)).tolist() == [y for s in (1, 4, 7, 10, 13) for y in range(3 + 8 * s, 11 + 8 * s)]
    assert TR.strip_count(125, (3, 125)) == 16 and TR.owned_rows(125, (3, 125), (16, 15)).tolist() == [123, 124]      # ragged: 2 rows
    assert TR.strip_count(125, (5, 77)) == 9 and TR.owned_rows(125, (5, 77), (5, 3), 1, 0).tolist() == list(range(29, 37)) + list(range(69, 77))
    assert TR.owned_rows(40, None, (2, 1), 2, 1).tolist() == list(range(24, 32))                    # strip 3 of 5: si + sn * j = 3
    assert TR.owned_rows(21, (2, 21), None, 3, 2).tolist() == [18, 19, 20]
    for bad in (dict(rows=(5, 4)), dict(rows=(0, 126)), dict(rows=(-1, 4)), dict(strips=(2, 2)), dict(strips=(0, 0)), dict(slots=2, slot=2)):
        kw = dict(rows=None, strips=None, slots=1, slot=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            TR.owned_rows(125, kw["rows"], kw["strips"], kw["slots"], kw["slot"])


@pytest.mark.parametrize("h", HEIGHTS)
def test_whole_image_strips_equal_tiling_strip_rows(h):
    for n in STRIPS + [8, 17]:
        for i in range(n):
            want = tiling.strip_rows(h, n, i)
            for rows in (None, (0, 0), (0, h)):
                assert np.array_equal(TR.owned_rows(h, rows, (n, i)), want), (h, n, i, rows)
            assert np.array_equal(TR.owned_rows(h, None, None, n, i), want), (h, n, i)     # a context's slots deal strips the same way
    for sn, slots in ((2, 2), (3, 2), (2, 3)):                                              # strips of a call, dealt again among slots
        for si in range(sn):
            for j in range(slots):
                assert np.array_equal(TR.owned_rows(h, None, (sn, si), slots, j), tiling.strip_rows(h, sn * slots, si + sn * j))


@pytest.mark.parametrize("h", HEIGHTS)
def test_partition_rows_blocks_as_row_ranges(h):
    """tiling.partition_rows deals contiguous blocks on the 8-row grid: passed as `rows` they tile the image, and strips inside a
    block lie on the image's own 8-row grid (so they are strips of the whole image too)."""
    for world in (1, 2, 3, 5):
        blocks = [tiling.partition_rows(h, world, r) for r in range(world)]
        got = []
        for rb, re in blocks:
            assert rb % 8 == 0 and 0 <= rb <= re <= h
            if rb == re:
                continue                              # more ranks than strips: (rb, rb) with rb > 0 is an empty range (0, 0 means all rows)
            rows = TR.call_rows(h, (rb, re), None)
            assert np.array_equal(rows, np.arange(rb, re))
            got.append(rows)
            for sn in (2, 3):
                for si in range(sn):
                    mine = TR.owned_rows(h, (rb, re), (sn, si))
                    assert all(len(set(y // 8 for y in mine[k:k + 8])) == 1 for k in range(0, len(mine), 8))
                    whole = [tiling.strip_rows(h, 1, 0)[s * 8:s * 8 + 8] for s in range(rb // 8 + si, (re + 7) // 8, sn)]
                    assert np.array_equal(mine, np.concatenate(whole) if whole else np.zeros(0, np.int64))
        assert np.array_equal(np.concatenate(got), np.arange(h))
