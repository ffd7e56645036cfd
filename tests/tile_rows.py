"""Which rows of a frame a call owns: a restatement of the tile rules of include/hip_raytrace.h (hrt_render_opts, hrt_device_views),
written from the header's words and independent of the arithmetic in csrc/hrt_runtime.hip and the pixel kernels.

A call names a row range [row_begin, row_end) (0, 0: all rows).  The range is cut into 8-row strips counted from row_begin: strip s
holds rows row_begin + 8 s .. row_begin + 8 s + 7, the last one only what is left below row_end.  The call owns the strips s with
s % strip_n == strip_i.  A context over `slots` device slots deals the call's strips again: slot j takes every slots-th of them,
starting with the call's j-th.  Together: row y of [rb, re) belongs to slot j iff ((y - rb) // 8) % (sn * slots) == si + sn * j.

tests/test_tile_rows.py holds this module's own checks (a second formulation with counters, tiling.strip_rows, tiling.partition_rows);
it needs no GPU."""
import numpy as np

STRIP = 8


def _range(height, rows):
    rb, re = (0, 0) if rows is None else (int(rows[0]), int(rows[1]))
    if rb == 0 and re == 0:
        re = height
    if not 0 <= rb <= re <= height:
        raise ValueError("row range %r outside an image of %d rows" % (rows, height))
    return rb, re


def _strips(strips):
    sn, si = (1, 0) if strips is None else (int(strips[0]), int(strips[1]))
    if sn < 1 or not 0 <= si < sn:
        raise ValueError("strips %r: strip_i must be in [0, strip_n)" % (strips,))
    return sn, si


def strip_count(height, rows):
    """S: the number of 8-row strips of the range, the last one possibly ragged."""
    rb, re = _range(height, rows)
    return (re - rb + STRIP - 1) // STRIP


def owned_rows(height, rows, strips, slots=1, slot=0):
    """Sorted rows (int64 array) that slot `slot` of a context over `slots` device slots owns in a call with rows=(rb, re) (None or
    (0, 0): all rows) and strips=(sn, si) (None: (1, 0))."""
    rb, re = _range(height, rows)
    sn, si = _strips(strips)
    if slots < 1 or not 0 <= slot < slots:
        raise ValueError("slot %r of %r" % (slot, slots))
    y = np.arange(rb, re, dtype=np.int64)
    return y[((y - rb) // STRIP) % (sn * slots) == si + sn * slot]


def call_rows(height, rows, strips, slots=1):
    """Sorted rows the whole call owns: the union over the slots of its context."""
    parts = [owned_rows(height, rows, strips, slots, j) for j in range(slots)]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.int64)


def owns_nothing(height, rows, strips, slots=1, slot=0):
    """The header's "a call may own no strip": true iff the first strip of the slot, si + sn * slot, lies past the last strip."""
    sn, si = _strips(strips)
    return si + sn * slot >= strip_count(height, rows)
