"""Known answers of tests/guards.py itself: planted one-byte writes at the four extreme guard positions must fail `check` with the right
offsets, the alignment arithmetic must give "this alignment and no better", and `written` must tell a produced payload from a stale
one.  Without these the guard-band tests on the GPU could be vacuous.  No GPU needed: the device flavour runs over CPU torch tensors."""
import re

import numpy as np
import pytest
import torch

from ilgpu_raytracing_amd import _types as T
from tests import guards as G

# the (align, lead) pairs tests/test_guard_bands_gpu.py uses, (16, 16), (8, 8), (4, 4), and others of the arithmetic: a lead that is
# a multiple of align, no lead, the whole modulus
ALIGNMENTS = [(16, 16), (8, 8), (4, 4), (4, 12), (16, 0), (256, 0)]
SHAPES = [((1,), np.int32), ((65, 3), np.float32), ((257,), T.np_dtype(T.RayHit)), ((5, 16), T.np_dtype(T.RayHit)), ((4097, 8), np.float32)]
TORCH_DTYPE = {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


def _make(kind, shape, dtype, align, lead):
    """(buffer, writable flat uint8 view of the whole allocation, payload offset, payload bytes)"""
    if kind == "host":
        buf = G.host(shape, dtype, align, lead)
        whole, off, nbytes = G._whole(buf)
        return buf, whole, off, nbytes
    dt = np.dtype(dtype)
    if dt.names:                                       # records travel to the device as rows of 32-bit words
        shape, dt = tuple(shape) + (dt.itemsize // 4,), np.dtype(np.float32)
    buf = G.device(torch, shape, TORCH_DTYPE[dt], align, lead, device="cpu")
    _, off, nbytes = G._whole(buf)
    whole = torch.empty(0, dtype=torch.uint8).set_(buf.untyped_storage()).numpy()       # shares memory with the tensor
    return buf, whole, off, nbytes


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("shape,dtype", SHAPES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_planted_writes_are_found_with_their_offsets(kind, shape, dtype):
    buf, whole, off, nbytes = _make(kind, shape, dtype, 16, 16)
    G.check(buf, "fresh")                              # a fresh buffer passes
    assert G.untouched(buf) and not G.written(buf)
    back = whole.size - off - nbytes
    record = nbytes // shape[0]
    assert off >= G.MIN_GUARD and back >= G.MIN_GUARD and off >= G.MIN_RECORDS * record and back >= G.MIN_RECORDS * record
    plants = {
        "immediately before": (off - 1, r"-1 \.\. -1 bytes before the start \(1 bytes changed\)"),
        "immediately after": (off + nbytes, r"\+0 \.\. \+0 bytes after the end \(1 bytes changed\)"),
        "first byte of the front guard": (0, r"-%d \.\. -%d bytes before the start" % (off, off)),
        "last byte of the back guard": (whole.size - 1, r"\+%d \.\. \+%d bytes after the end" % (back - 1, back - 1)),
    }
    for name, (pos, pattern) in plants.items():
        whole[pos] = 0x5A
        with pytest.raises(AssertionError) as e:
            G.check(buf, name)
        assert re.search(pattern, str(e.value)) and name in str(e.value), str(e.value)
        whole[pos] = G.FILL
        G.check(buf, "restored")
    # one 48-byte record past the end, and both sides at once
    whole[off + nbytes:off + nbytes + 48] = 0
    whole[off - 12:off] = 0
    with pytest.raises(AssertionError) as e:
        G.check(buf, "record")
    assert "-12 .. -1 bytes before the start (12 bytes changed)" in str(e.value) and "+0 .. +47 bytes after the end (48 bytes changed)" in str(e.value)
    # a write to the payload is no guard failure
    whole[off - 12:off] = G.FILL
    whole[off + nbytes:off + nbytes + 48] = G.FILL
    whole[off:off + nbytes] = 0
    G.check(buf, "payload written")
    assert G.written(buf) and not G.untouched(buf)


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("align,lead", ALIGNMENTS)
def test_alignment_is_what_was_asked_for_and_no_better(kind, align, lead):
    for shape, dtype in SHAPES:
        for _ in range(3):                             # several allocations: the arithmetic must not depend on the base address
            buf, whole, off, nbytes = _make(kind, shape, dtype, align, lead)
            addr = buf.ctypes.data if kind == "host" else buf.data_ptr()
            assert addr % G.MODULUS == lead and addr % align == 0
            if lead == align and align < G.MODULUS:
                assert addr % (2 * align) != 0         # "16-byte aligned and no better"
            assert nbytes == int(np.prod(shape)) * np.dtype(dtype).itemsize
            assert (whole == G.FILL).all()             # payload and both sides pre-filled


def test_bad_alignment_requests_are_refused():
    for align, lead in [(3, 0), (16, 8), (16, 256), (0, 0), (16, -16)]:
        with pytest.raises(ValueError):
            G.host((4,), np.int32, align, lead)


def test_foreign_arrays_are_refused():
    with pytest.raises(ValueError):
        G.check(np.zeros(16, np.int32), "plain numpy")
    with pytest.raises(ValueError):
        G.check(torch.zeros(16, dtype=torch.int32), "plain torch")


@pytest.mark.parametrize("kind", ["host", "device"])
def test_written_sees_one_stale_word(kind):
    buf, whole, off, nbytes = _make(kind, (65, 3), np.float32, 4, 4)
    assert G.unwritten_words(buf) == 65 * 3
    buf[...] = 1.0
    assert G.written(buf) and G.unwritten_words(buf) == 0
    whole[off + nbytes - 4:off + nbytes] = G.FILL      # the last word stale: a tail that was not produced
    assert not G.written(buf) and G.unwritten_words(buf) == 1 and not G.untouched(buf)
    whole[off + nbytes - 4] = 0                        # three of four bytes: the word was written
    assert G.written(buf)
    G.check(buf, "after all that")


def test_views_of_a_guarded_buffer_are_checked_as_the_buffer():
    buf = G.host((9, 33), np.int32, 4, 4)
    row = buf[3]
    whole, off, nbytes = G._whole(row)
    assert nbytes == buf.nbytes
    whole[off + nbytes] ^= 0xFF
    with pytest.raises(AssertionError):
        G.check(row, "through a view")
