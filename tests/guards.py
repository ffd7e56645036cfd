"""Guard bands around caller memory: a destination (or an input) handed to the C ABI is the middle of a larger allocation whose both
sides, and the payload itself, are pre-filled with the byte 0xA5.  After the call `check` reads every guard byte back: an entry point
that writes one record, one row or one block past what its contract names shows up as changed bytes, never as a fault.  `written`
says whether the whole payload was produced.  The guards hold nothing else, ever.

The payload's address is congruent to `lead` modulo 256 (`lead` a multiple of `align`), so a test can ask for the weakest alignment
the header allows ("16-byte aligned and no better": align = lead = 16) instead of whatever numpy or torch return.

tests/test_guards.py holds this module's own known answers (planted writes, the alignment arithmetic); it needs no GPU."""
import numpy as np

FILL = 0xA5
FILL_WORD = 0xA5A5A5A5
MIN_GUARD = 256 * 1024          # bytes on each side, at least
MIN_RECORDS = 256               # ... and at least this many records of the buffer itself: a block-sized tail stays inside
MODULUS = 256

_HOST = {}                      # address of the whole allocation -> (its length, payload offset, payload bytes)
_DEVICE = {}                    # the same, keyed by (device index, address of the storage)


def _layout(shape, itemsize, align, lead, base_addr):
    """(total bytes, payload offset, payload bytes, guard bytes) of an allocation that starts at base_addr."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    if align <= 0 or MODULUS % align or lead % align or not 0 <= lead < MODULUS:
        raise ValueError("align must divide %d and lead must be a multiple of align below %d: align=%r lead=%r" % (MODULUS, MODULUS, align, lead))
    nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
    record = int(np.prod(shape[1:], dtype=np.int64)) * itemsize
    guard = max(MIN_GUARD, MIN_RECORDS * record)
    guard = (guard + MODULUS - 1) // MODULUS * MODULUS
    off = guard + (lead - (base_addr + guard)) % MODULUS          # first offset >= guard whose address is lead modulo 256
    return off + nbytes + guard, off, nbytes, guard


def host(shape, dtype, align, lead=0):
    """A numpy array of `shape` / `dtype` (structured dtypes included) in the middle of a larger uint8 allocation.  Payload and both
    guards hold 0xA5; address % 256 == lead; each guard is at least 256 KiB and at least 256 records (a record = one element of
    axis 0) long."""
    dt = np.dtype(dtype)
    probe, _, _, _ = _layout(shape, dt.itemsize, align, lead, 0)
    whole = np.full(probe + MODULUS, FILL, np.uint8)               # + 256: room for the alignment shift at any base address
    total, off, nbytes, _ = _layout(shape, dt.itemsize, align, lead, whole.ctypes.data)
    assert total <= whole.size
    _HOST[whole.ctypes.data] = (whole.size, off, nbytes)
    out = whole[off:off + nbytes].view(dt).reshape(shape)
    assert out.ctypes.data % MODULUS == lead and out.ctypes.data == whole.ctypes.data + off
    return out


def device(torch, shape, dtype, align, lead=0, device="cuda:0"):
    """The same over one torch.uint8 tensor on `device`: returns the interior tensor (torch dtype `dtype`), which shares storage
    with the whole.  The device is synchronized before it returns, so the fill is in memory before any other stream can write."""
    itemsize = torch.empty(0, dtype=dtype).element_size()
    probe, _, _, _ = _layout(shape, itemsize, align, lead, 0)
    whole = torch.full((probe + MODULUS,), FILL, dtype=torch.uint8, device=device)
    total, off, nbytes, _ = _layout(shape, itemsize, align, lead, whole.data_ptr())
    assert total <= whole.numel()
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    out = whole[off:off + nbytes].view(dtype).reshape(shape)
    assert out.data_ptr() % MODULUS == lead and out.data_ptr() == whole.data_ptr() + off
    _DEVICE[(whole.device.index, whole.data_ptr())] = (whole.numel(), off, nbytes)
    if whole.device.type == "cuda":                    # the fill ran on torch's stream; the library works on streams of its own that
        torch.cuda.synchronize(whole.device)           # do not wait for it: a fill that lands after the call would hide an overrun
    return out


def _is_torch(buf):
    return type(buf).__module__.split(".")[0] == "torch"


def _whole(buf):
    """(whole allocation as a flat uint8 numpy array, payload offset, payload bytes) of a buffer host() or device() returned (or of a
    view of one).  A device buffer is read back after torch.cuda.synchronize."""
    if _is_torch(buf):
        import torch
        if buf.device.type == "cuda":
            torch.cuda.synchronize(buf.device)
        st = buf.untyped_storage()
        meta = _DEVICE.get((buf.device.index, st.data_ptr()))
        if meta is None or meta[0] != st.nbytes():
            raise ValueError("not a buffer of guards.device()")
        flat = torch.empty(0, dtype=torch.uint8, device=buf.device).set_(st)
        return flat.cpu().numpy(), meta[1], meta[2]
    a = buf
    while a.base is not None:
        a = a.base
    meta = _HOST.get(a.ctypes.data) if isinstance(a, np.ndarray) else None
    if meta is None or a.dtype != np.uint8 or a.ndim != 1 or meta[0] != a.size:
        raise ValueError("not a buffer of guards.host()")
    return a, meta[1], meta[2]


def check(buf, what):
    """Asserts that every guard byte of `buf` still holds 0xA5.  The failure names the first and last touched offsets relative to
    the payload: '+0 .. +47 bytes after the end' is one 48-byte record, a row or a block look different."""
    whole, off, nbytes = _whole(buf)
    problems = []
    front = np.flatnonzero(whole[:off] != FILL)
    if front.size:
        problems.append("%d .. %d bytes before the start (%d bytes changed)" % (int(front[0]) - off, int(front[-1]) - off, front.size))
    back = np.flatnonzero(whole[off + nbytes:] != FILL)
    if back.size:
        problems.append("+%d .. +%d bytes after the end (%d bytes changed)" % (int(back[0]), int(back[-1]), back.size))
    assert not problems, "%s: guard touched at %s; payload of %d bytes" % (what, " and ".join(problems), nbytes)


def _payload_words(buf):
    whole, off, nbytes = _whole(buf)
    return np.ascontiguousarray(whole[off:off + nbytes - nbytes % 4]).view(np.uint32)


def unwritten_words(buf):
    """Number of 4-byte words of the payload that still hold 0xA5A5A5A5."""
    return int(np.count_nonzero(_payload_words(buf) == FILL_WORD))


def written(buf):
    """True when no 4-byte word of the payload still holds 0xA5A5A5A5: the whole payload was produced."""
    return unwritten_words(buf) == 0


def untouched(buf):
    """True when every byte of the payload still holds 0xA5: nothing was written."""
    whole, off, nbytes = _whole(buf)
    return bool((whole[off:off + nbytes] == FILL).all())
