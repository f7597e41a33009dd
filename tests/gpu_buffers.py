"""Device buffers for the GPU tests (a plain helper module; its self-tests are in test_gpu_buffers.py).

offset_view: inputs 4 bytes past a 16-byte boundary (the kernels' scalar load paths).

guarded: outputs and workspaces for the C-ABI tests of the memory contract (every output element is
written, nothing is written outside an output or the workspace, no result depends on what the
workspace held).  One uint8 allocation laid out as

    front guard (>= 8 KiB) | payload (exactly numel * itemsize bytes) | back guard (8 KiB)

every byte of which starts as the repeating 32-bit word 0x7FF8A5A5: a quiet NaN as fp32, a NaN as
fp64 whichever way two words pair up, 2147001765 as int32 (outside every index range), and not the
canonical NaN 0x7FC00000 the kernels write for logZ of an empty sequence, so a payload element that
still holds it was not written.  The payload starts 16 bytes past a 256-byte boundary: the weakest
alignment include/vqhmm.h allows for outputs and workspaces.  The back guard starts at the very next
byte after the payload (a workspace size is not rounded up).  The guards are 8 KiB: twice the widest
store a 256-thread workgroup issues (256 x 16 B)."""
import ctypes

import numpy as np
import torch

SENTINEL = 0x7FF8A5A5
GUARD_BYTES = 8192
_WORD = np.array([SENTINEL], np.uint32).view(np.uint8)  # the sentinel's bytes in memory order


def offset_view(a):
    """A contiguous device copy of `a` (numpy array or tensor) whose data pointer is 4 bytes past a
    16-byte boundary: element 1 onward of an allocation one element larger.  `.contiguous()` returns
    such a view unchanged, so the kernels see the misaligned pointer."""
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    assert a.element_size() == 4
    buf = torch.empty(a.numel() + 1, dtype=a.dtype, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(a)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


class Guarded:
    """See guarded().  buf: the whole uint8 allocation; start / nbytes: the payload's byte range in
    it; t: the payload as a tensor; ptr: the payload's address (valid for an empty payload too, where
    torch reports a null data pointer)."""

    def __init__(self, shape, dtype, fill=None, offset=False):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * item
        total = (GUARD_BYTES + 256 + 20 + self.nbytes + GUARD_BYTES + 3) // 4 * 4
        self.buf = torch.empty(total, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        assert base % 16 == 0
        self.buf.view(torch.int32).fill_(SENTINEL)
        lead = 16 + (4 if offset else 0)
        assert item == 4 or not offset
        self.start = GUARD_BYTES + (lead - (base + GUARD_BYTES)) % 256
        self.stop = self.start + self.nbytes
        assert (base + self.start) % 256 == lead and self.stop + GUARD_BYTES <= total
        self.address = base + self.start
        self.t = self.buf[self.start:self.stop].view(dtype).view(shape)
        assert self.nbytes == 0 or self.t.data_ptr() == self.address
        if fill is not None:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.address)

    def _pattern(self):
        return torch.from_numpy(np.tile(_WORD, self.buf.numel() // 4)).cuda()

    def check_guards(self):
        """Both guards still hold the sentinel (compared on the device); else fails with the offset
        of the first changed byte relative to the payload (negative: in front of it; >= nbytes: behind)."""
        bad = self.buf != self._pattern()
        bad[self.start:self.stop] = False
        if bool(bad.any()):
            off = int(bad.nonzero()[0, 0])
            where = "front" if off < self.start else "back"
            raise AssertionError(f"{where} guard overwritten: first changed byte at offset {off - self.start} "
                                 f"from the payload's start (payload of {self.nbytes} bytes, shape "
                                 f"{tuple(self.t.shape)} {self.t.dtype}), {int(bad.sum())} guard bytes changed")

    def unwritten(self):
        """Mask (payload's shape) of the elements whose bits still equal the sentinel."""
        item = self.t.element_size()
        raw = self.buf[self.start:self.stop]
        if item == 4:
            m = raw.view(torch.int32) == SENTINEL
        elif item == 8:
            m = raw.view(torch.int64) == (SENTINEL << 32 | SENTINEL)
        else:
            raise TypeError(f"unwritten(): 4- and 8-byte element types only, not {self.t.dtype}")
        return m.view(self.t.shape)

    def poison(self, byte=None):
        """The payload back to the sentinel, or (byte given) every payload byte to that value."""
        if byte is None:
            self.buf[self.start:self.stop] = self._pattern()[self.start:self.stop]
        else:
            self.buf[self.start:self.stop] = byte
        return self


def guarded(shape, dtype, fill=None, offset=False):
    """A guarded, sentinel-poisoned device buffer of `shape` / `dtype` (module docstring); `fill`
    overwrites the payload.  A workspace of n bytes is guarded(n, torch.uint8).  offset (4-byte
    element types): the payload starts 4 bytes further on, as offset_view's does, for the entries
    whose header allows 4-byte-aligned outputs; the guards go around that view."""
    return Guarded(shape, dtype, fill, offset)


def check_all(*bufs):
    """Synchronize, then check_guards() on every Guarded among `bufs` (None entries are skipped)."""
    torch.cuda.synchronize()
    for g in bufs:
        if g is not None:
            g.check_guards()
