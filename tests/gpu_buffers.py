"""Device buffers for the GPU tests (a plain helper module, no tests of its own)."""
import numpy as np
import torch


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
