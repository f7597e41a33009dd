"""Self-tests of gpu_buffers.guarded (torch ops only, no library call): a write just outside the
payload trips check_guards(), an element never assigned shows in unwritten().  Without these a
broken helper would let every guarded test pass."""
import struct

import pytest
import torch

from gpu_buffers import GUARD_BYTES, SENTINEL, guarded

pytestmark = pytest.mark.gpu


def write_float(g, byte_offset, value=1.0):
    """One fp32 stored through the underlying allocation at `byte_offset` from the payload's start."""
    raw = torch.frombuffer(bytearray(struct.pack("<f", value)), dtype=torch.uint8).cuda()
    o = g.start + byte_offset
    g.buf[o:o + 4] = raw


@pytest.mark.parametrize("shape,dtype", [((3, 5), torch.float32), ((7,), torch.int32), ((2, 3), torch.float64),
                                         ((594,), torch.uint8), ((0, 4), torch.float32)])
def test_layout(shape, dtype):
    g = guarded(shape, dtype)
    assert g.t.shape == shape and g.t.dtype == dtype and g.t.is_contiguous()
    assert g.address % 256 == 16
    assert g.nbytes == g.t.numel() * g.t.element_size() and g.stop - g.start == g.nbytes
    assert g.start >= GUARD_BYTES and g.buf.numel() - g.stop >= GUARD_BYTES
    if g.nbytes:
        assert g.t.data_ptr() == g.address
    words = g.buf.view(torch.int32)
    assert bool((words == SENTINEL).all())
    g.check_guards()
    if dtype != torch.uint8:
        assert bool(g.unwritten().all())
    if dtype == torch.float32:
        assert bool(torch.isnan(g.t).all())
        assert not bool((g.t.view(torch.int32) == 0x7FC00000).any())  # not the kernels' canonical NaN
    if dtype == torch.float64:
        assert bool(torch.isnan(g.t).all())
        assert bool(torch.isnan(g.buf[g.start + 4:g.start + 20].clone().view(torch.float64)).all())  # the other pairing
    if dtype == torch.int32:
        assert SENTINEL == 2147001765 and bool((g.t == SENTINEL).all())  # outside every index range


def test_offset_payload_is_four_bytes_past_a_16_byte_boundary():
    g = guarded((3, 5), torch.float32, fill=7.0, offset=True)
    assert g.address % 256 == 20 and g.t.data_ptr() % 16 == 4 and g.t.is_contiguous()
    g.check_guards()
    write_float(g, g.nbytes)
    with pytest.raises(AssertionError, match="back guard"):
        g.check_guards()
    g = guarded((3, 5), torch.int32, offset=True)
    write_float(g, -4)
    with pytest.raises(AssertionError, match="front guard"):
        g.check_guards()


def test_write_after_payload_trips_the_back_guard():
    g = guarded((3, 5), torch.float32, fill=7.0)
    g.check_guards()
    write_float(g, g.nbytes)
    with pytest.raises(AssertionError, match=f"back guard overwritten: first changed byte at offset {g.nbytes} "):
        g.check_guards()


def test_write_before_payload_trips_the_front_guard():
    g = guarded((3, 5), torch.float32, fill=7.0)
    write_float(g, -4)  # its last byte is the byte just before the payload
    with pytest.raises(AssertionError, match="front guard overwritten: first changed byte at offset -4 "):
        g.check_guards()
    g = guarded((3, 5), torch.float32)
    g.buf[g.start - 1] = 0
    with pytest.raises(AssertionError, match="first changed byte at offset -1 "):
        g.check_guards()


def test_far_ends_of_the_guards_are_checked():
    g = guarded((4,), torch.float32)
    g.buf[g.stop + GUARD_BYTES - 1] = 0
    with pytest.raises(AssertionError, match=f"offset {g.nbytes + GUARD_BYTES - 1} "):
        g.check_guards()
    g = guarded((4,), torch.float32)
    g.buf[g.start - GUARD_BYTES] = 0
    with pytest.raises(AssertionError, match=f"offset {-GUARD_BYTES} "):
        g.check_guards()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.float64])
def test_unassigned_element_shows_in_unwritten(dtype):
    g = guarded((4, 6), dtype)
    g.t[:] = 0
    assert not bool(g.unwritten().any())
    g = guarded((4, 6), dtype)
    keep = torch.ones(4, 6, dtype=torch.bool, device="cuda")
    keep[2, 5] = False
    g.t[keep] = 0  # every element but (2, 5)
    assert g.unwritten().nonzero().tolist() == [[2, 5]]
    g.check_guards()


def test_writes_inside_the_payload_leave_the_guards_alone():
    g = guarded((5,), torch.float32)
    write_float(g, 0)
    write_float(g, g.nbytes - 4)
    g.check_guards()
    assert g.unwritten().tolist() == [False, True, True, True, False]
    g.poison(0x3C)
    assert not bool(g.unwritten().any()) and bool((g.buf[g.start:g.stop] == 0x3C).all())
    g.check_guards()
    g.poison()
    assert bool(g.unwritten().all())
