"""The guarded buffers of tests/helpers.py (guarded / Guarded.check) on CPU tensors: the alignment they promise, and that a byte written next
to the payload or at the far end of a guard is reported - the check the pointer-alignment GPU tests rely on can fail."""
import numpy as np
import pytest
import torch

from tests import helpers as T


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("offset", range(16))
def test_payload_alignment_and_prefill(offset, fill):
    view, h = T.guarded((3, 5, 7), offset, fill)
    assert view.data_ptr() % 256 == offset and view.shape == (3, 5, 7) and view.dtype == torch.uint8
    assert h.stop - h.start == 105 and h.start >= T.GUARD_BYTES + offset and h.buf.numel() - h.stop >= T.GUARD_BYTES
    assert (h.buf == fill).all()  # the payload of an output carries the fill too
    assert h.check() == []


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_untouched_buffer_with_contents_reports_nothing(fill):
    a = np.arange(60, dtype=np.uint8).reshape(3, 4, 5)
    view, h = T.guarded(a, 7, fill)
    assert np.array_equal(view.numpy(), a) and h.check() == []
    view[:] = 255 - fill  # writes inside the payload are not the guards' business
    assert h.check() == []


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("offset", [0, 1, 15])
def test_stray_bytes_are_reported(offset, fill):
    view, h = T.guarded(18, offset, fill)
    n = h.buf.numel()
    for where in (h.start - 1, h.stop, 0, n - 1, h.start - T.GUARD_BYTES, h.stop + T.GUARD_BYTES - 1):
        h.buf[where] = fill ^ 0x01
        assert h.check() == [where]
        h.buf[where] = fill
    h.buf[h.start - 1] = h.buf[h.stop] = 0x5A
    assert h.check() == [h.start - 1, h.stop]


def test_payload_view_aliases_the_allocation():
    view, h = T.guarded((4, 6), 3, 0xFF)
    assert view.data_ptr() == h.buf.data_ptr() + h.start
    view[1, 2] = 9
    assert int(h.buf[h.start + 8]) == 9
    h.buf[h.start] = 77
    assert int(view[0, 0]) == 77 and h.check() == []


def test_wider_elements_and_tensors():
    src = torch.arange(10, dtype=torch.int16)
    view, h = T.guarded(src, 2, 0x00)
    assert view.dtype == torch.int16 and view.data_ptr() % 256 == 2 and torch.equal(view, src) and h.stop - h.start == 20
    out, g = T.guarded((2, 3), 8, 0xFF, dtype=np.int32)
    assert out.dtype == torch.int32 and (out == -1).all() and g.check() == []
    with pytest.raises(AssertionError):
        T.guarded(src, 1, 0x00)  # a 16-bit payload cannot start at an odd byte
