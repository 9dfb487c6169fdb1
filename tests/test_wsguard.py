"""tests/wsguard.py on the CPU: the helper that holds the workspaces of the GPU tests between guards must itself report a byte
written next to the region, and must find the highest byte a call wrote."""
import numpy as np
import pytest
import torch

import wsguard
from wsguard import G, GuardedBytes

CPU = torch.device("cpu")


@pytest.mark.parametrize("fill", wsguard.FILLS)
def test_layout_and_fill(fill):
    g = GuardedBytes(1000, CPU, fill, seed=3)
    assert g.mid.numel() == 1000 and g.mid.data_ptr() % 256 == 0 and g.mid.dtype == torch.uint8
    assert g.off >= G and g.buf.numel() - g.off - 1000 >= G
    want = wsguard.fill_bytes(fill, g.buf.numel(), 3)
    assert (g.buf.numpy() == want).all()
    if fill == "seeded":
        assert len(np.unique(want[:4096])) > 200                                            # bytes of every value
        assert (want == wsguard.fill_bytes(fill, g.buf.numel(), 3)).all()                    # the seed decides them
        assert (want[:4096] != wsguard.fill_bytes(fill, 4096, 4)).mean() > 0.9
    else:
        assert (want == (0xFF if fill == "ff" else 0)).all()


@pytest.mark.parametrize("fill", wsguard.FILLS)
def test_untouched_buffer_is_intact(fill):
    g = GuardedBytes(777, CPU, fill)
    g.mid.fill_(0x5A)                  # (writing all of the middle is what the library is allowed to do)
    c = g.intact()
    assert c and c.count == 0 and c.first is None
    g.check("untouched")


@pytest.mark.parametrize("fill", wsguard.FILLS)
def test_one_byte_behind_the_middle_is_reported(fill):
    g = GuardedBytes(777, CPU, fill)
    g.buf[g.off + 777] ^= 0x01         # mid[-1] + 1
    c = g.intact()
    assert not c and (c.first, c.last, c.count) == (777, 777, 1)
    with pytest.raises(AssertionError, match="777"):
        g.check("one byte behind")


@pytest.mark.parametrize("fill", wsguard.FILLS)
def test_one_byte_in_front_of_the_middle_is_reported(fill):
    g = GuardedBytes(777, CPU, fill)
    g.buf[g.off - 1] ^= 0x80           # mid[0] - 1
    c = g.intact()
    assert not c and (c.first, c.last, c.count) == (-1, -1, 1)


def test_first_and_last_changed_offset_and_the_far_ends():
    g = GuardedBytes(512, CPU, "seeded")
    g.buf[0] ^= 0xFF
    g.buf[-1] ^= 0xFF
    g.buf[g.off + 512 + 300] ^= 0xFF
    c = g.intact()
    assert (c.first, c.last, c.count) == (-g.off, g.buf.numel() - 1 - g.off, 3)
    g.restore()
    assert g.intact()


def test_span_reaches_into_the_guard_and_the_helper_sees_it():
    g = GuardedBytes(512, CPU, "zero")
    s = g.span(512 + 256)
    assert s.data_ptr() == g.mid.data_ptr() and s.numel() == 768
    s[-1] = 7
    c = g.intact()
    assert (c.first, c.last) == (767, 767)
    with pytest.raises(AssertionError):
        g.span(512 + G + 1)


def test_highest_written_on_a_hand_made_example():
    a, b = GuardedBytes(1000, CPU, "ff"), GuardedBytes(1000, CPU, "zero")
    assert a.highest_written(b) == -1 and b.highest_written(a) == -1
    # "the call" writes 0xFF at 10 and 600 and 0x00 at 20 and 700: each run shows only the bytes that differ from its own fill
    for g in (a, b):
        g.mid[10] = 0xFF
        g.mid[600] = 0xFF
        g.mid[20] = 0
        g.mid[700] = 0
    assert np.nonzero(a.written())[0].tolist() == [20, 700] and np.nonzero(b.written())[0].tolist() == [10, 600]
    assert a.highest_written(b) == 700 and b.highest_written(a) == 700
    b.mid[999] = 1
    assert a.highest_written(b) == 999
    with pytest.raises(AssertionError):
        a.highest_written(GuardedBytes(1000, CPU, "ff"))          # the same fill twice sees nothing new
    with pytest.raises(AssertionError):
        a.highest_written(GuardedBytes(999, CPU, "zero"))


def test_empty_region():
    g = GuardedBytes(0, CPU, "seeded")
    assert g.mid.numel() == 0 and g.intact()
    g.buf[g.off] ^= 1
    assert g.intact().first == 0
