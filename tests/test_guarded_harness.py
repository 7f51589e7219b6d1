"""Negative controls of tests/guarded.py on the CPU (no faulty kernel needed): each kind of bug the guarded-memory tests look for,
committed here by torch code, is caught."""
import pytest
import torch

from guarded import GUARD, NAN16, NAN32, Arena


def test_layout_alignment_and_fills():
    a = Arena(device="cpu")
    x = a.guarded((3, 5), torch.float32, name="x")
    y = a.guarded((7,), torch.bfloat16, name="y")
    i = a.guarded((9,), torch.int32, name="idx")
    for t, raw in ((x, a.buffers[0][1]), (y, a.buffers[1][1]), (i, a.buffers[2][1])):
        off = t.data_ptr() - raw.data_ptr()
        assert off == GUARD and t.is_contiguous()
        # the tail guard starts at the byte after the last element: no rounding gap
        assert raw.numel() * raw.element_size() == 2 * GUARD + t.numel() * t.element_size()
    assert torch.isnan(x).all() and torch.isnan(y).all()                  # outputs start NaN: unwritten elements show
    assert int(x.view(torch.int32)[0, 0]) == NAN32 and int(y.view(torch.int16)[0]) == NAN16
    assert (i == 0).all() and (a.buffers[2][1] == 0).all()                # integer guards: a valid index, never a NaN pattern
    # the bf16 guard stays NaN through round-to-nearest-even f2bf of its fp32 twin, and so does the fp32 one
    for bits in (NAN32, NAN16 << 16):
        u = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffffffff
        assert (u >> 16) & 0x7f80 == 0x7f80 and (u >> 16) & 0x7f
    a.check_guards()


def test_write_into_a_guard_is_caught():
    a = Arena(device="cpu")
    x = a.guarded((4, 6), torch.float32, "zero", name="sink")
    raw = a.buffers[0][1]
    lo = a.buffers[0][2]
    raw[lo + x.numel()] = 1.0                                              # one element past the end, through the base tensor
    with pytest.raises(AssertionError, match=r"sink: tail guard changed at element \+0"):
        a.check_guards()
    b = Arena(device="cpu")
    y = b.guarded((8,), torch.bfloat16, "zero", name="y")
    b.buffers[0][1][b.buffers[0][2] - 3] = 0.0                              # before the start
    with pytest.raises(AssertionError, match="y: head guard changed at element -3"):
        b.check_guards()
    del y


def test_read_past_the_end_is_caught():
    a = Arena(device="cpu")
    x = a.guarded_copy(torch.ones(10), "x")
    raw, lo = a.buffers[0][1], a.buffers[0][2]
    assert torch.isfinite(x.sum())
    widened = raw[lo:lo + x.numel() + 1]                                   # a view widened by one element
    assert torch.isnan(widened.sum())
    i = a.guarded_copy(torch.arange(10, dtype=torch.int32), "idx")
    iraw, ilo = a.buffers[1][1], a.buffers[1][2]
    assert int(iraw[ilo + 10]) == 0                                         # an index read past the list: a valid index (0)


def test_exact_workspace_and_unwritten_scratch_words():
    a = Arena(ws_fill="nan", device="cpu")
    ws = a.workspace(40, torch.device("cpu"))
    assert ws.numel() == 40                                                # exactly the requested size
    f = ws.view(torch.float32)
    f[:9] = 2.0                                                            # a "kernel" writes 9 of its 10 words ...
    assert torch.isnan(f.sum())                                            # ... and reads the tenth: NaN
    a.buffers[0][1][a.buffers[0][2] + 40] = 7                              # one byte past the workspace
    with pytest.raises(AssertionError, match="workspace"):
        a.check_guards()
