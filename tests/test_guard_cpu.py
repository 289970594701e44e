"""The guard helper itself (tests/guard.py), on CPU tensors: every kind of stray access it exists to catch is simulated with a
plain torch write and must be reported with the right tensor, side, count and offset."""
import numpy as np
import pytest
import torch

from guard import MiB, GuardError, Guards, guarded_input, guarded_output, poisoned_workspace


def test_layout_and_alignment():
    a = guarded_output((3, 5, 7), device="cpu", name="y")
    assert a.t.shape == (3, 5, 7) and a.t.is_contiguous()
    assert a.g * 4 >= MiB and (a.g * 4) % 256 == 0
    assert (a.t.data_ptr() - a.buf.data_ptr()) % 256 == 0
    b = guarded_output((3, 5, 7), device="cpu", offset=1)
    assert (b.t.data_ptr() - b.buf.data_ptr()) % 256 == 4
    big = guarded_output((5 * MiB // 4,), device="cpu")
    assert big.g == 5 * MiB // 4                       # guard >= the tensor's size
    h = guarded_output((2, 2, 3, 8), torch.float16, device="cpu", offset=1)
    assert (h.t.data_ptr() - h.buf.data_ptr()) % 256 == 2
    assert torch.isnan(a.t).all() and torch.isnan(h.t).all()


def test_guard_patterns_are_nans():
    a = guarded_output((4,), device="cpu")
    assert a.buf.view(torch.int32)[0].item() == 0x7FA5A5A5 and torch.isnan(a.buf).all()
    w = poisoned_workspace(64, device="cpu")
    assert torch.isnan(w.t.view(torch.float32)).all() and torch.isnan(w.t.view(torch.float16)).all()
    assert w.t.numel() == 64


def test_tail_overrun_one_element():
    a = guarded_output((2, 3, 10), device="cpu", name="logits")
    a.t.fill_(1.0)
    a.buf[a.lo + a.n] = 0.0                             # one element past the end
    with pytest.raises(GuardError, match=r"logits: tail guard: 1 element\(s\) changed, first at offset \+0 past"):
        a.check()


def test_tail_overrun_far():
    a = guarded_output((8,), device="cpu", name="y")
    a.t.fill_(1.0)
    a.buf[a.lo + a.n + 5: a.lo + a.n + 9] = 2.0
    with pytest.raises(GuardError, match=r"y: tail guard: 4 element\(s\) changed, first at offset \+5 past.*farthest \+8"):
        a.check()


def test_lead_underrun():
    a = guarded_output((4, 4), device="cpu", name="x")
    a.t.fill_(0.5)
    a.buf[a.lo - 1] = 3.0
    a.buf[a.lo - 3] = 3.0
    with pytest.raises(GuardError, match=r"x: lead guard: 2 element\(s\) changed, nearest at offset -1 .*farthest -3"):
        a.check()


def test_lead_underrun_misaligned_f16():
    a = guarded_output((1, 2, 5, 8), torch.float16, device="cpu", name="c8", offset=1)
    a.t.fill_(0.0)
    a.buf[a.lo - 1] = 1.0
    with pytest.raises(GuardError, match=r"c8: lead guard: 1 element\(s\) changed, nearest at offset -1"):
        a.check()


def test_unwritten_output_element():
    a = guarded_output((2, 3, 4), device="cpu", name="out")
    a.t.fill_(0.0)
    a.t[1, 2, 3] = a.buf[0]                             # the pattern left in the last element
    with pytest.raises(GuardError, match=r"out: 1 element\(s\) left unwritten, 0 written that must not be; first at offset 23"):
        a.check()
    # a contract that says exactly that element is not written
    m = torch.zeros(2, 3, 4, dtype=torch.bool)
    m[1, 2, 3] = True
    a.check(expect_unwritten=m)
    # and an element written that the contract says is not
    a.t[1, 2, 3] = 0.0
    with pytest.raises(GuardError, match=r"0 element\(s\) left unwritten, 1 written that must not be"):
        a.check(expect_unwritten=m)


def test_written_nan_that_is_not_the_pattern_counts_as_written():
    a = guarded_output((3,), device="cpu")
    a.t.fill_(float("nan"))
    a.check()


def test_modified_input():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    a = guarded_input(x, device="cpu", name="X")
    assert np.array_equal(a.t.numpy(), x)
    a.check()
    a.t[2, 1] = -1.0
    with pytest.raises(GuardError, match=r"X: data: 1 element\(s\) of the input changed, first at offset 9"):
        a.check()


def test_input_overrun_and_underrun_together():
    a = guarded_input(np.ones(7, np.float32), device="cpu", name="X", offset=1)
    a.buf[a.lo - 2] = 0.0
    a.buf[a.lo + a.n] = 0.0
    with pytest.raises(GuardError) as e:
        a.check()
    assert "X: lead guard: 1 element(s) changed, nearest at offset -2" in str(e.value)
    assert "X: tail guard: 1 element(s) changed, first at offset +0" in str(e.value)


def test_workspace_overrun_and_repoison():
    w = poisoned_workspace(1000, device="cpu", name="ws")
    w.t[:10] = 0
    w.check()                                          # writes inside the workspace are its business
    w.repoison()
    assert (w.t == 0xFF).all()
    w.buf[w.lo + 1000 + 3] = 0
    with pytest.raises(GuardError, match=r"ws: tail guard: 1 element\(s\) changed, first at offset \+3"):
        w.check()


def test_guards_collects_every_arena():
    g = Guards(device="cpu")
    x = g.input(np.ones((2, 3), np.float32), name="x")
    y = g.output((2, 3), name="y")
    w = g.workspace(256, name="ws")
    y.t.copy_(x.t * 2)
    g.check()
    y.buf[y.lo + y.n] = 1.0
    w.buf[w.lo - 1] = 0
    with pytest.raises(GuardError) as e:
        g.check()
    assert "y: tail guard" in str(e.value) and "ws: lead guard" in str(e.value) and "x:" not in str(e.value)
    g.repoison()
    assert bool(y.unwritten().all()) and (w.t == 0xFF).all()
