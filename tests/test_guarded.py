"""The guard-zone checker of tests/guarded.py can fail: on device="cpu", with stand-in "kernels" written in torch, every kind of violation
the GPU tests rely on it to see is reported, and the report names the placement.  A clean stand-in passes."""
import pytest
import torch

import guarded
from guarded import Arena, run_twice

X = torch.arange(1, 14, dtype=torch.float32).reshape(13, 1) * torch.tensor([1.0, -2.0, 0.5])      # (13, 3)


def _clean(arena, flaw=None):
    """y = 2 x into an (13, 3) output, s = first 5 row sums into a (9,) output of which 5 rows are owned; `flaw` plants one violation."""
    x = arena.inp(X, name="x")
    y = arena.out(X.shape, torch.float32, misalign=4, name="y")
    s = arena.out((9,), torch.float32, owned=5, name="rowsum")
    y.copy_(2 * x)
    s[:5] = x[:5].sum(1)
    flat = arena.buf
    y0, y1 = arena.placement_of(y).start, arena.placement_of(y).start + y.numel() * 4
    if flaw == "byte_before":
        flat[y0 - 1] = 7
    elif flaw == "element_after":
        flat[y1:y1 + 4].view(torch.float32)[0] = 1.0
    elif flaw == "unowned_rows":
        s[5] = 3.0
    elif flaw == "unwritten":
        flat[y0 + 4 * 17:y0 + 4 * 18] = arena.poison            # element 17 of y is never stored
    elif flaw == "overread":
        x0 = arena.placement_of(x).start
        past = flat[x0 + x.numel() * 4:x0 + x.numel() * 4 + 4].view(torch.float32)[0]        # the float just past x
        y[12, 2] = torch.nan_to_num(past, nan=5.0)               # finite in both runs, as stale data would be, yet not the same
    elif flaw == "input_written":
        x[3, 1] = 0.0                                           # was -8.0: the two differ in their top byte alone
    return [y, s[:5]]


def test_clean_stand_in_passes_and_returns_both_runs():
    a, b = run_twice(_clean, "cpu")
    for run in (a, b):
        assert guarded.same_bits(run[0], 2 * X) and guarded.same_bits(run[1], X[:5].sum(1))


def test_placements_are_aligned_misaligned_and_guarded():
    arena = Arena("cpu", 0x5A, capacity=8 << 20)
    a = arena.out((5, 3), torch.float32, name="a")
    b = arena.out((1 << 19,), torch.float32, misalign=4, name="b")           # 2 MiB: its guard is capped at 1 MiB
    c = arena.out((7,), torch.float16, misalign=2, name="c")
    e = arena.out((0, 4), torch.int32, name="empty")
    assert a.data_ptr() % 256 == 0 and b.data_ptr() % 256 == 4 and b.data_ptr() % 16 == 4 and c.data_ptr() % 256 == 2
    assert a.is_contiguous() and b.is_contiguous() and c.is_contiguous()
    pa, pb, pc = (arena.placement_of(t) for t in (a, b, c))
    assert pa.start - pa.lo >= 4096 and pb.start - pb.lo >= (1 << 20) and pc.start - pc.lo >= 4096
    assert pb.lo >= pa.hi and pc.lo >= pb.hi and arena.placement_of(e).lo >= pc.hi        # guards are not shared
    assert guarded.guard_bytes(60) == 4096 and guarded.guard_bytes(70000) == 70000 and guarded.guard_bytes(3 << 20) == 1 << 20
    assert e.numel() == 0 and (arena.base + arena.placement_of(e).start) % 256 == 0
    assert a.view(torch.int32)[0, 0].item() == 0x5A5A5A5A and torch.isnan(Arena("cpu", 0xFF, 1 << 16).out((2,), torch.float32)).all()
    assert abs(a[0, 0].item() - 1.5e16) < 1e15 and torch.isfinite(c).all()
    arena.check_guards()
    with pytest.raises(AssertionError, match="multiple of the element size"):
        arena.out((4,), torch.float32, misalign=2)


@pytest.mark.parametrize("flaw, message", [
    ("byte_before", r"placement 'y' were overwritten \(before it\): 1 bytes, first at offset -1, last at offset -1 "),
    ("element_after", r"placement 'y' were overwritten \(after it\): 4 bytes, first at offset 156, last at offset 159 "),
    ("unowned_rows", r"placement 'rowsum' were overwritten \(in its unowned rows\): 4 bytes, first at offset 20, last at offset 23 "),
    ("input_written", r"input placement 'x' was overwritten: 1 bytes, first at offset 43, last at offset 43$"),
])
def test_a_planted_write_outside_the_owned_bytes_is_reported(flaw, message):
    with pytest.raises(AssertionError, match=message):
        run_twice(lambda arena: _clean(arena, flaw), "cpu")


def test_an_unwritten_element_is_reported():
    with pytest.raises(AssertionError, match=r"output 'y' depends on the poison .*: 1 of 39 elements differ .* first flat index 17 "):
        run_twice(lambda arena: _clean(arena, "unwritten"), "cpu")
    # ... and is not, where the caller says the output is no deterministic function of its inputs
    run_twice(lambda arena: _clean(arena, "unwritten"), "cpu", deterministic=[1])


def test_a_value_read_past_an_input_is_reported():
    with pytest.raises(AssertionError, match=r"output 'y' depends on the poison .*: 1 of 39 elements differ .* first flat index 38 "):
        run_twice(lambda arena: _clean(arena, "overread"), "cpu")


def _with_scratch(arena, flaw=None):
    """y = 2 x through a 100-byte scratch that ends up holding the poison's own byte + 1 (so its contents differ between the runs)"""
    x = arena.inp(X, name="x")
    ws = arena.scratch(100, name="ws")
    y = arena.out(X.shape, torch.float32, name="y")
    assert ws.dtype == torch.uint8 and ws.numel() == 100 and ws.data_ptr() % 256 == 0 and arena.address(ws) == ws.data_ptr()
    ws.fill_((arena.poison + 1) & 0xFF)
    y.copy_(2 * x)
    if flaw == "past_scratch":
        p = arena.placement_of(ws)
        arena.buf[p.start + 100] = 7
    return [y]


def test_scratch_is_guarded_but_stays_out_of_the_comparison():
    a, b = run_twice(_with_scratch, "cpu")
    assert guarded.same_bits(a[0], 2 * X) and guarded.same_bits(b[0], 2 * X)
    with pytest.raises(AssertionError, match=r"placement 'ws' were overwritten \(after it\): 1 bytes, first at offset 100, last at offset 100 "):
        run_twice(lambda arena: _with_scratch(arena, "past_scratch"), "cpu")


def test_address_of_an_empty_placement():
    arena = Arena("cpu", 0xFF, capacity=1 << 20)
    e = arena.out((0,), torch.float32, misalign=12, name="empty")
    a = arena.out((3,), torch.float32, misalign=4, name="a")
    assert e.numel() == 0 and arena.address(e) % 256 == 12 and arena.address(e) >= arena.base + 4096
    assert arena.address(a) == a.data_ptr() and arena.address(a) - arena.address(e) >= 2 * 4096 - 12
    arena.check_guards()


def test_the_minus_one_a_knn_leaves_is_not_mistaken_for_poison():
    def fn(arena):
        idx = arena.out((4, 3), torch.int32, name="idx")
        idx.fill_(-1)                                                            # the 0xFF poison as an int32, written on purpose
        return [idx]
    a, b = run_twice(fn, "cpu")
    assert (a[0] == -1).all() and (b[0] == -1).all()

    def lazy(arena):
        idx = arena.out((4, 3), torch.int32, name="idx")
        idx[:3].fill_(-1)                                                        # row 3 is left to the poison: -1 in one run only
        return [idx]
    with pytest.raises(AssertionError, match=r"output 'idx' depends on the poison .*: 3 of 12 elements differ .* first flat index 9 "):
        run_twice(lazy, "cpu")
