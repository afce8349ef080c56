"""Guard zones for calling the C entry points directly: every pointer a kernel gets points into one poisoned allocation, so a store past
the end of an output, an element nobody wrote and a load past the end of an input all become visible.  (A plain helper module, imported
by the tests that use it; tests/test_guarded.py proves on the CPU that each of those is reported.)

    def case(arena):
        x = arena.inp(x_cpu, name="x")                       # data copied in, poison on both sides
        y = arena.out((m, c), torch.float32, name="y")       # still holds the poison
        assert lib.u3d_something(m, c, _lib.ptr(x), _lib.ptr(y), stream) == 0
        return [y]
    (y_a,), (y_b,) = run_twice(case, "cuda")

`run_twice` runs the case under two different poisons and compares the owned outputs bit for bit: an element nobody wrote keeps its poison
and a value read from outside an input carries it, so both differ between the runs whatever the legitimate value range is (-1, the 0xFF
poison as an int, is a legitimate kNN / FPS index, which is why one sentinel would not do).
"""
from __future__ import annotations

import math

import torch

ALIGN = 256                 # a placement starts at a 256-byte boundary (+ misalign)
GUARD_MIN, GUARD_MAX = 4096, 1 << 20
POISONS = (0xFF, 0x5A)      # fp32: NaN / ~1.5e16   fp16: NaN / 209.25   int32: -1 / 1515870810


def guard_bytes(nbytes: int) -> int:
    """Width of the guard before and after a placement of `nbytes`: as wide as the placement, so that a store one element, vector, row or
    plane off still lands inside the arena; at least 4096 bytes, at most 1 MiB."""
    return min(max(GUARD_MIN, nbytes), GUARD_MAX)


class _Placement:
    __slots__ = ("name", "start", "nbytes", "owned_bytes", "lo", "hi", "row_bytes", "rows", "view", "expect")

    def __init__(self, name, start, nbytes, guard, row_bytes, rows, view):
        self.name, self.start, self.nbytes, self.owned_bytes = name, start, nbytes, nbytes
        self.lo, self.hi = start - guard, start + nbytes + guard     # [lo, hi): the placement with its two guards
        self.row_bytes, self.rows, self.view, self.expect = row_bytes, rows, view, None


class Arena:
    """One uint8 allocation filled with `poison_byte`, out of which inputs and outputs are placed with guards around each."""

    def __init__(self, device, poison_byte: int, capacity: int = 32 << 20):
        self.device, self.poison = torch.device(device), int(poison_byte)
        self.buf = torch.full((capacity,), self.poison, dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.placements: list[_Placement] = []

    # -- placing -------------------------------------------------------------------------------------------------------------------
    def _place(self, shape, dtype, misalign, name):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        assert misalign >= 0 and misalign % item == 0, f"misalign {misalign} is no multiple of the element size {item}"
        nbytes = item * math.prod(shape)
        guard = guard_bytes(nbytes)
        start = self.cursor + guard
        start += -(self.base + start) % ALIGN + misalign
        end = start + nbytes + guard
        assert end <= self.buf.numel(), f"arena of {self.buf.numel()} bytes is too small for {name} ({nbytes} bytes + guards)"
        self.cursor = end
        view = self.buf[start:start + nbytes].view(dtype).view(shape)
        assert view.is_contiguous() and (self.base + start - misalign) % ALIGN == 0 and (nbytes == 0 or view.data_ptr() == self.base + start)
        rows = shape[0] if shape else 1
        p = _Placement(name or f"#{len(self.placements)}", start, nbytes, guard, (nbytes // rows if rows else 0), rows, view)
        self.placements.append(p)
        return p

    def inp(self, cpu_tensor, misalign: int = 0, name: str | None = None):
        """Copies `cpu_tensor` in and returns the contiguous view of it.  The entry points only read their inputs, so check_guards() also
        holds the bytes of an input to what was copied in."""
        t = cpu_tensor.detach().contiguous()
        p = self._place(t.shape, t.dtype, misalign, name)
        p.view.copy_(t)
        p.expect = t.cpu().clone()
        return p.view

    def out(self, shape, dtype, misalign: int = 0, owned: int | None = None, name: str | None = None):
        """A contiguous view that still holds the poison.  owned=None: the kernel owns the whole view; owned=M: only the first M rows (the
        leading dimension), and the rest of the view counts as guard."""
        p = self._place(shape, dtype, misalign, name)
        if owned is not None:
            self.own(p.view, owned)
        return p.view

    def scratch(self, nbytes: int, name: str = "scratch"):
        """A uint8 placement of exactly `nbytes` bytes at a 256-byte boundary for a scratch, workspace or partials buffer: guarded like
        any output, and simply not returned from the case, so that its bytes (which may hold anything) stay out of the bit comparison."""
        view = self.out((int(nbytes),), torch.uint8, name=name)
        assert self.address(view) % ALIGN == 0
        return view

    def address(self, view) -> int:
        """Device address of a placement's first byte (an empty tensor's data_ptr() is 0; its placement still has an address)."""
        return self.base + self.placement_of(view).start

    def own(self, view, rows: int):
        """Narrows the owned region of an out() placement to its first `rows` rows (for counts only known after the call) and returns that
        prefix view."""
        p = self.placement_of(view)
        assert 0 <= rows <= p.rows, f"{p.name}: {rows} owned rows of {p.rows}"
        p.owned_bytes = rows * p.row_bytes
        return p.view[:rows]

    def placement_of(self, view) -> _Placement:
        for p in self.placements:
            if p.view is view:
                return p
        off = view.data_ptr() - self.base      # (an empty tensor's data_ptr() is 0: it is only found by identity)
        for p in self.placements:
            if view.numel() and p.start <= off < p.start + p.nbytes:
                return p
        raise AssertionError("tensor is not a placement of this arena")

    # -- checking ------------------------------------------------------------------------------------------------------------------
    def check_guards(self):
        """Every byte outside an owned region still equals the poison, and every input still holds what was copied in."""
        clean = self.buf == self.poison
        for p in self.placements:
            clean[p.start:p.start + p.owned_bytes] = True
        if not bool(clean.all()):
            bad = torch.nonzero(~clean).flatten().cpu()
            first = int(bad[0])
            # the placement whose guards hold the first such byte; in the alignment slack between two guards, or beyond the last, the nearest
            p = next((q for q in self.placements if q.lo <= first < q.hi), None) or \
                min(self.placements, key=lambda q: min(abs(first - q.start), abs(first - (q.start + q.nbytes))))
            mine = bad[(bad >= min(p.lo, first)) & (bad < max(p.hi, first + 1))]
            where = "before it" if first < p.start else ("in its unowned rows" if first < p.start + p.nbytes else "after it")
            raise AssertionError(
                f"guard bytes of placement '{p.name}' were overwritten ({where}): {mine.numel()} bytes, first at offset "
                f"{int(mine[0]) - p.start}, last at offset {int(mine[-1]) - p.start} relative to its start "
                f"(the placement has {p.nbytes} bytes, of which {p.owned_bytes} are owned); {bad.numel()} bytes in the whole arena")
        for p in self.placements:
            if p.expect is not None:
                same = _bytes(p.view.cpu()).flatten() == _bytes(p.expect).flatten()
                if not bool(same.all()):
                    bad = torch.nonzero(~same).flatten()
                    raise AssertionError(f"input placement '{p.name}' was overwritten: {bad.numel()} bytes, first at offset {int(bad[0])}, "
                                         f"last at offset {int(bad[-1])}")


def _bytes(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.numel() else torch.zeros(0, dtype=torch.uint8)


def run_twice(fn, device="cuda", deterministic=True, capacity: int = 32 << 20):
    """Runs fn(arena) once per poison.  fn returns the list of owned outputs (arena views; prefix views where only a prefix is owned).
    After each run the device is synchronised and the guards are checked.  Returns the two runs' outputs as host copies, after asserting
    that they are bit-identical across the runs: for every output (deterministic=True), for none (False), or for the listed positions
    (an iterable of indices into fn's list; the others are float sums through atomics, which the caller bounds itself)."""
    runs, names = [], []
    for poison in POISONS:
        arena = Arena(device, poison, capacity)
        outs = list(fn(arena))
        if arena.device.type == "cuda":
            torch.cuda.synchronize(arena.device)
        arena.check_guards()
        names = []
        for i, o in enumerate(outs):
            try:
                names.append(arena.placement_of(o).name)
            except AssertionError:
                names.append(f"output {i}")
        runs.append([o.detach().cpu().clone() for o in outs])
    a, b = runs
    assert len(a) == len(b), "the two runs returned different numbers of outputs"
    which = range(len(a)) if deterministic is True else (() if deterministic is False else tuple(deterministic))
    for i in which:
        assert a[i].shape == b[i].shape and a[i].dtype == b[i].dtype, \
            f"output '{names[i]}': {tuple(a[i].shape)} {a[i].dtype} under poison 0xFF, {tuple(b[i].shape)} {b[i].dtype} under 0x5A"
        item = a[i].element_size()
        diff = torch.nonzero(_bytes(a[i]).flatten() != _bytes(b[i]).flatten()).flatten()
        if diff.numel():
            elems = torch.unique(diff // item)
            e = int(elems[0])
            raise AssertionError(
                f"output '{names[i]}' depends on the poison (an element nobody wrote, or a value read outside an input): {elems.numel()} of "
                f"{a[i].numel()} elements differ between the two runs, first flat index {e} "
                f"({a[i].flatten()[e].item()!r} under 0xFF, {b[i].flatten()[e].item()!r} under 0x5A), last flat index {int(elems[-1])}")
    return a, b


def same_bits(got, want) -> bool:
    """Bit-for-bit equality of two host tensors (NaNs of the same bit pattern compare equal, -0.0 and 0.0 do not)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    return got.shape == want.shape and got.dtype == want.dtype and bool(torch.equal(_bytes(got), _bytes(want)))
