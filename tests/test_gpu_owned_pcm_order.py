"""The PCM entry points of libunipre3d_serialization.so write every element they own and nothing else: called directly, with every
pointer inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrappers on ordinary tensors,
bit for bit (tests/test_gpu_pcm_order.py holds the wrappers to the torch restatement).

Cases of the first four: B = 2 items of N = 1 and N = 65 points (one row each; one row past a wave), under xyz on a cloud with constant
y (codes go negative) and under hilbert.

  entry point             what it owns
  u3d_ser_pcm_grid        grid (B N, 3) int32, whole; meta (8 + 3 B,) int32, whole: three maxima, depth, flag, three zero words, then
                          the items' maxima
  u3d_ser_pcm_encode      code (B N,) int64, whole
  u3d_ser_sort_signed     order (B N,) and inverse (B N,) int64, whole; the scratch is a guarded placement of
                          u3d_ser_scratch_bytes(1, B N) bytes whose contents are not compared
  u3d_ser_pcm_order       all of the above in one call: its own grid, meta, code, order, inverse and scratch placements
  u3d_ser_gather_rows     each dst (rows, C) fp32, whole.  8 tensors in one launch, C = 1, 3, 4, 5, 8, 384, 2047, 2048 (scalar and
                          16-byte rows), the 4-channel pair misaligned by 4 bytes (scalar loads on a multiple of 4); run a second
                          time with the inverse as the index (the backward), at rows = 2 and rows = 130
"""
import ctypes

import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

GS = 0.02
CHANNELS = (1, 3, 4, 5, 8, 384, 2047, 2048)


def _pos(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(0, 60, (B, N, 3), generator=g).float() * 0.005
    pos[:, :, 1] = 0.05                                   # constant y: m2 = 0 under xyz
    pos[:, :, 2] = pos[:, :, 2] * 0.45                    # z cells 0 .. 6, then one point in cell 7: an odd m3
    pos[0, 0, 2], pos[-1, -1, 2] = 0.001, 0.001 + 7 * GS     # (N = 1: the items' minima differ, each cell is 0)
    return pos


@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("order", ["xyz", "hilbert"])
def test_pcm_order_entry_points_write_what_they_own(N, order):
    from unipre3d_amd import _lib, pcm_order, serialization as ser
    lib = ser.load()
    B, rows, oid = 2, 2 * N, pcm_order.ORDERS[order]
    pos_cpu = _pos(B, N, N)
    want_index, want_inverse, want_code = pcm_order.point_order(pos_cpu.cuda(), order, GS)
    code_cpu = want_code.cpu()
    nbytes = int(lib.u3d_ser_scratch_bytes(1, rows))
    nmeta = pcm_order.META_HEAD + 3 * B

    def case(arena):
        p, st = _lib.ptr, _lib.stream_ptr(torch.device("cuda:0"))
        pos, code_in = arena.inp(pos_cpu, name="pos"), arena.inp(code_cpu, name="code_in")
        grid, meta = arena.out((rows, 3), torch.int32, name="grid"), arena.out((nmeta,), torch.int32, name="meta")
        assert lib.u3d_ser_pcm_grid(B, N, p(pos), GS, p(grid), p(meta), st) == 0
        code = arena.out((rows,), torch.int64, name="code")
        assert lib.u3d_ser_pcm_encode(B, N, oid, p(grid), p(meta), p(code), st) == 0
        index, inverse = arena.out((rows,), torch.int64, name="order"), arena.out((rows,), torch.int64, name="inverse")
        scratch = arena.scratch(nbytes, name="sort scratch")
        assert lib.u3d_ser_sort_signed(rows, p(code_in), p(index), p(inverse), p(scratch), st) == 0
        grid2, meta2 = arena.out((rows, 3), torch.int32, name="pcm_order grid"), arena.out((nmeta,), torch.int32, name="pcm_order meta")
        code2, index2, inverse2 = (arena.out((rows,), torch.int64, name=f"pcm_order {n}") for n in ("code", "order", "inverse"))
        scratch2 = arena.scratch(nbytes, name="pcm_order scratch")
        assert lib.u3d_ser_pcm_order(B, N, p(pos), GS, oid, p(grid2), p(meta2), p(code2), p(index2), p(inverse2), p(scratch2), st) == 0
        return [grid, meta, code, index, inverse, grid2, meta2, code2, index2, inverse2]

    run, _ = run_twice(case, "cuda")
    cell = torch.floor(pos_cpu / GS).to(torch.int64)
    cell = (cell - cell.min(dim=1, keepdim=True)[0]).flatten(0, 1)
    top = cell.max(0)[0]
    depth = int(top.max()).bit_length()
    for grid, meta in ((run[0], run[1]), (run[5], run[6])):
        assert same_bits(grid, cell.to(torch.int32)), "grid"
        assert meta[:8].tolist() == top.tolist() + [depth, 0, 0, 0, 0], "meta"
        assert same_bits(meta[8:].view(B, 3), cell.view(B, N, 3).max(1)[0].to(torch.int32)), "meta: the items' maxima"
    if order == "xyz" and N == 65:
        assert int(code_cpu.min()) < 0
    for got, exp, name in zip(run[2:5] + run[7:], [want_code, want_index, want_inverse] * 2, ["code", "order", "inverse"] * 2):
        assert same_bits(got, exp), name


@pytest.mark.parametrize("N", [1, 65])
def test_gather_rows_writes_what_it_owns(N):
    from unipre3d_amd import _lib, pcm_order, serialization as ser
    lib = ser.load()
    rows = 2 * N
    g = torch.Generator().manual_seed(40 + N)
    index_cpu = torch.randperm(rows, generator=g)
    inverse_cpu = torch.argsort(index_cpu)
    src_cpu = [torch.randn(rows, c, generator=g) for c in CHANNELS]

    def launch(arena, index, srcs, tag):
        T = len(srcs)
        dsts = [arena.out((rows, c), torch.float32, misalign=4 if c == 4 else 0, name=f"{tag} dst {c}") for c in CHANNELS]
        sp = (ctypes.c_void_p * T)(*[arena.address(t) for t in srcs])
        dp = (ctypes.c_void_p * T)(*[arena.address(t) for t in dsts])
        ch = (ctypes.c_int32 * T)(*CHANNELS)
        assert lib.u3d_ser_gather_rows(rows, T, _lib.ptr(index), ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(dp, ctypes.c_void_p),
                                       ctypes.cast(ch, ctypes.c_void_p), _lib.stream_ptr(index.device)) == 0
        return dsts

    def case(arena):
        index, inverse = arena.inp(index_cpu, name="index"), arena.inp(inverse_cpu, name="inverse")
        srcs = [arena.inp(t, misalign=4 if t.shape[1] == 4 else 0, name=f"src {t.shape[1]}") for t in src_cpu]
        moved = launch(arena, index, srcs, "forward")
        back = launch(arena, inverse, moved, "backward")           # reads the first launch's outputs: dx[j] = dy[inverse[j]]
        return moved + back

    run, _ = run_twice(case, "cuda")
    T = len(CHANNELS)
    want = pcm_order.reorder(index_cpu.cuda(), inverse_cpu.cuda(), *[t.cuda() for t in src_cpu])
    for got, exp, src, c in zip(run[:T], want, src_cpu, CHANNELS):
        assert same_bits(got, exp) and same_bits(got, src[index_cpu]), f"forward, {c} channels"
    for got, src, c in zip(run[T:], src_cpu, CHANNELS):
        assert same_bits(got, src), f"backward, {c} channels: the inverse gather undoes the gather"
