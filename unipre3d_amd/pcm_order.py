"""PCM's order serialization on the device: the `serialization(pos, feat, x_res, order, layers_outputs, grid_size)` that
`PointMambaEncoder.serialization_func` (openpoints/models/PCM/PCM.py:265-278) calls before each Mamba layer
(openpoints/models/PCM/PCM_utils.py:21-47), over the PCM entry points of libunipre3d_serialization.so
(include/unipre3d_serialization.h).  `from unipre3d_amd.pcm_order import serialization` is the switch.

  serialization(pos, feat, x_res=None, order="z", layers_outputs=[], grid_size=0.02)   the reference's call, differentiable
  point_order(pos, order, grid_size=0.02) -> (order, inverse, code)                       the permutation alone, int64 (B N,)
  reorder(index, inverse, *tensors)                                                       the autograd function over the row gather

Orders: z, z-trans, hilbert, hilbert-trans (the library's curves at depth = bit_length of the largest cell over the whole batch, the
batch id shifted above them) and xyz, xzy, yxz, yzx, zxy, zyx as the reference's `encode_cts` computes them, which is NOT a
lexicographic order of the cells: the code depends on the first-named axis, the batch id and three global maxima only, it may be
negative, and with a zero maximum the items interleave.  It is reproduced bit for bit and sorted as a signed key.

What is pinned where the reference leaves it open.  Cells are floor(pos / float32(grid_size)) with IEEE fp32 division, which is what
the reference computes on the CPU.  Ties: every sort is stable, equal codes keep ascending row index (`torch.argsort(stable=True)`).
With the whole batch in one cell the depth is 0 and a curve code is the batch id (the reference's hilbert encode raises there).

Per call: four launches for the permutation up to 8192 rows (grid, maxima, codes, a one-workgroup sort), one gather launch per eight
tensors; no host read and no synchronisation, so the call captures into a HIP graph.  The reference's `assert depth <= 16` is a flag on
the device: `check=True` reads it (one host read) and raises.  The backward of the gather is the same kernel with `inverse` as the
index: exact, deterministic, no atomics.

Scope: fp32 tensors on the device, B N <= 2^30 rows, 1 .. 2048 channels per tensor; anything else raises (there is no fallback).
Strided inputs are copied (`.contiguous()`), `feat` given as a view included; the copy is part of the autograd graph."""
from __future__ import annotations

import ctypes

import torch

from . import serialization as _ser
from ._lib import call, on_device

ORDERS = {"z": 0, "z-trans": 1, "hilbert": 2, "hilbert-trans": 3, "xyz": 4, "xzy": 5, "yxz": 6, "yzx": 7, "zxy": 8, "zyx": 9}
META_HEAD, GATHER_MAX, MAX_CHANNELS = 8, 8, 2048          # include/unipre3d_serialization.h
MAX_ROWS, SMALL_SORT = _ser.MAX_ROWS, 8192                 # rows per call; most rows of the one-workgroup sort


def _order_id(order):
    if isinstance(order, (list, tuple)):
        if len(order) != 1:
            raise NotImplementedError(f"order: a list of {len(order)} orders is not implemented (one order per call)")
        order = order[0]
    if order not in ORDERS:
        raise ValueError(f"order={order!r}: expected one of {', '.join(ORDERS)}")
    return ORDERS[order]


def _check_pos(pos, grid_size):
    if pos.dim() != 3 or pos.shape[2] != 3:
        raise ValueError(f"pos: expected (B, N, 3), got {tuple(pos.shape)}")
    B, N = pos.shape[0], pos.shape[1]
    if B < 1 or N < 1 or B * N > MAX_ROWS:
        raise ValueError(f"pos: 1 .. {MAX_ROWS} rows, got B = {B}, N = {N}")
    if pos.dtype != torch.float32:
        raise NotImplementedError(f"pos: dtype {pos.dtype} is not implemented (float32)")
    gs = float(grid_size)
    if not 0.0 < gs < 3.0e38:
        raise ValueError(f"grid_size={grid_size!r}: a positive finite number")
    return B, N, gs


def _rows2d(t, rows, what):
    """t as a contiguous (rows, C) fp32 tensor (a view where t is contiguous, else a copy)."""
    if t.dtype != torch.float32:
        raise NotImplementedError(f"{what}: dtype {t.dtype} is not implemented (float32)")
    if t.dim() < 2 or t.numel() == 0 or t.numel() % rows or t.shape[:-1].numel() != rows:
        raise ValueError(f"{what}: expected {rows} rows of channels, got {tuple(t.shape)}")
    if not 1 <= t.shape[-1] <= MAX_CHANNELS:
        raise NotImplementedError(f"{what}: {t.shape[-1]} channels are not implemented (1 .. {MAX_CHANNELS})")
    return t.contiguous().view(rows, t.shape[-1])


def _gather(index, tensors):
    """[t[index] for t in tensors], each (rows, C_t) fp32 contiguous: one launch per GATHER_MAX tensors."""
    lib = _ser.load()
    rows, dev = index.shape[0], index.device
    outs = [torch.empty_like(t) for t in tensors]
    for k in range(0, len(tensors), GATHER_MAX):
        src, dst = tensors[k:k + GATHER_MAX], outs[k:k + GATHER_MAX]
        T = len(src)
        srcs = (ctypes.c_void_p * T)(*[t.data_ptr() for t in src])
        dsts = (ctypes.c_void_p * T)(*[t.data_ptr() for t in dst])
        chans = (ctypes.c_int32 * T)(*[t.shape[1] for t in src])
        call(lib.u3d_ser_gather_rows, rows, T, index, ctypes.cast(srcs, ctypes.c_void_p), ctypes.cast(dsts, ctypes.c_void_p),
             ctypes.cast(chans, ctypes.c_void_p), dev=dev)
    return outs


class _Reorder(torch.autograd.Function):
    """(index, inverse, *tensors (rows, C_t)) -> the tensors' rows in the order of index.  Kept for the backward: inverse."""

    @staticmethod
    def forward(ctx, index, inverse, *tensors):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(inverse)
        outs = _gather(index, list(tensors))
        ctx.mark_non_differentiable(*[o for i, o in enumerate(outs) if not ctx.needs_input_grad[2 + i]])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        (inverse,) = ctx.saved_tensors
        need = [i for i, g in enumerate(grads) if g is not None and ctx.needs_input_grad[2 + i]]
        out = [None] * len(grads)
        if need:
            gs = [_rows2d(grads[i], inverse.shape[0], "gradient") for i in need]
            for i, g in zip(need, _gather(inverse, gs)):            # dx[j] = dy[inverse[j]]
                out[i] = g
        return (None, None, *out)


def _check_index(index, inverse):
    dev = on_device("pcm_order", index, inverse)
    for t, what in ((index, "index"), (inverse, "inverse")):
        if t.dim() != 1 or t.dtype != torch.int64 or not t.is_contiguous() or t.shape != index.shape or not 1 <= t.shape[0] <= MAX_ROWS:
            raise ValueError(f"{what}: expected a contiguous (rows,) int64 tensor, got {tuple(t.shape)} {t.dtype}")
    return dev


def reorder(index, inverse, *tensors):
    """Each tensor (..., C) fp32 with index.numel() rows in its leading dimensions -> the same shape with row i = the input's row
    index[i].  index and inverse (rows,) int64 must be each other's inverse permutations (`point_order` returns such a pair): the
    backward is dx[j] = dy[inverse[j]].  An index outside [0, rows) gives a row of zeros.  Returns a tuple."""
    _check_index(index, inverse)
    on_device("pcm_order", index, *tensors)
    if not tensors:
        return ()
    rows = index.shape[0]
    flat = [_rows2d(t, rows, f"tensor {i}") for i, t in enumerate(tensors)]
    return tuple(o.view(t.shape) for o, t in zip(_Reorder.apply(index, inverse, *flat), tensors))


@torch.no_grad()
def point_order(pos, order, grid_size=0.02, check=False):
    """pos (B, N, 3) fp32 -> (order, inverse, code), each (B N,) int64: code the serialization code of `order` for every point in
    row-major (item, point) order, order its stable ascending signed sort over all B N rows, inverse[order[i]] = i.  No host read
    unless check=True, which raises where a cell needs more than 16 bits (the reference's `assert depth <= 16`) or is not finite."""
    oid = _order_id(order)
    B, N, gs = _check_pos(pos, grid_size)
    dev = on_device("pcm_order", pos)
    lib = _ser.load()
    rows = B * N
    pos = pos.detach().contiguous()
    grid = torch.empty(rows, 3, dtype=torch.int32, device=dev)
    meta = torch.empty(META_HEAD + 3 * B, dtype=torch.int32, device=dev)
    code = torch.empty(rows, dtype=torch.int64, device=dev)
    index, inverse = torch.empty_like(code), torch.empty_like(code)
    scratch = torch.empty(lib.u3d_ser_scratch_bytes(1, rows), dtype=torch.uint8, device=dev)
    call(lib.u3d_ser_pcm_order, B, N, pos, gs, oid, grid, meta, code, index, inverse, scratch, dev=dev)
    if check and int(meta[4].item()):
        raise ValueError(f"pos / grid_size={grid_size}: a cell needs more than 16 bits (depth {int(meta[3].item())}) or is not finite")
    return index, inverse, code


def serialization(pos, feat, x_res=None, order="z", layers_outputs=[], grid_size=0.02, check=False):
    """PCM_utils.serialization: pos (B, N, 3), feat (B, N, C), x_res (B, N, C') or None and every tensor of `layers_outputs` with their
    B N rows in the order of `order` (see point_order), reshaped to (B, N, -1) as the reference does.  Returns (pos, feat, x_res) and
    replaces the entries of `layers_outputs` in place in the caller's list.  Differentiable in feat, x_res and the list's tensors (and
    pos, as a gather; the permutation itself has no gradient).  A list of one order is accepted."""
    _order_id(order)
    B, N, _ = _check_pos(pos, grid_size)
    extra = [] if x_res is None else [x_res]
    on_device("pcm_order", pos, feat, *extra, *layers_outputs)
    index, inverse, _ = point_order(pos, order, grid_size, check=check)
    moved = reorder(index, inverse, pos, feat, *extra, *layers_outputs)
    moved = [t.reshape(B, N, -1) for t in moved]
    for i in range(len(layers_outputs)):
        layers_outputs[i] = moved[2 + len(extra) + i]
    return moved[0], moved[1], (moved[2] if extra else None)
