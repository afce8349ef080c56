"""PTv3's index plumbing on the device (libunipre3d_serialization.so, include/unipre3d_serialization.h): the serialization codes of
pointcept's `encode` / `Point.serialization`, the pad / unpad / cu_seqlens of `SerializedAttention.get_padding_and_inverse` and the
clusters of `SerializedPooling`.  Integers only, so there is no autograd and every result is bit-identical from call to call.

Tie rule: every sort is STABLE, equal codes (repeated sites) and the points of one cluster come out in ascending point index, which is
`torch.argsort(stable=True)`; the reference's plain argsort / sort leaves that order unspecified.

Host reads per call: encode and serialize none (serialize captures into a graph) unless depth=None, which reads grid_coord.max() once
as the reference does; patch_padding none for a host `offset`, one read of the B offsets for a device `offset`; pool_clusters one read
of the cluster count M (torch.unique synchronises there as well).

Pass count of the sort: ceil(key width / 8) with key width 3 * depth + bit_length(batch_size - 1).  `batch_size` (the number of
items) is a host int; without it a batched code is taken to be 63 bits wide (8 passes).  Batch ids at or above batch_size break the
order, not memory safety.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_serialization.so")
ABI_VERSION = 1
ORDERS = {"z": 0, "z-trans": 1, "hilbert": 2, "hilbert-trans": 3}
MAX_ORDERS = 4
MAX_ROWS = 1 << 30

_i, _ll, _vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_serialization.h
    "u3d_ser_abi_version": (_i, []),
    "u3d_ser_scratch_bytes": (ctypes.c_size_t, [_i, _i]),
    "u3d_ser_encode": (_i, [_i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "u3d_ser_sort": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_ser_serialize": (_i, [_i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_ser_patch_padding": (_i, [_i, _i, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp]),
    "u3d_ser_pool_count": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_ser_pool_emit": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # PCM's order serialization (unipre3d_amd/pcm_order.py)
    "u3d_ser_pcm_grid": (_i, [_i, _i, _vp, ctypes.c_float, _vp, _vp, _vp]),
    "u3d_ser_pcm_encode": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_ser_sort_signed": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_ser_pcm_order": (_i, [_i, _i, _vp, ctypes.c_float, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "u3d_ser_gather_rows": (_i, [_ll, _i, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_serialization.so", SIGNATURES, ("u3d_ser_abi_version", ABI_VERSION))


def _order_bits(orders):
    if isinstance(orders, str):
        orders = (orders,)
    orders = tuple(orders)
    if not 1 <= len(orders) <= MAX_ORDERS:
        raise NotImplementedError(f"orders: {len(orders)} orders are not implemented (1 .. {MAX_ORDERS})")
    bits = 0
    for k, o in enumerate(orders):
        if o not in ORDERS:
            raise ValueError(f"order={o!r}: expected one of {', '.join(ORDERS)}")
        bits |= ORDERS[o] << (2 * k)
    return len(orders), bits


def _check_points(grid_coord, batch, depth, batch_size):
    """Validates the inputs of encode / serialize; returns (device, key width in bits)."""
    ts = (grid_coord,) if batch is None else (grid_coord, batch)
    dev = on_device("serialization", *ts)
    if grid_coord.dim() != 2 or grid_coord.shape[1] != 3:
        raise ValueError(f"grid_coord: expected (N, 3), got {tuple(grid_coord.shape)}")
    N = grid_coord.shape[0]
    if not 1 <= N <= MAX_ROWS:
        raise ValueError(f"grid_coord: 1 .. {MAX_ROWS} points, got {N}")
    if grid_coord.dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"grid_coord: dtype {grid_coord.dtype} is not implemented (int32 or int64)")
    if not grid_coord.is_contiguous():
        raise ValueError("grid_coord: a non-contiguous tensor is not supported (call .contiguous())")
    if batch is not None:
        if batch.dim() != 1 or batch.shape[0] != N:
            raise ValueError(f"batch: expected ({N},), got {tuple(batch.shape)}")
        if batch.dtype not in (torch.int32, torch.int64):
            raise NotImplementedError(f"batch: dtype {batch.dtype} is not implemented (int32 or int64)")
        if not batch.is_contiguous():
            raise ValueError("batch: a non-contiguous tensor is not supported (call .contiguous())")
    if isinstance(depth, bool) or not isinstance(depth, int) or not 1 <= depth <= 16:
        raise ValueError(f"depth={depth!r}: an int in 1 .. 16")
    if batch is None:
        if batch_size not in (None, 1):
            raise ValueError(f"batch_size={batch_size} without batch")
        return dev, 3 * depth
    if batch_size is None:
        return dev, 63
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}: at least one item")
    if 3 * depth + batch_size.bit_length() > 63:      # the reference's bound (structure.py)
        raise ValueError(f"depth={depth} with batch_size={batch_size}: 3 * depth + bit_length(batch_size) exceeds 63 bits")
    return dev, max(3 * depth + (batch_size - 1).bit_length(), 1)


def _check_code(code):
    dev = on_device("serialization", code)
    if code.dim() != 2 or code.dtype != torch.int64:
        raise ValueError(f"code: expected a (K, N) int64 tensor, got {tuple(code.shape)} {code.dtype}")
    K, N = code.shape
    if not 1 <= K <= MAX_ORDERS:
        raise NotImplementedError(f"code: {K} rows are not implemented (1 .. {MAX_ORDERS})")
    if not 1 <= N <= MAX_ROWS:
        raise ValueError(f"code: 1 .. {MAX_ROWS} points, got {N}")
    if not code.is_contiguous():
        raise ValueError("code: a non-contiguous tensor is not supported (call .contiguous())")
    return dev, K, N


def _scratch(lib, K, N, dev):
    return torch.empty(lib.u3d_ser_scratch_bytes(K, N), dtype=torch.uint8, device=dev)


def adaptive_depth(grid_coord) -> int:
    """The reference's adaptive rule: bit_length of the largest coordinate.  Reads grid_coord.max() from the device (one host read)."""
    return max(int(grid_coord.max()).bit_length(), 1)


def encode(grid_coord, batch=None, depth=16, order="z"):
    """pointcept's `encode`: grid_coord (N, 3) int32 / int64 on the device with 0 <= v < 2**depth, batch (N,) int32 / int64 or None,
    depth 1 .. 16.  Returns (N,) int64 batch << 3*depth | code; `order` may also be a sequence of 1 .. 4 orders, which returns (K, N)."""
    lib = load()
    K, bits = _order_bits(order)
    dev, _ = _check_points(grid_coord, batch, depth, None)
    N = grid_coord.shape[0]
    code = torch.empty(K, N, dtype=torch.int64, device=dev)
    call(lib.u3d_ser_encode, N, grid_coord, int(grid_coord.dtype == torch.int64), batch,
         int(batch is not None and batch.dtype == torch.int64), depth, K, bits, code, dev=dev)
    return code[0] if isinstance(order, str) else code


def sort_codes(code, key_bits=63):
    """order, inverse (K, N) int64 of code (K, N) int64 with 0 <= code < 2**key_bits: order[k] is the stable ascending sort of code[k],
    inverse[k][order[k][i]] = i.  No host read."""
    lib = load()
    dev, K, N = _check_code(code)
    if not 1 <= int(key_bits) <= 63:
        raise ValueError(f"key_bits={key_bits}: 1 .. 63")
    order, inverse = torch.empty_like(code), torch.empty_like(code)
    scratch = _scratch(lib, K, N, dev)
    call(lib.u3d_ser_sort, K, N, int(key_bits), code, order, inverse, scratch, dev=dev)
    return order, inverse


def serialize(grid_coord, batch, depth, orders, batch_size=None, shuffle_orders=False):
    """Point.serialization: (code, order, inverse), each (K, N) int64 for K = len(orders) in 1 .. 4; see the module docstring for the
    tie rule, batch_size and depth=None (the one case with a host read).  shuffle_orders permutes the K rows with torch.randperm."""
    lib = load()
    K, bits = _order_bits(orders)
    if depth is None:
        depth = adaptive_depth(grid_coord)
    dev, key_bits = _check_points(grid_coord, batch, depth, batch_size)
    N = grid_coord.shape[0]
    code = torch.empty(K, N, dtype=torch.int64, device=dev)
    order, inverse = torch.empty_like(code), torch.empty_like(code)
    scratch = _scratch(lib, K, N, dev)
    call(lib.u3d_ser_serialize, N, grid_coord, int(grid_coord.dtype == torch.int64), batch,
         int(batch is not None and batch.dtype == torch.int64), depth, K, bits, key_bits, code, order, inverse, scratch, dev=dev)
    if shuffle_orders:
        perm = torch.randperm(K).to(dev)
        code, order, inverse = code[perm], order[perm], inverse[perm]
    return code, order, inverse


def patch_padding(offset, patch_size, device=None):
    """SerializedAttention.get_padding_and_inverse: (pad int64, unpad int64, cu_seqlens int32) for items ending at `offset` (B,).
    offset as a host sequence or CPU tensor: no host read (`device` says where the outputs go, default the current device); as a
    device tensor: one read of its B values.  Every item must hold at least one point."""
    lib = load()
    if torch.is_tensor(offset):
        if offset.dim() != 1 or offset.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"offset: expected a (B,) int32 / int64 tensor, got {tuple(offset.shape)} {offset.dtype}")
        if offset.device.type == "cuda":
            device = offset.device
        ends = offset.tolist()           # device offset: the one host read
    else:
        ends = [int(e) for e in offset]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("unipre3d_amd.serialization needs a HIP device; there is no CPU fallback")
    P = int(patch_size)
    if P < 1:
        raise ValueError(f"patch_size={patch_size}: must be at least 1")
    if not ends:
        raise ValueError("offset: at least one item")
    off, offp, offs = [0], [0], [0]
    for e in ends:
        n = e - off[-1]
        if n < 1:
            raise ValueError(f"offset: every item must hold at least one point (item {len(off) - 1} has {n})")
        off.append(e)
        offp.append(offp[-1] + (n if n <= P else (n + P - 1) // P * P))
        offs.append(offs[-1] + (1 if n <= P else (n + P - 1) // P))
    B, T, T_pad, S = len(ends), off[-1], offp[-1], offs[-1]
    if T_pad >= 1 << 31:
        raise NotImplementedError(f"offset: {T_pad} padded points do not fit cu_seqlens' int32")
    meta = torch.tensor([off, offp, offs], dtype=torch.int64).to(dev)
    pad = torch.empty(T_pad, dtype=torch.int64, device=dev)
    unpad = torch.empty(T, dtype=torch.int64, device=dev)
    cu = torch.empty(S + 1, dtype=torch.int32, device=dev)
    call(lib.u3d_ser_patch_padding, B, P, T, T_pad, S, meta, pad, unpad, cu, dev=dev)
    return pad, unpad, cu


def pool_clusters(code, pooling_depth, depth=None, batch_size=None):
    """SerializedPooling's index half for code (K, N) int64 from serialize: returns (cluster (N,), indices (N,), idx_ptr (M+1,),
    head_indices (M,), code, order, inverse (K, M)), all int64.  cluster = rank of code[0] >> 3*pooling_depth among its distinct
    values; indices = the stable sort of cluster; idx_ptr its CSR pointer (scatter.segment_csr's indptr); head_indices =
    indices[idx_ptr[:-1]]; the pooled code is (code >> 3*pooling_depth)[:, head_indices] with order / inverse as in serialize.
    depth (the serialization depth) and batch_size give the sort its key width; without both, 63 bits.  One host read (M)."""
    lib = load()
    dev, K, N = _check_code(code)
    pd = int(pooling_depth)
    if not 0 <= pd <= 16:
        raise ValueError(f"pooling_depth={pooling_depth}: 0 .. 16")
    key_bits = 63 - 3 * pd
    if depth is not None and batch_size is not None:
        if not 1 <= int(depth) <= 16 or pd > int(depth) or int(batch_size) < 1 or 3 * int(depth) + int(batch_size).bit_length() > 63:
            raise ValueError(f"depth={depth}, batch_size={batch_size}, pooling_depth={pd}: not a serialization's")
        key_bits = max(3 * (int(depth) - pd) + (int(batch_size) - 1).bit_length(), 1)
    scratch = _scratch(lib, K, N, dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)
    call(lib.u3d_ser_pool_count, K, N, 3 * pd, key_bits, code, meta, scratch, dev=dev)
    M = int(meta[0].item())                    # the one device -> host read: the cluster count
    new = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
    cluster, indices, idx_ptr, head = new(N), new(N), new(M + 1), new(M)
    pcode, porder, pinverse = new(K, M), new(K, M), new(K, M)
    call(lib.u3d_ser_pool_emit, K, N, M, 3 * pd, key_bits, code, cluster, indices, idx_ptr, head, pcode, porder, pinverse, scratch,
         dev=dev)
    return cluster, indices, idx_ptr, head, pcode, porder, pinverse
