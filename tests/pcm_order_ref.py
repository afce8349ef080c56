"""PCM's order serialization (openpoints/models/PCM/PCM_utils.py `serialization`, PCM/serialization.py `encode` / `encode_cts`) restated
in plain torch, from what the reference computes: runs on the CPU and on the device; it is what unipre3d_amd/pcm_order.py is compared
with (and timed against), next to the reference's recorded values in tests/golden/g23_pcm_order.npz.

Cells: floor(pos / float32(grid_size)) as int64 minus the item's minimum per axis.  The division is IEEE fp32 division, computed here
as the fp64 quotient rounded to fp32 (for two fp32 operands that double rounding is exact: fp64 carries more than 2 * 24 + 2 bits), with
the divisor as a tensor, so that no device's scalar fast path (x * (1 / grid_size)) and no division kernel's rounding enters.
Depth: bit_length of the largest cell over all items and axes (0 when the batch sits in one cell; `depth=` passes a known value and
saves the host read).  z / z-trans / hilbert / hilbert-trans: batch << 3 depth | curve (tests/serialization_ref.py; depth 0: the batch
id).  The six axis orders, as `encode_cts` is written: with c1 the cell on the first-named axis, m1 m2 m3 the global maxima in the
order's sequence, s(m) = +1 for even m else -1, e(m) = m + (m mod 2):
    code = batch m1 m2 m3 + e(m3) m1 m2 + s(m3) (e(m2) m1 + s(m2) c1)
`axis_code_literal` is the same value the reference's way, a loop with float sign tensors.  Sorts are stable."""
import numpy as np
import torch

import serialization_ref as sref

CURVES = ("z", "z-trans", "hilbert", "hilbert-trans")
AXIS_ORDERS = ("xyz", "xzy", "yxz", "yzx", "zxy", "zyx")
ORDERS = CURVES + AXIS_ORDERS
SHIPPED = ("xyz", "xzy", "yxz", "yzx", "zxy", "zyx", "hilbert", "z", "z-trans")      # model/point_predictor.py:161-171


def grid_cells(pos, grid_size):
    """(B, N, 3) int64: floor(pos / float32(grid_size)) minus the per-item, per-axis minimum."""
    gs = torch.full((), float(np.float32(grid_size)), dtype=torch.float64, device=pos.device)      # (a fill: captures into a graph)
    cell = torch.floor((pos.double() / gs).float()).to(torch.int64)
    return cell - cell.min(dim=1, keepdim=True)[0]


def axis_code_closed(c1, batch, m1, m2, m3):
    s = lambda m: 1 - 2 * (m % 2)
    e = lambda m: m + m % 2
    return batch * m1 * m2 * m3 + e(m3) * m1 * m2 + s(m3) * (e(m2) * m1 + s(m2) * c1)


def axis_code_literal(c1, batch, m1, m2, m3):
    """The reference's loop: the maxima take the place of the second and third coordinate, signs and parities go through fp32."""
    low, base = c1, m1
    for new in (m2, m3):
        sign = (new % 2 == 0).to(torch.float32) * 2 - 1
        bumped = ((1 - (sign + 1) / 2) + new).to(torch.int64)
        low = bumped * base + sign.to(torch.int64) * low
        base = base * new
    return batch * base + low


def encode(grid, order, depth=None, literal=False):
    """grid (B, N, 3) int64 -> code (B N,) int64."""
    assert order in ORDERS, order
    B, N, _ = grid.shape
    batch = torch.arange(B, device=grid.device).view(B, 1).expand(B, N).reshape(B * N)
    flat = grid.reshape(B * N, 3)
    if depth is None:
        depth = int(flat.max()).bit_length()           # the reference's host read, before every order (the axis orders do not use it)
    if order in AXIS_ORDERS:
        ax = ["xyz".index(ch) for ch in order]
        m1, m2, m3 = (flat[:, a].max() for a in ax)
        return (axis_code_literal if literal else axis_code_closed)(flat[:, ax[0]], batch, m1, m2, m3)
    if depth == 0:
        return batch.clone()
    return sref.encode(flat, batch, depth, order)


def order_inverse(code):
    order = torch.argsort(code, stable=True)
    inverse = torch.zeros_like(order).scatter_(0, order, torch.arange(code.numel(), device=code.device))
    return order, inverse


def point_order(pos, order, grid_size=0.02, depth=None, literal=False):
    code = encode(grid_cells(pos, grid_size), order, depth, literal)
    return (*order_inverse(code), code)


def serialization(pos, feat, x_res=None, order="z", layers_outputs=[], grid_size=0.02, depth=None):
    if isinstance(order, (list, tuple)):
        (order,) = order
    B, N, _ = pos.shape
    index = point_order(pos, order, grid_size, depth)[0]
    move = lambda t: t.flatten(0, 1)[index].reshape(B, N, -1).contiguous()
    for i in range(len(layers_outputs)):
        layers_outputs[i] = move(layers_outputs[i])
    return move(pos), move(feat), (None if x_res is None else move(x_res))
