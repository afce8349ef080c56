"""The PointNetFeaturePropagation of PointMLP (openpoints/models/backbone/pointmlp.py:356-422) and of PCM
(openpoints/models/PCM/PointMLP_layers.py:228-299), the upward half of both backbones:
`from unipre3d_amd.feature_propagation import PointNetFeaturePropagation` (PointMLP) and
`from unipre3d_amd.feature_propagation import PCMPointNetFeaturePropagation as PointNetFeaturePropagation` (PCM) are the two switches.
The (B, N, S) distance matrix, its full sort, the (B, N, 3, D2) gather, the weighted sum, the cat and the permute are one operator in
libunipre3d_feature_propagation.so (include/unipre3d_feature_propagation.h, csrc/u3d_feature_propagation.hip): the result is written once
as the (B, D1 + D2, N) tensor the `fuse` convolution reads, and nothing of size (B, N, S) or (B, N, 3, D2) exists.

  neighbours(xyz1, xyz2) -> (idx (B, N, 3) int32, weight (B, N, 3))      the three nearest support points and their weights
  propagate(xyz1, xyz2, points1, points2, neighbours=None)               the autograd function
  PointNetFeaturePropagation, PCMPointNetFeaturePropagation              the reference's two modules

Two departures from the reference.  The squared distance is the direct (dx dx + dy dy) + dz dz of unipre3d_amd.knn, not
|a|^2 + |b|^2 - 2ab: where xyz2 is a subset of xyz1, which every stage's sampling makes it, the matmul form gives the coincident
neighbour a distance of +-1e-7 of rounding noise instead of 0, 1 / (d + 1e-8) swings and some weights come out negative; against fp64
the reference's own fp32 run lies at up to 2e-4 of the largest value, the direct form at 1e-7 (tests/golden/make_g22_feature_propagation.py
records both; both forms select the same three indices as fp64 on every recorded row).  And `sort`'s unspecified order among equal
distances becomes "the lower index first".  PCM's eval branch (chunked topk(k, sorted=True)) selects the same pairs in the same order, so
there is one path, and its `k` must be 3: the reference's view(B, N, 3, 1) admits nothing else.

Scope: fp32 on the device, 1 <= N <= 16384, S == 1 or 3 <= S <= 16384 (S == 2 raises ValueError, as the reference's view fails on two
columns), 0 <= D1 <= 2048, 1 <= D2 <= 2048, B N < 2^24; anything else raises (there is no fallback).  Inputs in other floating types or
strided are cast or copied.  There is no gradient to xyz1 and xyz2: they are input data in both callers, and requires_grad on either
raises."""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib
from ._lib import as_f32, byte_buffer, call, on_device

ABI_VERSION = 1
MAX_POINTS, MAX_CHANNELS, TILE = 16384, 2048, 1024          # include/unipre3d_feature_propagation.h

_i, _vp = ctypes.c_int, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_feature_propagation.h
    "u3d_feature_propagation_abi_version": (_i, []),
    "u3d_feature_propagation_scratch_bytes": (ctypes.c_size_t, [_i] * 3),
    "u3d_feature_propagation_search": (_i, [_vp] * 4 + [_i] * 3 + [_vp]),
    "u3d_feature_propagation_lists": (_i, [_vp] * 4 + [_i] * 3 + [_vp]),
    "u3d_feature_propagation_fwd": (_i, [_vp] * 5 + [_i] * 5 + [_vp]),
    "u3d_feature_propagation_bwd": (_i, [_vp] * 5 + [_i] * 5 + [_vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_feature_propagation.so", SIGNATURES, ("u3d_feature_propagation_abi_version", ABI_VERSION))


def _check_clouds(xyz1, xyz2):
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError(f"xyz1 (B, N, 3) and xyz2 (B, S, 3) expected, got {tuple(xyz1.shape)} and {tuple(xyz2.shape)}")
    if xyz1.requires_grad or xyz2.requires_grad:
        raise NotImplementedError("xyz.requires_grad: there is no gradient to xyz1 or xyz2 (they are input data in every caller)")
    B, N, S = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if B < 1 or N < 1 or S < 1:
        raise ValueError(f"an empty tensor is not supported (B, N, S = {B}, {N}, {S})")
    if S == 2:
        raise ValueError("S = 2: three neighbours need three support points (the reference's weight.view(B, N, 3, 1) fails as well)")
    if N > MAX_POINTS or S > MAX_POINTS:
        raise NotImplementedError(f"N={N}, S={S} is not implemented (at most {MAX_POINTS})")
    if B * N >= 1 << 24:
        raise NotImplementedError(f"B N = {B * N} is not implemented (below 2^24)")
    return B, N, S


@torch.no_grad()
def neighbours(xyz1, xyz2):
    """xyz1 (B, N, 3), xyz2 (B, S, 3) -> (idx (B, N, 3) int32, weight (B, N, 3) fp32): per query the three smallest (squared distance,
    index) pairs over xyz2 in lexicographic order -- bit for bit knn.knn_query(3, xyz2, xyz1)[1] -- and w_j = r_j / ((r_0 + r_1) + r_2),
    r_j = 1 / (d2_j + 1e-8).  With S == 1: idx = (0, 0, 0), weight = (1, 0, 0)."""
    B, N, S = _check_clouds(xyz1, xyz2)
    dev = on_device("feature_propagation", xyz1, xyz2)
    xyz1, xyz2 = as_f32(xyz1, "xyz1"), as_f32(xyz2, "xyz2")
    idx = torch.empty(B, N, 3, dtype=torch.int32, device=dev)
    weight = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    call(load().u3d_feature_propagation_search, xyz1, xyz2, idx, weight, B, N, S, dev=dev)
    return idx, weight


_search = neighbours          # (propagate's `neighbours` argument shadows the function)


class _Propagate(torch.autograd.Function):
    """(points1 or None, points2, idx, weight) -> out (B, D1 + D2, N).  Kept for the backward: idx's two list arrays and weight."""

    @staticmethod
    def forward(ctx, points1, points2, idx, weight):
        B, D2, S = points2.shape
        N = idx.shape[1]
        D1 = 0 if points1 is None else points1.shape[1]
        dev = points2.device
        lib = load()
        out = torch.empty(B, D1 + D2, N, dtype=torch.float32, device=dev)
        call(lib.u3d_feature_propagation_fwd, idx, weight, points1, points2, out, B, N, S, D1, D2, dev=dev)
        ctx.dims = (B, N, S, D1, D2)
        if ctx.needs_input_grad[1]:
            ptr = torch.empty(B, S + 1, dtype=torch.int32, device=dev)
            ent = torch.empty(B, 3 * N, dtype=torch.int32, device=dev)
            scratch = byte_buffer(lib.u3d_feature_propagation_scratch_bytes(B, N, S), dev)
            call(lib.u3d_feature_propagation_lists, idx, ptr, ent, scratch, B, N, S, dev=dev)
            ctx.save_for_backward(ptr, ent, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, N, S, D1, D2 = ctx.dims
        dpoints1 = dout[:, :D1, :] if (D1 and ctx.needs_input_grad[0]) else None          # the view: no kernel, no copy
        dpoints2 = None
        if ctx.needs_input_grad[1]:
            ptr, ent, weight = ctx.saved_tensors
            g = dout.to(torch.float32).contiguous()
            if g.data_ptr() % 16 != 0:
                g = g.clone()
            dpoints2 = torch.empty(B, D2, S, dtype=torch.float32, device=g.device)
            call(load().u3d_feature_propagation_bwd, ptr, ent, weight, g, dpoints2, B, N, S, D1, D2, dev=g.device)
        return dpoints1, dpoints2, None, None


def propagate(xyz1, xyz2, points1, points2, neighbours=None):
    """xyz1 (B, N, 3), xyz2 (B, S, 3), points1 (B, D1, N) or None, points2 (B, D2, S) -> (B, D1 + D2, N) contiguous fp32:
    out[:, :D1] = points1 and out[b, D1 + c, n] = (w_0 p2[c, i_0] + w_1 p2[c, i_1]) + w_2 p2[c, i_2] over the three nearest support points
    of n (see `neighbours`; with S == 1 the one support point's features, repeated).  `neighbours` = (idx, weight) overrides the search;
    an idx entry outside [0, S) contributes 0 and receives no gradient.  Differentiable with respect to points1 (the gradient is the
    dout[:, :D1] view itself) and points2 (summed over the inverse lists of idx in ascending order in f64, without float atomics: two
    calls and a graph replay give the same bits).  Kept for the backward: weight (B, N, 3) and the two list arrays (B, S + 1), (B, 3N)."""
    B, N, S = _check_clouds(xyz1, xyz2)
    if points2 is None or points2.dim() != 3 or points2.shape[0] != B or points2.shape[2] != S:
        raise ValueError(f"points2: expected (B, D2, S) = ({B}, D2, {S}), got {None if points2 is None else tuple(points2.shape)}")
    if points1 is not None and (points1.dim() != 3 or points1.shape[0] != B or points1.shape[2] != N):
        raise ValueError(f"points1: expected (B, D1, N) = ({B}, D1, {N}) or None, got {tuple(points1.shape)}")
    D1, D2 = (0 if points1 is None else points1.shape[1]), points2.shape[1]
    if D1 == 0:
        points1 = None
    if D2 < 1 or D2 > MAX_CHANNELS or D1 > MAX_CHANNELS:
        raise NotImplementedError(f"D1={D1}, D2={D2} is not implemented (0 <= D1 <= {MAX_CHANNELS}, 1 <= D2 <= {MAX_CHANNELS})")
    override = neighbours
    on_device("feature_propagation", xyz1, xyz2, points1, points2, *(override or ()))
    if override is None:
        idx, weight = _search(xyz1, xyz2)
    else:
        idx, weight = override
        if tuple(idx.shape) != (B, N, 3) or tuple(weight.shape) != (B, N, 3):
            raise ValueError(f"neighbours: expected idx and weight of shape ({B}, {N}, 3), got {tuple(idx.shape)} and {tuple(weight.shape)}")
        if idx.dtype not in (torch.int32, torch.int64):
            raise NotImplementedError(f"neighbours: idx dtype {idx.dtype} is not implemented (int32 or int64)")
        if weight.requires_grad:
            raise NotImplementedError("neighbours: there is no gradient to the weights")
        idx, weight = idx.to(torch.int32).contiguous(), as_f32(weight, "weight")
    points2 = as_f32(points2, "points2")
    if points1 is not None:
        points1 = as_f32(points1, "points1")
    return _Propagate.apply(points1, points2, idx, weight)


def _activation(name):
    table = {"gelu": nn.GELU, "rrelu": nn.RReLU, "selu": nn.SELU, "silu": nn.SiLU, "hardswish": nn.Hardswish, "leakyrelu": nn.LeakyReLU}
    kind = table.get(name.lower())
    if kind is None:
        return nn.ReLU(inplace=True)
    return kind() if kind is nn.GELU else kind(inplace=True)


class _ConvBNAct(nn.Module):
    """Conv1d(k = 1) + BatchNorm1d + activation under the reference's names (`net.0`, `net.1`)."""

    def __init__(self, cin, cout, bias=True, activation="relu"):
        super().__init__()
        self.act = _activation(activation)
        self.net = nn.Sequential(nn.Conv1d(cin, cout, 1, bias=bias), nn.BatchNorm1d(cout), self.act)

    def forward(self, x):
        return self.net(x)


class _ResBlock(nn.Module):
    """The reference's residual bottleneck of two (three with groups > 1) k = 1 convolutions under its names (`net1`, `net2`)."""

    def __init__(self, channel, groups=1, res_expansion=1.0, bias=True, activation="relu"):
        super().__init__()
        mid = int(channel * res_expansion)
        self.act = _activation(activation)
        self.net1 = nn.Sequential(nn.Conv1d(channel, mid, 1, groups=groups, bias=bias), nn.BatchNorm1d(mid), self.act)
        if groups > 1:
            self.net2 = nn.Sequential(nn.Conv1d(mid, channel, 1, groups=groups, bias=bias), nn.BatchNorm1d(channel), self.act,
                                      nn.Conv1d(channel, channel, 1, bias=bias), nn.BatchNorm1d(channel))
        else:
            self.net2 = nn.Sequential(nn.Conv1d(mid, channel, 1, bias=bias), nn.BatchNorm1d(channel))

    def forward(self, x):
        return self.act(self.net2(self.net1(x)) + x)


class _Blocks(nn.Module):
    """`blocks` residual blocks in a row under the reference's name (`operation`)."""

    def __init__(self, channels, blocks=1, groups=1, res_expansion=1.0, bias=True, activation="relu"):
        super().__init__()
        self.operation = nn.Sequential(*[_ResBlock(channels, groups, res_expansion, bias, activation) for _ in range(blocks)])

    def forward(self, x):
        return self.operation(x)


class PointNetFeaturePropagation(nn.Module):
    """PointMLP's PointNetFeaturePropagation (pointmlp.py:356-422) with its constructor and its state_dict keys (`fuse.net.0.weight`,
    `extraction.operation.0.net1.0.weight`, ...).  forward(xyz1 (B, N, 3), xyz2 (B, S, 3), points1 (B, D1, N) or None, points2 (B, D2, S))
    -> (B, out_channel, N), or the (B, D1 + D2, N) result of `propagate` with has_MLP=False.  The convolutions, BatchNorm and activations
    are torch modules; `fuse` reads propagate's result as it is."""

    def __init__(self, in_channel, out_channel, blocks=1, groups=1, res_expansion=1.0, bias=True, activation="relu", has_MLP=True):
        super().__init__()
        if has_MLP:
            self.fuse = _ConvBNAct(in_channel, out_channel, bias=bias)
            self.extraction = _Blocks(out_channel, blocks, groups, res_expansion, bias, activation)
        self.has_MLP = has_MLP

    def forward(self, xyz1, xyz2, points1, points2):
        new_points = propagate(xyz1, xyz2, points1, points2)
        if self.has_MLP:
            new_points = self.extraction(self.fuse(new_points))
        return new_points


class PCMPointNetFeaturePropagation(nn.Module):
    """PCM's PointNetFeaturePropagation (PointMLP_layers.py:228-299): no has_MLP, blocks == 0 makes `extraction` an nn.Identity, and
    forward takes k, which must be 3.  Training and eval run the same search (the reference's two branches select the same pairs)."""

    def __init__(self, in_channel, out_channel, blocks=1, groups=1, res_expansion=1.0, bias=True, activation="relu"):
        super().__init__()
        self.fuse = _ConvBNAct(in_channel, out_channel, bias=bias)
        self.extraction = nn.Identity() if blocks == 0 else _Blocks(out_channel, blocks, groups, res_expansion, bias, activation)

    def forward(self, xyz1, xyz2, points1, points2, k=3):
        if k != 3:
            raise ValueError(f"k={k}: the interpolation takes three neighbours (the reference's weight.view(B, N, 3, 1) admits nothing else)")
        return self.extraction(self.fuse(propagate(xyz1, xyz2, points1, points2)))
