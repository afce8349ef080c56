"""Scene-level 2D->3D PointFusion: `PointFusion` with the reference's interface
(fusion/point_fusion.py:10-195) and pointcept's `GridSample(hash_type="fnv")` as a device op, `grid_sample`, both running in
libunipre3d_pointfusion.so (include/unipre3d_pointfusion.h).  The reference copies every valid pixel to the host for numpy's
hash / argsort / unique; here the points stay on the device and each call reads one 4-word record to size its outputs.

Semantics pinned (tests/pointfusion_ref.py restates them in numpy):
  grid = floor(fp32(fp32(coord - min_coord) / grid_size)) with an explicit min_coord (what PointFusion passes), and with min_coord=None
  the reference's default origin g = floor(fp32(coord / grid_size)), grid = g - g.min(0) (the cells of the absolute grid, not cells
  anchored at coord.min(0)); float -> int64 as numpy on x86 (exact where the floor fits, INT64_MIN otherwise); key = the reference's FNV loop (multiply, then xor) over the three axes,
  voxels in ascending key order, points inside a voxel in ascending index order, train pick = start + r % count with
  r in [0, count.max()) (replayed from `draws`, or drawn on the device from a seed taken from torch's CPU generator), test pick
  part i = start + i % count.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_pointfusion.so")
ABI_VERSION = 2
MODES = {"train": 0, "test": 1}

_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_pointfusion.h
    "u3d_pointfusion_abi_version": (_i, []),
    "u3d_pointfusion_scratch_bytes": (ctypes.c_size_t, [_i, _i]),
    "u3d_pointfusion_minmax": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "u3d_pointfusion_compact": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "u3d_pointfusion_voxelize": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "u3d_pointfusion_pick": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _i, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "u3d_pointfusion_inverse": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_pointfusion_gather_forward": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_pointfusion_gather_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_pointfusion.so", SIGNATURES, ("u3d_pointfusion_abi_version", ABI_VERSION))


def _seed(generator=None) -> int:
    """Seed of the device draw from torch's CPU generator (torch.manual_seed reproduces the picks; no device sync)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=generator).item())


def _min_rows(min_coord, S, dev):
    m = torch.as_tensor(min_coord, dtype=torch.float32).to(dev).reshape(-1, 3).contiguous()
    if m.shape[0] == 1 and S > 1:
        m = m.expand(S, 3).contiguous()
    if m.shape[0] != S:
        raise ValueError(f"min_coord: expected 1 or {S} rows of 3, got {tuple(m.shape)}")
    return m


def _voxelize(coord, grid_size, mins, min_stride, origin, S, offsets, n_max, n, scratch, meta):
    dev = coord.device
    voxel_offsets = torch.empty(S + 1, dtype=torch.int32, device=dev)
    call(load().u3d_pointfusion_voxelize, n_max, n, S, offsets, coord, mins, min_stride, origin, float(np.float32(grid_size)), meta,
         voxel_offsets, scratch, dev=dev)
    return voxel_offsets


def _pick(M, n_max, S, offsets, voxel_offsets, coord, mins, min_stride, origin, grid_size, mode, part, draws, generator, src_map, scratch):
    dev = coord.device
    if mode not in MODES:
        raise ValueError(f"mode must be 'train' or 'test', got {mode!r}")
    if draws is not None:
        draws = torch.as_tensor(draws).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if draws.numel() != M:
            raise ValueError(f"draws: one per voxel expected ({M}), got {draws.numel()}")
    seed = _seed(generator) if (mode == "train" and draws is None and M > 0) else 0
    index = torch.empty(M, dtype=torch.int64, device=dev)
    out_coord = torch.empty(M, 3, dtype=torch.float32, device=dev)
    grid = torch.empty(M, 3, dtype=torch.int64, device=dev)
    src = torch.empty(M, dtype=torch.int32, device=dev) if src_map is not None else None
    call(load().u3d_pointfusion_pick, M, n_max, S, offsets, voxel_offsets, coord, mins, min_stride, origin, float(np.float32(grid_size)),
         MODES[mode], int(part), draws, seed, src_map, index, out_coord, grid, src, scratch, dev=dev)
    return index, out_coord, grid, src


def grid_sample(coord, grid_size=0.02, min_coord=None, mode="train", draws=None, return_inverse=False, sizes=None, part=0,
                generator=None):
    """pointcept's GridSample(hash_type="fnv", return_grid_coord=True) on the device.

    coord (N,3) fp32 on the device; min_coord: (3,) or one row per set: grid = floor((coord - min_coord) / grid_size).  None = the
    reference's default origin, per set: g = floor(coord / grid_size), grid = g - g.min(0) (computed on the device from the set's own
    minimum; NaN coordinates are not pinned on this path).
    mode="train" picks one point per voxel (draws: one recorded int per voxel, else a seeded device draw); mode="test" returns
    part `part` (start + part % count).  sizes: a ragged batch of sets stored back to back; the voxels come out grouped by set and each
    group equals a single-set call.  Returns a dict: index (M,) int64 (set-local point index of each voxel's pick), coord (M,3),
    grid_coord (M,3) int64, voxel_sizes (S,) int64 (voxels per set), max_count (int, largest voxel), inverse (N,) int64 set-local
    voxel of each point when return_inverse."""
    dev = on_device("pointfusion", coord)   # (min_coord may be a host value, as the reference's numpy one)
    coord = coord.detach().contiguous()
    if coord.dtype != torch.float32 or coord.dim() != 2 or coord.shape[1] != 3:
        raise ValueError(f"coord: expected (N,3) float32, got {tuple(coord.shape)} {coord.dtype}")
    N = coord.shape[0]
    if N >= 1 << 31:
        raise ValueError("grid_sample: at most 2^31 - 1 points")
    if sizes is None:
        sizes = (N,)
    sizes = tuple(int(s) for s in sizes)
    if sum(sizes) != N or min(sizes, default=0) < 0 or not sizes:
        raise ValueError(f"sizes {sizes} do not add up to the {N} points")
    S = len(sizes)
    offsets = None
    if S > 1:
        from .rasterizer import ragged_layout
        offsets = ragged_layout(sizes, dev)[0] if N > 0 else torch.zeros(S + 1, dtype=torch.int32, device=dev)
    lib = load()
    if min_coord is None:
        mins = torch.empty(S, 6, dtype=torch.float32, device=dev)
        call(lib.u3d_pointfusion_minmax, N, S, offsets, coord, mins, dev=dev)
        stride, origin = 6, 1
    else:
        mins, stride, origin = _min_rows(min_coord, S, dev), 3, 0
    scratch = torch.empty(lib.u3d_pointfusion_scratch_bytes(N, S), dtype=torch.uint8, device=dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)
    voxel_offsets = _voxelize(coord, grid_size, mins, stride, origin, S, offsets, N, N, scratch, meta)
    _, M, max_count, _ = meta.tolist()              # the call's one device -> host read
    index, out_coord, grid, _ = _pick(M, N, S, offsets, voxel_offsets, coord, mins, stride, origin, grid_size, mode, part, draws,
                                      generator, None, scratch)
    out = {"index": index, "coord": out_coord, "grid_coord": grid, "voxel_sizes": (voxel_offsets[1:] - voxel_offsets[:-1]).long(),
           "max_count": max_count}
    if return_inverse:
        inverse = torch.empty(N, dtype=torch.int64, device=dev)
        call(lib.u3d_pointfusion_inverse, N, N, S, offsets, voxel_offsets, inverse, scratch, dev=dev)
        out["inverse"] = inverse
    return out


class _PixelGather(torch.autograd.Function):
    """feat (M,C) = feat_2d[view][:, y, x] of each voxel's source pixel, read straight from NCHW; backward in gather form."""

    @staticmethod
    def forward(ctx, feat_2d, src):
        V, C, H, W = feat_2d.shape
        f = feat_2d.detach().contiguous()
        if f.dtype != torch.float32:
            raise ValueError(f"feat_2d_all: expected float32, got {f.dtype}")
        M = src.shape[0]
        out = torch.empty(M, C, dtype=torch.float32, device=f.device)
        call(load().u3d_pointfusion_gather_forward, M, C, H * W, f, src, out, dev=f.device)
        ctx.save_for_backward(src)
        ctx.shape = (V, C, H, W)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (src,) = ctx.saved_tensors
        V, C, H, W = ctx.shape
        g = grad_out.contiguous().float()
        grad = torch.empty(V, C, H, W, dtype=torch.float32, device=src.device)   # every element written once by the kernel
        pixel_map = torch.empty(V * H * W, dtype=torch.int32, device=src.device)
        call(load().u3d_pointfusion_gather_backward, V, C, H * W, src.shape[0], g, src, pixel_map, grad, dev=src.device)
        return grad, None


def pixel_gather(feat_2d_all, src_pixel):
    """(M,C) rows of the NCHW features at flat (view, row, column) pixel indices src_pixel (int32); differentiable in feat_2d_all.
    src_pixel must name every pixel at most once (as a grid sample's picks do): the backward writes each picked pixel's row, it does
    not sum repeats."""
    on_device("pointfusion", feat_2d_all, src_pixel)
    return _PixelGather.apply(feat_2d_all, src_pixel.to(torch.int32).contiguous())


def fuse_pixels(feat_2d_all, unprojected_coord, init_coord, grid_size=0.02, mode="train", draws=None, part=0, generator=None):
    """The device half of PointFusion.forward: filter (w != 0, inclusive box of init_coord), grid-sample with min = init_coord.min(0),
    gather the picked pixels' features.  Returns None when no pixel survives, else a dict: coord (M,3), grid_coord (M,3) int64,
    feat (M,C), src_pixel (M,) int32 flat (view, row, column) pixel of each voxel's pick, n (points that passed the filters)."""
    dev = on_device("pointfusion", feat_2d_all, unprojected_coord, init_coord)
    uc = unprojected_coord[0].detach().float().contiguous().reshape(-1, 4)
    if uc.data_ptr() % 16:
        uc = uc.clone()
    V, C, H, W = feat_2d_all.shape
    P = uc.shape[0]
    if P != V * H * W:
        raise ValueError(f"unprojected_coord[0] has {P} pixels, feat_2d_all {V}x{H}x{W}")
    if P >= 1 << 31:
        raise ValueError("PointFusion: at most 2^31 - 1 pixels")
    init = init_coord.detach().float().contiguous()
    lib = load()
    box = torch.empty(1, 6, dtype=torch.float32, device=dev)    # min xyz, max xyz of init_coord: the box and the grid origin
    call(lib.u3d_pointfusion_minmax, init.shape[0], 1, None, init, box, dev=dev)
    scratch = torch.empty(lib.u3d_pointfusion_scratch_bytes(P, 1), dtype=torch.uint8, device=dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)
    coord = torch.empty(P, 3, dtype=torch.float32, device=dev)
    src_of_point = torch.empty(P, dtype=torch.int32, device=dev)
    call(lib.u3d_pointfusion_compact, P, uc, box, coord, src_of_point, meta, scratch, dev=dev)
    voxel_offsets = _voxelize(coord, grid_size, box, 6, 0, 1, None, P, -1, scratch, meta)
    n, M, _, _ = meta.tolist()                      # the call's one device -> host read
    if n == 0:
        return None
    _, out_coord, grid, src = _pick(M, P, 1, None, voxel_offsets, coord, box, 6, 0, grid_size, mode, part, draws, generator,
                                    src_of_point, scratch)
    return {"coord": out_coord, "grid_coord": grid, "feat": _PixelGather.apply(feat_2d_all, src), "src_pixel": src, "n": n}


class PointFusion(nn.Module):
    """Same constructor / forward signature as the reference's module (fusion/point_fusion.py:10-131).  `feat_3d` is any sparse
    tensor type with `features`, `indices`, `spatial_shape`, `batch_size` and that constructor (spconv's SparseConvTensor).
    `draws` (keyword only) replays recorded numpy draws; without it the picks follow torch's seeded CPU generator."""

    def __init__(self, fusion_mlp: nn.Module, fea2d_dim: int = 128, viewNum: int = 8):
        super().__init__()
        self.viewNum = viewNum
        self.fea2d_dim = fea2d_dim
        self.fuseTo3d = fusion_mlp

    def forward(self, feat_2d_all, feat_3d, unprojected_coord, init_3d_data: dict, grid_size: float = 0.02, *, draws=None):
        fused = fuse_pixels(feat_2d_all, unprojected_coord, init_3d_data["coord"], grid_size, draws=draws)
        if fused is None:
            return feat_3d   # the reference's "no valid unprojected coordinates" early return
        grid = fused["grid_coord"]
        indices = torch.cat([torch.zeros(grid.shape[0], 1, dtype=torch.int32, device=grid.device), grid.int()], dim=1).contiguous()
        all_indices = torch.cat([feat_3d.indices, indices], dim=0)
        all_features = torch.cat([feat_3d.features, fused["feat"]], dim=0)
        combined = type(feat_3d)(features=all_features, indices=all_indices, spatial_shape=feat_3d.spatial_shape,
                                 batch_size=feat_3d.batch_size)
        out = self.fuseTo3d(combined)
        init_coords = init_3d_data["coord"]
        init_3d_data.update({"coord": torch.cat((init_coords, fused["coord"].to(init_coords.dtype)), dim=0),
                             "batch": all_indices[:, 0], "grid_coord": all_indices[:, 1:]})
        return out
