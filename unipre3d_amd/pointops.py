"""Point sampling / grouping operators with the reference's Python names and signatures:
openpoints/models/layers/subsample.py:77-148 (`furthest_point_sample`, `gather_operation`, `fps`) and
openpoints/models/layers/group.py:76-203 (`grouping_operation`, `ball_query`), the `QueryAndGroup` module
(:208-260), and openpoints/models/layers/upsampling.py:11-101 (`three_nn`, `three_interpolate`, `three_interpolation`).  Backed by libunipre3d_pointops.so (include/unipre3d_pointops.h); no CPU fallback."""
from __future__ import annotations

import ctypes
import os
from typing import Tuple

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_pointops.so")   # (U3D_LIB_DIRNAME: experiment builds, see _lib.py)
CONTRACTIONS = {"fma_llvm": 0, "fma_chain": 1, "none": 2}    # include/unipre3d_pointops.h: U3D_PO_*


def set_contraction(mode: str) -> None:
    """How the reference's three-term sums (squared distances, interpolation) are contracted -- what nvcc's -fmad=true would have
    chosen decides FPS ties.  'fma_llvm' (default: LLVM's combiner order, NVVM is LLVM), 'fma_chain' (rounds 1-3 of this build),
    'none' (-fmad=false).  Process-wide, applies to the launches that follow."""
    rc = load().u3d_pointops_set_contraction(CONTRACTIONS[mode])
    if rc != 0:
        raise ValueError(f"unknown contraction mode {mode!r}")


_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_pointops.h
    "u3d_furthest_point_sampling": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_fps_grid_workspace_bytes": (ctypes.c_size_t, [_i]),
    "u3d_fps_grid_points_per_workgroup": (_i, []),
    "u3d_furthest_point_sampling_grid": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_offset_furthest_sampling": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "u3d_ball_query": (_i, [_i, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "u3d_group_points": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_group_points_grad": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_gather_points": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_gather_points_grad": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "u3d_three_nn": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_three_interpolate": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_three_interpolate_grad": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_pointops_set_contraction": (_i, [_i]),
    "u3d_pointops_get_contraction": (_i, []),
    "u3d_group_points_grad_rows": (_i, [_i, _i, _i]),
    "u3d_three_interpolate_grad_rows": (_i, [_i, _i, _i]),
    "u3d_group_points_form": (_i, [_i, _i, _vp, _vp]),
    "u3d_three_interpolate_form": (_i, [_i, _i]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_pointops.so", SIGNATURES)


def _f32(t, what):
    """The kernels read raw fp32: anything else (fp16/bf16 under autocast, float64) is cast, never reinterpreted."""
    if not t.is_floating_point():
        raise TypeError(f"{what} must be a floating-point tensor, got {t.dtype}")
    return t if t.dtype == torch.float32 else t.float()


def _i32(idx, what):
    """Index tensors are int32 in the C-ABI (what furthest_point_sample / ball_query return); int64 ones (.long(), torch.topk)
    are converted, anything else is refused."""
    if idx.dtype == torch.int32:
        return idx
    if idx.dtype == torch.int64:
        return idx.to(torch.int32)
    raise TypeError(f"{what} must be an int32 (or int64) index tensor, got {idx.dtype}")


# Clouds above N_GRID points are sampled by the grid kernel (one cloud over several workgroups, csrc/u3d_fps_grid.h); at or below it, and
# beyond the grid's capacity, by the one-workgroup-per-cloud kernels.  From tools/fps_bench.py's table (profiles/fps/): the grid
# kernel is ahead at every measured shape from 16 384 points up (2.4 x there, 7.8 x and 12 x at the loader's); nothing was measured between
# 8192 and 16 384, so those clouds keep their path.  Never below 8192.
N_GRID = 16383
STATUS_OVER_CAPACITY = 2                                       # include/unipre3d_pointops.h

_grid_ws = {}


def grid_workspace(b: int, dev) -> torch.Tensor:
    """The device's workspace of the grid kernel for b segments: slots, counters and the status word (a few hundred bytes).  One tensor
    per device is kept and reused on every stream: the library clears it on the call's stream behind its one-grid-in-flight wait."""
    need = int(load().u3d_fps_grid_workspace_bytes(int(b)))
    ws = _grid_ws.get(dev)
    if ws is None or ws.numel() < need:
        ws = _grid_ws[dev] = torch.zeros(max(need, 4096), dtype=torch.uint8, device=dev)
    return ws


def grid_status(dev) -> int:
    """The status word the device's last grid call left (0: sound; non-zero: a wait inside the kernel gave up and -1 was written).
    Synchronises."""
    ws = _grid_ws.get(dev)
    return 0 if ws is None else int(ws[:4].view(torch.int32).item())


class FurthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz: torch.Tensor, npoint: int) -> torch.Tensor:
        """xyz (B,N,3) -> (B,npoint) int32 indices, starting from index 0 (subsample.py:77-100)."""
        assert xyz.is_contiguous()
        dev = on_device("pointops", xyz)
        xyz = _f32(xyz, "xyz")
        B, N, _ = xyz.size()
        out = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
        if N > N_GRID and B > 0 and npoint > 0:
            rc = call(load().u3d_furthest_point_sampling_grid, B, N, npoint, xyz, grid_workspace(B, xyz.device), out, dev=dev,
                      what="fps (grid)", accept=(STATUS_OVER_CAPACITY,))
            if rc != STATUS_OVER_CAPACITY:
                return out
        temp = torch.empty(B, N, dtype=torch.float32, device=xyz.device) if N > 8192 else None
        call(load().u3d_furthest_point_sampling, B, N, npoint, xyz, temp, out, dev=dev, what="fps")
        return out

    @staticmethod
    def backward(ctx, a=None):
        return None, None


furthest_point_sample = FurthestPointSampling.apply


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """features (B,C,N), idx (B,npoint) -> (B,C,npoint) (subsample.py:110-131)."""
        assert features.is_contiguous() and idx.is_contiguous()
        dev = on_device("pointops", features, idx)
        features, idx = _f32(features, "features"), _i32(idx, "idx")
        B, npoint = idx.size()
        _, C, N = features.size()
        out = torch.empty(B, C, npoint, dtype=torch.float32, device=features.device)
        call(load().u3d_gather_points, B, C, N, npoint, features, idx, out, dev=dev, what="gather")
        ctx.for_backwards = (idx, C, N)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, C, N = ctx.for_backwards
        B, npoint = idx.size()
        grad = torch.zeros(B, C, N, dtype=torch.float32, device=grad_out.device)
        g = _f32(grad_out, "grad_out").contiguous()
        call(load().u3d_gather_points_grad, B, C, N, npoint, g, idx, grad, dev=on_device("pointops", g, idx), what="gather grad")
        return grad, None


gather_operation = GatherOperation.apply


def fps(data: torch.Tensor, number: int) -> torch.Tensor:
    """data (B,N,C) -> the `number` furthest-point-sampled rows (subsample.py:151-160)."""
    idx = furthest_point_sample(data[:, :, :3].contiguous(), number)
    return torch.gather(data, 1, idx.unsqueeze(-1).long().expand(-1, -1, data.shape[-1]))


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """features (B,C,N), idx (B,npoint,nsample) -> (B,C,npoint,nsample) (group.py:76-99)."""
        assert features.is_contiguous() and idx.is_contiguous()
        dev = on_device("pointops", features, idx)
        features, idx = _f32(features, "features"), _i32(idx, "idx")
        B, npoint, nsample = idx.size()
        _, C, N = features.size()
        out = torch.empty(B, C, npoint, nsample, dtype=torch.float32, device=features.device)
        call(load().u3d_group_points, B, C, N, npoint, nsample, features, idx, out, dev=dev, what="group")
        ctx.for_backwards = (idx, N)
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor) -> Tuple[torch.Tensor, None]:
        idx, N = ctx.for_backwards
        B, C, npoint, nsample = grad_out.size()
        grad = torch.zeros(B, C, N, dtype=torch.float32, device=grad_out.device)
        g = _f32(grad_out, "grad_out").contiguous()
        call(load().u3d_group_points_grad, B, C, N, npoint, nsample, g, idx, grad, dev=on_device("pointops", g, idx), what="group grad")
        return grad, None


grouping_operation = GroupingOperation.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor) -> torch.Tensor:
        """xyz (B,N,3) support, new_xyz (B,npoint,3) centres -> (B,npoint,nsample) int32 (group.py:175-196)."""
        assert new_xyz.is_contiguous() and xyz.is_contiguous()
        dev = on_device("pointops", xyz, new_xyz)
        xyz, new_xyz = _f32(xyz, "xyz"), _f32(new_xyz, "new_xyz")
        B, N, _ = xyz.size()
        npoint = new_xyz.size(1)
        idx = torch.empty(B, npoint, nsample, dtype=torch.int32, device=xyz.device)
        call(load().u3d_ball_query, B, N, npoint, float(radius), nsample, new_xyz, xyz, idx, dev=dev, what="ball query")
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


ball_query = BallQuery.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown: torch.Tensor, known: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """unknown (B,N,3), known (B,M,3) -> (dist (B,N,3) L2 distances to the three nearest known points, idx (B,N,3) int32)
        (upsampling.py:11-35; the kernel returns squared distances, the wrapper takes the root like the reference)."""
        assert unknown.is_contiguous() and known.is_contiguous()
        dev = on_device("pointops", unknown, known)
        unknown, known = _f32(unknown, "unknown"), _f32(known, "known")
        B, N, _ = unknown.size()
        m = known.size(1)
        dist2 = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        idx = torch.empty(B, N, 3, dtype=torch.int32, device=dev)
        call(load().u3d_three_nn, B, N, m, unknown, known, dist2, idx, dev=dev, what="three_nn")
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
        """features (B,C,M), idx (B,n,3), weight (B,n,3) -> (B,C,n) (upsampling.py:43-67; inputs are cast to fp32 like the
        reference's custom_fwd(cast_inputs=torch.float32))."""
        assert features.is_contiguous() and idx.is_contiguous() and weight.is_contiguous()
        dev = on_device("pointops", features, idx, weight)
        features, idx, weight = _f32(features, "features"), _i32(idx, "idx"), _f32(weight, "weight")
        B, c, m = features.size()
        n = idx.size(1)
        ctx.three_interpolate_for_backward = (idx, weight, m)
        out = torch.empty(B, c, n, dtype=torch.float32, device=dev)
        call(load().u3d_three_interpolate, B, c, m, n, features, idx, weight, out, dev=dev, what="three_interpolate")
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        idx, weight, m = ctx.three_interpolate_for_backward
        B, c, n = grad_out.size()
        grad_features = torch.zeros(B, c, m, dtype=torch.float32, device=grad_out.device)
        g = _f32(grad_out, "grad_out").contiguous()
        call(load().u3d_three_interpolate_grad, B, c, n, m, g, idx, weight, grad_features, dev=on_device("pointops", g, idx, weight),
             what="three_interpolate grad")
        return grad_features, None, None


three_interpolate = ThreeInterpolate.apply


def three_interpolation(unknown_xyz, known_xyz, know_feat):
    """Inverse-distance interpolation of `know_feat` (B,C,M) at `unknown_xyz` (B,N,3) (upsampling.py:92-101)."""
    dist, idx = three_nn(unknown_xyz, known_xyz)
    dist_recip = 1.0 / (dist + 1e-8)
    norm = torch.sum(dist_recip, dim=2, keepdim=True)
    weight = dist_recip / norm
    return three_interpolate(know_feat, idx, weight)


class QueryAndGroup(nn.Module):
    """group.py:208-260 (relative_xyz / normalize_dp / return_only_idx options)."""

    def __init__(self, radius: float, nsample: int, relative_xyz=True, normalize_dp=False, return_only_idx=False, **kwargs):
        super().__init__()
        self.radius, self.nsample = radius, nsample
        self.relative_xyz, self.normalize_dp, self.return_only_idx = relative_xyz, normalize_dp, return_only_idx

    def forward(self, query_xyz: torch.Tensor, support_xyz: torch.Tensor, features: torch.Tensor = None):
        idx = ball_query(self.radius, self.nsample, support_xyz, query_xyz)
        if self.return_only_idx:
            return idx
        grouped_xyz = grouping_operation(support_xyz.transpose(1, 2).contiguous(), idx)
        if self.relative_xyz:
            grouped_xyz = grouped_xyz - query_xyz.transpose(1, 2).unsqueeze(-1)
            if self.normalize_dp:
                grouped_xyz = grouped_xyz / self.radius
        grouped_features = grouping_operation(features, idx) if features is not None else None
        return grouped_xyz, grouped_features
