"""The object-level image branch evaluated only at the pixels the fusion reads.  The reference runs
`image_conv = Sequential(GroupNorm(32, 128, eps=1e-6), Conv2d(128, feature_dim, 1))` over the whole decoder map
(model/gaussian_predictor.py:139, 210-214) and `FeatureFusion` then reads one pixel column per point that wins its z-test
(fusion/feat_fusion.py:86-131).  Here the map is read once, for GroupNorm's statistics; normalisation and convolution run on the
gathered rows in libunipre3d_image_fusion.so (include/unipre3d_image_fusion.h, csrc/u3d_image_fusion.hip), forward and backward, and
no (B, ., H, W) tensor is made or kept:

  ImageConv(in_channels, out_channels, num_groups=32, eps=1e-6)
        the reference's Sequential (children "0" and "1", the same state_dict keys); forward(x) stays the dense evaluation,
        deferred(x) returns a DeferredImageFeatures handle that the backbones pass through like the tensor
  FeatureFusion(fusion_mlp)
        fusion.FeatureFusion whose mapped_features takes the sparse path for a handle and the existing path for a tensor
  sample_at_points(conv, decoder_features, camera_points, fx, fy, cx, cy, stats=None) -> (mapped (B, N, Cout), sel (B, N))
        the functional core: one autograd function with gradients to the four parameters and none to the map

Selection and gather are the existing u3d_zbuffer_fusion_forward on the raw map with C = Cin, so the pixel rounding, the H/W swap and
the ties are the ones already pinned to the reference.  Deterministic, no host read, graph-capturable.

Scope: fp32, contiguous NCHW on the device, in_channels % num_groups == 0, in_channels and out_channels <= 8192, B N < 2^31.  The map is
frozen (the VAE is): a map that requires grad raises NotImplementedError -- forward(x) is the path for that.  A non-contiguous map raises
ValueError (no hidden copy of a 268 MB tensor), other dtypes NotImplementedError, CPU tensors RuntimeError; a missing library raises.
The scene-level PointFusion uses every pixel and keeps the dense path."""
from __future__ import annotations

import ctypes
import os

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, fusion
from ._lib import byte_buffer, call, dense, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_image_fusion.so")
ABI_VERSION = 1
MAX_CHANNELS = 8192                               # include/unipre3d_image_fusion.h

_i, _f, _vp, _ll = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong
SIGNATURES = {   # include/unipre3d_image_fusion.h
    "u3d_imgfus_abi_version": (_i, []),
    "u3d_imgfus_stats_chunks": (_i, [_i, _i, _i, _i]),
    "u3d_imgfus_row_splits": (_i, [_ll]),
    "u3d_imgfus_stats_scratch_bytes": (ctypes.c_size_t, [_i] * 5),
    "u3d_imgfus_backward_scratch_bytes": (ctypes.c_size_t, [_i] * 4),
    "u3d_imgfus_stats": (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "u3d_imgfus_rows_forward": (_i, [_vp] * 7 + [_i] * 5 + [_vp, _vp]),
    "u3d_imgfus_rows_backward": (_i, [_vp] * 7 + [_i] * 5 + [_vp] * 6),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_image_fusion.so", SIGNATURES, ("u3d_imgfus_abi_version", ABI_VERSION))


def _check_map(x, num_groups):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError("the decoder map must be a (B, C, H, W) tensor")
    dev = on_device("image_fusion", x)
    if x.dtype != torch.float32:
        raise NotImplementedError(f"unipre3d_amd.image_fusion is fp32 only (got {x.dtype}); ImageConv.forward is the dense path")
    if x.requires_grad:
        raise NotImplementedError("the sparse path treats the decoder map as frozen; a map that requires grad takes ImageConv.forward")
    if not x.is_contiguous():
        raise ValueError("the decoder map must be contiguous NCHW (no hidden copy of the map is made)")
    if x.data_ptr() % 16:
        raise ValueError("the decoder map must be 16-byte aligned")
    C = x.shape[1]
    if C % num_groups or C > MAX_CHANNELS:
        raise ValueError(f"{C} channels in {num_groups} groups is outside the library's shapes")
    return dev


def group_stats(x: torch.Tensor, num_groups: int, eps: float) -> torch.Tensor:
    """(B, G, 2) fp32: mean and 1 / sqrt(biased variance + eps) of every (image, group) of the contiguous fp32 map."""
    dev = _check_map(x, num_groups)
    lib = load()
    B, C, H, W = x.shape
    stats = torch.empty(B, num_groups, 2, dtype=torch.float32, device=dev)
    scratch = byte_buffer(lib.u3d_imgfus_stats_scratch_bytes(B, C, num_groups, H, W), dev)
    call(lib.u3d_imgfus_stats, x, B, C, num_groups, H, W, float(eps), stats, scratch, dev=dev)
    return stats


class _SampleRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gamma, beta, weight, bias, x, stats, cp, G, fx, fy, cx, cy):
        dev = on_device("image_fusion", x, stats, cp, gamma, beta, weight, bias)
        B, Cin, H, W = x.shape
        N = cp.shape[1]
        Cout = weight.shape[0]
        cp = cp.detach().contiguous().float()
        if cp.data_ptr() % 16:                       # (a slice of a larger tensor)
            cp = cp.clone()
        rows = torch.empty(B, N, Cin, dtype=torch.float32, device=dev)
        sel = torch.empty(B, N, dtype=torch.int32, device=dev)
        flib = fusion.load()
        zbuf = torch.empty((flib.u3d_zbuffer_fusion_zbuf_bytes(B, H, W) + 7) // 8, dtype=torch.int64, device=dev)
        call(flib.u3d_zbuffer_fusion_forward, B, N, Cin, H, W, fx, fy, cx, cy, cp, x, rows, sel, zbuf, dev=dev)
        g, b, w, bi = dense(gamma, (Cin,)), dense(beta, (Cin,)), dense(weight, (Cout, Cin)), dense(bias, (Cout,))
        out = torch.empty(B, N, Cout, dtype=torch.float32, device=dev)
        call(load().u3d_imgfus_rows_forward, rows, sel, stats, g, b, w, bi, B, N, Cin, G, Cout, out, dev=dev)
        ctx.save_for_backward(rows, sel, stats, g, b, w)
        ctx.dims = (B, N, Cin, G, Cout)
        ctx.shapes = (gamma.shape, beta.shape, weight.shape, bias.shape)
        ctx.mark_non_differentiable(sel)
        return out, sel

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dsel):
        rows, sel, stats, g, b, w = ctx.saved_tensors
        B, N, Cin, G, Cout = ctx.dims
        dev = rows.device
        lib = load()
        dout = dout.contiguous().float()
        if dout.data_ptr() % 16:
            dout = dout.clone()
        f32 = dict(dtype=torch.float32, device=dev)
        dW, dbias = torch.empty(Cout, Cin, **f32), torch.empty(Cout, **f32)
        dgamma, dbeta = torch.empty(Cin, **f32), torch.empty(Cin, **f32)
        scratch = byte_buffer(lib.u3d_imgfus_backward_scratch_bytes(B, N, Cin, Cout), dev)
        call(lib.u3d_imgfus_rows_backward, dout, rows, sel, stats, g, b, w, B, N, Cin, G, Cout, dW, dbias, dgamma, dbeta, scratch, dev=dev)
        sg, sb, sw, sbi = ctx.shapes
        return (dgamma.reshape(sg), dbeta.reshape(sb), dW.reshape(sw), dbias.reshape(sbi)) + (None,) * 8


def sample_at_points(conv, decoder_features, camera_points, fx, fy, cx, cy, stats=None):
    """conv(decoder_features) at the pixels of the points that win their z-test: (mapped (B, N, Cout) with +0.0 rows for every other
    point, sel (B, N) int32 pixel index px * W + py or -1).  camera_points (B, N, 4) are fusion.FeatureFusion.camera_points; `stats` are
    group_stats of the map where they are already known (DeferredImageFeatures keeps them)."""
    norm, lin = conv[0], conv[1]
    dev = _check_map(decoder_features, norm.num_groups)
    on_device("image_fusion", camera_points, norm.weight, norm.bias, lin.weight, lin.bias)
    if camera_points.dim() != 3 or camera_points.shape[0] != decoder_features.shape[0] or camera_points.shape[2] != 4:
        raise ValueError("camera_points must be (B, N, 4) with one image of the map per item")
    if decoder_features.shape[1] != norm.num_channels or lin.weight.shape[1] != norm.num_channels or lin.weight.shape[2:] != (1, 1):
        raise ValueError("the map's channels do not fit the modules")
    if lin.weight.shape[0] > MAX_CHANNELS:
        raise ValueError("more output channels than the library takes")
    for p in (norm.weight, norm.bias, lin.weight, lin.bias):
        if p is None or p.dtype != torch.float32:
            raise NotImplementedError("unipre3d_amd.image_fusion needs fp32 affine GroupNorm and a biased convolution")
    if stats is None:
        stats = group_stats(decoder_features, norm.num_groups, norm.eps)
    assert stats.device == dev
    return _SampleRows.apply(norm.weight, norm.bias, lin.weight, lin.bias, decoder_features, stats, camera_points, norm.num_groups,
                             float(fx), float(fy), float(cx), float(cy))


class DeferredImageFeatures:
    """What ImageConv would return for `x`, not evaluated: the backbones hand it on to FeatureFusion, which evaluates it at the fused
    pixels.  GroupNorm's statistics are computed once, at the first use (PointMLP and PCM may fuse at more than one stage)."""

    def __init__(self, conv: "ImageConv", x: torch.Tensor):
        _check_map(x, conv[0].num_groups)
        self.conv, self.x = conv, x
        self._stats = None

    @property
    def shape(self):
        B, _, H, W = self.x.shape
        return torch.Size((B, self.conv[1].out_channels, H, W))

    @property
    def device(self):
        return self.x.device

    @property
    def dtype(self):
        return self.x.dtype

    def stats(self) -> torch.Tensor:
        if self._stats is None:
            self._stats = group_stats(self.x, self.conv[0].num_groups, self.conv[0].eps)
        return self._stats

    def materialize(self) -> torch.Tensor:
        return self.conv(self.x)


class ImageConv(nn.Sequential):
    """model/gaussian_predictor.py:210-214 as a module of its own: the same children under the same names."""

    def __init__(self, in_channels: int, out_channels: int, num_groups: int = 32, eps: float = 1e-6):
        super().__init__(nn.GroupNorm(num_groups, in_channels, eps=eps), nn.Conv2d(in_channels, out_channels, kernel_size=1))

    def deferred(self, x: torch.Tensor) -> DeferredImageFeatures:
        return DeferredImageFeatures(self, x)


class FeatureFusion(fusion.FeatureFusion):
    """fusion.FeatureFusion that also takes a DeferredImageFeatures where the reference takes the image features."""

    def mapped_features(self, center, image_features, c2w_projection_matrix, intrinsic):
        if not isinstance(image_features, DeferredImageFeatures):
            return super().mapped_features(center, image_features, c2w_projection_matrix, intrinsic)
        if image_features.shape[0] != center.shape[0]:
            raise ValueError("one image per item of `center` is needed")
        if c2w_projection_matrix.dim() == 4:
            c2w_projection_matrix = c2w_projection_matrix[:, 0]
        cp = self.camera_points(center, c2w_projection_matrix)
        fx, fy = float(intrinsic[0][0]), float(intrinsic[1][1])
        cx, cy = float(intrinsic[0][2]), float(intrinsic[1][2])
        mapped, _ = sample_at_points(image_features.conv, image_features.x, cp, fx, fy, cx, cy, stats=image_features.stats())
        return mapped
