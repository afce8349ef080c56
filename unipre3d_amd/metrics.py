"""PSNR and SSIM of image stacks on the device, with the names and call shapes of the reference's evaluation loop, backed by
libunipre3d_metrics.so (include/unipre3d_metrics.h); no CPU fallback.

  ssim             utils/loss_utils.py:58-87 (`from utils.loss_utils import ssim as ssim_fn`, eval.py:17), differentiable in img1
  psnr             eval.py:28-30, per image
  image_metrics    both and the "target is not all zero" flag of eval.py:122 from one pass, without a host read
  evaluate_views   the aggregation of eval.py:121-176 (PSNR / SSIM of the conditioning and of the novel views)

One forward pass reads both stacks once and yields, per image, the mean SSIM, the sum of squared differences and whether the target is
all zero; per-tile partial sums are added in a fixed order, so the same input gives the same bits.  SSIM's gradient with respect to
img1 is a second kernel over three derivative maps the forward stores only when a gradient is needed.  Everything runs on torch's
current stream; `image_metrics` is capturable into a HIP graph.  A NaN in one image reaches that image's outputs only.

Deviation from the reference, in `evaluate_views` only: where eval.py divides by zero -- an example none of whose conditioning (or novel)
views has a non-zero target -- that example is left out of that class's mean over examples; with no example left the result is NaN.
LPIPS is not built (its VGG weights are not part of this project)."""
from __future__ import annotations

import ctypes
import math
import os

import torch

from . import _lib
from ._lib import as_f32, call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_metrics.so")
TILE, HALO = 32, 5                                             # include/unipre3d_metrics.h: U3D_METRICS_TILE, U3D_METRICS_HALO

_i, _vp = ctypes.c_int, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_metrics.h
    "u3d_metrics_tiles": (_i, [_i, _i, _i]),
    "u3d_metrics_forward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "u3d_metrics_ssim_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_metrics.so", SIGNATURES)


def _pair(img1, img2, what):
    """Both stacks as contiguous fp32 (N, C, H, W) on one HIP device; a 3-D input is one image."""
    if not torch.is_tensor(img1) or not torch.is_tensor(img2):
        raise TypeError(f"{what}: tensors expected")
    dev = on_device("metrics", img1, img2)
    if img1.shape != img2.shape:
        raise ValueError(f"{what}: the two stacks differ in shape, {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.dim() not in (3, 4):
        raise ValueError(f"{what}: (N,C,H,W) or (C,H,W) expected, got {tuple(img1.shape)}")
    a, b = as_f32(img1, "img1"), as_f32(img2, "img2")
    if a.dim() == 3:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.size(0) > 0 and min(a.shape[1:]) < 1:
        raise ValueError(f"{what}: empty images, {tuple(img1.shape)}")
    return dev, a, b


def _forward(dev, a, b, save):
    """-> (ssim (N,), sqsum (N,), all_zero (N,) int32, dmaps (3,N,C,H,W) or None)"""
    N, C, H, W = a.shape
    lib = load()
    tiles = lib.u3d_metrics_tiles(C, H, W) if N else 0
    partial = torch.empty(N * tiles * 3, dtype=torch.float32, device=dev)
    ssim_n = torch.empty(N, dtype=torch.float32, device=dev)
    sqsum = torch.empty(N, dtype=torch.float32, device=dev)
    all_zero = torch.empty(N, dtype=torch.int32, device=dev)
    dmaps = torch.empty((3, N, C, H, W), dtype=torch.float32, device=dev) if save else None
    if N:
        call(lib.u3d_metrics_forward, N, C, H, W, a, b, partial, ssim_n, sqsum, all_zero, dmaps, dev=dev, what="metrics forward")
    return ssim_n, sqsum, all_zero, dmaps


class _SSIM(torch.autograd.Function):
    """(N,C,H,W) fp32 contiguous pair -> per-image mean SSIM (N,); the gradient flows to img1 alone."""

    @staticmethod
    def forward(ctx, a, b, need):
        ssim_n, _, _, dmaps = _forward(a.device, a, b, need)
        if need:
            ctx.save_for_backward(a, b, dmaps)
        return ssim_n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        a, b, dmaps = ctx.saved_tensors
        N, C, H, W = a.shape
        weight = as_f32(grad, "grad_output")
        out = torch.empty_like(a)
        if N:
            call(load().u3d_metrics_ssim_backward, N, C, H, W, a, b, dmaps, weight, out, dev=a.device, what="ssim backward")
        return out, None, None


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """utils/loss_utils.py `ssim`: the mean of the SSIM map over everything (0-dim), or per image (N,) for size_average=False.
    Differentiable in img1; the map is symmetric, so a caller who needs the gradient of the other argument swaps the two."""
    if window_size != 11:
        raise NotImplementedError(f"SSIM is built for the reference's 11-tap window, got window_size = {window_size}")
    if torch.is_tensor(img2) and img2.requires_grad:
        raise NotImplementedError("SSIM's gradient is built for img1 only: swap the arguments (the map is symmetric)")
    _, a, b = _pair(img1, img2, "ssim")
    per_image = _SSIM.apply(a, b, a.requires_grad and torch.is_grad_enabled())
    return per_image.mean() if size_average else per_image


def _psnr(sqsum, count):
    """The division and the logarithm in fp64 on the (N,) vector, rounded to fp32 once: at 20-30 dB one fp32 rounding of log10's
    result is already 2e-6 dB, as much as the whole distance of the reference's fp32 line from its fp64 one."""
    return (-10.0 * torch.log10(sqsum.double() / count)).float()


@torch.no_grad()
def psnr(images: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """eval.py:28-30 per image: -10 log10(mean((image - target)^2)) -> (N,); identical images give +inf."""
    dev, a, b = _pair(images, targets, "psnr")
    _, sqsum, _, _ = _forward(dev, a, b, False)
    return _psnr(sqsum, float(math.prod(a.shape[1:])))


@torch.no_grad()
def image_metrics(images: torch.Tensor, targets: torch.Tensor) -> dict:
    """{"psnr": (N,), "ssim": (N,), "valid": (N,) bool}: `valid` is eval.py:122's `not torch.all(target == 0)`.  One launch chain on
    the current stream, no host read."""
    dev, a, b = _pair(images, targets, "image_metrics")
    ssim_n, sqsum, all_zero, _ = _forward(dev, a, b, False)
    return {"psnr": _psnr(sqsum, float(math.prod(a.shape[1:]))), "ssim": ssim_n, "valid": all_zero == 0}


@torch.no_grad()
def evaluate_views(images: torch.Tensor, targets: torch.Tensor, n_views: int, input_images: int) -> dict:
    """images, targets (B * n_views, 3, H, W), item-major as renderer.render_views stacks them -> 0-dim device tensors PSNR_cond,
    SSIM_cond, PSNR_novel, SSIM_novel as eval.py:121-176 forms them: per example the mean over its valid views of a class (view index
    below `input_images`: conditioning), then the mean over examples (module docstring: examples without a valid view of a class)."""
    n_views, input_images = int(n_views), int(input_images)
    if images.dim() != 4 or n_views < 1 or images.size(0) % n_views or not 0 <= input_images <= n_views:
        raise ValueError(f"(B * n_views, C, H, W) stacks with 0 <= input_images <= n_views expected, got {tuple(images.shape)}, "
                         f"n_views = {n_views}, input_images = {input_images}")
    m = image_metrics(images, targets)
    valid = m["valid"].view(-1, n_views)
    cond = torch.arange(n_views, device=valid.device) < input_images
    out = {}
    for cls, sel in (("cond", valid & cond), ("novel", valid & ~cond)):
        cnt = sel.sum(1)
        for name, key in (("PSNR", "psnr"), ("SSIM", "ssim")):
            v = m[key].view(-1, n_views)
            per_example = torch.where(sel, v, torch.zeros_like(v)).sum(1) / cnt.clamp(min=1)
            out[f"{name}_{cls}"] = torch.where(cnt > 0, per_example, torch.zeros_like(per_example)).sum() / (cnt > 0).sum()   # 0 / 0 = NaN
    return out
