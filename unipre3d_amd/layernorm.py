"""mamba_ssm's fused residual-add + LayerNorm / RMSNorm (`ops/triton/layernorm.py`) on the device, with its names and argument orders:
`RMSNorm`, `layer_norm_fn` and `rms_norm_fn` are what PCM.py, PCM's mamba_layer.py and Mamba3D's mamba_simple.py import
(INTEGRATION.md).  Kernels: libunipre3d_mambaops.so (include/unipre3d_mambaops.h, csrc/u3d_mambaops.hip), which
unipre3d_amd.causal_conv1d binds: one wave per row with the row in registers, the centred variance, one forward launch, one backward
launch plus a fixed-order reduce of the per-wave weight / bias partials (no float atomics: two calls give the same bits).

Scope: fp32, 1 <= N <= max_n() (1024); anything else raises (there is no fallback).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call, on_device
from .causal_conv1d import load

EXPORTS = ("u3d_addnorm_max_n", "u3d_addnorm_bwd_waves", "u3d_addnorm_bwd_scratch_bytes", "u3d_addnorm_fwd", "u3d_addnorm_bwd")


def max_n() -> int:
    """The widest row the kernels take."""
    return int(load().u3d_addnorm_max_n())


def bwd_waves(M: int) -> int:
    """Waves that share the M rows in the backward: wave g owns M // waves rows, one more when g < M % waves."""
    return int(load().u3d_addnorm_bwd_waves(int(M)))


class _AddNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, eps, prenorm, is_rms_norm):
        lib = load()
        shape = x.shape
        N = shape[-1]
        x2 = x.reshape(-1, N).contiguous()
        M = x2.shape[0]
        res2 = residual.reshape(-1, N).contiguous() if residual is not None else None
        weight = weight.contiguous()
        bias = bias.contiguous() if bias is not None else None
        dev = x.device
        y = torch.empty_like(x2)
        r = torch.empty_like(x2) if (residual is not None or prenorm) else None
        mean = torch.empty(M, dtype=torch.float32, device=dev) if not is_rms_norm else None
        rstd = torch.empty(M, dtype=torch.float32, device=dev)
        call(lib.u3d_addnorm_fwd, x2, res2, weight, bias, y, r, mean, rstd, M, N, float(eps), int(is_rms_norm), dev=dev)
        ctx.save_for_backward(r if r is not None else x2, weight, mean, rstd)
        ctx.cfg = (shape, residual is not None, bias is not None, prenorm, is_rms_norm)
        return (y.reshape(shape), r.reshape(shape)) if prenorm else y.reshape(shape)

    @staticmethod
    def backward(ctx, dy, *rest):
        r, weight, mean, rstd = ctx.saved_tensors
        shape, has_residual, has_bias, prenorm, is_rms_norm = ctx.cfg
        lib = load()
        M, N = r.shape
        dev = r.device
        dy = dy.to(torch.float32).reshape(M, N).contiguous()
        dres = rest[0].to(torch.float32).reshape(M, N).contiguous() if prenorm else None
        dx = torch.empty_like(r)
        dweight = torch.empty_like(weight)
        dbias = torch.empty_like(weight) if has_bias else None
        nbytes = int(lib.u3d_addnorm_bwd_scratch_bytes(M, N))
        buf, base = _lib.scratch(nbytes, dev)
        call(lib.u3d_addnorm_bwd, dy, dres, r, weight, mean, rstd, dx, dweight, dbias, base, nbytes, M, N, int(is_rms_norm), dev=dev)
        dx = dx.reshape(shape)
        return dx, dweight, dbias, (dx if has_residual else None), None, None, None


def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False):
    """mamba_ssm's layer_norm_fn:  r = x (+ residual);  y = (r - mean) rsqrt(var + eps) weight (+ bias) with the centred variance, or
    y = r rsqrt(mean(r^2) + eps) weight (+ bias) when is_rms_norm.  x (..., N), residual like x, weight and bias (N,), fp32 on the device.
    Returns y, or (y, r) when prenorm; both have x's shape.  Differentiable in x, weight, bias and residual (x and residual receive the
    same gradient, to which the gradient arriving on r is added).  residual_in_fp32 is accepted; everything is fp32 already."""
    for name, t in (("x", x), ("weight", weight), ("bias", bias), ("residual", residual)):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"{name}: dtype {t.dtype} is not implemented (fp32 only)")
    if x.dim() < 1 or x.numel() < 1:
        raise ValueError(f"x: expected a non-empty (..., N) tensor, got {tuple(x.shape)}")
    N = x.shape[-1]
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"residual: expected {tuple(x.shape)}, got {tuple(residual.shape)}")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and tuple(t.shape) != (N,):
            raise ValueError(f"{name}: expected ({N},), got {tuple(t.shape)}")
    if N > max_n():
        raise NotImplementedError(f"x: rows of {N} elements are not implemented (at most {max_n()})")
    on_device("layernorm", x, weight, bias, residual)
    return _AddNorm.apply(x, weight, bias, residual, float(eps), bool(prenorm), bool(is_rms_norm))


def rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6):
    """mamba_ssm's rms_norm_fn: layer_norm_fn with is_rms_norm (note the argument order: eps is last)."""
    return layer_norm_fn(x, weight, bias, residual, eps, prenorm, residual_in_fp32, True)


class RMSNorm(torch.nn.Module):
    """mamba_ssm's RMSNorm module: weight initialised to ones, bias registered as None, eps 1e-5."""

    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.empty(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False):
        return rms_norm_fn(x, self.weight, self.bias, residual=residual, prenorm=prenorm, residual_in_fp32=residual_in_fp32, eps=self.eps)
