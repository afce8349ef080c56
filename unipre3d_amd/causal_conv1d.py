"""The causal depthwise conv1d (+ SiLU) of a Mamba block on the device, with the `causal_conv1d` package's names and argument order:
`causal_conv1d_fn` is what the mamba3d and pcm trees' `selective_scan_interface.py` and `mamba_simple.py` import.
The kernels are in libunipre3d_mambaops.so (include/unipre3d_mambaops.h, csrc/u3d_mambaops.hip), which unipre3d_amd.layernorm shares:
one wave per (batch, channel) row, one step per lane, the earlier taps taken from the neighbouring lanes.

Scope: fp32, width 2 .. 4, activation None | "silu" | "swish"; anything else raises (there is no fallback).  `causal_conv1d_update`
(the inference step) is not provided and is None, the value the reference's `if causal_conv1d_update is None` branches test for.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import call, on_device

ABI_VERSION = 1
MIN_WIDTH, MAX_WIDTH = 2, 4

_i, _vp, _sz, _i64, _f = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_float
SIGNATURES = {   # include/unipre3d_mambaops.h
    "u3d_mambaops_abi_version": (_i, []),
    "u3d_cconv_chunk_len": (_i, [_i]),
    "u3d_cconv_bwd_scratch_bytes": (_sz, [_i, _i]),
    "u3d_cconv_fwd": (_i, [_vp] * 4 + [_i64] * 2 + [_i] * 5 + [_vp]),
    "u3d_cconv_bwd": (_i, [_vp] * 8 + [_sz] + [_i64] * 2 + [_i] * 5 + [_vp]),
    "u3d_addnorm_max_n": (_i, []),
    "u3d_addnorm_bwd_waves": (_i, [_i]),
    "u3d_addnorm_bwd_scratch_bytes": (_sz, [_i, _i]),
    "u3d_addnorm_fwd": (_i, [_vp] * 8 + [_i, _i, _f, _i] + [_vp]),
    "u3d_addnorm_bwd": (_i, [_vp] * 10 + [_sz] + [_i] * 3 + [_vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_mambaops.so", SIGNATURES, ("u3d_mambaops_abi_version", ABI_VERSION))


def chunk_len(L: int) -> int:
    """Steps a wave covers of its row before it moves on, at sequence length L (64 lanes x 1 .. 4 steps)."""
    return int(load().u3d_cconv_chunk_len(int(L)))


class _CausalConv1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, silu):
        lib = load()
        Bsz, D, L = x.shape
        out = torch.empty(Bsz, D, L, dtype=torch.float32, device=x.device)
        call(lib.u3d_cconv_fwd, x, weight, bias, out, x.stride(0), x.stride(1), Bsz, D, L, weight.shape[1], int(silu), dev=x.device)
        ctx.save_for_backward(x, weight, bias)
        ctx.silu = silu
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, bias = ctx.saved_tensors
        lib = load()
        Bsz, D, L = x.shape
        dout = dout.to(torch.float32).contiguous()
        dx = torch.empty(Bsz, D, L, dtype=torch.float32, device=x.device)
        dweight = torch.empty_like(weight)
        dbias = torch.empty_like(bias) if bias is not None else None
        nbytes = int(lib.u3d_cconv_bwd_scratch_bytes(Bsz, D))
        buf, base = _lib.scratch(nbytes, x.device)
        call(lib.u3d_cconv_bwd, x, weight, bias, dout, dx, dweight, dbias, base, nbytes, x.stride(0), x.stride(1), Bsz, D, L,
             weight.shape[1], int(ctx.silu), dev=x.device)
        return dx, dweight, dbias, None


def causal_conv1d_fn(x, weight, bias=None, activation=None):
    """causal_conv1d's causal_conv1d_fn:  out[b,d,l] = act(bias[d] + sum_w weight[d,w] x[b,d,l-(W-1)+w]),  x zero at negative steps.
    x (B, D, L); weight (D, W) with W in 2 .. 4; bias (D,) or None; activation None | "silu" | "swish"; all fp32 on the device.
    Returns out (B, D, L), dense.  Differentiable in x, weight and bias; the backward recomputes the pre-activation from x.
    x needs only stride(2) == 1: a channel slice such as xz.chunk(2, dim=1)[0] is read in place; any other layout is made dense."""
    if activation not in (None, "silu", "swish"):
        raise NotImplementedError("activation must be None, silu, or swish")
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"{name}: dtype {t.dtype} is not implemented (fp32 only)")
    if x.dim() != 3:
        raise ValueError(f"x: expected (B, D, L), got {tuple(x.shape)}")
    Bsz, D, L = x.shape
    if Bsz < 1 or D < 1 or L < 1:
        raise ValueError(f"x: empty tensor {tuple(x.shape)}")
    if weight.dim() != 2 or weight.shape[0] != D:
        raise ValueError(f"weight: expected ({D}, W), got {tuple(weight.shape)}")
    if not MIN_WIDTH <= weight.shape[1] <= MAX_WIDTH:
        raise NotImplementedError(f"weight: width {weight.shape[1]} is not implemented ({MIN_WIDTH} .. {MAX_WIDTH} only)")
    if bias is not None and tuple(bias.shape) != (D,):
        raise ValueError(f"bias: expected ({D},), got {tuple(bias.shape)}")
    load()
    on_device("causal_conv1d", x, weight, bias)
    if x.stride(2) != 1:
        x = x.contiguous()
    return _CausalConv1d.apply(x, weight.contiguous(), None if bias is None else bias.contiguous(), activation is not None)


causal_conv1d_update = None
