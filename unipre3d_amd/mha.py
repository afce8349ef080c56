"""Dense fp32 multi-head attention for the transformer backbone (openpoints' PointTransformerEncoder, the reference's default
configuration): `from unipre3d_amd.mha import Attention` is the switch for the class of openpoints/models/backbone/transformer.py and
openpoints/models/layers/attention.py.  The kernels are in libunipre3d_mha.so (include/unipre3d_mha.h, csrc/u3d_mha.hip):
v_mfma_f32_16x16x4_f32 tiles (exact f32 fma chains), an online softmax over blocks of 64 keys, the packed qkv of the Linear read where
it lies and the (B, N, C) layout of proj written directly; the backward recomputes P from the row log-sum-exp.

Scope: fp32, head dim 64, N <= 1024, no mask, no dropout, not causal; anything else raises (there is no fallback).
"""
from __future__ import annotations

import ctypes
import os

import torch
from torch import nn

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_mha.so")
ABI_VERSION = 1
MAX_SEQLEN = 1024
HEAD_DIM = 64

_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_mha.h
    "u3d_mha_abi_version": (_i, []),
    "u3d_mha_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "u3d_mha_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_mha.so", SIGNATURES, ("u3d_mha_abi_version", ABI_VERSION))


class _PackedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, softmax_scale):
        B, N, _, H, D = qkv.shape
        out = torch.empty(B, N, H, D, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
        call(load().u3d_mha_fwd, qkv, out, lse, B, N, H, D, softmax_scale, dev=qkv.device)
        ctx.save_for_backward(qkv, out, lse)
        ctx.softmax_scale = softmax_scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, N, _, H, D = qkv.shape
        dout = dout.to(torch.float32).contiguous()
        dqkv = torch.empty_like(qkv)
        call(load().u3d_mha_bwd, qkv, out, dout, lse, dqkv, B, N, H, D, ctx.softmax_scale, dev=qkv.device)
        return dqkv, None


def attention_qkvpacked(qkv, softmax_scale=None):
    """out[b, n, h] = softmax_m(softmax_scale * q[b, n, h] . k[b, m, h]) @ v[b, m, h] with q, k, v = qkv[:, :, 0 / 1 / 2].

    qkv (B, N, 3, H, 64) fp32 contiguous on the device -- nn.Linear(dim, 3 dim)'s output, viewed; B, N, H >= 1, N <= 1024.
    softmax_scale None = 64 ** -0.5; it must be positive.  Returns (B, N, H, 64) fp32, which .view(B, N, C) turns into proj's input
    without a copy; differentiable with respect to qkv.  Between forward and backward qkv, the output and the (B, H, N) row
    log-sum-exp are kept; no N x N tensor exists at any time."""
    on_device("mha", qkv)
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"qkv: expected (B, N, 3, H, D), got {tuple(qkv.shape)}")
    if qkv.dtype != torch.float32:
        raise NotImplementedError(f"qkv: dtype {qkv.dtype} is not implemented (fp32 only)")
    B, N, _, H, D = qkv.shape
    if D != HEAD_DIM:
        raise NotImplementedError(f"qkv: head dim {D} is not implemented (D == {HEAD_DIM} only)")
    if N > MAX_SEQLEN:
        raise NotImplementedError(f"qkv: N={N} is not implemented (at most {MAX_SEQLEN})")
    if B < 1 or N < 1 or H < 1:
        raise ValueError(f"qkv: an empty tensor {tuple(qkv.shape)} is not supported")
    if not qkv.is_contiguous():
        raise ValueError("qkv: a non-contiguous tensor is not supported (call .contiguous())")
    scale = float(HEAD_DIM ** -0.5 if softmax_scale is None else softmax_scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"softmax_scale={scale}: must be a positive finite number")
    load()
    return _PackedAttention.apply(qkv, scale)


class Attention(nn.Module):
    """openpoints' Attention (models/backbone/transformer.py and models/layers/attention.py) with its constructor, its forward(x) for
    x (B, N, C) and its submodule names, so its state_dict loads unchanged; the core between qkv and proj is attention_qkvpacked."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        if attn_drop > 0:
            raise NotImplementedError(f"attn_drop={attn_drop}: dropout inside attention is not implemented (pass 0.0)")
        if dim % num_heads != 0 or dim // num_heads != HEAD_DIM:
            raise NotImplementedError(f"dim={dim}, num_heads={num_heads}: only heads of {HEAD_DIM} channels are implemented")
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        B, N, C = x.shape
        o = attention_qkvpacked(self.qkv(x).view(B, N, 3, self.num_heads, C // self.num_heads), self.scale)
        return self.proj_drop(self.proj(o.view(B, N, C)))
