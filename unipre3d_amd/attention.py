"""Variable-length packed-QKV attention on the device, with flash-attn's name and argument order:
`import unipre3d_amd.attention as flash_attn` is the switch for PTv3's SerializedAttention.  The kernels are in
libunipre3d_attention.so (include/unipre3d_attention.h, csrc/u3d_attention.hip): fp16 v_mfma_f32_16x16x16_f16 tiles, fp32 scores,
row statistics and accumulation, one rounding on the way out; one wave per (sequence, head) up to 64 keys, one workgroup above.

Scope: fp16, head dim 16, non-causal, no dropout, max_seqlen <= 1024; anything else raises (there is no fallback).
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_attention.so")
ABI_VERSION = 1
MAX_SEQLEN = 1024
HEAD_DIM = 16

_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_attention.h (the segment_csr pair is scatter.py's)
    "u3d_attn_abi_version": (_i, []),
    "u3d_attn_varlen_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "u3d_attn_varlen_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "u3d_segment_csr_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "u3d_segment_csr_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_attention.so", SIGNATURES, ("u3d_attn_abi_version", ABI_VERSION))


class _VarlenAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, softmax_scale):
        T, _, H, D = qkv.shape
        S = cu_seqlens.numel() - 1
        out = torch.empty(T, H, D, dtype=torch.float16, device=qkv.device)
        lse = torch.empty(H, T, dtype=torch.float32, device=qkv.device)
        if T > 0:
            call(load().u3d_attn_varlen_fwd, qkv, cu_seqlens, out, lse, T, S, H, D, max_seqlen, softmax_scale, dev=qkv.device)
        ctx.save_for_backward(qkv, cu_seqlens, out, lse)
        ctx.args = (max_seqlen, softmax_scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, cu_seqlens, out, lse = ctx.saved_tensors
        max_seqlen, softmax_scale = ctx.args
        T, _, H, D = qkv.shape
        dout = dout.to(torch.float16).contiguous()
        dqkv = torch.empty_like(qkv)
        if T > 0:
            call(load().u3d_attn_varlen_bwd, qkv, cu_seqlens, out, dout, lse, dqkv, T, cu_seqlens.numel() - 1, H, D, max_seqlen,
                 softmax_scale, dev=qkv.device)
        return dqkv, None, None, None


def flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False, **kw):
    """flash-attn's varlen packed-QKV attention, non-causal: for every sequence s and head h, with rows
    r = cu_seqlens[s] .. cu_seqlens[s+1]-1, out[r, h] = softmax(softmax_scale * q[r, h] . k[r', h]) @ v[r', h].

    qkv (T, 3, H, 16) fp16 contiguous on the device; cu_seqlens (S+1,) int32 on the device, ascending from 0, last entry <= T;
    max_seqlen: a host int in 1 .. 1024 (it selects the kernel and sizes its LDS; the device is never read from the host).
    softmax_scale None = 16 ** -0.5.  Returns (T, H, 16) fp16; differentiable with respect to qkv.  Rows at or beyond cu_seqlens[S]
    come out as zeros and receive a zero gradient.  A zero-length sequence is legal.  A sequence longer than max_seqlen is a caller
    error: only its first max_seqlen rows attend (to one another); the rows after them come out as zeros with a zero gradient, and
    nothing outside the tensors is read or written.  Keyword arguments of flash-attn that change the result (window_size,
    softcap, alibi_slopes, return_attn_probs) must be at their neutral values; `deterministic` is accepted and always true."""
    if dropout_p != 0.0:
        raise NotImplementedError(f"dropout_p={dropout_p}: dropout inside attention is not implemented (pass 0.0)")
    if causal:
        raise NotImplementedError("causal=True is not implemented")
    for name, neutral in (("window_size", ((-1, -1), [-1, -1], None)), ("softcap", (0.0, None)), ("alibi_slopes", (None,)),
                          ("return_attn_probs", (False, None))):
        if name in kw and not any(kw[name] is n or kw[name] == n for n in neutral):
            raise NotImplementedError(f"{name}={kw[name]!r} is not implemented")
    unknown = set(kw) - {"window_size", "softcap", "alibi_slopes", "return_attn_probs", "deterministic"}
    if unknown:
        raise TypeError(f"flash_attn_varlen_qkvpacked_func: unexpected arguments {sorted(unknown)}")
    load()
    dev = on_device("attention", qkv, cu_seqlens)
    if qkv.dim() != 4 or qkv.shape[1] != 3:
        raise ValueError(f"qkv: expected (T, 3, H, D), got {tuple(qkv.shape)}")
    if qkv.dtype != torch.float16:
        raise NotImplementedError(f"qkv: dtype {qkv.dtype} is not implemented (fp16 only)")
    if qkv.shape[3] != HEAD_DIM:
        raise NotImplementedError(f"qkv: head dim {qkv.shape[3]} is not implemented (D == {HEAD_DIM} only)")
    if qkv.shape[2] < 1:
        raise ValueError("qkv: at least one head")
    if not qkv.is_contiguous():
        raise ValueError("qkv: a non-contiguous tensor is not supported (call .contiguous())")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1 or not cu_seqlens.is_contiguous():
        raise ValueError(f"cu_seqlens: expected a contiguous (S+1,) int32 tensor, got {tuple(cu_seqlens.shape)} {cu_seqlens.dtype}")
    max_seqlen = int(max_seqlen)
    if max_seqlen > MAX_SEQLEN:
        raise NotImplementedError(f"max_seqlen={max_seqlen} is not implemented (at most {MAX_SEQLEN})")
    if max_seqlen < 1:
        raise ValueError(f"max_seqlen={max_seqlen}: must be at least 1")
    scale = float(HEAD_DIM ** -0.5 if softmax_scale is None else softmax_scale)
    return _VarlenAttention.apply(qkv, cu_seqlens, max_seqlen, scale)
