"""Mamba's selective scan on the device, with mamba_ssm's names and argument order: `selective_scan_fn`, `mamba_inner_fn` and
`mamba_inner_fn_no_out_proj` are what the mamba3d and pcm mixers import from `selective_scan_interface`.  The kernels
are in libunipre3d_selective_scan.so (include/unipre3d_selective_scan.h, csrc/u3d_selective_scan.hip): a pair scan over L across the
lanes of a wave, the state carried from pass to pass, the backward as the same scan in reversed time.

Scope: fp32, real A of shape (D, 16), input-dependent B and C ((B, N, L) or (B, G, N, L)); anything else raises (there is no fallback).
"""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_selective_scan.so")
ABI_VERSION = 1
D_STATE = 16

_i, _vp, _sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
SIGNATURES = {   # include/unipre3d_selective_scan.h
    "u3d_sscan_abi_version": (_i, []),
    "u3d_sscan_pass_len": (_i, [_i]),
    "u3d_sscan_bwd_scratch_bytes": (_sz, [_i, _i, _i, _i]),
    "u3d_sscan_fwd": (_i, [_vp] * 11 + [_i] * 6 + [_vp]),
    "u3d_sscan_bwd": (_i, [_vp] * 19 + [_sz] + [_i] * 6 + [_vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_selective_scan.so", SIGNATURES, ("u3d_sscan_abi_version", ABI_VERSION))


def pass_len(L: int) -> int:
    """Steps one pass of a wave covers at sequence length L (the state is carried across ceil(L / pass_len) passes)."""
    return int(load().u3d_sscan_pass_len(int(L)))


class _SelectiveScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state):
        lib = load()
        Bsz, Dm, L = u.shape
        G = B.shape[1]
        npass = -(-L // lib.u3d_sscan_pass_len(L))
        out = torch.empty_like(u)
        last = torch.empty(Bsz, Dm, D_STATE, dtype=torch.float32, device=u.device) if return_last_state else None
        xsave = torch.empty(Bsz, Dm, npass, D_STATE, dtype=torch.float32, device=u.device) if npass > 1 else None
        call(lib.u3d_sscan_fwd, u, delta, A, B, C, D, z, delta_bias, out, last, xsave, Bsz, Dm, G, D_STATE, L, int(delta_softplus),
             dev=u.device)
        ctx.save_for_backward(u, delta, A, B, C, D, z, delta_bias, xsave)
        ctx.delta_softplus = bool(delta_softplus)
        if return_last_state:
            ctx.mark_non_differentiable(last)
            return out, last
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        u, delta, A, B, C, D, z, delta_bias, xsave = ctx.saved_tensors
        lib = load()
        Bsz, Dm, L = u.shape
        G = B.shape[1]
        dout = dout.to(torch.float32).contiguous()
        dev = u.device
        du, ddelta = torch.empty_like(u), torch.empty_like(u)
        dA, dB, dC = torch.empty_like(A), torch.empty_like(B), torch.empty_like(C)
        dD = torch.empty_like(D) if D is not None else None
        dz = torch.empty_like(z) if z is not None else None
        dbias = torch.empty_like(delta_bias) if delta_bias is not None else None
        nbytes = int(lib.u3d_sscan_bwd_scratch_bytes(Bsz, Dm, G, L))
        buf, base = _lib.scratch(nbytes, dev)
        call(lib.u3d_sscan_bwd, u, delta, A, B, C, D, z, delta_bias, dout, xsave, du, ddelta, dA, dB, dC, dD, dz, dbias, base, nbytes,
             Bsz, Dm, G, D_STATE, L, int(ctx.delta_softplus), dev=dev)
        return du, ddelta, dA, dB, dC, dD, dz, dbias, None, None


def _dense(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, return_last_state=False):
    """mamba_ssm's selective_scan_fn, real-valued case:
        dt = delta (+ delta_bias[d]), softplus when delta_softplus;  x_l = exp(dt_l A) x_{l-1} + dt_l B_l u_l;  y_l = C_l . x_l (+ D u_l);
        out = y (* silu(z)).
    u, delta, z (B, D, L); A (D, 16); B, C (B, 16, L) or (B, G, 16, L) with G dividing D; D, delta_bias (D); all fp32 on the device.
    Returns out (B, D, L), or (out, last_state (B, D, 16)) when return_last_state; the last state is detached, as upstream.
    Differentiable in every tensor argument; gradients of 3-D B / C come back 3-D.  Views (e.g. xz.chunk(2, dim=1)) are made dense."""
    load()
    tensors = {"u": u, "delta": delta, "A": A, "B": B, "C": C, "D": D, "z": z, "delta_bias": delta_bias}
    on_device("selective_scan", *tensors.values())
    if A.is_complex():
        raise NotImplementedError("A: complex A is not implemented (real A only)")
    for name, t in tensors.items():
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"{name}: dtype {t.dtype} is not implemented (fp32 only)")
    if u.dim() != 3 or delta.shape != u.shape:
        raise ValueError(f"u, delta: expected two (B, D, L) tensors, got {tuple(u.shape)} and {tuple(delta.shape)}")
    Bsz, Dm, L = u.shape
    if Bsz < 1 or Dm < 1 or L < 1:
        raise ValueError(f"u: empty tensor {tuple(u.shape)}")
    if A.dim() != 2 or A.shape[0] != Dm or A.shape[1] != D_STATE:
        raise NotImplementedError(f"A: expected ({Dm}, {D_STATE}), got {tuple(A.shape)} (d_state == {D_STATE} only)")
    for name, t in (("B", B), ("C", C)):
        if t.dim() == 2:
            raise NotImplementedError(f"{name}: a constant (D, N) {name} is not implemented (input-dependent (B, N, L) or (B, G, N, L) only)")
        if t.dim() not in (3, 4):
            raise ValueError(f"{name}: expected (B, N, L) or (B, G, N, L), got {tuple(t.shape)}")
    B4 = B.unsqueeze(1) if B.dim() == 3 else B
    C4 = C.unsqueeze(1) if C.dim() == 3 else C
    G = B4.shape[1]
    if tuple(B4.shape) != (Bsz, G, D_STATE, L) or tuple(C4.shape) != (Bsz, G, D_STATE, L):
        raise ValueError(f"B, C: expected ({Bsz}, G, {D_STATE}, {L}) with one G, got {tuple(B.shape)} and {tuple(C.shape)}")
    if G < 1 or Dm % G != 0:
        raise ValueError(f"B, C: {G} groups do not divide D = {Dm}")
    for name, t in (("D", D), ("delta_bias", delta_bias)):
        if t is not None and tuple(t.shape) != (Dm,):
            raise ValueError(f"{name}: expected ({Dm},), got {tuple(t.shape)}")
    if z is not None and z.shape != u.shape:
        raise ValueError(f"z: expected {tuple(u.shape)}, got {tuple(z.shape)}")
    return _SelectiveScan.apply(_dense(u), _dense(delta), _dense(A), _dense(B4), _dense(C4), _dense(D), _dense(z), _dense(delta_bias),
                                bool(delta_softplus), bool(return_last_state))


def mamba_inner_fn_no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B=None, C=None, D=None,
                               delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True):
    """The Mamba mixer between in_proj and out_proj, mamba_ssm's argument list: xz (B, 2 d_inner, L) -> (B, d_inner, L).
    Depthwise causal conv1d (left padding width - 1) + SiLU on x, x_proj, the dt_proj weight product, B and C from x_proj unless given,
    then the selective scan gated by z.  The conv and the projections are torch (MIOpen / hipBLASLt); the scan is this module's."""
    L = xz.shape[-1]
    dt_rank = delta_proj_weight.shape[1]
    x, z = xz.chunk(2, dim=1)
    d_inner, width = conv1d_weight.shape[0], conv1d_weight.shape[-1]
    x = F.silu(F.conv1d(x, conv1d_weight.reshape(d_inner, 1, width), conv1d_bias, padding=width - 1, groups=d_inner)[..., :L])
    x_dbl = F.linear(x.transpose(1, 2).reshape(-1, d_inner), x_proj_weight)                    # (B L, dt_rank + 2 N)
    delta = (delta_proj_weight @ x_dbl[:, :dt_rank].t()).reshape(d_inner, -1, L).transpose(0, 1)
    if B is None:
        B = x_dbl[:, dt_rank:dt_rank + D_STATE]
        if B_proj_bias is not None:
            B = B + B_proj_bias.to(B.dtype)
        B = B.reshape(-1, L, D_STATE).transpose(1, 2)
    if C is None:
        C = x_dbl[:, -D_STATE:]
        if C_proj_bias is not None:
            C = C + C_proj_bias.to(C.dtype)
        C = C.reshape(-1, L, D_STATE).transpose(1, 2)
    return selective_scan_fn(x, delta, A, B, C, D, z=z, delta_bias=delta_bias, delta_softplus=delta_softplus)


def mamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, B=None, C=None,
                   D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True):
    """mamba_inner_fn_no_out_proj followed by out_proj: (B, 2 d_inner, L) -> (B, L, d_model)."""
    y = mamba_inner_fn_no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B, C, D, delta_bias,
                                   B_proj_bias, C_proj_bias, delta_softplus)
    return F.linear(y.transpose(1, 2), out_proj_weight, out_proj_bias)
