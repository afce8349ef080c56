"""The group tokenizer of the transformer and Mamba3D backbones (openpoints/models/backbone/transformer.py:210-243 and
openpoints/models/Mamba3D/Mamba3D.py:59-92, the same text twice): `from unipre3d_amd.tokenizer import Encoder` is the switch.  The
mini-PointNet that turns every group of n neighbours into one token runs in libunipre3d_tokenizer.so (include/unipre3d_tokenizer.h,
csrc/u3d_tokenizer.hip), forward and backward, in fp32:

  Encoder(encoder_channel)     the reference's module: same constructor, forward(point_groups) and state_dict keys
  tokenize(point_groups, params, *, training, eps, momentum, running=None, stat_reduce=None, need_dx=False)
                               the functional form, one autograd function with gradients to the twelve parameters and to the input

Three rewrites against the op-by-op form: BN1's batch statistics come from nine moments of the coordinates, the
cat is a per-group bias (the 512 x 512 product becomes 256 x 512 per point and 256 x 512 per group), and the backward is three phases
separated by BatchNorm's two global sums.  Kept from forward to backward at row size: f2 (256 floats a point) and y3 (512).

`stat_reduce` receives every phase's f64 block of partial sums (count first) on the device and returns the reduced block; Encoder
passes an all-reduce when its BN modules are SyncBatchNorm in an initialised world larger than one, which is what makes it correct under
the reference's convert_sync_batchnorm.  Deterministic, no host read, graph-capturable when no process group is involved.

Scope: fp32, 1 <= n <= 256, 1 <= C <= 1024, the reference's widths 128 / 256 / 512; in training mode at least two points in all.  On the
device there is no fallback; CPU tensors take the reference's op-by-op lines in torch."""
from __future__ import annotations

import ctypes
import os

import torch
from torch import nn

from . import _lib
from ._lib import byte_buffer, call, dense, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_tokenizer.so")
ABI_VERSION = 1
MAX_N, MAX_CHANNELS = 256, 1024                   # include/unipre3d_tokenizer.h
FOLD1_FLOATS, FOLD2_FLOATS = 1280, 2048
C1, C2, C3 = 128, 256, 512
PARAM_NAMES = ("W1", "b1", "g1", "be1", "W2", "b2", "W3", "b3", "g2", "be2", "W4", "b4")

_i, _f, _vp, _ll = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong
_x = [_vp, _ll, _ll, _ll, _ll, _i, _i, _i]        # x, its four strides, B, G, n
SIGNATURES = {   # include/unipre3d_tokenizer.h
    "u3d_tok_abi_version": (_i, []),
    "u3d_tok_wgrad_splits": (_i, [_ll]),
    "u3d_tok_scratch_bytes": (ctypes.c_size_t, [_ll, _i, _i, _i, _i]),
    "u3d_tok_moments": (_i, _x + [_vp, _vp, _vp]),
    "u3d_tok_fwd_a": (_i, _x + [_vp] * 8 + [_vp, _vp, _vp, _vp, _f, _f] + [_vp] * 8),
    "u3d_tok_fwd_b": (_i, [_vp, _ll, _i, _i] + [_vp] * 4 + [_vp, _vp, _vp, _vp, _f, _f] + [_vp] * 5),
    "u3d_tok_bwd_1": (_i, [_vp] * 5 + [_ll, _i, _i] + [_vp] * 6),
    "u3d_tok_bwd_2": (_i, _x + [_vp] * 12 + [_i] + [_vp] * 13),
    "u3d_tok_bwd_3": (_i, _x + [_vp] * 7 + [_i] + [_vp] * 8),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_tokenizer.so", SIGNATURES, ("u3d_tok_abi_version", ABI_VERSION))


def _xargs(x):
    B, G, n, _ = x.shape
    return [x, x.stride(0), x.stride(1), x.stride(2), x.stride(3), B, G, n]


def _scratch(lib, M, n, C, phase, training, dev):
    return byte_buffer(lib.u3d_tok_scratch_bytes(M, n, C, phase, int(training)), dev)


def _reduced(block, stat_reduce, keep_local):
    """The block after the caller's reduction (a copy goes in where the local sums are still needed)."""
    if stat_reduce is None:
        return block
    out = stat_reduce(block.clone() if keep_local else block)
    if not (torch.is_tensor(out) and out.dtype == torch.float64 and out.shape == block.shape and out.device == block.device):
        raise ValueError("stat_reduce must return an fp64 tensor of the shape and on the device of the one it was given")
    out = out.contiguous()
    return out.clone() if out.data_ptr() % 16 else out


class _Cfg:
    __slots__ = ("training", "eps", "momentum", "running", "stat_reduce", "need_dx")


class _Tokenize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, *params):
        lib = load()
        dev = x.device
        B, G, n, _ = x.shape
        M = B * G
        rows = M * n
        C = params[10].shape[0]
        W1, b1, g1, be1, W2, b2, W3, b3, g2, be2, W4, b4 = (
            dense(p, s) for p, s in zip(params, ((C1, 3), (C1,), (C1,), (C1,), (C2, C1), (C2,), (C3, C3), (C3,), (C3,), (C3,), (C, C3), (C,))))
        f32 = dict(dtype=torch.float32, device=dev)
        training = cfg.training
        reduce = cfg.stat_reduce if training else None
        rm1, rv1, nbt1, rm2, rv2, nbt2 = cfg.running if cfg.running is not None else (None,) * 6
        if not training:
            nbt1 = nbt2 = None                       # eval mode reads the running statistics and updates nothing
        mom = [-1.0 if m is None else float(m) for m in cfg.momentum]
        sums1 = sums2 = loc1 = loc2 = None
        if training:
            sums1 = torch.empty(10, dtype=torch.float64, device=dev)
            call(lib.u3d_tok_moments, *_xargs(x), sums1, _scratch(lib, M, n, 1, 0, 1, dev), dev=dev)
            loc1, sums1 = sums1, _reduced(sums1, reduce, True)
            sums2 = torch.empty(1 + 2 * C3, dtype=torch.float64, device=dev)
        fold1, fold2 = torch.empty(FOLD1_FLOATS, **f32), torch.empty(FOLD2_FLOATS, **f32)
        f2, y3 = torch.empty(rows, C2, **f32), torch.empty(rows, C3, **f32)
        g, arg2 = torch.empty(M, C2, **f32), torch.empty(M, C2, dtype=torch.int32, device=dev)
        call(lib.u3d_tok_fwd_a, *_xargs(x), W1, b1, g1, be1, W2, b2, W3, b3, sums1, rm1, rv1, nbt1, cfg.eps[0], mom[0], fold1,
             f2, g, arg2, y3, sums2, _scratch(lib, M, n, 1, 1, training, dev), dev=dev)
        if training:
            loc2, sums2 = sums2, _reduced(sums2, reduce, True)
        out, arg4 = torch.empty(B, G, C, **f32), torch.empty(M, C, dtype=torch.int32, device=dev)
        call(lib.u3d_tok_fwd_b, y3, M, n, C, g2, be2, W4, b4, sums2, rm2, rv2, nbt2, cfg.eps[1], mom[1], fold2, out, arg4,
             _scratch(lib, M, n, C, 2, 1, dev), dev=dev)
        ctx.save_for_backward(x, W1, g1, W2, W3, g2, W4, fold1, fold2, f2, y3, g, arg2, arg4)
        ctx.cfg, ctx.shapes = cfg, [p.shape for p in params]
        ctx.fwd_sums = (loc1, sums1, loc2, sums2)         # this process's and the reduced statistics blocks (None in eval mode)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, W1, g1, W2, W3, g2, W4, fold1, fold2, f2, y3, g, arg2, arg4 = ctx.saved_tensors
        cfg = ctx.cfg
        loc1, sums1, loc2, sums2 = ctx.fwd_sums
        lib = load()
        dev = x.device
        B, G, n, _ = x.shape
        M = B * G
        rows = M * n
        C = W4.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        training = int(cfg.training)
        reduce = cfg.stat_reduce if cfg.training else None
        dout = dout.to(torch.float32).reshape(M, C).contiguous()
        if dout.data_ptr() % 16:
            dout = dout.clone()
        dW4, db4, dh3m = torch.empty(C, C3, **f32), torch.empty(C, **f32), torch.empty(rows, C3, **f32)
        sums3 = torch.empty(1 + 2 * C3, dtype=torch.float64, device=dev)
        call(lib.u3d_tok_bwd_1, dout, y3, arg4, fold2, W4, M, n, C, dW4, db4, dh3m, sums3, _scratch(lib, M, n, C, 3, 1, dev), dev=dev)
        red3 = _reduced(sums3, reduce, True)
        dg2, dbe2, dW3, db3 = torch.empty(C3, **f32), torch.empty(C3, **f32), torch.empty(C3, C3, **f32), torch.empty(C3, **f32)
        dW2, db2 = torch.empty(C2, C1, **f32), torch.empty(C2, **f32)
        df2, dh1m = torch.empty(rows, C2, **f32), torch.empty(rows, C1, **f32)
        sums1b = torch.empty(1 + 2 * C1, dtype=torch.float64, device=dev)
        call(lib.u3d_tok_bwd_2, *_xargs(x), dh3m, y3, f2, g, arg2, fold1, fold2, g2, loc2, sums2, sums3, red3, training, W2, W3,
             dg2, dbe2, dW3, db3, dW2, db2, df2, dh1m, sums1b, _scratch(lib, M, n, 1, 4, 1, dev), dev=dev)
        del dh3m, df2
        red1 = _reduced(sums1b, reduce, True)
        dg1, dbe1, dW1, db1 = torch.empty(C1, **f32), torch.empty(C1, **f32), torch.empty(C1, 3, **f32), torch.empty(C1, **f32)
        dx = torch.empty(B, G, n, 3, **f32) if (ctx.needs_input_grad[0] or cfg.need_dx) else None
        call(lib.u3d_tok_bwd_3, *_xargs(x), dh1m, fold1, g1, loc1, sums1, sums1b, red1, training, W1, dg1, dbe1, dW1, db1, dx,
             _scratch(lib, M, n, 1, 5, 1, dev), dev=dev)
        grads = (dW1, db1, dg1, dbe1, dW2, db2, dW3, db3, dg2, dbe2, dW4, db4)
        return (dx if ctx.needs_input_grad[0] else None, None) + tuple(t.view(s) for t, s in zip(grads, ctx.shapes))


def _pair(v, name):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name}: expected one value or one per BatchNorm, got {len(v)}")
        return tuple(v)
    return (v, v)


def tokenize(point_groups, params, *, training, eps=1e-5, momentum=0.1, running=None, stat_reduce=None, need_dx=False):
    """point_groups (B, G, n, 3) fp32 with any strides (read in place) -> (B, G, C).

    params    the twelve tensors W1 b1 g1 be1 W2 b2 W3 b3 g2 be2 W4 b4 in the modules' shapes (Conv1d weights (out, in, 1) or (out, in)).
    training  True: batch statistics; `running` = (running_mean1, running_var1, num_batches_tracked1, running_mean2, running_var2,
              num_batches_tracked2) is then updated in place as BatchNorm1d does (unbiased variance; momentum None = cumulative
              average), any entry or the whole may be None.  False: the running statistics are folded and no statistics pass runs.
    eps, momentum   one value, or one per BatchNorm.
    stat_reduce     None, or a callable that takes each phase's f64 block of partial sums (count first) and returns the reduced block.
    need_dx   compute the input gradient in the backward even where autograd does not ask for it."""
    params = tuple(params)
    if len(params) != 12:
        raise ValueError(f"params: expected the twelve tensors {' '.join(PARAM_NAMES)}, got {len(params)}")
    if point_groups.dim() != 4 or point_groups.shape[3] != 3:
        raise ValueError(f"point_groups: expected (B, G, n, 3), got {tuple(point_groups.shape)}")
    for name, t in (("point_groups", point_groups),) + tuple(zip(PARAM_NAMES, params)):
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: dtype {t.dtype} is not implemented (fp32 only)")
    B, G, n, _ = point_groups.shape
    if B < 1 or G < 1 or n < 1:
        raise ValueError(f"point_groups: an empty tensor {tuple(point_groups.shape)} is not supported")
    if n > MAX_N:
        raise ValueError(f"point_groups: n={n} is not implemented (at most {MAX_N})")
    if B * G * n >= 2 ** 31:
        raise ValueError(f"point_groups: {B * G * n} points are not implemented (fewer than 2^31)")
    C = params[10].shape[0]
    want = ((C1, 3), (C1,), (C1,), (C1,), (C2, C1), (C2,), (C3, C3), (C3,), (C3,), (C3,), (C, C3), (C,))
    for name, t, s in zip(PARAM_NAMES, params, want):
        if t.numel() != torch.Size(s).numel() or t.shape[0] != s[0]:
            raise ValueError(f"{name}: expected {s} (the reference's widths are fixed), got {tuple(t.shape)}")
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"C={C} is not implemented (1 to {MAX_CHANNELS})")
    training = bool(training)
    if training and B * G * n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(point_groups.shape)}")
    cfg = _Cfg()
    cfg.training, cfg.stat_reduce, cfg.need_dx = training, stat_reduce, bool(need_dx)
    cfg.eps = tuple(float(e) for e in _pair(eps, "eps"))
    cfg.momentum = _pair(momentum, "momentum")
    if any(not 0.0 <= e < float("inf") for e in cfg.eps):
        raise ValueError(f"eps={eps}: must be a non-negative finite number")
    if any(m is not None and not 0.0 <= float(m) <= 1.0 for m in cfg.momentum):
        raise ValueError(f"momentum={momentum}: must be None or lie in [0, 1]")
    if running is not None:
        running = tuple(running)
        if len(running) != 6:
            raise ValueError("running: expected (running_mean1, running_var1, num_batches_tracked1, running_mean2, running_var2, "
                             "num_batches_tracked2)")
        for i, (t, size) in enumerate(zip(running, (C1, C1, 1, C3, C3, 1))):
            if t is None:
                continue
            dt = torch.int64 if i % 3 == 2 else torch.float32
            if t.dtype != dt or t.numel() != size or not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError(f"running[{i}]: expected a contiguous, 16-byte aligned {dt} tensor of {size} values")
    if not training and (running is None or any(running[i] is None for i in (0, 1, 3, 4))):
        raise ValueError("eval mode needs the running means and variances of both BatchNorms")
    cfg.running = running
    on_device("tokenizer", point_groups, *params, *(running or ()))
    load()
    return _Tokenize.apply(point_groups, cfg, *params)


def _all_reduce(block):
    torch.distributed.all_reduce(block)
    return block


class Encoder(nn.Module):
    """The reference's Encoder with its constructor, module layout (first_conv / second_conv: 0 Conv1d, 1 BatchNorm1d, 2 ReLU, 3 Conv1d)
    and state_dict keys, so checkpoints, `apply(_init_weights)` and SyncBatchNorm.convert_sync_batchnorm work unchanged.
    forward(point_groups): (B, G, n, 3) with any strides -> (B, G, encoder_channel)."""

    def __init__(self, encoder_channel):
        super().__init__()
        self.encoder_channel = encoder_channel
        self.first_conv = nn.Sequential(nn.Conv1d(3, C1, 1), nn.BatchNorm1d(C1), nn.ReLU(inplace=True), nn.Conv1d(C1, C2, 1))
        self.second_conv = nn.Sequential(nn.Conv1d(C3, C3, 1), nn.BatchNorm1d(C3), nn.ReLU(inplace=True),
                                         nn.Conv1d(C3, self.encoder_channel, 1))

    def _reference_lines(self, point_groups):
        bs, g, n, _ = point_groups.shape
        point_groups = point_groups.reshape(bs * g, n, 3)
        feature = self.first_conv(point_groups.transpose(2, 1))
        feature_global = torch.max(feature, dim=2, keepdim=True)[0]
        feature = torch.cat([feature_global.expand(-1, -1, n), feature], dim=1)
        feature = self.second_conv(feature)
        feature_global = torch.max(feature, dim=2, keepdim=False)[0]
        return feature_global.reshape(bs, g, self.encoder_channel)

    def forward(self, point_groups):
        if not point_groups.is_cuda:
            return self._reference_lines(point_groups)
        c1, bn1, c2 = self.first_conv[0], self.first_conv[1], self.first_conv[3]
        c3, bn2, c4 = self.second_conv[0], self.second_conv[1], self.second_conv[3]
        training = self.training or bn1.running_mean is None or bn2.running_mean is None
        reduce = None
        if training and isinstance(bn1, nn.SyncBatchNorm) and isinstance(bn2, nn.SyncBatchNorm) and \
                torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            reduce = _all_reduce
        track = self.training
        running = (bn1.running_mean, bn1.running_var, bn1.num_batches_tracked, bn2.running_mean, bn2.running_var,
                   bn2.num_batches_tracked)
        if training and not track:
            running = None
        return tokenize(point_groups, (c1.weight, c1.bias, bn1.weight, bn1.bias, c2.weight, c2.bias, c3.weight, c3.bias, bn2.weight,
                                       bn2.bias, c4.weight, c4.bias), training=training, eps=(bn1.eps, bn2.eps),
                        momentum=(bn1.momentum, bn2.momentum), running=running, stat_reduce=reduce)
