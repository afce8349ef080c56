"""BatchNorm1d over channels-first (B, C, L) tensors fused with its activation, the residual add and the max over L behind it: the most
numerous layer of the two object-level backbones PointMLP and PCM (openpoints/models/backbone/pointmlp.py:198-353,
openpoints/models/PCM/PointMLP_layers.py:112-225: every ConvBNReLU1D is Conv1d(k=1), BatchNorm1d, act; every ConvBNReLURes1D ends in
act(bn(.) + x); every PreExtraction ends in adaptive_max_pool1d(x, 1) over the K neighbours).  It runs in libunipre3d_batchnorm_cf.so
(include/unipre3d_batchnorm_cf.h, csrc/u3d_batchnorm_cf.hip), forward and backward, in fp32; the Conv1d products stay torch's.

  batch_norm_act_cf(x, weight, bias, running_mean, running_var, num_batches_tracked=None, *, training, momentum, eps, act="none",
                    residual=None, pool=None, pool_groups=1, stat_reduce=None)
                                                       one autograd function, gradients to x, weight, bias and residual
  BatchNormActCF(num_features, ..., act="none")        an nn.BatchNorm1d subclass (same state_dict keys),
                                                       forward(x, residual=None, pool=None, pool_groups=1); 2-D inputs go to batchnorm.py
  ConvBNReLU1D, ConvBNReLURes1D, PreExtraction, PosExtraction   the reference's four classes: same constructors, child names and keys
  fuse_pointmlp_blocks(model)                          opt-in: replaces modules of those four class names in place
  plan(C, L, aligned=True)                             the kernels' dispatch class of a shape; parts(B, C, L) the partial rows

y = act((x - mean) (invstd gamma) + beta [+ residual]) as in batchnorm.py; the count per channel is B L.  The statistics pass writes f64
partial sums per batch chunk; their fixed-order sum, mean / invstd, the running statistics and the SyncBatchNorm block are
libunipre3d_batchnorm.so's u3d_bn_sum / u3d_bn_finalize, unchanged, and `stat_reduce` follows batchnorm.py's contract.

pool="max": the result is max over L, (B, C), or with pool_groups = S > 1 (B % S == 0) the contiguous (B / S, C, S) tensor whose
[i, c, j] is row i S + j -- what PreExtraction returns.  No (B, C, L) tensor is written forward; kept for the backward are x, mean and
invstd, the pooled tensor and the int32 argmax (the lowest l on a tie), and neither y nor the residual.  The backward writes every element
of dx (and dresidual) once, without a memset and without a dy-sized tensor.  Non-finite inputs are outside the pooled form's contract.
Without pool it keeps what batchnorm.py keeps: x, mean, invstd and, for ReLU only, y.

Scope: fp32, contiguous x (B, C, L), 1 <= C <= 1024; a residual with "none" and "relu" only.  A non-contiguous residual is copied.  On the
device there is no fallback; CPU tensors take torch's own lines."""
from __future__ import annotations

import collections
import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, batchnorm
from ._lib import call, on_device
from .batchnorm import ACTS, _check_act, _reduced

ABI_VERSION = 1
MAX_CHANNELS = 1024                                # include/unipre3d_batchnorm_cf.h

_i, _f, _vp, _ll = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong
_ip = ctypes.POINTER(ctypes.c_int)
SIGNATURES = {   # include/unipre3d_batchnorm_cf.h
    "u3d_bncf_abi_version": (_i, []),
    "u3d_bncf_plan": (_i, [_i, _i, _i, _ip, _ip, _ip, _ip]),
    "u3d_bncf_parts": (_ll, [_ll, _i, _i]),
    "u3d_bncf_stats": (_i, [_vp, _ll, _i, _i, _vp, _vp, _vp]),
    "u3d_bncf_apply": (_i, [_vp, _vp, _ll, _i, _i, _i, _i, _f] + [_vp] * 7 + [_ll, _vp]),
    "u3d_bncf_bwd_reduce": (_i, [_vp] * 4 + [_ll, _i, _i, _i, _i, _f] + [_vp] * 4 + [_ll, _vp, _vp]),
    "u3d_bncf_bwd_apply": (_i, [_vp] * 4 + [_ll, _i, _i, _i, _i, _f] + [_vp] * 5 + [_ll, _vp, _vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)

Plan = collections.namedtuple("Plan", "lanes_per_row channel_tile batch_chunk vec sweeps")


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_batchnorm_cf.so", SIGNATURES, ("u3d_bncf_abi_version", ABI_VERSION))


def plan(C: int, L: int, aligned: bool = True) -> Plan:
    """The dispatch class of a (., C, L) call (u3d_bncf_plan): `lanes_per_row` lanes own one (b, c) row at a time, `vec` floats each
    (4 where L % 4 == 0 and every (B, C, L) tensor of the call is 16-byte aligned, which `aligned` stands for), in `sweeps` sweeps; a
    workgroup takes `channel_tile` channels x `batch_chunk` batch entries."""
    out = [ctypes.c_int() for _ in range(4)]
    if load().u3d_bncf_plan(C, L, int(bool(aligned)), *[ctypes.byref(o) for o in out]) != 0:
        raise NotImplementedError(f"C={C}, L={L} is not implemented (1 <= C <= {MAX_CHANNELS}, L >= 1)")
    g, ct, bc, v = (o.value for o in out)
    return Plan(g, ct, bc, v, -(-(-(-L // v)) // g))


def parts(B: int, C: int, L: int) -> int:
    """Rows of the f64 partials of a (B, C, L) call (u3d_bncf_parts) = ceil(B / batch_chunk)."""
    n = load().u3d_bncf_parts(B, C, L)
    if n < 1:
        raise NotImplementedError(f"B={B}, C={C}, L={L} is not implemented")
    return n


class _Cfg:
    __slots__ = ("training", "eps", "momentum", "act", "stat_reduce", "running", "pool", "groups")


class _BatchNormActCF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, cfg):
        lib, bn = load(), batchnorm.load()
        dev = x.device
        B, C, L = x.shape
        act, S = ACTS[cfg.act], cfg.groups
        rm, rv, nbt = cfg.running
        gamma = None if weight is None else weight.detach().contiguous()
        beta = None if bias is None else bias.detach().contiguous()
        res = None if residual is None else residual.detach().contiguous()
        if cfg.training:
            n = parts(B, C, L)
            partials = torch.empty(n, 2 * C, dtype=torch.float64, device=dev)
            block = torch.empty(1 + 2 * C, dtype=torch.float64, device=dev)
            mi = torch.empty(2 * C, dtype=torch.float32, device=dev)
            mom = -1.0 if cfg.momentum is None else float(cfg.momentum)
            call(lib.u3d_bncf_stats, x, B, C, L, nbt, partials, dev=dev)
            if cfg.stat_reduce is None:
                call(bn.u3d_bn_finalize, partials, n, float(B * L), block, C, cfg.eps, mom, rm, rv, nbt, mi, dev=dev)
            else:
                call(bn.u3d_bn_sum, partials, n, C, float(B * L), block, None, None, dev=dev)
                block = _reduced(block, cfg.stat_reduce)
                call(bn.u3d_bn_finalize, None, 0, 0.0, block, C, cfg.eps, mom, rm, rv, nbt, mi, dev=dev)
            mean, second = mi[:C], mi[C:]
        else:
            mean, second = rm, rv
        ev = int(not cfg.training)
        if cfg.pool:
            shape = (B, C) if S == 1 else (B // S, C, S)
            pooled = torch.empty(shape, dtype=torch.float32, device=dev)
            arg = torch.empty(shape, dtype=torch.int32, device=dev)
            call(lib.u3d_bncf_apply, x, res, B, C, L, act, ev, cfg.eps, mean, second, gamma, beta, None, pooled, arg, S, dev=dev)
            ctx.save_for_backward(x, mean, second, gamma, beta, pooled if cfg.act == "relu" else None, arg)
            ctx.mark_non_differentiable(arg)
            ctx.cfg = cfg
            return pooled, arg
        y = torch.empty_like(x)
        call(lib.u3d_bncf_apply, x, res, B, C, L, act, ev, cfg.eps, mean, second, gamma, beta, y, None, None, 1, dev=dev)
        ctx.save_for_backward(x, mean, second, gamma, beta, y if cfg.act == "relu" else None, None)
        ctx.cfg = cfg
        return y, None

    @staticmethod
    def backward(ctx, dy, _darg=None):
        x, mean, second, gamma, beta, y, arg = ctx.saved_tensors
        cfg = ctx.cfg
        lib, bn = load(), batchnorm.load()
        dev = x.device
        B, C, L = x.shape
        act, ev, S = ACTS[cfg.act], int(not cfg.training), cfg.groups
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        dy = dy.to(torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        dgamma = torch.empty(C, **f32) if need_w else None
        dbeta = torch.empty(C, **f32) if need_b else None
        block = None
        if cfg.training or need_w or need_b:
            n = parts(B, C, L)
            partials = torch.empty(n, 2 * C, dtype=torch.float64, device=dev)
            block = torch.empty(1 + 2 * C, dtype=torch.float64, device=dev)
            call(lib.u3d_bncf_bwd_reduce, dy, x, y, arg, B, C, L, act, ev, cfg.eps, mean, second, gamma, beta, S, partials, dev=dev)
            call(bn.u3d_bn_sum, partials, n, C, float(B * L), block, dbeta, dgamma, dev=dev)
            block = _reduced(block, cfg.stat_reduce) if cfg.training else None
        dx = torch.empty_like(x) if need_x else None
        dres = None
        if need_r:
            dres = dy if (cfg.act == "none" and not cfg.pool) else torch.empty_like(x)
        if dx is not None or (dres is not None and dres is not dy):
            call(lib.u3d_bncf_bwd_apply, dy, x, y, arg, B, C, L, act, ev, cfg.eps, mean, second, gamma, beta, block, S, dx,
                 None if dres is dy else dres, dev=dev)
        return dx, dgamma, dbeta, dres, None


def _torch_lines(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, residual, pool, groups):
    """torch's own lines (CPU tensors): batchnorm.py's, then the reference's adaptive_max_pool1d and its reshape."""
    out = batchnorm._torch_lines(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, residual)
    arg = None
    if pool:
        B, C, _ = x.shape
        out, arg = F.adaptive_max_pool1d(out, 1, return_indices=True)
        out, arg = out.view(B, -1), arg.view(B, -1).int()
        if groups > 1:
            out, arg = (t.reshape(B // groups, groups, C).permute(0, 2, 1) for t in (out, arg))
    return out, arg


def batch_norm_act_cf(x, weight, bias, running_mean, running_var, num_batches_tracked=None, *, training, momentum, eps, act="none",
                      residual=None, pool=None, pool_groups=1, stat_reduce=None, return_arg=False):
    """x (B, C, L) fp32 contiguous -> act(batch_norm(x) [+ residual]) (B, C, L), or with pool="max" its max over L: (B, C), or
    (B / pool_groups, C, pool_groups) contiguous with row b at [b // pool_groups, :, b % pool_groups].

    weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, stat_reduce: as batchnorm.batch_norm_act.
    residual          (B, C, L), added before the activation; with "none" and "relu" only.  A non-contiguous residual is copied.
    return_arg        with pool="max": -> (pooled, arg), arg the int32 index of each maximum (the lowest l on a tie), in pooled's layout."""
    _check_act(act)
    if residual is not None and act == "gelu":
        raise NotImplementedError("act='gelu' with a residual is not implemented (no reference layer has it)")
    if pool not in (None, "max"):
        raise NotImplementedError(f"pool={pool!r} is not implemented (None or 'max')")
    if x.dim() != 3:
        raise ValueError(f"x: expected (B, C, L), got {tuple(x.shape)}")
    B, C, L = x.shape
    pool_groups = int(pool_groups)
    if pool_groups < 1 or (pool is None and pool_groups != 1):
        raise ValueError(f"pool_groups={pool_groups}: must be at least 1, and 1 without pool")
    if pool and B % pool_groups:
        raise ValueError(f"pool_groups={pool_groups} does not divide B={B}")
    named = (("x", x, (B, C, L)), ("weight", weight, (C,)), ("bias", bias, (C,)), ("running_mean", running_mean, (C,)),
             ("running_var", running_var, (C,)), ("residual", residual, (B, C, L)))
    for name, t, shape in named:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise NotImplementedError(f"{name}: dtype {t.dtype} is not implemented (fp32 only)")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected {shape}, got {tuple(t.shape)}")
    if C > MAX_CHANNELS:
        raise NotImplementedError(f"C={C} is not implemented (1 to {MAX_CHANNELS})")
    if C < 1:
        raise ValueError(f"x: expected at least one channel, got {tuple(x.shape)}")
    for name, t in (("x", x), ("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor, got strides {t.stride()}")
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
        raise ValueError("num_batches_tracked: expected one int64 value")
    training = bool(training)
    if not training and (running_mean is None or running_var is None):
        raise ValueError("eval mode needs running_mean and running_var")
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var: expected both or neither")
    if training and momentum is None and running_mean is not None and num_batches_tracked is None:
        raise ValueError("momentum=None (cumulative average) needs num_batches_tracked")
    if momentum is not None and not 0.0 <= float(momentum) <= 1.0:
        raise ValueError(f"momentum={momentum}: must be None or lie in [0, 1]")
    if not 0.0 <= float(eps) < float("inf"):
        raise ValueError(f"eps={eps}: must be a non-negative finite number")
    if B == 0 or L == 0:
        if not pool:
            return x.new_empty(B, C, L)
        if L == 0 and B > 0:
            raise ValueError(f"pool='max' over an empty dimension, got input size {x.size()}")
        shape = (0, C) if pool_groups == 1 else (0, C, pool_groups)
        return (x.new_empty(shape), x.new_empty(shape, dtype=torch.int32)) if return_arg else x.new_empty(shape)
    if training and B * L < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
    if not x.is_cuda:
        out = _torch_lines(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, residual, pool,
                           pool_groups)
        return out if pool and return_arg else out[0]
    on_device("batchnorm_cf", x, weight, bias, running_mean, running_var, num_batches_tracked, residual)
    load()
    cfg = _Cfg()
    cfg.training, cfg.eps, cfg.momentum, cfg.act = training, float(eps), momentum, act
    cfg.stat_reduce = stat_reduce if training else None
    cfg.running = (running_mean, running_var, num_batches_tracked if training and running_mean is not None else None)
    cfg.pool, cfg.groups = bool(pool), pool_groups
    out = _BatchNormActCF.apply(x, weight, bias, residual, cfg)
    return out if pool and return_arg else out[0]


class BatchNormActCF(batchnorm.BatchNormAct):
    """nn.BatchNorm1d over (B, C, L) with the activation, the residual add before it and, with pool="max", the max over L behind it in
    the same kernels.  Same constructor plus `act`, same parameters, buffers and state_dict keys.  A 2-D input is
    batchnorm.BatchNormAct's."""

    def forward(self, x, residual=None, pool=None, pool_groups=1):
        if x.dim() == 2:
            if pool is not None:
                raise ValueError("pool needs a (B, C, L) input")
            return super().forward(x, residual)
        training = self.training or self.running_mean is None
        reduce = None
        if training and self.sync and x.is_cuda and torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size(self.process_group) > 1:
            reduce = self._all_reduce
        track = self.training and self.track_running_stats
        return batch_norm_act_cf(x, self.weight, self.bias, self.running_mean if (track or not training) else None,
                                 self.running_var if (track or not training) else None, self.num_batches_tracked if track else None,
                                 training=training, momentum=self.momentum, eps=self.eps, act=self.act, residual=residual, pool=pool,
                                 pool_groups=pool_groups, stat_reduce=reduce)


def _act_name(activation, residual):
    """The reference's get_activation(): "gelu" is nn.GELU(), every name it does not know is ReLU; the names it maps to an activation
    without a kernel raise, and so does gelu in a residual block."""
    name = activation.lower()
    if name in ("rrelu", "selu", "silu", "hardswish", "leakyrelu"):
        raise NotImplementedError(f"activation={activation!r} is not implemented (relu and the erf gelu only)")
    if name == "gelu" and residual:
        raise NotImplementedError("activation='gelu' in a residual block is not implemented (gelu takes no residual)")
    return "gelu" if name == "gelu" else "relu"


def _conv_bn(cin, cout, kernel_size, groups, bias, act):
    """(Conv1d, BatchNormActCF, Identity): the reference's (Conv1d, BatchNorm1d, act) with the activation inside the norm."""
    return [nn.Conv1d(cin, cout, kernel_size, groups=groups, bias=bias), BatchNormActCF(cout, act=act), nn.Identity()]


class ConvBNReLU1D(nn.Module):
    """pointmlp.py:198-216 / PointMLP_layers.py:112-123: net = (Conv1d, BatchNorm1d, act); keys net.0.*, net.1.*."""

    def __init__(self, in_channels, out_channels, kernel_size=1, bias=True, activation="relu"):
        super().__init__()
        self.act = nn.Identity()
        self.net = nn.Sequential(*_conv_bn(in_channels, out_channels, kernel_size, 1, bias, _act_name(activation, False)))

    def forward(self, x, pool=None, pool_groups=1):
        return self.net[1](self.net[0](x), None, pool, pool_groups)


class ConvBNReLURes1D(nn.Module):
    """pointmlp.py:219-273 / PointMLP_layers.py:126-154: act(net2(net1(x)) + x); the last norm, the add and the activation are one
    call.  groups == 1: net2 = (Conv1d, BatchNorm1d); groups > 1: net2 = (Conv1d, BatchNorm1d, act, Conv1d, BatchNorm1d)."""

    def __init__(self, channel, kernel_size=1, groups=1, res_expansion=1.0, bias=True, activation="relu"):
        super().__init__()
        act = _act_name(activation, True)
        mid = int(channel * res_expansion)
        self.act = nn.Identity()
        self.net1 = nn.Sequential(*_conv_bn(channel, mid, kernel_size, groups, bias, act))
        if groups > 1:
            self.net2 = nn.Sequential(*_conv_bn(mid, channel, kernel_size, groups, bias, act),
                                      *_conv_bn(channel, channel, kernel_size, 1, bias, act)[:2])
        else:
            self.net2 = nn.Sequential(*_conv_bn(mid, channel, kernel_size, 1, bias, act)[:2])

    def forward(self, x, pool=None, pool_groups=1):
        if not x.is_contiguous():
            x = x.contiguous()
        h = self.net1[1](self.net1[0](x))
        if len(self.net2) == 5:
            h = self.net2[1](self.net2[0](h))
        return self.net2[-1](self.net2[-2](h), x, pool, pool_groups)


class PreExtraction(nn.Module):
    """pointmlp.py:276-320 / PointMLP_layers.py:157-188: (b, n, s, d) -> (b, d', n).  The max over the s neighbours is part of the last
    block's final call (of `transfer`'s with blocks == 0), which writes (b, d', n) contiguous: the reference's shape and values, other
    strides.  For the permute view that local_group(channels_first=True) returns the reshape in front is a view."""

    def __init__(self, channels, out_channels, blocks=1, groups=1, res_expansion=1, bias=True, activation="relu", use_xyz=True,
                 knn_grouper=True):
        super().__init__()
        if knn_grouper:
            in_channels = 3 + 2 * channels if use_xyz else 2 * channels
        else:
            in_channels = 3 + channels if use_xyz else channels
        self.transfer = ConvBNReLU1D(in_channels, out_channels, bias=bias, activation=activation)
        self.operation = nn.Sequential(*[ConvBNReLURes1D(out_channels, groups=groups, res_expansion=res_expansion, bias=bias,
                                                         activation=activation) for _ in range(blocks)])

    def forward(self, x):
        b, n, s, d = x.size()
        x = x.permute(0, 1, 3, 2).reshape(-1, d, s)
        if len(self.operation) == 0:
            return self.transfer(x, "max", n)
        x = self.transfer(x)
        for block in self.operation[:-1]:
            x = block(x)
        return self.operation[-1](x, "max", n)


class PosExtraction(nn.Module):
    """pointmlp.py:323-353 / PointMLP_layers.py:210-226: (b, d, g) -> (b, d, g) through `blocks` residual blocks."""

    def __init__(self, channels, blocks=1, groups=1, res_expansion=1, bias=True, activation="relu"):
        super().__init__()
        self.operation = nn.Sequential(*[ConvBNReLURes1D(channels, groups=groups, res_expansion=res_expansion, bias=bias,
                                                         activation=activation) for _ in range(blocks)])

    def forward(self, x):
        return self.operation(x)


def _act_of_block(block):
    act = block.act
    if type(act) is nn.ReLU:
        return "relu"
    if type(act) is nn.GELU and act.approximate == "none":
        return "gelu"
    raise NotImplementedError(f"fuse_pointmlp_blocks: activation {type(act).__name__} is not implemented (relu and the erf gelu only)")


def _fused_seq(seq, act):
    """The reference's Sequential with its own Conv1d objects, every norm as a BatchNormActCF over the same Parameters and buffers and
    nn.Identity in the activation slots."""
    out = []
    for child in seq:
        if isinstance(child, (nn.BatchNorm1d, nn.SyncBatchNorm)):
            child = child if isinstance(child, BatchNormActCF) else BatchNormActCF.from_norm(child, act)
        elif not isinstance(child, nn.Conv1d):
            child = nn.Identity()
        out.append(child)
    return nn.Sequential(*out)


def _rebuild(old):
    """A module of this file for a module of one of the four class names, sharing its convolutions, Parameters and buffers."""
    kind = type(old).__name__
    cls = {c.__name__: c for c in (ConvBNReLU1D, ConvBNReLURes1D, PreExtraction, PosExtraction)}[kind]
    new = cls.__new__(cls)
    nn.Module.__init__(new)
    if kind == "ConvBNReLU1D":
        new.act, new.net = nn.Identity(), _fused_seq(old.net, _act_of_block(old))
    elif kind == "ConvBNReLURes1D":
        act = _act_of_block(old)
        if act == "gelu":
            raise NotImplementedError("fuse_pointmlp_blocks: gelu in a residual block is not implemented (gelu takes no residual)")
        new.act, new.net1, new.net2 = nn.Identity(), _fused_seq(old.net1, act), _fused_seq(old.net2, act)
    else:
        if kind == "PreExtraction":
            new.transfer = _rebuild(old.transfer)
        new.operation = nn.Sequential(*[_rebuild(b) for b in old.operation])
    new.train(old.training)
    return new


FUSED_NAMES = ("ConvBNReLU1D", "ConvBNReLURes1D", "PreExtraction", "PosExtraction")


def fuse_pointmlp_blocks(model):
    """Replaces, in place, every module whose class name is ConvBNReLU1D, ConvBNReLURes1D, PreExtraction or PosExtraction (and that is
    not already one of this file's classes) by this file's class of that name, sharing every Conv1d, Parameter and buffer.  Call it
    after convert_sync_batchnorm.  Returns the number of modules replaced (an outer module counts once, with what it contains)."""
    mine = (ConvBNReLU1D, ConvBNReLURes1D, PreExtraction, PosExtraction)
    count = 0

    def walk(parent):
        nonlocal count
        for name, child in list(parent._modules.items()):
            if child is None:
                continue
            if type(child).__name__ in FUSED_NAMES and not isinstance(child, mine):
                parent._modules[name] = _rebuild(child)
                count += 1
            else:
                walk(child)

    walk(model)
    return count
