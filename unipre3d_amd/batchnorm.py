"""BatchNorm1d over (N, C) point rows fused with its activation and the residual add: the second kind of layer of the scene-level
backbones (pointcept/models/sparse_unet/spconv_unet_v1m1_base.py:87-104, 149-164, 205-260: BatchNorm1d(eps=1e-3, momentum=0.01) + ReLU
after every sparse convolution and `bn2 + proj(residual) + relu` at the end of every BasicBlock; point_transformer_v3m1_base.py:461-470,
501-514, 578-588: the same pair with GELU).  It runs in libunipre3d_batchnorm.so (include/unipre3d_batchnorm.h, csrc/u3d_batchnorm.hip),
forward and backward, in fp32:

  batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked=None, *, training, momentum, eps, act="none",
                 residual=None, stat_reduce=None)      one autograd function, gradients to x, weight, bias and residual
  BatchNormAct(num_features, ..., act="none")          an nn.BatchNorm1d subclass (same state_dict keys), forward(x, residual=None)
  BasicBlock(in_channels, embed_channels, ...)         the reference's block over unipre3d_amd.sparseconv: `block = BasicBlock`
  fuse_norm_act(model)                                 opt-in: replaces (BatchNorm1d | SyncBatchNorm, ReLU | GELU) pairs in place
  row_chunk(C)                                         rows one workgroup takes (the kernels' dispatch edge)

y = act((x - mean) (invstd gamma) + beta [+ residual]).  Training: a statistics pass (f64 sums per row chunk, added in a fixed order),
a finalize that also moves running_mean / running_var (unbiased variance; momentum None = cumulative average) and
num_batches_tracked on the device, and one apply pass.  Eval: the apply pass alone.  Backward: one reduce pass and one apply pass.
Kept for the backward: x, mean and invstd (2C floats) and, for ReLU only, y (its mask stands in for the residual).

`stat_reduce` receives the f64 block `count | sum [C] | sum [C]` of the forward and of the backward on the device and returns the
reduced block; BatchNormAct passes an all-reduce when it was made from an nn.SyncBatchNorm in an initialised world larger than one.
dgamma and dbeta stay this process's sums, as SyncBatchNorm leaves them to the gradient all-reduce.  Deterministic bit for bit, no host
read, graph-capturable when no process group is involved.

Scope: fp32, x (N, C) with contiguous rows, 1 <= C <= 1024; a residual with "none" and "relu" only.  On the device there is no
fallback; CPU tensors take torch's own lines."""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_batchnorm.so")
ABI_VERSION = 1
MAX_CHANNELS = 1024                                # include/unipre3d_batchnorm.h
ACTS = {"none": 0, "relu": 1, "gelu": 2}
CHUNK_FLOATS, MIN_ROWS = 4096, 32                  # csrc/u3d_batchnorm.hip

_i, _f, _d, _vp, _ll = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_longlong
SIGNATURES = {   # include/unipre3d_batchnorm.h
    "u3d_bn_abi_version": (_i, []),
    "u3d_bn_row_chunk": (_i, [_i]),
    "u3d_bn_stats": (_i, [_vp, _ll, _i, _vp, _vp, _vp]),
    "u3d_bn_sum": (_i, [_vp, _ll, _i, _d, _vp, _vp, _vp, _vp]),
    "u3d_bn_finalize": (_i, [_vp, _ll, _d, _vp, _i, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "u3d_bn_apply": (_i, [_vp, _vp, _ll, _i, _i, _i, _f] + [_vp] * 6),
    "u3d_bn_bwd_reduce": (_i, [_vp, _vp, _vp, _ll, _i, _i, _i, _f] + [_vp] * 6),
    "u3d_bn_bwd_apply": (_i, [_vp, _vp, _vp, _ll, _i, _i, _i, _f] + [_vp] * 8),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_batchnorm.so", SIGNATURES, ("u3d_bn_abi_version", ABI_VERSION))


def row_chunk(C: int) -> int:
    """Rows of a (N, C) tensor one workgroup takes (u3d_bn_row_chunk): N rows make ceil(N / row_chunk(C)) partial sums."""
    if not 1 <= C <= MAX_CHANNELS:
        raise NotImplementedError(f"C={C} is not implemented (1 to {MAX_CHANNELS})")
    return max(CHUNK_FLOATS // C, MIN_ROWS)


def _reduced(block, stat_reduce):
    if stat_reduce is None:
        return block
    out = stat_reduce(block.clone())
    if not (torch.is_tensor(out) and out.dtype == torch.float64 and out.shape == block.shape and out.device == block.device):
        raise ValueError("stat_reduce must return an fp64 tensor of the shape and on the device of the one it was given")
    return out.contiguous()


class _Cfg:
    __slots__ = ("training", "eps", "momentum", "act", "stat_reduce", "running")


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, cfg):
        lib = load()
        dev = x.device
        N, C = x.shape
        act = ACTS[cfg.act]
        rm, rv, nbt = cfg.running
        gamma = None if weight is None else weight.detach().contiguous()
        beta = None if bias is None else bias.detach().contiguous()
        res = None if residual is None else residual.detach()
        y = torch.empty_like(x)
        if cfg.training:
            parts = -(-N // row_chunk(C))
            partials = torch.empty(parts, 2 * C, dtype=torch.float64, device=dev)
            block = torch.empty(1 + 2 * C, dtype=torch.float64, device=dev)
            mi = torch.empty(2 * C, dtype=torch.float32, device=dev)
            mom = -1.0 if cfg.momentum is None else float(cfg.momentum)
            call(lib.u3d_bn_stats, x, N, C, nbt, partials, dev=dev)
            if cfg.stat_reduce is None:
                call(lib.u3d_bn_finalize, partials, parts, float(N), block, C, cfg.eps, mom, rm, rv, nbt, mi, dev=dev)
            else:
                call(lib.u3d_bn_sum, partials, parts, C, float(N), block, None, None, dev=dev)
                block = _reduced(block, cfg.stat_reduce)
                call(lib.u3d_bn_finalize, None, 0, 0.0, block, C, cfg.eps, mom, rm, rv, nbt, mi, dev=dev)
            mean, second = mi[:C], mi[C:]
        else:
            mean, second = rm, rv
        call(lib.u3d_bn_apply, x, res, N, C, act, int(not cfg.training), cfg.eps, mean, second, gamma, beta, y, dev=dev)
        ctx.save_for_backward(x, mean, second, gamma, beta, y if cfg.act == "relu" else None)
        ctx.cfg = cfg
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, second, gamma, beta, y = ctx.saved_tensors
        cfg = ctx.cfg
        lib = load()
        dev = x.device
        N, C = x.shape
        act, ev = ACTS[cfg.act], int(not cfg.training)
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        dy = dy.to(torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        dgamma = torch.empty(C, **f32) if need_w else None
        dbeta = torch.empty(C, **f32) if need_b else None
        block = None
        if cfg.training or need_w or need_b:
            parts = -(-N // row_chunk(C))
            partials = torch.empty(parts, 2 * C, dtype=torch.float64, device=dev)
            block = torch.empty(1 + 2 * C, dtype=torch.float64, device=dev)
            call(lib.u3d_bn_bwd_reduce, dy, x, y, N, C, act, ev, cfg.eps, mean, second, gamma, beta, partials, dev=dev)
            call(lib.u3d_bn_sum, partials, parts, C, float(N), block, dbeta, dgamma, dev=dev)
            block = _reduced(block, cfg.stat_reduce) if cfg.training else None
        dx = torch.empty_like(x) if need_x else None
        dres = None
        if need_r:
            dres = dy if cfg.act == "none" else torch.empty_like(x)
        if dx is not None or (dres is not None and dres is not dy):
            call(lib.u3d_bn_bwd_apply, dy, x, y, N, C, act, ev, cfg.eps, mean, second, gamma, beta, block, dx,
                 None if dres is dy else dres, dev=dev)
        return dx, dgamma, dbeta, dres, None


def _check_act(act):
    if act not in ACTS:
        raise NotImplementedError(f"act={act!r} is not implemented (one of {', '.join(ACTS)}; gelu is the erf form, there is no tanh GELU)")


def _torch_lines(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, residual):
    """torch's own lines (CPU tensors): _BatchNorm.forward's bookkeeping, F.batch_norm, the add and the activation."""
    factor = 0.0 if momentum is None else momentum
    if training and num_batches_tracked is not None:
        num_batches_tracked.add_(1)
        if momentum is None:
            factor = 1.0 / float(num_batches_tracked)
    out = F.batch_norm(x, running_mean, running_var, weight, bias, training, factor, eps)
    if residual is not None:
        out = out + residual
    return F.relu(out) if act == "relu" else F.gelu(out) if act == "gelu" else out


def batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked=None, *, training, momentum, eps, act="none",
                   residual=None, stat_reduce=None):
    """x (N, C) fp32 with contiguous rows -> act(batch_norm(x) [+ residual]) (N, C).

    weight, bias      (C) or None (affine=False).
    running_mean, running_var, num_batches_tracked   the module's buffers or None.  training=True: batch statistics; the buffers are
                      updated in place as BatchNorm1d does (momentum None = cumulative average, which needs num_batches_tracked).
                      training=False: the running statistics are folded and the forward is one pass.
    act               "none", "relu" or "gelu" (the erf form); residual (N, C) is added before it and goes with "none" and "relu" only.
    stat_reduce       None, or a callable that takes the f64 block `count | sum [C] | sum [C]` of the forward and of the backward and
                      returns the reduced block."""
    _check_act(act)
    if residual is not None and act == "gelu":
        raise NotImplementedError("act='gelu' with a residual is not implemented (no reference layer has it)")
    if x.dim() != 2:
        raise ValueError(f"x: expected (N, C), got {tuple(x.shape)}")
    N, C = x.shape
    named = (("x", x, (N, C)), ("weight", weight, (C,)), ("bias", bias, (C,)), ("running_mean", running_mean, (C,)),
             ("running_var", running_var, (C,)), ("residual", residual, (N, C)))
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
    for name, t in (("x", x), ("residual", residual), ("running_mean", running_mean), ("running_var", running_var)):
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
    if N == 0:
        return x.new_empty(0, C)
    if training and N < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
    if not x.is_cuda:
        return _torch_lines(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, act, residual)
    on_device("batchnorm", x, weight, bias, running_mean, running_var, num_batches_tracked, residual)
    load()
    cfg = _Cfg()
    cfg.training, cfg.eps, cfg.momentum, cfg.act = training, float(eps), momentum, act
    cfg.stat_reduce = stat_reduce if training else None
    # (eval mode reads the running statistics and updates nothing; without them there is no count to advance either)
    cfg.running = (running_mean, running_var, num_batches_tracked if training and running_mean is not None else None)
    return _BatchNormAct.apply(x, weight, bias, residual, cfg)


class BatchNormAct(nn.BatchNorm1d):
    """nn.BatchNorm1d over (N, C) rows with the activation (and the residual add before it) in the same kernels.  Same constructor
    plus `act`, same parameters, buffers and state_dict keys.  forward(x, residual=None)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, act="none", device=None, dtype=None):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)
        _check_act(act)
        self.act = act
        self.sync = False                       # made from an nn.SyncBatchNorm: statistics are all-reduced over process_group
        self.process_group = None

    def extra_repr(self):
        return super().extra_repr() + f", act={self.act!r}" + (", sync=True" if self.sync else "")

    def _all_reduce(self, block):
        torch.distributed.all_reduce(block, group=self.process_group)
        return block

    def forward(self, x, residual=None):
        training = self.training or self.running_mean is None
        reduce = None
        if training and self.sync and x.is_cuda and torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size(self.process_group) > 1:
            reduce = self._all_reduce
        track = self.training and self.track_running_stats
        return batch_norm_act(x, self.weight, self.bias, self.running_mean if (track or not training) else None,
                              self.running_var if (track or not training) else None, self.num_batches_tracked if track else None,
                              training=training, momentum=self.momentum, eps=self.eps, act=self.act, residual=residual,
                              stat_reduce=reduce)

    @classmethod
    def from_norm(cls, norm, act="none"):
        """A BatchNormAct that shares `norm`'s Parameter and buffer objects (nn.BatchNorm1d or nn.SyncBatchNorm)."""
        new = cls(norm.num_features, norm.eps, norm.momentum, False, False, act=act)
        new.affine, new.track_running_stats = norm.affine, norm.track_running_stats
        for name in ("weight", "bias"):
            new._parameters[name] = norm._parameters[name]
        for name in ("running_mean", "running_var", "num_batches_tracked"):
            new._buffers[name] = norm._buffers[name]
        new.training = norm.training
        if isinstance(norm, nn.SyncBatchNorm):
            new.sync, new.process_group = True, norm.process_group
        return new


def _act_of(module):
    """"relu" / "gelu" for an activation module the kernels have, None otherwise (a tanh GELU among them)."""
    if type(module) is nn.ReLU:
        return "relu"
    if type(module) is nn.GELU and module.approximate == "none":
        return "gelu"
    return None


def fuse_norm_act(model, sequential_types=("PointSequential",)):
    """Replaces, in place, every BatchNorm1d / SyncBatchNorm of an nn.Sequential subclass (SparseSequential included) or of a container
    whose class name is in `sequential_types` by a BatchNormAct that shares its Parameters and buffers; an nn.ReLU or exact nn.GELU
    right behind it moves into it and becomes nn.Identity (a pair with a tanh GELU is left as it is).  Call it after convert_sync_batchnorm.  Returns the number of replacements."""
    count = 0
    for container in list(model.modules()):
        if not (isinstance(container, nn.Sequential) or type(container).__name__ in sequential_types):
            continue
        names = list(container._modules)
        for k, name in enumerate(names):
            norm = container._modules[name]
            if type(norm) not in (nn.BatchNorm1d, nn.SyncBatchNorm):
                continue
            nxt = container._modules[names[k + 1]] if k + 1 < len(names) else None
            if type(nxt) is nn.GELU and nxt.approximate != "none":
                continue                            # a tanh GELU has no kernel: the pair is left alone
            act = _act_of(nxt) if nxt is not None else None
            container._modules[name] = BatchNormAct.from_norm(norm, act or "none")
            if act is not None:
                container._modules[names[k + 1]] = nn.Identity()
            count += 1
    return count


class BasicBlock(nn.Module):
    """The reference's residual block (spconv_unet_v1m1_base.py:25-104) over unipre3d_amd.sparseconv: same constructor, child names
    and state_dict keys (proj.0, proj.1, conv1, bn1, conv2, bn2); bn1 + relu is one call and bn2 + residual + relu is one call.
    norm_fn is called as in the reference; what it returns must be an nn.BatchNorm1d or nn.SyncBatchNorm, whose settings are kept."""

    expansion = 1

    def __init__(self, in_channels, embed_channels, stride=1, norm_fn=None, indice_key=None, bias=False):
        super().__init__()
        from . import sparseconv as spconv
        assert norm_fn is not None
        if in_channels == embed_channels:
            self.proj = spconv.SparseSequential(nn.Identity())
        else:
            self.proj = spconv.SparseSequential(spconv.SubMConv3d(in_channels, embed_channels, kernel_size=1, bias=False),
                                                self._norm(norm_fn, embed_channels, "none"))
        self.conv1 = spconv.SubMConv3d(in_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias,
                                       indice_key=indice_key)
        self.bn1 = self._norm(norm_fn, embed_channels, "relu")
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias,
                                       indice_key=indice_key)
        self.bn2 = self._norm(norm_fn, embed_channels, "relu")
        self.stride = stride

    @staticmethod
    def _norm(norm_fn, channels, act):
        norm = norm_fn(channels)
        if isinstance(norm, BatchNormAct):
            norm.act = act
            return norm
        if type(norm) not in (nn.BatchNorm1d, nn.SyncBatchNorm):
            raise NotImplementedError(f"BasicBlock: norm_fn gave {type(norm).__name__} (nn.BatchNorm1d or nn.SyncBatchNorm only)")
        return BatchNormAct.from_norm(norm, act)

    def forward(self, x):
        residual = x
        out = self.conv1(x)
        out = out.replace_feature(self.bn1(out.features))
        out = self.conv2(out)
        out = out.replace_feature(self.bn2(out.features, self.proj(residual).features))
        return out
