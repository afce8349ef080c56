"""The LocalGrouper of PointMLP (openpoints/models/backbone/pointmlp.py:116-195) and of PCM (openpoints/models/PCM/PointMLP_layers.py:23-82):
`from unipre3d_amd.local_grouper import LocalGrouper` (PointMLP) and `from unipre3d_amd.local_grouper import PCMLocalGrouper as LocalGrouper`
(PCM) are the two switches.  The two gathers, the cat with the coordinates, the subtraction of the group mean or of the anchor, the one
std per batch element, the affine, the repeat and the second cat are one operator in libunipre3d_local_grouper.so
(include/unipre3d_local_grouper.h, csrc/u3d_local_grouper.hip): the (B, S, K, 2D+A) result is written once, and nothing of its size is
kept for the backward.

  local_group(xyz, points, fps_idx, idx, alpha, beta, normalize, use_xyz, eps, channels_first)   the autograd function
  LocalGrouper, PCMLocalGrouper                                                                    the reference's two modules

`points` is read in place when its rows are contiguous or when it is the permute(0, 2, 1) view of a (B, D, N) tensor (what both callers
pass), and its gradient comes back in the same layout.  channels_first=True stores the result as (B, S, C, K) and returns the
permute(0, 1, 3, 2) view of it: shape and values are the reference's, and PreExtraction's permute(0, 1, 3, 2).reshape(-1, d, s) is a view.

Two departures from the reference: a std of exactly 0 gives zero, not NaN, for the variance term of the gradient; and without the
`idx` override the neighbours along K come in this project's order (ascending distance, ties to the lower index), where PointMLP's
topk(sorted=False) leaves the order unspecified -- every consumer max-pools over K.

Scope: fp32, 1 <= S <= N <= 16384, 2 <= K <= 64, D a multiple of 4 and at most 512, B S K < 2^24 and B N < 2^24; anything else raises
(there is no fallback).  There is no gradient to xyz: it is input data in every caller, and xyz.requires_grad raises."""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib, knn, pointops
from ._lib import byte_buffer, call, on_device

ABI_VERSION = 1
MAX_POINTS, MAX_K, MAX_CHANNELS = 16384, 64, 512          # include/unipre3d_local_grouper.h
NORMALIZE = {None: 0, "none": 0, "center": 1, "anchor": 2}

_i, _f, _vp, _ll = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong
SIGNATURES = {   # include/unipre3d_local_grouper.h
    "u3d_local_grouper_abi_version": (_i, []),
    "u3d_local_grouper_scratch_bytes": (ctypes.c_size_t, [_i] * 8),
    "u3d_local_grouper_lists": (_i, [_vp] * 7 + [_i] * 4 + [_vp]),
    "u3d_local_grouper_fwd": (_i, [_vp, _vp, _ll, _ll, _ll] + [_vp] * 9 + [_i] * 8 + [_f, _vp]),
    "u3d_local_grouper_bwd": (_i, [_vp, _vp, _ll, _ll, _ll] + [_vp] * 11 + [_ll, _ll, _ll] + [_vp] * 3 + [_i] * 8 + [_vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_local_grouper.so", SIGNATURES, ("u3d_local_grouper_abi_version", ABI_VERSION))


def _strides(t, N, D):
    """(batch, point, channel) strides of a (B, N, D) tensor in one of the two forms the library reads, or None."""
    sb, sp, sc = t.stride()
    if t.shape[0] == 1:
        sb = N * D
    if t.data_ptr() % 16 != 0 or sb < N * D:
        return None
    if (sp, sc) == (D, 1) or (N == 1 and sc == 1):
        return sb, D, 1
    if (sp, sc) == (1, N) or (D == 1 and sp == 1):
        return sb, 1, N
    return None


class _LocalGroup(torch.autograd.Function):
    """(xyz, points, alpha, beta, fps, idx, normalize, use_xyz, eps, channels_first) -> (out storage, new_xyz, stats)."""

    @staticmethod
    def forward(ctx, xyz, points, alpha, beta, fps, idx, normalize, use_xyz, eps, cf):
        B, N, D = points.shape
        S, K = idx.shape[1], idx.shape[2]
        A = 3 if use_xyz else 0
        Cn, C = D + A, 2 * D + A
        dev = points.device
        lib = load()
        sb, sp, sc = _strides(points, N, D)
        out = torch.empty((B, S, C, K) if cf else (B, S, K, C), dtype=torch.float32, device=dev)
        new_xyz = torch.empty(B, S, 3, dtype=torch.float32, device=dev)
        mean = stats = None
        if normalize:
            mean = torch.empty(B, S, Cn, dtype=torch.float32, device=dev)
            stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
        scratch = byte_buffer(lib.u3d_local_grouper_scratch_bytes(B, N, S, K, D, int(use_xyz), normalize, 0), dev)
        call(lib.u3d_local_grouper_fwd, xyz, points, sb, sp, sc, fps, idx, alpha, beta, out, new_xyz, mean, stats, scratch,
             B, N, S, K, D, int(use_xyz), normalize, int(cf), eps, dev=dev)
        ctx.lists = None
        if any(ctx.needs_input_grad):
            ptr = torch.empty(B, N + 1, dtype=torch.int32, device=dev)
            ent = torch.empty(B, S * K, dtype=torch.int32, device=dev)
            fptr = torch.empty(B, N + 1, dtype=torch.int32, device=dev)
            fent = torch.empty(B, S, dtype=torch.int32, device=dev)
            ls = byte_buffer(lib.u3d_local_grouper_scratch_bytes(B, N, S, K, D, int(use_xyz), normalize, 2), dev)
            call(lib.u3d_local_grouper_lists, fps, idx, ptr, ent, fptr, fent, ls, B, N, S, K, dev=dev)
            ctx.lists = (ptr, ent, fptr, fent)
        ctx.save_for_backward(xyz, points, alpha, mean, stats)
        ctx.fps, ctx.idx = fps, idx
        ctx.args = (normalize, int(use_xyz), cf)
        if stats is None:
            stats = torch.empty(0, 4, dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(new_xyz, stats)
        return out, new_xyz, stats

    @staticmethod
    def backward(ctx, dout, _dxyz, _dstats):
        xyz, points, alpha, mean, stats = ctx.saved_tensors
        normalize, use_xyz, cf = ctx.args
        fps, idx = ctx.fps, ctx.idx
        ptr, ent, fptr, fent = ctx.lists
        B, N, D = points.shape
        S, K = idx.shape[1], idx.shape[2]
        Cn = D + (3 if use_xyz else 0)
        dev = points.device
        lib = load()
        # dout in the logical (B, S, K, C) shape, read in place in either storage order
        g = (dout.permute(0, 1, 3, 2) if cf else dout).to(torch.float32)
        if g.is_contiguous() and g.data_ptr() % 16 == 0:
            dcf = 0
        elif g.permute(0, 1, 3, 2).is_contiguous() and g.data_ptr() % 16 == 0:
            dcf = 1
        else:
            g, dcf = g.contiguous(), 0
        sb, sp, sc = _strides(points, N, D)
        if sp == 1 and N > 1:
            dpoints = torch.empty(B, D, N, dtype=torch.float32, device=dev).permute(0, 2, 1)
        else:
            dpoints = torch.empty(B, N, D, dtype=torch.float32, device=dev)
        gb, gp, gc = _strides(dpoints, N, D)
        dalpha = dbeta = None
        if normalize:
            dalpha, dbeta = torch.empty(Cn, dtype=torch.float32, device=dev), torch.empty(Cn, dtype=torch.float32, device=dev)
        scratch = byte_buffer(lib.u3d_local_grouper_scratch_bytes(B, N, S, K, D, use_xyz, normalize, 1), dev)
        call(lib.u3d_local_grouper_bwd, xyz, points, sb, sp, sc, fps, idx, ptr, ent, fptr, fent, alpha, mean, stats, g,
             dpoints, gb, gp, gc, dalpha, dbeta, scratch, B, N, S, K, D, use_xyz, normalize, dcf, dev=dev)
        return None, dpoints, dalpha, dbeta, None, None, None, None, None, None


def local_group_with_stats(xyz, points, fps_idx, idx, alpha, beta, normalize, use_xyz, eps: float = 1e-5, channels_first: bool = True):
    """local_group, and the per-batch (B, 4) statistics mu, s, r, r^2 / ((n - 1) s) behind it ((0, 4) with normalize = none)."""
    if normalize is not None and not isinstance(normalize, str):
        raise ValueError(f"normalize={normalize!r}: expected None, 'none', 'center' or 'anchor'")
    key = normalize.lower() if isinstance(normalize, str) else None
    if key not in NORMALIZE:
        raise ValueError(f"normalize={normalize!r}: expected None, 'none', 'center' or 'anchor'")
    mode = NORMALIZE[key]
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz: expected (B, N, 3), got {tuple(xyz.shape)}")
    if points.dim() != 3 or points.shape[:2] != xyz.shape[:2]:
        raise ValueError(f"points: expected (B, N, D) with xyz's B and N, got {tuple(points.shape)}")
    if idx.dim() != 3:
        raise ValueError(f"idx: expected (B, S, K), got {tuple(idx.shape)}")
    if xyz.requires_grad:
        raise NotImplementedError("xyz.requires_grad: there is no gradient to xyz (it is input data in every caller)")
    B, N, D = points.shape
    S, K = idx.shape[1], idx.shape[2]
    use_xyz = bool(use_xyz)
    Cn = D + (3 if use_xyz else 0)
    if B < 1 or N < 1 or S < 1:
        raise ValueError(f"an empty tensor is not supported (B, N, S = {B}, {N}, {S})")
    tensors = [("xyz", xyz), ("points", points)] + ([("alpha", alpha), ("beta", beta)] if mode else [])
    for name, t in tensors:
        if t is None or t.dtype != torch.float32:
            raise NotImplementedError(f"{name}: dtype {None if t is None else t.dtype} is not implemented (fp32 only)")
    if not S <= N <= MAX_POINTS:
        raise NotImplementedError(f"N={N}, S={S} is not implemented (S <= N <= {MAX_POINTS})")
    if not 2 <= K <= MAX_K:
        raise NotImplementedError(f"idx: K={K} is not implemented (2 to {MAX_K})")
    if D % 4 != 0 or not 4 <= D <= MAX_CHANNELS:
        raise NotImplementedError(f"points: D={D} is not implemented (a multiple of 4, at most {MAX_CHANNELS})")
    if B * S * K >= 1 << 24 or B * N >= 1 << 24:
        raise NotImplementedError(f"B S K = {B * S * K}, B N = {B * N} is not implemented (both below 2^24)")
    if fps_idx is None and S != N:
        raise ValueError(f"fps_idx=None is the identity and needs S == N, got S={S}, N={N}")
    eps = float(eps)
    if not 0.0 <= eps < float("inf"):
        raise ValueError(f"eps={eps}: must be a non-negative finite number")
    if mode and (alpha.numel() != Cn or beta.numel() != Cn):
        raise ValueError(f"alpha, beta: expected D + A = {Cn} values, got {alpha.numel()} and {beta.numel()}")
    for name, t, shape in (("idx", idx, (B, S, K)), ("fps_idx", fps_idx, (B, S))):
        if t is not None and t.dtype not in (torch.int32, torch.int64):
            raise NotImplementedError(f"{name}: dtype {t.dtype} is not implemented (int32 or int64)")
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected {shape}, got {tuple(t.shape)}")
    on_device("local_grouper", xyz, points, fps_idx, idx, alpha if mode else None, beta if mode else None)
    idx = idx.to(torch.int32).contiguous()
    fps = None if fps_idx is None else fps_idx.to(torch.int32).contiguous()
    alpha, beta = (alpha.reshape(-1), beta.reshape(-1)) if mode else (None, None)
    xyz = xyz.contiguous()
    if _strides(points, N, D) is None:
        points = points.contiguous()
    load()
    out, new_xyz, stats = _LocalGroup.apply(xyz, points, alpha, beta, fps, idx, mode, use_xyz, eps, bool(channels_first))
    return new_xyz, (out.permute(0, 1, 3, 2) if channels_first else out), stats


def local_group(xyz, points, fps_idx, idx, alpha, beta, normalize, use_xyz, eps: float = 1e-5, channels_first: bool = True):
    """The geometric affine grouping of the reference's LocalGrouper on xyz (B, N, 3), points (B, N, D) fp32, anchors fps_idx (B, S) (None:
    the identity, S == N) and neighbours idx (B, S, K) -> (new_xyz (B, S, 3), new_points (B, S, K, 2D + A)), A = 3 with use_xyz.

    Per batch element, with g = cat(points[idx], xyz[idx]), m = mean_k g (normalize 'center') or cat(points[fps], xyz[fps]) ('anchor'),
    d = g - m and s the std of all of d (n - 1 in the denominator): new_points = cat(alpha d / (s + eps) + beta, points[fps] repeated K
    times); with normalize None or 'none' the first part is g and alpha, beta are ignored.  An idx entry outside [0, N) counts as the
    anchor, an fps_idx entry outside [0, N) as point s.  alpha and beta hold D + A values in any shape (the reference's [1, 1, 1, D + A]).
    Differentiable with respect to points, alpha and beta.  Kept for the backward: the inputs, m (B, S, D + A), four scalars per batch
    element and the inverse lists of idx and fps_idx (int32, as many as idx and fps_idx have entries, plus 2 (N + 1) per batch element).
    channels_first=True returns the permute(0, 1, 3, 2) view of a (B, S, C, K) tensor, False a contiguous (B, S, K, C) one."""
    return local_group_with_stats(xyz, points, fps_idx, idx, alpha, beta, normalize, use_xyz, eps, channels_first)[:2]


def _gather_rows(t, index):
    return torch.gather(t, 1, index.long().unsqueeze(-1).expand(-1, -1, t.shape[-1]))


class LocalGrouper(nn.Module):
    """PointMLP's LocalGrouper (pointmlp.py:116-195) with its constructor and its state_dict keys (`affine_alpha`, `affine_beta`,
    [1, 1, 1, D + A]).  forward(xyz (B, N, 3), points (B, N, D), fps_idx=None, idx=None) -> (new_xyz (B, S, 3), new_points (B, S, K, 2D + A)).
    Without the overrides the anchors are pointops.furthest_point_sample's and the neighbours knn.knn_query's, so the order along K is
    ascending distance with ties to the lower index (the reference's topk(sorted=False) leaves it unspecified; every consumer max-pools
    over K).  `channels_first` (an attribute, True) chooses the storage order of new_points, see local_group."""

    def __init__(self, channel, sample_ratio, kneighbors, use_xyz=True, normalize="center", **kwargs):
        super().__init__()
        self.sample_ratio = sample_ratio
        self.kneighbors = kneighbors
        self.use_xyz = use_xyz
        self.normalize = normalize.lower() if normalize is not None else None
        if self.normalize not in ["center", "anchor"]:
            self.normalize = None
        self.channels_first = True
        if self.normalize is not None:
            add_channel = 3 if self.use_xyz else 0
            self.affine_alpha = nn.Parameter(torch.ones([1, 1, 1, channel + add_channel]))
            self.affine_beta = nn.Parameter(torch.zeros([1, 1, 1, channel + add_channel]))

    def _group(self, xyz, points, fps_idx, idx):
        alpha, beta = (self.affine_alpha, self.affine_beta) if self.normalize is not None else (None, None)
        return local_group(xyz, points, fps_idx, idx, alpha, beta, self.normalize, self.use_xyz, 1e-5, self.channels_first)

    def forward(self, xyz, points, fps_idx=None, idx=None):
        B, N, _ = xyz.shape
        S = N // self.sample_ratio
        xyz = xyz.contiguous()
        if fps_idx is None:
            fps_idx = pointops.furthest_point_sample(xyz, S)
        if idx is None:
            idx = knn.knn_query(self.kneighbors, xyz, _gather_rows(xyz, fps_idx))[1]
        return self._group(xyz, points, fps_idx, idx)


class PCMLocalGrouper(LocalGrouper):
    """PCM's LocalGrouper (PointMLP_layers.py:23-82): PointMLP's plus `k_stride` (every k_stride-th of the kneighbors neighbours is
    kept), the sorted fps_idx, the S == N shortcut (no sampling: every point is its own anchor) and points_res, which is gathered at the
    anchors.  forward(xyz, points, points_res, fps_idx=None, idx=None) -> (new_xyz, new_points, points_res); an `idx` override is
    strided like the search's result."""

    def __init__(self, channel, sample_ratio, kneighbors=12, use_xyz=True, normalize="center", k_stride=1, **kwargs):
        super().__init__(channel, sample_ratio, kneighbors, use_xyz, normalize, **kwargs)
        self.k_stride = k_stride

    def forward(self, xyz, points, points_res, fps_idx=None, idx=None):
        B, N, _ = xyz.shape
        S = N // self.sample_ratio
        xyz = xyz.contiguous()
        if S == N:
            fps_idx, anchors = None, xyz
        else:
            if fps_idx is None:
                fps_idx = pointops.furthest_point_sample(xyz, S)
            fps_idx = torch.sort(fps_idx.long(), dim=-1)[0]
            anchors = _gather_rows(xyz, fps_idx)
            if points_res is not None:
                points_res = _gather_rows(points_res, fps_idx)
        if idx is None:
            idx = knn.knn_query(self.kneighbors, xyz, anchors)[1]
        idx = idx[:, :, ::self.k_stride]
        new_xyz, new_points = self._group(xyz, points, fps_idx, idx)
        return new_xyz, new_points, points_res
