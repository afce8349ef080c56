"""Offset-batched ("ragged") point operators with the names and argument order of openpoints/cpp/pointops/functions/pointops.py,
backed by libunipre3d_offsetops.so (include/unipre3d_offsetops.h); no CPU fallback.

A batch is concatenated: xyz (n,3) with `offset` (b) the cumulative ends of its clouds, queries new_xyz (m,3) with `new_offset` (b).
Offsets are int32 or int64 DEVICE tensors; nothing here reads them on the host (no .item(), no sync).

  knnquery         (nsample, xyz, new_xyz, offset, new_offset) -> (idx int32 (m,nsample), dist = sqrt(dist2))
  knn_query        (nsample, xyz, offset, new_xyz=None, new_offset=None): the Pointcept argument order of
                   pointcept/engines/hooks/evaluator.py:125-132 (`import unipre3d_amd.offset_ops as pointops`)
  knn_query_raw    the thin core -> (dist2, idx)
  ballquery        (radius, nsample, xyz, new_xyz, offset, new_offset) -> idx int32 (m,nsample)
  furthestsampling (xyz, offset, new_offset, m=None) -> idx int32 (m,): furthest point sampling per segment, absolute rows
                   (libunipre3d_pointops.so: u3d_offset_furthest_sampling, include/unipre3d_pointops.h)
  grouping, subtraction, aggregation, interpolation2      autograd Functions (fp32 kernels, first-order gradients)
  interpolation, querygroup, queryandgroup                compositions, as the reference writes them

Everywhere new_xyz=None means xyz and new_offset=None means offset.  (The reference asserts new_xyz.is_contiguous() before its own
None test in querygroup / queryandgroup and so raises on the documented None: SURVEY.md, defect appendix.)

kNN selects the k smallest (squared distance, index) pairs of the query's own segment in lexicographic order, ascending.  The
reference keeps a per-thread max-heap; on inputs without equal distances the two give the same rows, order and fill slots included
(tests/offsetops_ref.py transcribes the heap; tests/test_offsetops_ref.py compares), on exact ties the heap's choice is an accident
of its layout and this module's is the lower index.  nsample may exceed a segment's size: the extra slots hold the segment's first
row at distance 1e5 (= sqrt(1e10), the reference's initial value), or -1 where the segment is empty.

The scatter-add gradients (grouping, interpolation2, the second input of subtraction, the input of aggregation) are summed with
float atomics and may differ in their last bits from run to run.  An index outside its tensor is skipped, never dereferenced (the
header says what each operator writes then).  Coordinates must be 3-D (NotImplementedError otherwise); nsample above 64 raises
ValueError.  Everything runs on torch's current stream."""
from __future__ import annotations

import ctypes
import os

import torch
from torch.autograd import Function

from . import _lib
from . import pointops as _pointops
from ._lib import as_f32, as_i32, call, on_device

__all__ = ["knn_query_raw", "knnquery", "knn_query", "ballquery", "furthestsampling", "grouping", "subtraction", "aggregation",
           "interpolation2", "interpolation", "querygroup", "queryandgroup"]

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_offsetops.so")
MAX_K = 64                                                    # include/unipre3d_knn.h: U3D_KNN_MAX_K
FILL_DIST2 = 1e10

_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_offsetops.h
    "u3d_offset_knn": (_i, [_i, _i, _i, _i] + [_vp] * 7),
    "u3d_offset_ballquery": (_i, [_i, _i, _i, _f, _i] + [_vp] * 6),
    "u3d_offset_group_forward": (_i, [_i, _i, _i, _i] + [_vp] * 4),
    "u3d_offset_group_backward": (_i, [_i, _i, _i, _i] + [_vp] * 4),
    "u3d_offset_interpolate_forward": (_i, [_i, _i, _i, _i] + [_vp] * 5),
    "u3d_offset_interpolate_backward": (_i, [_i, _i, _i, _i] + [_vp] * 5),
    "u3d_offset_subtract_forward": (_i, [_i, _i, _i] + [_vp] * 5),
    "u3d_offset_subtract_backward": (_i, [_i, _i, _i] + [_vp] * 5),
    "u3d_offset_aggregate_forward": (_i, [_i, _i, _i, _i] + [_vp] * 6),
    "u3d_offset_aggregate_backward": (_i, [_i, _i, _i, _i] + [_vp] * 9),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_offsetops.so", SIGNATURES)


def _search_args(nsample, xyz, new_xyz, offset, new_offset):
    if new_xyz is None:
        new_xyz = xyz
    if new_offset is None:
        new_offset = offset
    if xyz.dim() != 2 or new_xyz.dim() != 2:
        raise ValueError(f"xyz (n,3) and new_xyz (m,3) expected, got {tuple(xyz.shape)} and {tuple(new_xyz.shape)}")
    if xyz.size(1) != 3 or new_xyz.size(1) != 3:
        raise NotImplementedError(f"the searches are built for 3 coordinates, got {xyz.size(1)} and {new_xyz.size(1)}")
    if offset.dim() != 1 or new_offset.dim() != 1 or offset.numel() != new_offset.numel():
        raise ValueError(f"offset (b) and new_offset (b) expected, got {tuple(offset.shape)} and {tuple(new_offset.shape)}")
    nsample = int(nsample)
    if nsample < 1 or nsample > MAX_K:
        raise ValueError(f"nsample = {nsample} is outside 1..{MAX_K}")
    dev = on_device("offset_ops", xyz, new_xyz, offset, new_offset)
    return nsample, as_f32(xyz, "xyz"), as_f32(new_xyz, "new_xyz"), as_i32(offset, "offset"), as_i32(new_offset, "new_offset"), dev


@torch.no_grad()
def knn_query_raw(nsample, xyz, new_xyz, offset, new_offset):
    """-> (dist2 (m,nsample) fp32 squared distances, idx (m,nsample) int32 global rows of xyz), ascending in (dist2, index)."""
    k, xyz, new_xyz, offset, new_offset, dev = _search_args(nsample, xyz, new_xyz, offset, new_offset)
    n, m, b = xyz.size(0), new_xyz.size(0), offset.numel()
    if b == 0:                                                    # no segment: every row gets the fill of an empty one
        return (torch.full((m, k), FILL_DIST2, dtype=torch.float32, device=dev), torch.full((m, k), -1, dtype=torch.int32, device=dev))
    dist2 = torch.empty(m, k, dtype=torch.float32, device=dev)
    idx = torch.empty(m, k, dtype=torch.int32, device=dev)
    call(load().u3d_offset_knn, b, n, m, k, xyz, new_xyz, offset, new_offset, dist2, idx, dev=dev)
    return dist2, idx


def knnquery(nsample, xyz, new_xyz, offset, new_offset):
    """pointops.py `knnquery`: -> (idx int32 (m,nsample), dist (m,nsample))."""
    dist2, idx = knn_query_raw(nsample, xyz, new_xyz, offset, new_offset)
    return idx, torch.sqrt(dist2)


def knn_query(nsample, xyz, offset, new_xyz=None, new_offset=None):
    """Pointcept's `pointops.knn_query(nsample, xyz, offset, new_xyz, new_offset)` -> (idx int32 (m,nsample), dist)."""
    return knnquery(nsample, xyz, new_xyz, offset, new_offset)


@torch.no_grad()
def ballquery(radius, nsample, xyz, new_xyz, offset, new_offset):
    """pointops.py `ballquery`: -> idx int32 (m,nsample): the segment's first nsample rows closer than `radius`, padded with the first
    hit; all 0 where nothing is that close."""
    ns, xyz, new_xyz, offset, new_offset, dev = _search_args(nsample, xyz, new_xyz, offset, new_offset)
    n, m, b = xyz.size(0), new_xyz.size(0), offset.numel()
    if b == 0:
        return torch.zeros(m, ns, dtype=torch.int32, device=dev)
    idx = torch.empty(m, ns, dtype=torch.int32, device=dev)
    call(load().u3d_offset_ballquery, b, n, m, float(radius), ns, xyz, new_xyz, offset, new_offset, idx, dev=dev)
    return idx


@torch.no_grad()
def furthestsampling(xyz, offset, new_offset, m=None):
    """pointops.py `furthestsampling`: xyz (n,3), offset (b), new_offset (b) -> idx int32 (m,): segment s contributes its
    new_offset[s] - new_offset[s-1] furthest-point-sampled rows, as ABSOLUTE rows of xyz, starting from its first row; equal distances
    resolve as the reference's block does for its largest segment.  m defaults to int(new_offset[-1]) -- the reference's one host
    sync; pass it to avoid the sync.  A segment asked for nothing writes nothing, an empty segment asked for rows gets -1 (SURVEY.md,
    defect appendix); any other -1 means the kernel's status word was set (unipre3d_amd.pointops.grid_status).  No autograd: indices.
    A batch beyond the grid's capacity of (256 - b) * 4096 rows raises."""
    if xyz.dim() != 2:
        raise ValueError(f"xyz (n,3) expected, got {tuple(xyz.shape)}")
    if xyz.size(1) != 3:
        raise NotImplementedError(f"furthest point sampling is built for 3 coordinates, got {xyz.size(1)}")
    if offset.dim() != 1 or new_offset.dim() != 1 or offset.numel() != new_offset.numel():
        raise ValueError(f"offset (b) and new_offset (b) expected, got {tuple(offset.shape)} and {tuple(new_offset.shape)}")
    dev = on_device("offset_ops", xyz, offset, new_offset)
    xyz, offset, new_offset = as_f32(xyz, "xyz"), as_i32(offset, "offset"), as_i32(new_offset, "new_offset")
    n, b = xyz.size(0), offset.numel()
    if m is None:
        m = int(new_offset[-1]) if b else 0
    m = int(m)
    if m < 0:
        raise ValueError(f"m = {m} is negative")
    idx = torch.full((m,), -1, dtype=torch.int32, device=dev)
    if b == 0 or m == 0:
        return idx
    rc = call(_pointops.load().u3d_offset_furthest_sampling, b, n, m, xyz, offset, new_offset, _pointops.grid_workspace(b, dev), idx,
              dev=dev, accept=(_pointops.STATUS_OVER_CAPACITY,))
    if rc == _pointops.STATUS_OVER_CAPACITY:
        raise RuntimeError(f"furthestsampling: {n} rows in {b} segments are beyond the grid kernel's capacity")
    return idx


def _idx2(idx, rows, what):
    if idx.dim() != 2 or idx.size(0) != rows:
        raise ValueError(f"{what}: idx ({rows},nsample) expected, got {tuple(idx.shape)}")
    return as_i32(idx, "idx")


def _out(empty, *shape, dev):
    """An output the library fills -- or zeros where the call is empty and the library writes nothing."""
    return (torch.zeros if empty else torch.empty)(*shape, dtype=torch.float32, device=dev)


class Grouping(Function):
    """input (n,c), idx (m,nsample) -> (m,nsample,c)"""

    @staticmethod
    def forward(ctx, input, idx):
        if input.dim() != 2:
            raise ValueError(f"grouping: input (n,c) expected, got {tuple(input.shape)}")
        dev = on_device("offset_ops", input, idx)
        idx = _idx2(idx, idx.size(0) if idx.dim() == 2 else -1, "grouping")
        x = as_f32(input, "input")
        (n, c), (m, ns) = x.shape, idx.shape
        out = torch.empty(m, ns, c, dtype=torch.float32, device=dev)
        call(load().u3d_offset_group_forward, m, ns, c, n, x, idx, out, dev=dev)
        ctx.n, ctx.in_dtype = n, input.dtype
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        idx, = ctx.saved_tensors
        g = as_f32(grad_output, "grad_output")
        m, ns, c = g.shape
        grad = _out(m * ns == 0, ctx.n, c, dev=g.device)
        call(load().u3d_offset_group_backward, m, ns, c, ctx.n, g, idx, grad, dev=g.device)
        return grad.to(ctx.in_dtype), None


grouping = Grouping.apply


class Subtraction(Function):
    """input1 (n,c), input2 (n,c), idx (n,nsample) -> (n,nsample,c): input1[i] - input2[idx[i,s]]"""

    @staticmethod
    def forward(ctx, input1, input2, idx):
        if input1.dim() != 2 or input1.shape != input2.shape:
            raise ValueError(f"subtraction: two (n,c) inputs expected, got {tuple(input1.shape)} and {tuple(input2.shape)}")
        dev = on_device("offset_ops", input1, input2, idx)
        idx = _idx2(idx, input1.size(0), "subtraction")
        a, b2 = as_f32(input1, "input1"), as_f32(input2, "input2")
        (n, c), ns = a.shape, idx.size(1)
        out = torch.empty(n, ns, c, dtype=torch.float32, device=dev)
        call(load().u3d_offset_subtract_forward, n, ns, c, a, b2, idx, out, dev=dev)
        ctx.dtypes = (input1.dtype, input2.dtype)
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        idx, = ctx.saved_tensors
        g = as_f32(grad_output, "grad_output")
        n, ns, c = g.shape
        g1 = torch.empty(n, c, dtype=torch.float32, device=g.device)
        g2 = torch.empty(n, c, dtype=torch.float32, device=g.device)
        call(load().u3d_offset_subtract_backward, n, ns, c, idx, g, g1, g2, dev=g.device)
        return g1.to(ctx.dtypes[0]), g2.to(ctx.dtypes[1]), None


subtraction = Subtraction.apply


class Aggregation(Function):
    """input (n,c), position (n,nsample,c), weight (n,nsample,w_c), idx (n,nsample) -> (n,c):
    sum_s (input[idx[i,s]] + position[i,s]) * weight[i,s, channel % w_c]"""

    @staticmethod
    def forward(ctx, input, position, weight, idx):
        if input.dim() != 2 or position.dim() != 3 or weight.dim() != 3 or position.shape[:2] != weight.shape[:2] \
                or position.size(0) != input.size(0) or position.size(2) != input.size(1):
            raise ValueError(f"aggregation: input (n,c), position (n,nsample,c), weight (n,nsample,w_c) expected, got "
                             f"{tuple(input.shape)}, {tuple(position.shape)}, {tuple(weight.shape)}")
        n, ns, c = position.shape
        w_c = weight.size(2)
        if w_c < 1 or c % w_c != 0:
            raise ValueError(f"aggregation: c = {c} is no multiple of w_c = {w_c}")
        dev = on_device("offset_ops", input, position, weight, idx)
        idx = _idx2(idx, n, "aggregation")
        if idx.size(1) != ns:
            raise ValueError(f"aggregation: idx ({n},{ns}) expected, got {tuple(idx.shape)}")
        x, p, w = as_f32(input, "input"), as_f32(position, "position"), as_f32(weight, "weight")
        out = torch.empty(n, c, dtype=torch.float32, device=dev)
        call(load().u3d_offset_aggregate_forward, n, ns, c, w_c, x, p, w, idx, out, dev=dev)
        ctx.dtypes = (input.dtype, position.dtype, weight.dtype)
        ctx.save_for_backward(x, p, w, idx)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        x, p, w, idx = ctx.saved_tensors
        g = as_f32(grad_output, "grad_output")
        n, ns, c = p.shape
        w_c, dev = w.size(2), g.device
        gx = torch.empty(n, c, dtype=torch.float32, device=dev)
        gp = torch.empty(n, ns, c, dtype=torch.float32, device=dev)
        gw = torch.empty(n, ns, w_c, dtype=torch.float32, device=dev)
        call(load().u3d_offset_aggregate_backward, n, ns, c, w_c, x, p, w, idx, g, gx, gp, gw, dev=dev)
        return gx.to(ctx.dtypes[0]), gp.to(ctx.dtypes[1]), gw.to(ctx.dtypes[2]), None


aggregation = Aggregation.apply


def _interpolation_weights(xyz, new_xyz, offset, new_offset, k):
    """The reference's inverse-distance weights, in torch as it computes them: 1 / (dist + 1e-8), normalised over the k neighbours."""
    idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)
    dist_recip = 1.0 / (dist + 1e-8)
    return idx, dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)


class _WeightedGather(Function):
    """input (m,c), idx (n,k), weight (n,k) -> (n,c): sum_j input[idx[i,j]] * weight[i,j]; gradient to `input` only."""

    @staticmethod
    def forward(ctx, input, idx, weight):
        dev = on_device("offset_ops", input, idx, weight)
        x, w, idx = as_f32(input, "input"), as_f32(weight, "weight"), as_i32(idx, "idx")
        (m_in, c), (n_out, k) = x.shape, idx.shape
        out = torch.empty(n_out, c, dtype=torch.float32, device=dev)
        call(load().u3d_offset_interpolate_forward, n_out, c, k, m_in, x, idx, w, out, dev=dev)
        ctx.m_in, ctx.in_dtype = m_in, input.dtype
        ctx.save_for_backward(idx, w)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        idx, w = ctx.saved_tensors
        g = as_f32(grad_output, "grad_output")
        n_out, c = g.shape
        grad = _out(n_out * idx.size(1) == 0, ctx.m_in, c, dev=g.device)
        call(load().u3d_offset_interpolate_backward, n_out, c, idx.size(1), ctx.m_in, g, idx, w, grad, dev=g.device)
        return grad.to(ctx.in_dtype), None, None


def interpolation2(xyz, new_xyz, input, offset, new_offset, k=3):
    """pointops.py `interpolation2`: xyz (m,3), new_xyz (n,3), input (m,c) -> (n,c), the inverse-distance mean of the k nearest rows of
    the query's own segment; differentiable in `input` (the reference's Function returns no other gradient either)."""
    if input.dim() != 2 or input.size(0) != xyz.size(0):
        raise ValueError(f"interpolation: input ({xyz.size(0)},c) expected, got {tuple(input.shape)}")
    idx, weight = _interpolation_weights(xyz, new_xyz, offset, new_offset, k)
    return _WeightedGather.apply(input, idx, weight)


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """pointops.py `interpolation` (its torch-indexing form of the same sum): one kernel here, same gradient."""
    return interpolation2(xyz, new_xyz, feat, offset, new_offset, k)


def querygroup(nsample, xyz, new_xyz, feat, offset, new_offset, radius=None, query_method="knn", normalize_dp=False, idx=None):
    """pointops.py `querygroup` -> (grouped_xyz (m,nsample,3) relative to the query, grouped_feat (m,nsample,c) or None); 'knn' /
    'knnquery' search by kNN, any other query_method by ball query with `radius`.  A given `idx` (m,nsample) is used as it is (the
    reference returns None there); nsample=None, whose branch in the reference indexes a third dimension (n,3) tensors do not
    have, raises."""
    if new_xyz is None:
        new_xyz = xyz
    if new_offset is None:
        new_offset = offset
    if idx is None:
        if nsample is None:
            raise ValueError("querygroup needs nsample or idx")
        if query_method in ("knn", "knnquery"):
            idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
        else:
            idx = ballquery(radius, nsample, xyz, new_xyz, offset, new_offset)
    grouped_xyz = grouping(xyz, idx) - new_xyz.unsqueeze(1)
    if normalize_dp:
        if query_method == "knn":
            grouped_xyz = grouped_xyz / (grouped_xyz.norm(dim=-1, p=2, keepdim=True).max(dim=-1, keepdim=True)[0] + 1.0e-8)
        else:
            grouped_xyz = grouped_xyz / radius
    return grouped_xyz, (grouping(feat, idx) if feat is not None else None)


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True):
    """pointops.py `queryandgroup` -> (m,nsample,3+c) (relative coordinates first) or (m,nsample,c) with use_xyz=False."""
    if new_xyz is None:
        new_xyz = xyz
    if new_offset is None:
        new_offset = offset
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
    grouped_feat = grouping(feat, idx)
    if not use_xyz:
        return grouped_feat
    return torch.cat((grouping(xyz, idx) - new_xyz.unsqueeze(1), grouped_feat), -1)
