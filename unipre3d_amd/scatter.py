"""torch_scatter's segment_csr on the device (`import unipre3d_amd.scatter as torch_scatter` is the switch for PTv3's
SerializedPooling).  Kernels: libunipre3d_attention.so (include/unipre3d_attention.h): gather form, one thread per (segment, channel)
walks its rows in ascending order, every output element is written once, no atomics, no host read.

Rules: an empty segment gives 0 (torch_scatter's).  sum / mean add in ascending row order in fp32.  max / min send the gradient to ONE row
per (segment, channel): the lowest row index that attains the extremum.  NaN: a NaN in a segment wins max and min alike (the result
is NaN) and the gradient goes to the lowest NaN row.  Rows outside [indptr[0], indptr[-1]) get a zero gradient.
"""
from __future__ import annotations

import torch

from ._lib import call, on_device
from .attention import load

REDUCE = {"sum": 0, "add": 0, "mean": 1, "max": 2, "min": 3}
EXPORTS = ("u3d_segment_csr_fwd", "u3d_segment_csr_bwd")


class _SegmentCSR(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, indptr, reduce):
        N, C = src.shape
        M = indptr.numel() - 1
        out = torch.empty(M, C, dtype=torch.float32, device=src.device)
        arg = torch.empty(M, C, dtype=torch.int64, device=src.device) if reduce >= 2 else None
        call(load().u3d_segment_csr_fwd, src, indptr, out, arg, N, M, C, reduce, dev=src.device)
        ctx.save_for_backward(indptr, arg)
        ctx.args = (N, M, C, reduce)
        ctx.mark_non_differentiable(indptr)
        return out

    @staticmethod
    def backward(ctx, dout):
        indptr, arg = ctx.saved_tensors
        N, M, C, reduce = ctx.args
        dout = dout.to(torch.float32).contiguous()
        dsrc = torch.empty(N, C, dtype=torch.float32, device=dout.device)
        call(load().u3d_segment_csr_bwd, dout, indptr, arg, dsrc, N, M, C, reduce, dev=dout.device)
        return dsrc, None, None


def segment_csr(src, indptr, out=None, reduce="sum"):
    """torch_scatter.segment_csr for src (N, C) fp32 contiguous and indptr (M+1,) int64 on the device, ascending, within 0 .. N:
    out[m] = reduce over rows indptr[m] .. indptr[m+1]-1, reduce in sum | mean | max | min.  Returns (M, C) (written into `out` when
    given); differentiable with respect to src.  See the module docstring for empty segments, ties and NaN."""
    if reduce not in REDUCE:
        raise ValueError(f"reduce={reduce!r}: expected one of sum, mean, max, min")
    load()
    on_device("scatter", src, indptr)
    if src.dim() != 2 or indptr.dim() != 1:
        raise NotImplementedError(f"segment_csr: src (N, C) with indptr (M+1,) only, got {tuple(src.shape)} and {tuple(indptr.shape)}")
    if src.dtype != torch.float32:
        raise NotImplementedError(f"src: dtype {src.dtype} is not implemented (fp32 only)")
    if indptr.dtype != torch.int64 or indptr.numel() < 1:
        raise ValueError(f"indptr: expected a non-empty int64 tensor, got {tuple(indptr.shape)} {indptr.dtype}")
    if src.shape[1] < 1:
        raise ValueError("src: at least one channel")
    if not src.is_contiguous():
        raise ValueError("src: a non-contiguous tensor is not supported (call .contiguous())")
    res = _SegmentCSR.apply(src, indptr.contiguous(), REDUCE[reduce])
    if out is not None:
        out.copy_(res)
        return out
    return res
