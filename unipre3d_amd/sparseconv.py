"""Sparse 3D convolution with the names the reference imports as `spconv.pytorch` (`import unipre3d_amd.sparseconv as spconv`):
SparseConvTensor, SparseModule, SparseSequential, Identity, SubMConv3d, SparseConv3d and SparseInverseConv3d.  Maps and GEMMs run in
libunipre3d_sparseconv.so (include/unipre3d_sparseconv.h); there is no CPU path.  fp32 only.

Weights are Parameters of shape (Cout, k, k, k, Cin), spconv >= 2.2's layout as recalled; spconv does not exist for ROCm, so the
layout could not be checked against it here.  Dense equivalents use `W.permute(0, 4, 1, 2, 3)` (Conv3d) and `W.permute(4, 0, 1, 2, 3)`
(ConvTranspose3d).  Tap t = (k0 * k + k1) * k + k2 reads the site at offset (k0, k1, k2) - k // 2 (SubM) or out * s + (k0, k1, k2)
(strided).

Semantics (tests/spconv_ref.py restates them):
  SubMConv3d      output rows are the input rows in the same order; `padding` is ignored; without repeated sites the result is
                  Conv3d(padding=k // 2) on the dense grid (empty sites 0) sampled at the active sites.  Odd k <= 5, dilation 1.
  SparseConv3d    kernel_size == stride = s, padding 0: output sites are {d // s} within out_shape = (D - s) // s + 1 (others are
                  dropped), rows in ascending (batch, d0, d1, d2); equals Conv3d(s, stride=s) sampled at them.
  SparseInverseConv3d  paired with a SparseConv3d through indice_key: output rows are that conv's input rows, in the same order,
                  with its spatial shape; equals ConvTranspose3d(s, stride=s) sampled at them (rows the conv dropped get the bias).
  bias            added at every output row.
  repeated sites  (PointFusion appends fused pixel voxels that often share a site with a 3D voxel) are deterministic: SubM reads the
                  site's LOWEST row at every tap, the centre included -- a repeated row still gets an output, its input gradient is 0;
                  SparseConv3d sums all rows at a site; the inverse writes every repeated row.
Maps are cached in the tensor's `indice_dict` under `indice_key` and reused (SpUNet's decoder meets the encoder's `subm{s}` keys).  Once
a map exists, SubM and inverse forward and backward never read the device from the host; building a strided map reads its output
count once.  Repeated calls are bit-identical (no float atomics; fixed-order reductions).
"""
from __future__ import annotations

import ctypes
import math
import os

import torch
import torch.nn as nn

from . import _lib
from ._lib import call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_sparseconv.so")
ABI_VERSION = 1

_i, _vp, _size = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
SIGNATURES = {   # include/unipre3d_sparseconv.h
    "u3d_spconv_abi_version": (_i, []),
    "u3d_spconv_scratch_bytes": (_size, [_i]),
    "u3d_spconv_subm_map": (_i, [_i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_spconv_down_map": (_i, [_i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "u3d_spconv_down_emit": (_i, [_i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "u3d_spconv_gemm": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "u3d_spconv_dupsum": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_spconv_wgrad_partial_floats": (_size, [_i, _i, _i, _i]),
    "u3d_spconv_wgrad": (_i, [_i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_spconv_colsum_partial_floats": (_size, [_i, _i]),
    "u3d_spconv_colsum": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_sparseconv.so", SIGNATURES, ("u3d_spconv_abi_version", ABI_VERSION))


def _indices(indices):
    idx = indices.to(torch.int32).contiguous()
    if idx.dim() != 2 or idx.shape[1] != 4:
        raise ValueError(f"indices: expected (N,4) (batch, d0, d1, d2), got {tuple(idx.shape)}")
    if idx.data_ptr() % 16:
        idx = idx.clone()   # the kernels read a row as one int4
    return idx


def _shape3(spatial_shape):
    s = [int(x) for x in spatial_shape]
    if len(s) != 3:
        raise ValueError(f"spatial_shape: expected 3 sizes, got {spatial_shape}")
    return s


# ---- maps ------------------------------------------------------------------------------------------------------------------------
class SubMMap:
    """table (N,K) int32: lowest row at each tap's site or -1; first (N): lowest row at the row's site; next (N): next row there."""
    kind = "subm"

    def __init__(self, k, table, first, next_):
        self.k, self.table, self.first, self.next = k, table, first, next_


class DownMap:
    """SparseConv3d (kernel == stride = s) map: out_indices (M,4), out_shape, table (M,K) lowest row per (output, tap), first / next over
    rows at the same input site, the (tap, output, row)-ordered list of all N rows (list_row, list_src = output * K + tap or -1), and the
    input's indices / spatial shape (restored by the paired inverse)."""
    kind = "down"

    def __init__(self, k, in_indices, in_shape, out_indices, out_shape, table, first, next_, list_row, list_src):
        self.k, self.in_indices, self.in_shape, self.out_indices, self.out_shape = k, in_indices, in_shape, out_indices, out_shape
        self.table, self.first, self.next, self.list_row, self.list_src = table, first, next_, list_row, list_src


def subm_map(indices, spatial_shape, batch_size, k) -> SubMMap:
    dev = on_device("sparseconv", indices)
    idx = _indices(indices)
    D = _shape3(spatial_shape)
    N, K = idx.shape[0], k ** 3
    lib = load()
    table = torch.empty(N, K, dtype=torch.int32, device=dev)
    first = torch.empty(N, dtype=torch.int32, device=dev)
    nxt = torch.empty(N, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(lib.u3d_spconv_scratch_bytes(N), 1), dtype=torch.uint8, device=dev)
    call(lib.u3d_spconv_subm_map, N, idx, int(batch_size), D[0], D[1], D[2], k, table, first, nxt, scratch, dev=dev)
    return SubMMap(k, table, first, nxt)


def down_map(indices, spatial_shape, batch_size, s) -> DownMap:
    dev = on_device("sparseconv", indices)
    idx = _indices(indices)
    D = _shape3(spatial_shape)
    if min(D) < s:
        raise ValueError(f"SparseConv3d: spatial shape {D} is smaller than the kernel {s}")
    N, K = idx.shape[0], s ** 3
    lib = load()
    scratch = torch.empty(max(lib.u3d_spconv_scratch_bytes(N), 1), dtype=torch.uint8, device=dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)
    call(lib.u3d_spconv_down_map, N, idx, int(batch_size), D[0], D[1], D[2], s, meta, scratch, dev=dev)
    M = int(meta[0].item())                    # the map's one device -> host read: the output count
    out_indices = torch.empty(M, 4, dtype=torch.int32, device=dev)
    table = torch.empty(M, K, dtype=torch.int32, device=dev)
    first = torch.empty(N, dtype=torch.int32, device=dev)
    nxt = torch.empty(N, dtype=torch.int32, device=dev)
    list_row = torch.empty(N, dtype=torch.int32, device=dev)
    list_src = torch.empty(N, dtype=torch.int32, device=dev)
    call(lib.u3d_spconv_down_emit, N, M, idx, int(batch_size), D[0], D[1], D[2], s, out_indices, table, first, nxt, list_row, list_src,
         scratch, dev=dev)
    out_shape = [(d - s) // s + 1 for d in D]
    return DownMap(s, idx, D, out_indices, out_shape, table, first, nxt, list_row, list_src)


# ---- device ops ------------------------------------------------------------------------------------------------------------------
def _gemm(R, K, A, W, bias, table, list_row=None, mask=None, out_rows=None):
    """Y (out_rows, Cout): table mode Y[o] = bias + sum_k A[table[o,k]] W[k]; list mode over list_row / table = list_src.  W (K,Cin,Cout)."""
    Cin, Cout = W.shape[1], W.shape[2]
    if A.shape[0] == 0:   # a strided conv that dropped every row: no entry has a source, the rows are bias (or 0); never read
        A = A.new_zeros(1, Cin)
    Y = torch.empty(R if out_rows is None else out_rows, Cout, dtype=torch.float32, device=A.device)
    call(load().u3d_spconv_gemm, R, K, Cin, Cout, table, list_row, A, W, bias, mask, Y, dev=A.device)
    return Y


def _dupsum(X, first, nxt):
    out = torch.empty_like(X)
    call(load().u3d_spconv_dupsum, X.shape[0], X.shape[1], first, nxt, X, out, dev=X.device)
    return out


def _wgrad(R, K, A, G, table, gather_g):
    """(K, Cin, Cout): dW[k] = sum_o A[ia]^T G[ig] with the table on A's side (gather_g=0) or G's side (gather_g=1)."""
    Cin, Cout = A.shape[1], G.shape[1]
    lib = load()
    part = torch.empty(max(lib.u3d_spconv_wgrad_partial_floats(R, K, Cin, Cout), 1), dtype=torch.float32, device=A.device)
    dW = torch.empty(K, Cin, Cout, dtype=torch.float32, device=A.device)
    call(lib.u3d_spconv_wgrad, R, K, Cin, Cout, table, int(gather_g), A, G, part, dW, dev=A.device)
    return dW


def _colsum(G):
    R, C = G.shape
    lib = load()
    part = torch.empty(max(lib.u3d_spconv_colsum_partial_floats(R, C), 1), dtype=torch.float32, device=G.device)
    db = torch.empty(C, dtype=torch.float32, device=G.device)
    call(lib.u3d_spconv_colsum, R, C, G, part, db, dev=G.device)
    return db


def _w_fwd(W):      # (Cout, K, Cin) -> (K, Cin, Cout)
    return W.permute(1, 2, 0).contiguous()


def _w_bwd(W):      # (Cout, K, Cin) -> (K, Cout, Cin): W_k^T
    return W.permute(1, 0, 2).contiguous()


def _f32(t, name):
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {t.dtype} (fp32 only)")
    return t.contiguous()


class _SubMConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, W, bias, m):
        Cout, K, Cin = W.shape[0], m.k ** 3, W.shape[-1]
        X, W3 = _f32(X.detach(), "features"), W.detach().reshape(Cout, K, Cin).contiguous()
        b = None if bias is None else bias.detach().contiguous()
        ctx.m, ctx.has_bias, ctx.shape = m, bias is not None, W.shape
        ctx.save_for_backward(X, W3)
        return _gemm(X.shape[0], K, X, _w_fwd(W3), b, m.table)

    @staticmethod
    def backward(ctx, gY):
        X, W3 = ctx.saved_tensors
        m = ctx.m
        Cout, K, Cin = W3.shape
        gY = gY.contiguous().float()
        N = X.shape[0]
        gX = gW = gb = None
        if ctx.needs_input_grad[0]:
            # dX[i] = sum_k S[T[i, K-1-k]] W_k^T at the lowest row of each site (0 elsewhere), S = dY summed over the site's rows
            S = _dupsum(gY, m.first, m.next)
            gX = _gemm(N, K, S, _w_bwd(W3).flip(0).contiguous(), None, m.table, mask=m.first)
        if ctx.needs_input_grad[1]:
            gW = _wgrad(N, K, X, gY, m.table, 0).permute(2, 0, 1).reshape(ctx.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _colsum(gY)
        return gX, gW, gb, None


class _DownConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, W, bias, m):
        Cout, K, Cin = W.shape[0], m.k ** 3, W.shape[-1]
        X, W3 = _f32(X.detach(), "features"), W.detach().reshape(Cout, K, Cin).contiguous()
        b = None if bias is None else bias.detach().contiguous()
        Xs = _dupsum(X, m.first, m.next)       # rows at one input site are summed
        ctx.m, ctx.has_bias, ctx.shape = m, bias is not None, W.shape
        ctx.save_for_backward(Xs, W3)
        return _gemm(m.table.shape[0], K, Xs, _w_fwd(W3), b, m.table)

    @staticmethod
    def backward(ctx, gY):
        Xs, W3 = ctx.saved_tensors
        m = ctx.m
        Cout, K, Cin = W3.shape
        gY = gY.contiguous().float()
        N, M = Xs.shape[0], gY.shape[0]
        gX = gW = gb = None
        if ctx.needs_input_grad[0]:   # dX[i] = dY[out(i)] W_tap(i)^T, every row (dropped rows 0)
            gX = _gemm(N, K, gY, _w_bwd(W3), None, m.list_src, list_row=m.list_row)
        if ctx.needs_input_grad[1]:
            gW = _wgrad(M, K, Xs, gY, m.table, 0).permute(2, 0, 1).reshape(ctx.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _colsum(gY)
        return gX, gW, gb, None


class _InverseConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, W, bias, m):
        Cout, K, Cin = W.shape[0], m.k ** 3, W.shape[-1]
        X, W3 = _f32(X.detach(), "features"), W.detach().reshape(Cout, K, Cin).contiguous()
        b = None if bias is None else bias.detach().contiguous()
        ctx.m, ctx.has_bias, ctx.shape = m, bias is not None, W.shape
        ctx.save_for_backward(X, W3)
        N = m.list_row.shape[0]
        return _gemm(N, K, X, _w_fwd(W3), b, m.list_src, list_row=m.list_row)

    @staticmethod
    def backward(ctx, gY):
        X, W3 = ctx.saved_tensors
        m = ctx.m
        Cout, K, Cin = W3.shape
        gY = gY.contiguous().float()
        M = X.shape[0]
        gX = gW = gb = None
        need_s = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        S = _dupsum(gY, m.first, m.next) if need_s else None   # dY summed over the rows of each fine site
        if ctx.needs_input_grad[0]:
            gX = _gemm(M, K, S, _w_bwd(W3), None, m.table)
        if ctx.needs_input_grad[1]:
            gW = _wgrad(M, K, X, S, m.table, 1).permute(2, 0, 1).reshape(ctx.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _colsum(gY)
        return gX, gW, gb, None


# ---- spconv.pytorch names -------------------------------------------------------------------------------------------------------
class SparseConvTensor:
    """features (N,C), indices (N,4) int32 (batch, d0, d1, d2), spatial_shape (3 ints), batch_size; maps in `indice_dict`."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None, voxel_num=None, indice_dict=None, benchmark=False):
        self._features = features
        self.indices = indices
        self.spatial_shape = [int(x) for x in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {} if indice_dict is None else indice_dict
        self.grid = grid
        self.voxel_num = voxel_num
        self.benchmark = benchmark
        self.benchmark_record = {}

    @property
    def features(self):
        return self._features

    @features.setter
    def features(self, value):
        self._features = value

    def replace_feature(self, feature):
        """A new tensor with the same sites, shape and maps and these features (spconv 2's way to change features)."""
        if feature.shape[0] != self.indices.shape[0]:
            raise ValueError(f"replace_feature: {feature.shape[0]} rows for {self.indices.shape[0]} sites")
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.grid, self.voxel_num, self.indice_dict,
                                self.benchmark)

    def find_indice_pair(self, key):
        return self.indice_dict.get(key) if key is not None else None

    @property
    def spatial_size(self):
        return math.prod(self.spatial_shape)

    def dense(self, channels_first: bool = True):
        """(B, C, D0, D1, D2) (channels_first) or (B, D0, D1, D2, C); rows at a repeated site are summed."""
        C = self.features.shape[1]
        out = self.features.new_zeros(self.batch_size, *self.spatial_shape, C)
        idx = self.indices.long()
        out = out.index_put((idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]), self.features, accumulate=True)
        return out.permute(0, 4, 1, 2, 3).contiguous() if channels_first else out


class SparseModule(nn.Module):
    """Base of the modules that take and return a SparseConvTensor."""


def _is_sparse_module(m):
    return isinstance(m, SparseModule)


class SparseSequential(nn.Sequential):
    """nn.Sequential over SparseConvTensor: sparse modules get the tensor, plain modules (BatchNorm1d, ReLU, Linear, ...) its features."""

    def forward(self, input):
        for module in self:
            if _is_sparse_module(module):
                input = module(input)
            elif isinstance(input, SparseConvTensor):
                if input.indices.shape[0] != 0:
                    input = input.replace_feature(module(input.features))
            else:
                input = module(input)
        return input


class Identity(SparseModule):
    def forward(self, input):
        return input


def _cube(v, what):
    if isinstance(v, int):
        return v
    v = tuple(int(x) for x in v)
    if len(v) != 3 or len(set(v)) != 1:
        raise NotImplementedError(f"{what} {v}: only equal sizes on the three axes")
    return v[0]


class _SparseConvNd(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None,
                 algo=None, fp32_accum=None, name=None, **unused):
        super().__init__()
        if groups != 1:
            raise NotImplementedError("groups != 1")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = _cube(kernel_size, "kernel_size")
        self.stride, self.padding, self.dilation = _cube(stride, "stride"), _cube(padding, "padding"), _cube(dilation, "dilation")
        self.groups, self.indice_key, self.algo, self.fp32_accum, self.name = groups, indice_key, algo, fp32_accum, name
        self._check_scope()
        k = self.kernel_size
        self.weight = nn.Parameter(torch.empty(self.out_channels, k, k, k, self.in_channels))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # torch's Conv default (kaiming_uniform with a = sqrt(5)): bound 1 / sqrt(fan_in), fan_in = Cin * k^3
        bound = 1.0 / math.sqrt(max(self.in_channels * self.kernel_size ** 3, 1))
        nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            nn.init.uniform_(self.bias, -bound, bound)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, bias={self.bias is not None}, indice_key={self.indice_key!r}")

    def _input(self, x):
        if not isinstance(x, SparseConvTensor):
            raise TypeError(f"{type(self).__name__} takes a SparseConvTensor, got {type(x).__name__}")
        if x.features.shape[1] != self.in_channels:
            raise ValueError(f"{type(self).__name__}: {x.features.shape[1]} input channels, expected {self.in_channels}")
        on_device("sparseconv", x.features, x.indices)


class SubMConv3d(_SparseConvNd):
    """Submanifold conv: output sites = input sites, same order.  Odd kernel_size <= 5, stride 1, dilation 1; padding is ignored."""

    def _check_scope(self):
        if self.kernel_size % 2 == 0 or self.kernel_size > 5:
            raise NotImplementedError(f"SubMConv3d: kernel_size {self.kernel_size} (odd sizes up to 5 only)")
        if self.stride != 1 or self.dilation != 1:
            raise NotImplementedError("SubMConv3d: stride and dilation 1 only")

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        self._input(x)
        N, k = x.indices.shape[0], self.kernel_size
        m = x.indice_dict.get(self.indice_key) if self.indice_key is not None else None
        if m is not None and (m.kind != "subm" or m.k != k or m.table.shape[0] != N):
            m = None if m.kind != "subm" else _mismatch(self.indice_key)
        if m is None:
            m = subm_map(x.indices, x.spatial_shape, x.batch_size, k)
            if self.indice_key is not None:
                x.indice_dict[self.indice_key] = m
        y = _SubMConv.apply(x.features, self.weight, self.bias, m)
        return x.replace_feature(y)


def _mismatch(key):
    raise ValueError(f"indice_key {key!r} names a map of another kernel size or site set")


class SparseConv3d(_SparseConvNd):
    """Strided sparse conv with kernel_size == stride and padding 0 (SpUNet's k = s = 2 down step)."""

    def _check_scope(self):
        if self.kernel_size != self.stride or self.padding != 0 or self.dilation != 1:
            raise NotImplementedError("SparseConv3d: kernel_size == stride, padding 0 and dilation 1 only")
        if self.kernel_size > 6:
            raise NotImplementedError("SparseConv3d: kernel_size up to 6")

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        self._input(x)
        m = x.indice_dict.get(self.indice_key) if self.indice_key is not None else None
        if m is not None and (m.kind != "down" or m.k != self.kernel_size or m.in_indices.shape[0] != x.indices.shape[0]):
            m = None if m.kind != "down" else _mismatch(self.indice_key)
        if m is None:
            m = down_map(x.indices, x.spatial_shape, x.batch_size, self.kernel_size)
            if self.indice_key is not None:
                x.indice_dict[self.indice_key] = m
        y = _DownConv.apply(x.features, self.weight, self.bias, m)
        return SparseConvTensor(y, m.out_indices, m.out_shape, x.batch_size, indice_dict=x.indice_dict, benchmark=x.benchmark)


class SparseInverseConv3d(_SparseConvNd):
    """Inverse of the SparseConv3d that stored its map under the same indice_key: back to that conv's input sites and shape."""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key=None, bias=True, **kw):
        if indice_key is None:
            raise ValueError("SparseInverseConv3d needs the indice_key of its SparseConv3d")
        kw.pop("stride", None)
        super().__init__(in_channels, out_channels, kernel_size, stride=kernel_size, bias=bias, indice_key=indice_key, **kw)

    def _check_scope(self):
        if self.padding != 0 or self.dilation != 1:
            raise NotImplementedError("SparseInverseConv3d: padding 0 and dilation 1 only")

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        self._input(x)
        m = x.indice_dict.get(self.indice_key)
        if m is None or m.kind != "down":
            raise ValueError(f"SparseInverseConv3d: no SparseConv3d map under indice_key {self.indice_key!r}")
        if m.k != self.kernel_size or m.out_indices.shape[0] != x.indices.shape[0]:
            _mismatch(self.indice_key)
        y = _InverseConv.apply(x.features, self.weight, self.bias, m)
        return SparseConvTensor(y, m.in_indices, m.in_shape, x.batch_size, indice_dict=x.indice_dict, benchmark=x.benchmark)


__all__ = ["SparseConvTensor", "SparseModule", "SparseSequential", "Identity", "SubMConv3d", "SparseConv3d", "SparseInverseConv3d",
           "subm_map", "down_map"]
