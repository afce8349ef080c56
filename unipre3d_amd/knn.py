"""k-nearest-neighbour search in 3-D with the names and call shapes of the reference's groupers, backed by libunipre3d_knn.so
(include/unipre3d_knn.h); no CPU fallback.

  knn_query        the thin core: squared distances and int32 indices
  KNN              `from knn_cuda import KNN` of openpoints/models/Mamba3D/Mamba3D.py:16 (`Group` :95-129, `GroupFeature` :132-175)
  knn_point        openpoints/models/layers/knn.py:7-20 (and its `KNN` module :23-61, whose forward is knn_point with `.int()` indices)
  OpenpointsKNN    `KNN` of openpoints/models/layers/group.py:12-28
  KNNGroup         openpoints/models/layers/group.py:275-320, over pointops.grouping_operation
  xyz_knn_point    `knn_point` of openpoints/models/PCM/PCM_utils.py:141-168 and of backbone/pointmlp.py:102-113

Every search selects the k smallest (squared distance, index) pairs in lexicographic order and returns them ascending: equal
distances go to the lower index.  The reference's forms leave ties to torch.topk and compute the distance in three different ways
(direct, |a|^2 + |b|^2 - 2ab, cdist); tests/golden/g16_knn.npz records that they all select these indices on seeded clouds.
Coordinates must be 3-D: anything else raises NotImplementedError (feature-space kNN is not built).  The search has no gradient and
runs under no_grad on torch's current stream."""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn as nn

from . import _lib
from ._lib import as_f32, call, on_device

LIB_PATH = os.path.join(_lib.LIB_DIR, "libunipre3d_knn.so")   # (U3D_LIB_DIRNAME: experiment builds, see _lib.py)
MAX_K, TILE, QUERIES = 64, 2048, 16                           # include/unipre3d_knn.h: U3D_KNN_MAX_K, U3D_KNN_TILE, U3D_KNN_QUERIES

_i, _vp = ctypes.c_int, ctypes.c_void_p
SIGNATURES = {   # include/unipre3d_knn.h
    "u3d_knn": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "u3d_knn_path": (_i, [_i, _i]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return _lib.open_library("libunipre3d_knn.so", SIGNATURES)


@torch.no_grad()
def knn_query(k: int, support: torch.Tensor, query: torch.Tensor):
    """support (B,N,3), query (B,M,3) -> (dist2 (B,M,k) fp32 squared distances, idx (B,M,k) int32), ascending in (dist2, index)."""
    if support.dim() != 3 or query.dim() != 3 or support.size(0) != query.size(0):
        raise ValueError(f"support (B,N,3) and query (B,M,3) expected, got {tuple(support.shape)} and {tuple(query.shape)}")
    if support.size(2) != 3 or query.size(2) != 3:
        raise NotImplementedError(f"kNN is built for 3 coordinates, got {support.size(2)} and {query.size(2)}")
    dev = on_device("knn", support, query)
    B, N, _ = support.shape
    M, k = query.size(1), int(k)
    if k < 1 or k > N or k > MAX_K:
        raise ValueError(f"k = {k} is outside 1..min(N = {N}, {MAX_K})")
    support, query = as_f32(support, "support"), as_f32(query, "query")
    dist2 = torch.empty(B, M, k, dtype=torch.float32, device=dev)
    idx = torch.empty(B, M, k, dtype=torch.int32, device=dev)
    call(load().u3d_knn, B, N, M, k, support, query, dist2, idx, dev=dev, what="knn")
    return dist2, idx


class KNN(nn.Module):
    """The `knn_cuda.KNN` Mamba3D imports: KNN(k, transpose_mode)(ref, query) -> (dist, idx int64).  transpose_mode=True takes
    (B,N,3) / (B,M,3) and returns (B,M,k); False takes (B,3,N) / (B,3,M) and returns (B,k,M).  Mamba3D adds an int64 base to idx and
    indexes with it.  [UPSTREAM-RECALL] knn_cuda is not part of the reference tree: these conventions (argument order, layouts,
    root distances, ascending order) are recalled from the upstream package and pinned by no recorded value."""

    def __init__(self, k: int, transpose_mode: bool = False):
        super().__init__()
        self.k, self._t = k, transpose_mode

    @torch.no_grad()
    def forward(self, ref: torch.Tensor, query: torch.Tensor):
        if not self._t:
            ref, query = ref.transpose(1, 2), query.transpose(1, 2)
        dist2, idx = knn_query(self.k, ref, query)
        dist, idx = torch.sqrt(dist2), idx.long()
        if not self._t:
            dist, idx = dist.transpose(1, 2).contiguous(), idx.transpose(1, 2).contiguous()
        return dist, idx


def knn_point(k: int, query: torch.Tensor, support: torch.Tensor = None):
    """layers/knn.py:7-20: query (B,M,3), support (B,N,3) (None: the queries themselves) -> (dist (B,M,k), idx int64 (B,M,k))."""
    dist2, idx = knn_query(k, query if support is None else support, query)
    return torch.sqrt(dist2), idx.long()


class OpenpointsKNN(nn.Module):
    """layers/group.py:12-28: forward(support (B,N,3), query (B,M,3)) -> (dist, idx int32 (B,M,k)).  Like the reference's, which takes
    topk along dim 1 of cdist(support, query) and transposes the indices alone, `dist` comes back as (B,k,M)."""

    def __init__(self, neighbors: int, transpose_mode: bool = True):
        super().__init__()
        self.neighbors = neighbors

    @torch.no_grad()
    def forward(self, support: torch.Tensor, query: torch.Tensor):
        dist2, idx = knn_query(self.neighbors, support, query)
        return torch.sqrt(dist2).transpose(1, 2), idx


class KNNGroup(nn.Module):
    """layers/group.py:275-320 (relative_xyz / normalize_dp / return_only_idx options)."""

    def __init__(self, nsample: int, relative_xyz=True, normalize_dp=False, return_only_idx=False, **kwargs):
        super().__init__()
        self.nsample = nsample
        self.knn = OpenpointsKNN(nsample, transpose_mode=True)
        self.relative_xyz, self.normalize_dp, self.return_only_idx = relative_xyz, normalize_dp, return_only_idx

    def forward(self, query_xyz: torch.Tensor, support_xyz: torch.Tensor, features: torch.Tensor = None):
        """query_xyz (B,npoint,3), support_xyz (B,N,3), features (B,C,N) -> (grouped_xyz (B,3,npoint,nsample), grouped features or None)."""
        from .pointops import grouping_operation
        _, idx = self.knn(support_xyz, query_xyz)
        if self.return_only_idx:
            return idx
        grouped_xyz = grouping_operation(support_xyz.transpose(1, 2).contiguous(), idx)
        if self.relative_xyz:
            grouped_xyz = grouped_xyz - query_xyz.transpose(1, 2).unsqueeze(-1)
        if self.normalize_dp:
            grouped_xyz = grouped_xyz / torch.amax(torch.sqrt(torch.sum(grouped_xyz ** 2, dim=1)), dim=(1, 2)).view(-1, 1, 1, 1)
        return grouped_xyz, (grouping_operation(features, idx) if features is not None else None)


def xyz_knn_point(nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor, training: bool = True) -> torch.Tensor:
    """PCM_utils.py:141-168 / pointmlp.py:102-113: xyz (B,N,3) all points, new_xyz (B,S,3) queries -> idx int64 (B,S,nsample).
    `training` only chooses how the reference splits its distance matrix; PointMLP asks topk for sorted=False, for which ascending
    order is one valid answer."""
    return knn_query(nsample, xyz, new_xyz)[1].long()
