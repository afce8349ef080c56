#!/usr/bin/env python3
"""Generates tests/golden/g12_ptv3_boundary.npz: what crosses the two library boundaries of the reference's OWN PTv3 blocks
(pointcept/models/point_transformer_v3/point_transformer_v3m1_base.py), run on the CPU: SerializedAttention(enable_flash=True) ->
flash_attn.flash_attn_varlen_qkvpacked_func and SerializedPooling -> torch_scatter.segment_csr, for unipre3d_amd/attention.py and
unipre3d_amd/scatter.py.

Stubs: flash_attn and torch_scatter (recorders that return zeros of the right shape), spconv.pytorch (a recording SparseConvTensor),
addict.Dict (an attribute dict), timm's DropPath, pointcept's registry / PDNorm and fusion.point_fusion (unused here).
Batch: items of 17, 96, 130 and 97 points at patch 48 (one below the patch, one exact multiple, two that are not), 32 channels, 2 heads.
Only recorded data is stored: shapes, dtypes, cu_seqlens, max_seqlen, softmax_scale, indptr, reduce names, item sizes.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
SIZES, PATCH, C, H = (17, 96, 130, 97), 48, 32, 2
REC = {"attn": [], "csr": []}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class Dict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size

    def replace_feature(self, f):
        return SparseConvTensor(f, self.indices, self.spatial_shape, self.batch_size)


def _flash(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, **kw):
    REC["attn"].append(dict(shape=tuple(qkv.shape), dtype=str(qkv.dtype), cu=cu_seqlens.clone(), cu_dtype=str(cu_seqlens.dtype),
                            max_seqlen=int(max_seqlen), dropout_p=float(dropout_p), scale=float(softmax_scale)))
    return torch.zeros(qkv.shape[0], qkv.shape[2], qkv.shape[3], dtype=qkv.dtype)


def _segment_csr(src, indptr, out=None, reduce="sum"):
    REC["csr"].append(dict(shape=tuple(src.shape), dtype=str(src.dtype), indptr=indptr.clone(), indptr_dtype=str(indptr.dtype), reduce=reduce))
    return torch.zeros(indptr.numel() - 1, src.shape[1], dtype=src.dtype)


class _Registry:
    def register_module(self, *a, **k):
        return lambda c: c


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    _stub("addict", Dict=Dict)
    _stub("flash_attn", flash_attn_varlen_qkvpacked_func=_flash)
    _stub("torch_scatter", segment_csr=_segment_csr)
    sp = _stub("spconv")
    sp.pytorch = _stub("spconv.pytorch", SparseConvTensor=SparseConvTensor, SparseModule=torch.nn.Module,
                       modules=types.SimpleNamespace(is_spconv_module=lambda m: False))
    _stub("timm")
    _stub("timm.models")
    _stub("timm.models.layers", DropPath=torch.nn.Identity)
    _stub("fusion")
    _stub("fusion.point_fusion", PointFusion=object)
    _stub("pointcept")
    _stub("pointcept.models")
    _stub("pointcept.models.point_prompt_training", PDNorm=object)
    _stub("pointcept.models.builder", MODELS=_Registry())
    utils = _stub("pointcept.models.utils")
    misc = _load("pointcept.models.utils.misc", "pointcept/models/utils/misc.py")
    for n in ("offset2batch", "offset2bincount", "batch2offset"):
        setattr(utils, n, getattr(misc, n))
    sdir = os.path.join(REF, "pointcept/models/utils/serialization")
    if os.path.isdir(sdir):
        pk = _stub("pointcept.models.utils.serialization")
        pk.__path__ = [sdir]
        for f in sorted(os.listdir(sdir)):
            if f.endswith(".py") and f != "__init__.py":
                _load("pointcept.models.utils.serialization." + f[:-3], "pointcept/models/utils/serialization/" + f)
        ser = _load("pointcept.models.utils.serialization", "pointcept/models/utils/serialization/__init__.py")
    else:
        ser = _load("pointcept.models.utils.serialization", "pointcept/models/utils/serialization.py")
    utils.encode, utils.decode = ser.encode, ser.decode
    _load("pointcept.models.utils.structure", "pointcept/models/utils/structure.py")
    _load("pointcept.models.modules", "pointcept/models/modules.py")
    ptv3 = _load("ptv3_ref", "pointcept/models/point_transformer_v3/point_transformer_v3m1_base.py")

    torch.manual_seed(12)
    N = sum(SIZES)
    coord = torch.rand(N, 3) * 2.0
    point = ptv3.Point(Dict(coord=coord, grid_coord=(coord / 0.05).long(), feat=torch.randn(N, C),
                            offset=torch.cumsum(torch.tensor(SIZES), 0)))
    point.serialization(order=("z", "z-trans"), shuffle_orders=False)
    attn = ptv3.SerializedAttention(channels=C, num_heads=H, patch_size=PATCH, order_index=0, enable_rpe=False, enable_flash=True,
                                    upcast_attention=False, upcast_softmax=False).eval()
    attn(point)
    pool = ptv3.SerializedPooling(C, 2 * C, stride=2, norm_layer=None, act_layer=None, reduce="max", shuffle_orders=False)
    pool.norm = pool.act = None
    pool(point)
    a, (c0, c1) = REC["attn"][0], REC["csr"]
    assert len(REC["attn"]) == 1 and len(REC["csr"]) == 2 and a["dropout_p"] == 0.0
    np.savez(os.path.join(OUT, "g12_ptv3_boundary.npz"),
             item_sizes=np.asarray(SIZES, np.int64), patch_size=np.int64(PATCH),
             attn_qkv_shape=np.asarray(a["shape"], np.int64), attn_qkv_dtype=np.asarray(a["dtype"]),
             attn_cu_seqlens=a["cu"].numpy(), attn_cu_seqlens_dtype=np.asarray(a["cu_dtype"]), attn_max_seqlen=np.int64(a["max_seqlen"]),
             attn_softmax_scale=np.float64(a["scale"]),
             pool_feat_src_shape=np.asarray(c0["shape"], np.int64), pool_feat_src_dtype=np.asarray(c0["dtype"]),
             pool_feat_reduce=np.asarray(c0["reduce"]), pool_coord_src_shape=np.asarray(c1["shape"], np.int64),
             pool_coord_reduce=np.asarray(c1["reduce"]), pool_indptr=c0["indptr"].numpy(), pool_indptr_dtype=np.asarray(c0["indptr_dtype"]),
             pool_indptr_coord=c1["indptr"].numpy())
    print("wrote g12_ptv3_boundary.npz:", a["shape"], a["dtype"], a["cu"].tolist(), a["max_seqlen"], a["scale"], c0["reduce"], c1["reduce"],
          tuple(c0["shape"]), len(c0["indptr"]))


if __name__ == "__main__":
    main()
