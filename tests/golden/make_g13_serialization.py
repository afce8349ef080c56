#!/usr/bin/env python3
"""Generates tests/golden/g13_serialization.npz: what the reference's OWN index plumbing computes on the CPU, for
unipre3d_amd/serialization.py: pointcept/models/utils/serialization (encode), Point.serialization (structure.py) and PTv3's
SerializedAttention.get_padding_and_inverse and SerializedPooling.forward (point_transformer_v3m1_base.py), loaded with the stubs
of make_g12_ptv3_boundary.py.  Only recorded data is stored (inputs and integer results).

  enc{d}_coord / _batch / _code   depth d in 1, 2, 3, 10, 16: 160 points with batch ids 0 .. 2, the corners 0 and 2^d - 1 among them
                                  (depth 16 with batch 2 is a 50-bit code); code (4, N) in the order z, z-trans, hilbert, hilbert-trans
  ser_*                           Point.serialization of 340 distinct sites in items of 17, 96, 130, 97 (adaptive depth, four orders)
  pad{a,b}_*                      get_padding_and_inverse at patch 48 for items (17, 96, 130, 97) and (1, 48, 49, 95)
  pool_*                          SerializedPooling at stride 2 on the ser_ points: cluster, indices, idx_ptr, head_indices and the
                                  pooled code / order / inverse
The reference's plain argsorts are recorded only where the codes are distinct.  Its torch.sort(cluster) has ties by construction and
is NOT the stable sort on the CPU at this size, see main(): pool_indices / pool_head_indices hold its result with each cluster's
points in ascending index, pool_indices_ref / pool_head_indices_ref the result as it came out.
"""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_g12_ptv3_boundary as g12  # noqa: E402

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
SIZES_A, SIZES_B, PATCH, C = (17, 96, 130, 97), (1, 48, 49, 95), 48, 8


def load_reference():
    _stub, _load = g12._stub, g12._load
    _stub("addict", Dict=g12.Dict)
    _stub("flash_attn", flash_attn_varlen_qkvpacked_func=g12._flash)
    _stub("torch_scatter", segment_csr=g12._segment_csr)
    sp = _stub("spconv")
    sp.pytorch = _stub("spconv.pytorch", SparseConvTensor=g12.SparseConvTensor, SparseModule=torch.nn.Module,
                       modules=types.SimpleNamespace(is_spconv_module=lambda m: False))
    _stub("timm")
    _stub("timm.models")
    _stub("timm.models.layers", DropPath=torch.nn.Identity)
    _stub("fusion")
    _stub("fusion.point_fusion", PointFusion=object)
    _stub("pointcept")
    _stub("pointcept.models")
    _stub("pointcept.models.point_prompt_training", PDNorm=object)
    _stub("pointcept.models.builder", MODELS=g12._Registry())
    utils = _stub("pointcept.models.utils")
    misc = _load("pointcept.models.utils.misc", "pointcept/models/utils/misc.py")
    for n in ("offset2batch", "offset2bincount", "batch2offset"):
        setattr(utils, n, getattr(misc, n))
    sdir = os.path.join(g12.REF, "pointcept/models/utils/serialization")
    pk = _stub("pointcept.models.utils.serialization")
    pk.__path__ = [sdir]
    for f in sorted(os.listdir(sdir)):
        if f.endswith(".py") and f != "__init__.py":
            _load("pointcept.models.utils.serialization." + f[:-3], "pointcept/models/utils/serialization/" + f)
    ser = _load("pointcept.models.utils.serialization", "pointcept/models/utils/serialization/__init__.py")
    utils.encode, utils.decode = ser.encode, ser.decode
    _load("pointcept.models.utils.structure", "pointcept/models/utils/structure.py")
    _load("pointcept.models.modules", "pointcept/models/modules.py")
    ptv3 = _load("ptv3_ref", "pointcept/models/point_transformer_v3/point_transformer_v3m1_base.py")
    return ser, ptv3


def main():
    ser, ptv3 = load_reference()
    g = torch.Generator().manual_seed(13)
    out = {"orders": np.asarray(ORDERS), "patch_size": np.int64(PATCH)}

    for d in (1, 2, 3, 10, 16):
        n, top = 160, (1 << d) - 1
        coord = torch.randint(0, top + 1, (n, 3), generator=g, dtype=torch.int64)
        batch = torch.randint(0, 3, (n,), generator=g, dtype=torch.int64)
        coord[0], coord[1], coord[2], coord[3] = 0, top, torch.tensor([top, 0, 0]), torch.tensor([0, 0, top])
        batch[0], batch[1], batch[2], batch[3] = 0, 2, 1, 2
        code = torch.stack([ser.encode(coord, batch, d, order=o) for o in ORDERS])
        assert code.dtype == torch.int64 and int(code.min()) >= 0
        if d == 16:
            assert int(code.max()).bit_length() == 50
        out[f"enc{d}_coord"], out[f"enc{d}_batch"], out[f"enc{d}_code"] = coord.int().numpy(), batch.numpy(), code.numpy()

    # Point.serialization on distinct sites (a plain argsort is then unambiguous)
    N = sum(SIZES_A)
    cells = torch.randperm(12 ** 3, generator=g)[:N]
    grid = torch.stack([cells // 144, cells // 12 % 12, cells % 12], 1) + torch.tensor([3, 0, 7])
    coord = grid.float() * 0.05
    coord[:, 0] = torch.arange(N)                     # segment_csr's second source is coord[indices]: column 0 records `indices`
    point = ptv3.Point(g12.Dict(coord=coord, grid_coord=grid, feat=torch.randn(N, C, generator=g),
                                offset=torch.cumsum(torch.tensor(SIZES_A), 0)))
    point.serialization(order=ORDERS, shuffle_orders=False)
    code = point.serialized_code
    assert all(len(torch.unique(r)) == N for r in code)
    out.update(ser_grid_coord=grid.int().numpy(), ser_batch=point.batch.numpy(), ser_offset=point.offset.numpy(),
               ser_depth=np.int64(point.serialized_depth), ser_code=code.numpy(), ser_order=point.serialized_order.numpy(),
               ser_inverse=point.serialized_inverse.numpy())

    attn = ptv3.SerializedAttention(channels=C, num_heads=1, patch_size=PATCH, order_index=0, enable_rpe=False, enable_flash=True,
                                    upcast_attention=False, upcast_softmax=False).eval()
    for tag, sizes in (("pada", SIZES_A), ("padb", SIZES_B)):
        pad, unpad, cu = attn.get_padding_and_inverse(g12.Dict(offset=torch.cumsum(torch.tensor(sizes), 0)))
        assert pad.dtype == torch.int64 and unpad.dtype == torch.int64 and cu.dtype == torch.int32
        out.update({f"{tag}_sizes": np.asarray(sizes, np.int64), f"{tag}_pad": pad.numpy(), f"{tag}_unpad": unpad.numpy(),
                    f"{tag}_cu_seqlens": cu.numpy()})

    # segment_csr stub that keeps its sources: `indices` is column 0 of the second (mean) source, coord[indices]
    seen = {}

    def _csr(src, indptr, out=None, reduce="sum"):
        seen[reduce] = (src.clone(), indptr.clone())
        return torch.zeros(indptr.numel() - 1, src.shape[1], dtype=src.dtype)

    ptv3.torch_scatter.segment_csr = _csr
    pool = ptv3.SerializedPooling(C, 2 * C, stride=2, norm_layer=None, act_layer=None, reduce="max", shuffle_orders=False)
    pool.norm = pool.act = None
    down = pool(point)
    cluster, idx_ptr = down.pooling_inverse, seen["max"][1]
    assert torch.equal(seen["mean"][1], idx_ptr)
    indices_ref = seen["mean"][0][:, 0].long()
    head_ref = indices_ref[idx_ptr[:-1]]
    # torch.sort(cluster) without stable=True leaves the order INSIDE a cluster unspecified, and on the CPU it is not the stable one at
    # this size (it is from about 1e5 elements up).  What the reference relies on holds for any such order and is asserted: `indices`
    # sorts the clusters, and each segment holds exactly its cluster's points.  pool_indices / pool_head_indices are the reference's
    # values with every segment put in ascending point index (the stable rule); the values as they came out are kept as *_ref.
    assert torch.equal(cluster[indices_ref], torch.repeat_interleave(torch.arange(len(idx_ptr) - 1), idx_ptr[1:] - idx_ptr[:-1]))
    assert torch.equal(torch.sort(indices_ref)[0], torch.arange(N))
    indices = torch.cat([torch.sort(indices_ref[a:b])[0] for a, b in zip(idx_ptr[:-1].tolist(), idx_ptr[1:].tolist())])
    print("reference torch.sort(cluster) equals the stable sort here:", torch.equal(indices_ref, indices))
    head = indices[idx_ptr[:-1]]
    assert torch.equal(cluster[head], cluster[head_ref])
    assert torch.equal(down.grid_coord, grid[head] >> 1) and torch.equal(down.batch, point.batch[head])
    pcode = down.serialized_code
    assert all(len(torch.unique(r)) == pcode.shape[1] for r in pcode) and pcode.shape[1] < N
    out.update(pool_depth=np.int64(1), pool_cluster=cluster.numpy(), pool_indices=indices.numpy(), pool_idx_ptr=idx_ptr.numpy(),
               pool_head_indices=head.numpy(), pool_indices_ref=indices_ref.numpy(), pool_head_indices_ref=head_ref.numpy(), pool_code=pcode.numpy(), pool_order=down.serialized_order.numpy(),
               pool_inverse=down.serialized_inverse.numpy())

    path = os.path.join(OUT, "g13_serialization.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; depth", int(point.serialized_depth), "clusters", pcode.shape[1])


if __name__ == "__main__":
    main()
