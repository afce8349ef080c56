#!/usr/bin/env python3
"""Generates tests/golden/g11_point_fusion.npz: the reference's OWN scene-level PointFusion (fusion/point_fusion.py) with
pointcept's GridSample (pointcept/datasets/transform_with_extrinsic.py:1179-1326) run on the CPU, for unipre3d_amd/pointfusion.py.

Stubs: torchvision, spconv.pytorch.SparseConvTensor (a recording class), pointcept.utils.registry, openpoints' subsample; the
module's torch.zeros / torch.tensor calls have their device="cuda" dropped.  np.random.randint is recorded (the train-mode draw, one
int per voxel) and np.argsort forced to kind="stable" (the pinned within-voxel order: ascending point index).  grid_size is passed
as np.float32(0.02) so that numpy >= 2 divides in fp32 as the reference's numpy 1.26 does with a 0-d float64 divisor.

Scene: 2 views of 24 x 32 pixels, C = 8, depth maps of a room with boxes (unipre3d_amd.synthetic.point_fusion_scene, narrow field of
view so that neighbouring pixels share 2 cm voxels), with invalid
pixels (w = 0), NaN validity flags (valid: torch's .bool()), pixels outside init_coord's box, pixels placed exactly on fp32 voxel
boundaries, and pixels whose fp32 grid coordinate differs from the fp64 one (`fp64_rows`: their flat pixel indices).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
GS = 0.02


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class SparseConvTensor:
    made = []

    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size
        SparseConvTensor.made.append(self)


class _Registry:
    def __init__(self, *a, **k):
        pass

    def register_module(self, *a, **k):
        return (lambda c: c) if not a or not isinstance(a[0], type) else a[0]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _reference_modules():
    _stub("torchvision", transforms=types.SimpleNamespace())
    _stub("spconv"); _stub("spconv.pytorch", SparseConvTensor=SparseConvTensor)
    sys.modules["spconv"].pytorch = sys.modules["spconv.pytorch"]
    for n in ("pointcept", "pointcept.utils", "pointcept.datasets"):
        _stub(n)
    _stub("pointcept.utils.registry", Registry=_Registry)
    for n in ("openpoints", "openpoints.models", "openpoints.models.layers"):
        _stub(n)
    _stub("openpoints.models.layers.subsample", furthest_point_sample=None)
    _load("pointcept.datasets.transform_with_extrinsic", os.path.join(REF, "pointcept/datasets/transform_with_extrinsic.py"))
    return _load("ref_point_fusion", os.path.join(REF, "fusion/point_fusion.py"))


def _fp64_disagreeing(m, lo, hi, want=6):
    """fp32 coordinates x in [lo, hi] whose grid coordinate floor(fp32(x - m) / 0.02) differs between fp32 and fp64 division."""
    out = []
    for k in range(1, 400):
        x0 = np.float32(m + np.float32(k * GS))
        for u in range(-4, 5):
            x = np.float32(x0 + u * np.spacing(x0))
            if not lo <= x <= hi:
                continue
            d = np.float32(x - np.float32(m))
            if np.floor(d / np.float32(GS)) != np.floor(np.float64(d) / GS):
                out.append(x)
                break
        if len(out) >= want:
            break
    return out


def scene():
    from unipre3d_amd import synthetic
    s = synthetic.point_fusion_scene(V=2, H=24, W=32, C=8, seed=11, n_init=256, hole_rate=0.08, focal_scale=6.0)
    uc = s["unprojected_coord"].clone()
    flat = uc.view(-1, 4)
    init = s["init_coord"]
    lo, hi = init.min(0).values, init.max(0).values
    g = torch.Generator().manual_seed(3)
    inside = torch.nonzero((flat[:, 3] != 0) & torch.all((flat[:, :3] >= lo) & (flat[:, :3] <= hi), 1)).view(-1)
    perm = inside[torch.randperm(inside.numel(), generator=g)]
    flat[perm[:5], 3] = float("nan")                     # NaN validity: kept by .bool()
    # exactly on fp32 voxel boundaries: x = fp32(min + fp32(k * 0.02)) on every axis
    for j, p in enumerate(perm[5:17].tolist()):
        for a in range(3):
            k = int((flat[p, a] - lo[a]) / GS)
            flat[p, a] = float(np.float32(lo[a].item() + np.float32(k * GS)))
    # fp32 and fp64 division disagree on the x axis of these rows
    xs = _fp64_disagreeing(lo[0].item(), lo[0].item(), hi[0].item())
    fp64_rows = perm[17:17 + len(xs)]
    for p, x in zip(fp64_rows.tolist(), xs):
        flat[p, 0] = float(x)
    # the box's own faces (inclusive) and just outside them
    flat[perm[30], :3] = lo
    flat[perm[31], :3] = hi
    flat[perm[32], 0] = float(np.nextafter(np.float32(hi[0].item()), np.float32(np.inf)))
    flat[perm[33], 2] = float(np.nextafter(np.float32(lo[2].item()), np.float32(-np.inf)))
    return s["feat_2d_all"], uc, init, fp64_rows.numpy().astype(np.int64)


def main():
    pf = _reference_modules()
    feat, uc, init, fp64_rows = scene()
    V, C, H, W = feat.shape
    feat = feat.clone().requires_grad_(True)
    K = 40
    feat3d_features = torch.randn(K, C, generator=torch.Generator().manual_seed(4))
    feat3d_indices = torch.cat([torch.zeros(K, 1, dtype=torch.int32), torch.randint(0, 50, (K, 3), dtype=torch.int32,
                                                                                      generator=torch.Generator().manual_seed(5))], 1)
    feat_3d = SparseConvTensor(feat3d_features, feat3d_indices, [64, 64, 64], 1)

    draws = []
    orig = (np.random.randint, np.argsort, torch.zeros, torch.tensor)

    def randint(*a, **k):
        r = orig[0](*a, **k)
        draws.append(np.array(r))
        return r

    np.random.randint = randint
    np.argsort = lambda a, *x, **k: orig[1](a, kind="stable")
    torch.zeros = lambda *a, **k: orig[2](*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
    torch.tensor = lambda *a, **k: orig[3](*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
    np.random.seed(7)
    try:
        module = pf.PointFusion(lambda t: t, fea2d_dim=C, viewNum=V)
        data = {"coord": init.clone()}
        out = module(feat, feat_3d, uc, data, grid_size=np.float32(GS))
    finally:
        np.random.randint, np.argsort, torch.zeros, torch.tensor = orig
    assert len(draws) == 1, len(draws)
    cot = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(6))
    (out.features * cot).sum().backward()
    M = out.features.shape[0] - K
    np.savez_compressed(
        os.path.join(OUT, "g11_point_fusion.npz"),
        feat_2d_all=feat.detach().numpy(), unprojected_coord=uc.numpy(), init_coord=init.numpy(), grid_size=np.float32(GS),
        feat3d_features=feat3d_features.numpy(), feat3d_indices=feat3d_indices.numpy(), spatial_shape=np.array([64, 64, 64]),
        draws=draws[0].astype(np.int64), fp64_rows=fp64_rows,
        out_features=out.features.detach().numpy(), out_indices=out.indices.numpy(),
        fused_coord=data["coord"].numpy(), fused_batch=data["batch"].numpy(), fused_grid_coord=data["grid_coord"].numpy(),
        cotangent=cot.numpy(), feat_grad=feat.grad.numpy())
    print(f"g11: {V} views {H}x{W}, C={C}, {M} voxels, draws max {draws[0].max()}")


if __name__ == "__main__":
    main()
