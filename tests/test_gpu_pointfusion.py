"""Scene-level PointFusion on the MI355X: unipre3d_amd.pointfusion against the reference module's own outputs
(tests/golden/g11_point_fusion.npz) and the numpy restatement tests/pointfusion_ref.py, bit for bit."""
import numpy as np
import pytest
import torch

import pointfusion_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = 40


class SparseT:
    """Duck-typed stand-in of spconv's SparseConvTensor (features, indices, spatial_shape, batch_size)."""

    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size


def _np(t):
    return t.detach().cpu().numpy()


def _check_sample(out, ref, coord_np=None):
    assert np.array_equal(_np(out["index"]), ref["index"])
    assert np.array_equal(_np(out["grid_coord"]), ref["grid_coord"])
    assert np.array_equal(_np(out["coord"]), ref["coord"])
    if "inverse" in out:
        assert np.array_equal(_np(out["inverse"]), ref["inverse"])
    assert out["max_count"] == (ref["count"].max() if len(ref["count"]) else 0)


def test_point_fusion_equals_the_reference_module(golden):
    from unipre3d_amd.pointfusion import PointFusion
    g = golden("g11_point_fusion.npz")
    feat = torch.tensor(g["feat_2d_all"], device=DEV, requires_grad=True)
    f3 = SparseT(torch.tensor(g["feat3d_features"], device=DEV), torch.tensor(g["feat3d_indices"], device=DEV),
                 list(g["spatial_shape"]), 1)
    data = {"coord": torch.tensor(g["init_coord"], device=DEV)}
    out = PointFusion(lambda t: t, fea2d_dim=8, viewNum=2)(feat, f3, torch.tensor(g["unprojected_coord"], device=DEV), data,
                                                             grid_size=float(g["grid_size"]), draws=torch.tensor(g["draws"]))
    assert isinstance(out, SparseT)
    assert np.array_equal(_np(out.features), g["out_features"])
    assert np.array_equal(_np(out.indices), g["out_indices"])
    assert np.array_equal(_np(data["coord"]), g["fused_coord"])
    assert np.array_equal(_np(data["grid_coord"]), g["fused_grid_coord"])
    assert np.array_equal(_np(data["batch"]), g["fused_batch"])
    (out.features * torch.tensor(g["cotangent"], device=DEV)).sum().backward()
    assert np.array_equal(_np(feat.grad), g["feat_grad"])


def test_no_surviving_pixel_returns_feat_3d():
    from unipre3d_amd.pointfusion import PointFusion
    uc = torch.zeros(1, 2, 4, 5, 4, device=DEV)            # w == 0 everywhere
    f3 = SparseT(torch.randn(3, 4, device=DEV), torch.zeros(3, 4, dtype=torch.int32, device=DEV), [8, 8, 8], 1)
    data = {"coord": torch.rand(10, 3, device=DEV)}
    assert PointFusion(lambda t: t)(torch.randn(2, 4, 4, 5, device=DEV), f3, uc, data) is f3
    assert set(data) == {"coord"}


def _rand_coord(n, seed, spread=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, generator=g) * spread).float()


def _draws(ref_count, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, max(int(ref_count.max()), 1), len(ref_count)) if len(ref_count) else np.zeros(0, np.int64)


def _check_replayed_draws(n, spread):
    from unipre3d_amd.pointfusion import grid_sample
    c = _rand_coord(n, n, spread)
    vox = R.voxelize(c.numpy(), c.numpy().min(0), 0.02)
    d = _draws(vox["count"], n)
    ref = R.grid_sample(c.numpy(), None, 0.02, d)
    out = grid_sample(c.to(DEV), 0.02, draws=torch.tensor(d), return_inverse=True)
    _check_sample(out, ref)
    return ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4097, 10_007])
def test_grid_sample_sizes_with_replayed_draws(n):
    _check_replayed_draws(n, 0.1)


def test_grid_sample_above_1024_tiles():
    """1024 * 4096 + 1 points = 1025 sort tiles (five trips of the digit scan, the last with one tile; two entries per thread of the
    one-workgroup scan) in about 3.27 M voxels"""
    ref = _check_replayed_draws(1024 * 4096 + 1, 4.0)
    assert 3_000_000 < len(ref["index"]) < 1024 * 4096


def test_grid_sample_edge_cases():
    from unipre3d_amd.pointfusion import grid_sample
    out = grid_sample(torch.zeros(0, 3, device=DEV), return_inverse=True)
    assert out["index"].numel() == 0 and out["inverse"].numel() == 0 and out["max_count"] == 0
    one = torch.full((777, 3), 0.5, device=DEV) + torch.rand(777, 3, device=DEV) * 0.005   # every point in one voxel
    mn = torch.full((3,), 0.5)
    ref = R.grid_sample(_np(one), mn.numpy(), 0.02, np.array([500]))
    out = grid_sample(one, 0.02, min_coord=mn, draws=torch.tensor([500]), return_inverse=True)
    _check_sample(out, ref)
    assert out["index"].numel() == 1 and out["max_count"] == 777


@pytest.mark.parametrize("part", [0, 1, 5])
def test_grid_sample_test_mode_parts(part):
    from unipre3d_amd.pointfusion import grid_sample
    c = _rand_coord(5000, 3, spread=0.3)
    ref = R.grid_sample(c.numpy(), None, 0.02, mode="test", part=part)
    _check_sample(grid_sample(c.to(DEV), 0.02, mode="test", part=part), ref)


def test_ragged_equals_per_set_calls():
    from unipre3d_amd.pointfusion import grid_sample
    sizes = (3000, 0, 1, 5000, 777)
    cs = [_rand_coord(n, 100 + i, spread=0.2 + 0.1 * i) + i for i, n in enumerate(sizes)]
    singles = [grid_sample(c.to(DEV), 0.02, mode="test", part=2, return_inverse=True) for c in cs]
    rag = grid_sample(torch.cat(cs).to(DEV), 0.02, mode="test", part=2, return_inverse=True, sizes=sizes)
    for k in ("index", "coord", "grid_coord", "inverse"):
        assert torch.equal(rag[k], torch.cat([s[k] for s in singles])), k
    assert rag["voxel_sizes"].tolist() == [s["index"].numel() for s in singles]
    torch.manual_seed(5)
    seeded = [grid_sample(c.to(DEV), 0.02) for c in cs[:1]]
    torch.manual_seed(5)
    rs = grid_sample(torch.cat(cs[:2]).to(DEV), 0.02, sizes=sizes[:2])
    assert torch.equal(rs["index"], seeded[0]["index"])


def test_seeded_train_mode():
    from unipre3d_amd.pointfusion import grid_sample
    c = _rand_coord(20_000, 9, spread=0.2)
    vox = R.voxelize(c.numpy(), c.numpy().min(0), 0.02)
    cd = c.to(DEV)
    torch.manual_seed(1)
    a = grid_sample(cd, 0.02)["index"]
    torch.manual_seed(1)
    b = grid_sample(cd, 0.02)["index"]
    torch.manual_seed(2)
    d = grid_sample(cd, 0.02)["index"]
    assert torch.equal(a, b) and not torch.equal(a, d)
    ia = _np(a)
    # every pick lies in its voxel, each voxel picked once
    pos = np.empty(len(c), np.int64)
    pos[vox["order"]] = np.arange(len(c))
    p = pos[ia]
    assert np.all((p >= vox["start"]) & (p < vox["start"] + vox["count"]))
    assert len(np.unique(ia)) == len(ia) == len(vox["count"])


def test_backward_equals_index_select_autograd():
    from unipre3d_amd.pointfusion import pixel_gather
    V, C, H, W = 3, 12, 17, 29
    feat = torch.randn(V, C, H, W, device=DEV, requires_grad=True)
    src = torch.randperm(V * H * W, device=DEV)[:300].to(torch.int32)
    out = pixel_gather(feat, src)
    f2 = feat.detach().clone().requires_grad_(True)
    ref = f2.permute(0, 2, 3, 1).reshape(-1, C).index_select(0, src.long())
    assert torch.equal(out, ref)
    cot = torch.randn_like(out)
    (out * cot).sum().backward()
    (ref * cot).sum().backward()
    assert torch.equal(feat.grad, f2.grad)


@pytest.mark.parametrize("V,H,W", [(8, 120, 160), (8, 480, 640)])
def test_full_shapes_against_the_restatement(V, H, W):
    from unipre3d_amd import synthetic
    from unipre3d_amd.pointfusion import fuse_pixels
    s = synthetic.point_fusion_scene(V, H, W, C=32, seed=1)
    ref_coord, _ = R.filter_pixels(s["unprojected_coord"].numpy(), s["init_coord"].numpy())
    vox = R.voxelize(ref_coord, s["init_coord"].numpy().min(0), 0.02)
    d = _draws(vox["count"], 3)
    ref = R.point_fusion(s["feat_2d_all"].numpy(), s["unprojected_coord"].numpy(), s["init_coord"].numpy(), 0.02, draws=d)
    feat = s["feat_2d_all"].to(DEV).requires_grad_(True)
    out = fuse_pixels(feat, s["unprojected_coord"].to(DEV), s["init_coord"].to(DEV), 0.02, draws=torch.tensor(d))
    assert out["n"] == ref["n"]
    assert np.array_equal(_np(out["src_pixel"]), ref["src_pixel"])
    assert np.array_equal(_np(out["grid_coord"]), ref["grid_coord"])
    assert np.array_equal(_np(out["coord"]), ref["coord"])
    assert np.array_equal(_np(out["feat"]), ref["feat"])
    cot = torch.randn(out["feat"].shape, generator=torch.Generator().manual_seed(0))
    (out["feat"] * cot.to(DEV)).sum().backward()
    assert np.array_equal(_np(feat.grad), R.feat_grad(feat.shape, ref["src_pixel"], cot.numpy()))
