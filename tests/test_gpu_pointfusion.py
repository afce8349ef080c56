"""Scene-level PointFusion on the MI355X: unipre3d_amd.pointfusion against the reference module's own outputs
(tests/golden/g11_point_fusion.npz), pointcept's own GridSample with both origins (tests/golden/g17_grid_sample.npz) and the numpy
restatement tests/pointfusion_ref.py, bit for bit."""
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
    vox = R.voxelize(c.numpy(), None, 0.02)
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
    vox = R.voxelize(c.numpy(), None, 0.02)
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
    assert len(np.unique(_np(out["src_pixel"]))) == out["src_pixel"].numel()   # what pixel_gather's backward requires
    assert np.array_equal(_np(out["grid_coord"]), ref["grid_coord"])
    assert np.array_equal(_np(out["coord"]), ref["coord"])
    assert np.array_equal(_np(out["feat"]), ref["feat"])
    cot = torch.randn(out["feat"].shape, generator=torch.Generator().manual_seed(0))
    (out["feat"] * cot.to(DEV)).sum().backward()
    assert np.array_equal(_np(feat.grad), R.feat_grad(feat.shape, ref["src_pixel"], cot.numpy()))


# ---- pointcept's own GridSample, both origins (G17) ------------------------------------------------------------------------------
G17_DEF = ("shift", "neg", "straddle", "boundary", "fp64", "one", "onevoxel")
G17_CASES = [(n, "def") for n in G17_DEF] + [(n, "exp") for n in G17_DEF + ("range",)]


@pytest.mark.parametrize("name,origin", G17_CASES)
def test_grid_sample_equals_the_reference_class(golden, name, origin):
    """Train mode with the recorded draws, every test-mode part and the inverse of the reference's GridSample, with min_coord=None
    (g - g.min(0)) and with an explicit min_coord; `range`: coordinates at and beyond int64's ends (numpy's x86 conversion)."""
    from unipre3d_amd.pointfusion import grid_sample
    g = golden("g17_grid_sample.npz")
    coord, gs = g[f"{name}_coord"], float(g[f"{name}_grid_size"])
    mn = None if origin == "def" else torch.tensor(g[f"{name}_min_coord"])
    rec = lambda k: g[f"{name}_{origin}_{k}"]
    cd = torch.tensor(coord, device=DEV)
    count = np.bincount(rec("train_inverse"))
    assert len(rec("test_index")) == count.max()
    out = grid_sample(cd, gs, min_coord=mn, draws=torch.tensor(rec("draws")), return_inverse=True)
    _check_sample(out, {"index": rec("train_index"), "grid_coord": rec("train_grid_coord"), "coord": coord[rec("train_index")],
                        "inverse": rec("train_inverse"), "count": count})
    assert out["voxel_sizes"].tolist() == [len(count)]
    for part, (idx, grid) in enumerate(zip(rec("test_index"), rec("test_grid_coord"))):
        out = grid_sample(cd, gs, min_coord=mn, mode="test", part=part, return_inverse=part == 0)
        _check_sample(out, {"index": idx, "grid_coord": grid, "coord": coord[idx], "inverse": rec("test_inverse"), "count": count})


# ---- set-count classes of the radix sort: 0, 1 and 2 set-digit passes (S = 1, 2..256, 257..65536) ---------------------------------
@pytest.mark.parametrize("S", [256, 257, 300])
@pytest.mark.parametrize("explicit", [False, True], ids=["own_min", "min_rows"])
def test_ragged_many_tiny_sets(S, explicit):
    """Tiny sets (0..40 points, the first, the last and others empty): the ragged call equals the per-set calls and the restatement
    run per set, in test mode with the inverse and in train mode with replayed draws."""
    from unipre3d_amd.pointfusion import grid_sample
    rng = np.random.default_rng(S)
    sizes = rng.integers(0, 41, S)
    sizes[[0, 1, S // 2, S - 2, S - 1]] = 0
    sizes[[2, S - 3]] = (1, 40)
    shifts = (rng.random((S, 3)) * 4 - 2).astype(np.float32)
    cs = [(rng.random((n, 3), dtype=np.float32) * np.float32(0.05) + shifts[i]).astype(np.float32) for i, n in enumerate(sizes)]
    mins = (shifts - np.float32(0.007)).astype(np.float32) if explicit else None
    mn = lambda i: None if mins is None else mins[i]
    allc = torch.tensor(np.concatenate(cs), device=DEV)
    assert 2000 < len(allc) < 8000
    tmin = None if mins is None else torch.tensor(mins)
    rag = grid_sample(allc, 0.02, min_coord=tmin, mode="test", part=1, return_inverse=True, sizes=tuple(sizes))
    singles = [grid_sample(torch.tensor(c, device=DEV), 0.02, min_coord=None if mins is None else torch.tensor(mins[i]), mode="test",
                           part=1, return_inverse=True) for i, c in enumerate(cs)]
    refs = [R.grid_sample(c, mn(i), 0.02, mode="test", part=1) if len(c) else None for i, c in enumerate(cs)]
    for k in ("index", "coord", "grid_coord", "inverse"):
        assert torch.equal(rag[k], torch.cat([s[k] for s in singles])), k
        assert np.array_equal(_np(rag[k]), np.concatenate([r[k] for r in refs if r is not None])), k
    voxels = [0 if r is None else len(r["count"]) for r in refs]
    assert rag["voxel_sizes"].tolist() == voxels == [s["index"].numel() for s in singles]
    assert rag["max_count"] == max(r["count"].max() for r in refs if r is not None) > 1
    # train mode, replayed draws (one per voxel, in set order)
    draws = [_draws(r["count"], S + i) if r is not None else np.zeros(0, np.int64) for i, r in enumerate(refs)]
    rag = grid_sample(allc, 0.02, min_coord=tmin, draws=torch.tensor(np.concatenate(draws)), return_inverse=True, sizes=tuple(sizes))
    tr = [R.grid_sample(c, mn(i), 0.02, draws[i]) for i, c in enumerate(cs) if len(c)]
    for k in ("index", "coord", "grid_coord", "inverse"):
        assert np.array_equal(_np(rag[k]), np.concatenate([r[k] for r in tr])), k


# ---- fuse_pixels: the sort sees the survivor count only on the device (meta[0]) while n_max = P tiles are launched ------------------
@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 3 * 4096])
def test_fuse_pixels_survivor_counts(n):
    from unipre3d_amd.pointfusion import fuse_pixels
    V, C, H, W = 1, 4, 96, 128
    P = V * H * W
    assert P == 3 * 4096
    g = torch.Generator().manual_seed(n)
    uc = torch.zeros(1, V, H, W, 4)
    flat = uc.view(-1, 4)
    flat[:, :3] = torch.rand(P, 3, generator=g) * 0.3 + 0.1
    perm = torch.randperm(P, generator=g)
    keep, drop = perm[:n], perm[n:]
    flat[keep, 3] = 1.0
    flat[drop[0::2], 3] = 0.0                 # no depth
    flat[drop[1::2], 3] = 1.0                 # valid, outside the box
    flat[drop[1::2], 0] += 1.0
    init = torch.tensor([[0.1, 0.1, 0.1], [0.4, 0.4, 0.4], [0.2, 0.3, 0.15]])
    feat = torch.randn(V, C, H, W, generator=g)
    ref_coord, _ = R.filter_pixels(uc.numpy(), init.numpy())
    assert len(ref_coord) == n
    fd = feat.to(DEV).requires_grad_(True)
    if n == 0:
        assert R.point_fusion(feat.numpy(), uc.numpy(), init.numpy(), 0.02, draws=np.zeros(0, np.int64)) is None
        assert fuse_pixels(fd, uc.to(DEV), init.to(DEV), 0.02) is None
        return
    d = _draws(R.voxelize(ref_coord, init.numpy().min(0), 0.02)["count"], n)
    ref = R.point_fusion(feat.numpy(), uc.numpy(), init.numpy(), 0.02, draws=d)
    out = fuse_pixels(fd, uc.to(DEV), init.to(DEV), 0.02, draws=torch.tensor(d))
    assert out["n"] == ref["n"] == n
    assert np.array_equal(_np(out["src_pixel"]), ref["src_pixel"])
    assert len(np.unique(_np(out["src_pixel"]))) == out["src_pixel"].numel()
    assert np.array_equal(_np(out["coord"]), ref["coord"])
    assert np.array_equal(_np(out["grid_coord"]), ref["grid_coord"])
    assert np.array_equal(_np(out["feat"]), ref["feat"])
    cot = torch.randn(out["feat"].shape, generator=torch.Generator().manual_seed(0))
    (out["feat"] * cot.to(DEV)).sum().backward()
    assert np.array_equal(_np(fd.grad), R.feat_grad(feat.shape, ref["src_pixel"], cot.numpy()))


# ---- the seeded device draw, pinned to its documented formula ---------------------------------------------------------------------
def _mix64(z):
    """splitmix64's finaliser in uint64 (include/unipre3d_pointfusion.h: the counter-based hash of the seeded draw)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def test_mix64_restatement_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 (state += golden gamma, then the finaliser): Vigna's reference values
    assert int(_mix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(_mix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4


def test_seeded_draw_follows_its_formula():
    """r = mix64(seed ^ mix64(voxel rank IN ITS SET)) % max(THE SET's largest count, 1), pick = start + r % count, the seed taken
    from torch's CPU generator; three sets whose largest counts differ, so a global rank or a global maximum gives other picks."""
    from unipre3d_amd.pointfusion import grid_sample
    sizes = (800, 1500, 300)
    cs = [_rand_coord(800, 31, 0.5).numpy() - 0.2, _rand_coord(1500, 32, 0.06).numpy() + 1.0, _rand_coord(300, 33, 0.004).numpy() + 0.501]
    gen = torch.Generator().manual_seed(77)
    twin = torch.Generator()
    twin.set_state(gen.get_state())
    seed = np.uint64(int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=twin).item()))
    out = grid_sample(torch.tensor(np.concatenate(cs), device=DEV), 0.02, sizes=sizes, generator=gen)
    voxs = [R.voxelize(c, None, 0.02) for c in cs]
    maxes = [int(v["count"].max()) for v in voxs]
    assert len(set(maxes)) == 3 and maxes[2] == 300, maxes

    def picks(rank_base, modulus):
        res, base = [], 0
        for v, mx in zip(voxs, maxes):
            rank = np.arange(len(v["count"]), dtype=np.uint64) + np.uint64(base if rank_base == "global" else 0)
            r = _mix64(seed ^ _mix64(rank)) % np.uint64(max(mx if modulus == "set" else max(maxes), 1))
            res.append(v["order"][v["start"] + (r % v["count"].astype(np.uint64)).astype(np.int64)])
            base += len(v["count"])
        return np.concatenate(res)

    want = picks("set", "set")
    assert not np.array_equal(want, picks("global", "set")) and not np.array_equal(want, picks("set", "global"))
    assert np.array_equal(_np(out["index"]), want)
    assert out["voxel_sizes"].tolist() == [len(v["count"]) for v in voxs]


# ---- the gather kernels at their loop edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,C,H,W,M", [
    (3, 21846, 1, 7, 13),     # V * C = 65538 planes: more than the backward's 65535 grid rows, the plane-stride loop
    (2, 1, 5, 9, 37),         # one channel
    (5, 3, 1, 1, 4),          # one pixel per view
    (2, 6, 4, 5, 0),          # no voxel: an all-zero gradient
    (2, 7, 9, 11, 37),        # M * C = 259: the forward's last workgroup is partial
    (1, 256, 3, 3, 9),        # M * C a multiple of 256, every pixel picked
])
def test_pixel_gather_loop_edges(V, C, H, W, M):
    """Forward and backward against index_select's autograd; unique pixels, as pixel_gather requires."""
    from unipre3d_amd.pointfusion import pixel_gather
    g = torch.Generator().manual_seed(V * C + M)
    feat = torch.randn(V, C, H, W, generator=g).to(DEV).requires_grad_(True)
    src = torch.randperm(V * H * W, generator=g)[:M].to(DEV).to(torch.int32)
    assert src.unique().numel() == M
    out = pixel_gather(feat, src)
    f2 = feat.detach().clone().requires_grad_(True)
    ref = f2.permute(0, 2, 3, 1).reshape(-1, C).index_select(0, src.long())
    assert out.shape == ref.shape == (M, C) and torch.equal(out, ref)
    cot = torch.randn(M, C, generator=g).to(DEV)
    (out * cot).sum().backward()
    (ref * cot).sum().backward()
    assert torch.equal(feat.grad, f2.grad)
