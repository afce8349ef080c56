"""Scene-level PointFusion, host side: the numpy restatement tests/pointfusion_ref.py against golden vectors produced by
the reference's OWN fusion/point_fusion.py + pointcept GridSample (tests/golden/g11_point_fusion.npz, make_g11_point_fusion.py), the
fp32-division pin, pointcept's GridSample on its own with both origins (tests/golden/g17_grid_sample.npz, make_g17_grid_sample.py),
and the C-ABI of libunipre3d_pointfusion.so (loads without a GPU; no compute calls here)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pointfusion_ref as R
from conftest import ROOT

K = 40   # points of the recorded feat_3d in G11


@pytest.fixture(scope="module")
def g11(golden):
    return golden("g11_point_fusion.npz")


@pytest.fixture(scope="module")
def fused(g11):
    return R.point_fusion(g11["feat_2d_all"], g11["unprojected_coord"], g11["init_coord"], float(g11["grid_size"]), draws=g11["draws"])


def test_restatement_reproduces_the_reference_module(g11, fused):
    """Features, sparse indices, init_3d_data and the voxel picks of the reference module, bit for bit."""
    M = len(fused["count"])
    assert len(g11["draws"]) == M and g11["draws"].min() >= 0 and g11["draws"].max() < fused["count"].max()
    assert np.array_equal(g11["out_features"], np.concatenate([g11["feat3d_features"], fused["feat"]]))
    idx = np.concatenate([np.zeros((M, 1), np.int32), fused["grid_coord"].astype(np.int32)], 1)
    assert np.array_equal(g11["out_indices"], np.concatenate([g11["feat3d_indices"], idx]))
    assert np.array_equal(g11["fused_coord"], np.concatenate([g11["init_coord"], fused["coord"]]))
    assert np.array_equal(g11["fused_grid_coord"], g11["out_indices"][:, 1:])
    assert np.array_equal(g11["fused_batch"], g11["out_indices"][:, 0])


def test_restatement_gradient_matches_the_reference(g11, fused):
    grad = R.feat_grad(g11["feat_2d_all"].shape, fused["src_pixel"], g11["cotangent"][K:])
    assert np.array_equal(grad, g11["feat_grad"])


def test_voxel_order_keys_and_counts(g11):
    """Voxels by ascending 64-bit key, points inside a voxel by ascending index, counts covering every filtered point once."""
    coord, pix = R.filter_pixels(g11["unprojected_coord"], g11["init_coord"])
    vox = R.voxelize(coord, g11["init_coord"].min(0), float(g11["grid_size"]))
    keys = vox["key"][vox["order"]]
    heads = vox["start"]
    assert np.all(np.diff(keys[heads].astype(np.uint64)) > 0)
    assert vox["count"].sum() == len(coord) and np.all(vox["count"] >= 1)
    for s, c in zip(heads, vox["count"]):
        seg = vox["order"][s:s + c]
        assert np.all(np.diff(seg) > 0) and np.all(keys[s:s + c] == keys[s])
    assert np.array_equal(vox["inverse"][vox["order"]], np.repeat(np.arange(len(heads)), vox["count"]))
    assert vox["count"].max() > 8, "G11 should have voxels shared by many pixels"


def test_filters_keep_nan_validity_and_inclusive_box(g11):
    uc = g11["unprojected_coord"][0].reshape(-1, 4)
    coord, pix = R.filter_pixels(g11["unprojected_coord"], g11["init_coord"])
    nan_pix = np.nonzero(np.isnan(uc[:, 3]))[0]
    assert len(nan_pix) > 0 and np.isin(nan_pix, pix).all()
    assert (uc[:, 3] == 0).sum() > 0 and not np.isin(np.nonzero(uc[:, 3] == 0)[0], pix).any()
    lo, hi = g11["init_coord"].min(0), g11["init_coord"].max(0)
    on_face = np.nonzero(np.all(uc[:, :3] == lo, 1) | np.all(uc[:, :3] == hi, 1))[0]
    assert len(on_face) >= 2 and np.isin(on_face, pix).all()
    outside = np.nonzero((uc[:, 3] != 0) & ~np.all((uc[:, :3] >= lo) & (uc[:, :3] <= hi), 1))[0]
    assert len(outside) > 0 and not np.isin(outside, pix).any()


def test_fp32_division_pin_matters(g11):
    """The rows placed where fp32 and fp64 division disagree: the reference (numpy 1.26, fp32) follows the fp32 restatement."""
    rows = g11["fp64_rows"]
    assert len(rows) >= 3
    coord, pix = R.filter_pixels(g11["unprojected_coord"], g11["init_coord"])
    m = g11["init_coord"].min(0)
    sel = np.searchsorted(pix, rows)
    assert np.array_equal(pix[sel], rows)
    g32 = R.grid_coords(coord[sel], m, float(g11["grid_size"]))
    g64 = R.grid_coords(coord[sel], m, 0.02, fp64=True)   # numpy >= 2 with the python float 0.02
    assert np.all(g32[:, 0] != g64[:, 0])
    # and the reference's outputs hold the fp32 cells: each row's cell is among the voxels it produced
    cells = {tuple(r) for r in g11["out_indices"][K:, 1:]}
    assert all(tuple(r) in cells for r in g32)


def test_fnv_is_multiply_then_xor():
    g = np.array([[1, 2, 3], [0, 0, 0]], np.int64)
    h = 0xCBF29CE484222325
    for a in (1, 2, 3):
        h = ((h * 0x100000001B3) % (1 << 64)) ^ a
    assert int(R.fnv_keys(g)[0]) == h
    assert int(R.fnv_keys(g)[1]) != 0xCBF29CE484222325


# ---- GridSample on its own: both origins, both modes (G17) -----------------------------------------------------------------------
G17_DEF = ("shift", "neg", "straddle", "boundary", "fp64", "one", "onevoxel")
G17_EXP = G17_DEF + ("range",)


@pytest.fixture(scope="module")
def g17(golden):
    g = golden("g17_grid_sample.npz")
    assert tuple(g["names_def"]) == G17_DEF and tuple(g["names"]) == G17_EXP
    return g


def _g17_restatement_equals_the_record(g, name, origin):
    coord, gs = g[f"{name}_coord"], g[f"{name}_grid_size"]
    mn = None if origin == "def" else g[f"{name}_min_coord"]
    rec = lambda k: g[f"{name}_{origin}_{k}"]
    tr = R.grid_sample(coord, mn, gs, draws=rec("draws"))
    assert len(rec("draws")) == len(tr["count"]) and rec("draws").max() < tr["count"].max()
    assert np.array_equal(tr["index"], rec("train_index"))
    assert np.array_equal(tr["grid_coord"], rec("train_grid_coord"))
    assert np.array_equal(tr["inverse"], rec("train_inverse"))
    assert len(rec("test_index")) == tr["count"].max()          # one part per i < count.max()
    for part, (idx, grid) in enumerate(zip(rec("test_index"), rec("test_grid_coord"))):
        te = R.grid_sample(coord, mn, gs, mode="test", part=part)
        assert np.array_equal(te["index"], idx), part
        assert np.array_equal(te["grid_coord"], grid), part
        assert np.array_equal(te["inverse"], rec("test_inverse"))


@pytest.mark.parametrize("name", G17_DEF)
def test_restatement_reproduces_grid_sample_default_origin(g17, name):
    """min_coord=None: g = floor(coord / gs), grid = g - g.min(0); every recorded output of the reference's class, bit for bit."""
    _g17_restatement_equals_the_record(g17, name, "def")


@pytest.mark.parametrize("name", G17_EXP)
def test_restatement_reproduces_grid_sample_explicit_origin(g17, name):
    """min_coord given: grid = floor((coord - min_coord) / gs); `range` holds the coordinates at and beyond int64's ends."""
    _g17_restatement_equals_the_record(g17, name, "exp")


def test_g17_reaches_where_origins_and_precisions_part(g17):
    """The fixture's clouds do what they are there for (else the tests above could pass on a wrong origin or precision)."""
    gs = np.float32(0.02)
    for name in ("shift", "neg", "boundary"):        # anchoring the cells at coord.min(0) gives other voxels than the default origin
        c = g17[f"{name}_coord"]
        assert len(R.voxelize(c, c.min(0), gs)["count"]) != len(g17[f"{name}_def_draws"]), name
    c = g17["straddle_coord"]
    assert np.all(c.min(0) < 0) and np.all(c.max(0) > 0) and np.all(g17["neg_coord"] < 0)
    c, m = g17["boundary_coord"], g17["boundary_min_coord"]
    k = np.arange(-40, 40)
    on_abs = np.isin(c, (k * gs).astype(np.float32)).all(1)
    on_min = np.stack([np.isin(c[:, a], (m[a] + (k * gs).astype(np.float32)).astype(np.float32)) for a in range(3)], 1).all(1)
    assert on_abs.sum() >= 100 and on_min.sum() >= 100
    c, m = g17["fp64_coord"], g17["fp64_min_coord"]
    rd, re = g17["fp64_def_rows"], g17["fp64_exp_rows"]
    assert len(rd) >= 4 and len(re) >= 4
    assert np.all(np.floor(c[rd, 0] / gs) != np.floor(c[rd, 0].astype(np.float64) / 0.02))
    assert np.all(R.grid_coords(c[re], m, gs)[:, 1] != R.grid_coords(c[re], m, 0.02, fp64=True)[:, 1])
    assert len(g17["one_coord"]) == 1 and len(g17["onevoxel_def_draws"]) == len(g17["onevoxel_exp_draws"]) == 1
    c = g17["range_coord"]
    big = np.float32(2.0 ** 63 - 2.0 ** 39)
    for v in (np.inf, -np.inf, np.float32(3e30), big, -big, np.float32(2.0 ** 63), np.float32(-2.0 ** 63)):
        assert (c == v).any(), v
    assert not np.isnan(c).any()
    grid = g17["range_exp_train_grid_coord"]                 # numpy on x86: exact where the floor fits int64, INT64_MIN elsewhere
    assert (grid == 2 ** 63 - 2 ** 39).any() and (grid == -(2 ** 63 - 2 ** 39)).any() and (grid == -2 ** 63).any()


@pytest.mark.parametrize("name", G17_DEF)
def test_minimum_of_the_floors_is_the_floor_of_the_minimum(g17, name):
    """What the kernel's default origin rests on: floor and the fp32 division by a positive grid size are monotone, so (without NaN)
    g.min(0) == floor(fp32(coord.min(0) / gs)) and the per-set minimum already reduced on the device is all the origin needs."""
    c, gs = g17[f"{name}_coord"], g17[f"{name}_grid_size"]
    g = np.floor(c / gs).astype(np.int64)
    assert (c / gs).dtype == np.float32
    assert np.array_equal(g.min(0), np.floor(c.min(0) / gs).astype(np.int64))
    assert np.array_equal(R.grid_coords(c, None, gs), g - np.floor(c.min(0) / gs).astype(np.int64))


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def _declared():
    hdr = open(os.path.join(ROOT, "include", "unipre3d_pointfusion.h")).read()
    abi = int(re.search(r"#define U3D_POINTFUSION_ABI_VERSION (\d+)", hdr).group(1))
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(u3d_[a-z_0-9]+)\s*\(", hdr))), abi


def test_header_parses_and_every_symbol_is_exported():
    from unipre3d_amd import pointfusion
    names, abi = _declared()
    assert set(names) == set(pointfusion.EXPORTS)
    lib = pointfusion.load()
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.u3d_pointfusion_abi_version() == abi == pointfusion.ABI_VERSION


def test_scratch_query_and_argument_errors_without_the_device():
    from unipre3d_amd import pointfusion
    lib = pointfusion.load()
    b1, b2 = lib.u3d_pointfusion_scratch_bytes(1000, 1), lib.u3d_pointfusion_scratch_bytes(2_457_600, 1)
    assert 0 < b1 < b2 and b2 >= 2_457_600 * 32
    assert lib.u3d_pointfusion_scratch_bytes(-1, 1) == 0 and lib.u3d_pointfusion_scratch_bytes(10, 0) == 0
    null = None
    assert lib.u3d_pointfusion_minmax(-1, 1, null, null, null, null) == 1
    assert lib.u3d_pointfusion_compact(10, null, null, null, null, null, null, null) == 1
    assert lib.u3d_pointfusion_voxelize(10, 5, 1, null, null, null, 3, 0, ctypes.c_float(0.02), null, null, null, null) == 1
    assert lib.u3d_pointfusion_pick(5, 10, 1, null, null, null, null, 3, 0, ctypes.c_float(0.02), 2, 0, null, 0, null, null, null, null,
                                    null, null, null) == 1
    dummy = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)   # never read: the origin mode is refused first
    assert lib.u3d_pointfusion_voxelize(0, 0, 1, null, null, null, 3, 2, ctypes.c_float(0.02), dummy, dummy, dummy, null) == 1
    assert lib.u3d_pointfusion_pick(0, 0, 1, null, null, null, null, 3, -1, ctypes.c_float(0.02), 0, 0, null, 0, null, null, null, null,
                                    null, null, null) == 1
    assert lib.u3d_pointfusion_gather_forward(0, 8, 16, null, null, null, null) == 0   # empty: nothing to do


def test_product_path_refuses_cpu_tensors():
    import torch
    from unipre3d_amd import pointfusion
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointfusion.grid_sample(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointfusion.PointFusion(lambda t: t)(torch.zeros(1, 2, 3, 4), None, torch.zeros(1, 1, 3, 4, 4), {"coord": torch.zeros(3, 3)})
