"""numpy restatement of scene-level PointFusion (fusion/point_fusion.py:35-190 with pointcept's GridSample, mode "train" / "test",
hash_type "fnv") in explicit fp32 with a stable argsort: the checker of unipre3d_amd/pointfusion.py and its CPU baseline.

The reference's own arithmetic under its pinned numpy 1.26: `fp32 coord - fp32 min_coord` stays fp32 and `/ np.array(grid_size)`
stays fp32 too (value-based casting of the 0-d divisor), so the division is ONE correctly rounded fp32 division.  numpy >= 2 would
promote it to fp64; `grid_coords(..., fp64=True)` is that promotion, kept to show that the pin matters."""
from __future__ import annotations

import numpy as np

FNV_OFFSET = np.uint64(0xCBF29CE484222325)
FNV_PRIME = np.uint64(0x100000001B3)


def grid_coords(coord, min_coord, grid_size=0.02, fp64=False):
    """The reference's two origins: an explicit min_coord gives floor((coord - min_coord) / gs); min_coord=None gives
    g = floor(coord / gs), grid = g - g.min(0) (the cells are those of the absolute grid, NOT the ones anchored at coord.min(0))."""
    coord = np.asarray(coord, np.float32)
    d = coord if min_coord is None else coord - np.asarray(min_coord, np.float32).reshape(1, 3)
    q = d.astype(np.float64) / np.float64(grid_size) if fp64 else d / np.float32(grid_size)
    with np.errstate(invalid="ignore"):     # out of int64's range: the x86 conversion, INT64_MIN
        g = np.floor(q).astype(np.int64)
    if min_coord is None and len(g):
        g -= g.min(0)
    return g


def fnv_keys(grid):
    """The reference's loop: h = offset; per axis h *= prime, then h ^= axis (mod 2^64)."""
    arr = np.asarray(grid, np.int64).astype(np.uint64)
    h = np.full(arr.shape[0], FNV_OFFSET, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(arr.shape[1]):
            h = h * FNV_PRIME
            h = np.bitwise_xor(h, arr[:, j])
    return h


def voxelize(coord, min_coord, grid_size=0.02):
    """min_coord: (3,) or None (the default origin of grid_coords).
    -> dict grid (N,3), key (N,), order (N,) stable argsort of the keys, count / start (M,), inverse (N,)."""
    grid = grid_coords(coord, min_coord, grid_size)
    key = fnv_keys(grid)
    order = np.argsort(key, kind="stable")
    _, inv_sorted, count = np.unique(key[order], return_inverse=True, return_counts=True)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    inverse = np.zeros(len(key), np.int64)
    inverse[order] = inv_sorted.reshape(-1)
    return {"grid": grid, "key": key, "order": order, "count": count.astype(np.int64), "start": start, "inverse": inverse}


def pick(vox, draws=None, mode="train", part=0):
    """Index of each voxel's pick: start + r % count (train, r = draws) or start + part % count (test)."""
    if mode == "train":
        sel = vox["start"] + np.asarray(draws, np.int64) % vox["count"]
    else:
        sel = vox["start"] + part % vox["count"]
    return vox["order"][sel]


def grid_sample(coord, min_coord=None, grid_size=0.02, draws=None, mode="train", part=0):
    coord = np.asarray(coord, np.float32)
    vox = voxelize(coord, min_coord, grid_size)
    idx = pick(vox, draws, mode, part)
    return {"index": idx, "coord": coord[idx], "grid_coord": vox["grid"][idx], "inverse": vox["inverse"], "count": vox["count"],
            "voxel": vox}


def filter_pixels(unprojected_coord, init_coord):
    """Flatten (view, row, column); keep w != 0 (NaN is valid) and the inclusive fp32 box of init_coord.  -> (coord (n,3), pixel (n,))"""
    uc = np.asarray(unprojected_coord, np.float32)[0].reshape(-1, 4)
    ic = np.asarray(init_coord, np.float32)
    lo, hi = ic.min(0), ic.max(0)
    keep = uc[:, 3] != 0
    pix = np.nonzero(keep)[0]
    c = uc[pix, :3]
    box = np.all((c >= lo) & (c <= hi), axis=1)
    return c[box], pix[box]


def point_fusion(feat_2d_all, unprojected_coord, init_coord, grid_size=0.02, draws=None, mode="train", part=0):
    """The device half of PointFusion.forward: -> None (no pixel survives) or coord, grid_coord, feat, src_pixel."""
    feat = np.asarray(feat_2d_all, np.float32)
    V, C, H, W = feat.shape
    coord, pix = filter_pixels(unprojected_coord, init_coord)
    if len(coord) == 0:
        return None
    g = grid_sample(coord, np.asarray(init_coord, np.float32).min(0), grid_size, draws, mode, part)
    src = pix[g["index"]]
    view, hw = src // (H * W), src % (H * W)
    f = feat.reshape(V, C, H * W)[view, :, hw]
    return {"coord": g["coord"], "grid_coord": g["grid_coord"], "feat": f, "src_pixel": src, "count": g["count"], "n": len(coord)}


def feat_grad(shape, src_pixel, grad_feat):
    """d(feat_2d_all) of sum(feat * grad_feat): each picked pixel's row, zero elsewhere."""
    V, C, H, W = shape
    g = np.zeros((V, C, H * W), np.float32)
    g[src_pixel // (H * W), :, src_pixel % (H * W)] = np.asarray(grad_feat, np.float32)
    return g.reshape(V, C, H, W)
