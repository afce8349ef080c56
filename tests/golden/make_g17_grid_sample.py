#!/usr/bin/env python3
"""Generates tests/golden/g17_grid_sample.npz: pointcept's OWN GridSample(hash_type="fnv", return_grid_coord=True,
return_inverse=True) (pointcept/datasets/transform_with_extrinsic.py:1179-1326) run on the CPU, for
unipre3d_amd.pointfusion.grid_sample and its numpy restatement tests/pointfusion_ref.py.

The class is loaded with make_g11_point_fusion's stubs.  np.argsort is forced to kind="stable" (the pinned within-voxel order:
ascending point index), np.random.randint is recorded (the train-mode draw, one int per voxel) and grid_size is passed as
np.float32 so that numpy >= 2 divides in fp32 as the reference's numpy 1.26 does with a 0-d float64 divisor.

Every cloud is recorded with both origins -- "def": min_coord=None (g = floor(coord / gs); grid = g - g.min(0)) and "exp": an
explicit min_coord (grid = floor((coord - min_coord) / gs)) -- in train mode (index, grid_coord, inverse, the draws) and in
test mode (one part per i < count.max(): index and grid_coord of each, and the inverse).  Train mode returns no index of its own:
an arange rides along as a sampled key.  Keys of the file: `names`, `names_def` (the clouds that have a default-origin record) and per
cloud `<name>_coord`, `<name>_min_coord`, `<name>_grid_size`, `<name>_<origin>_{draws,train_index,train_grid_coord,
train_inverse,test_index (parts, M),test_grid_coord (parts, M, 3),test_inverse}`.

Clouds (grid 0.02 but for the last):
  shift     uniform in [0, 0.3) + 0.013: the minimum is not on a cell boundary, so the two origins cut different cells
  neg       uniform in [0, 0.1) - 1.237: negative coordinates, many points per voxel; explicit origin a little below the minimum
  straddle  uniform in [-0.15, 0.15): either side of zero on every axis; explicit origin zero (negative grid coordinates)
  boundary  points exactly on fp32 cell boundaries, fp32(k * 0.02) and fp32(min + fp32(k * 0.02)), and their fp32 neighbours
  fp64      rows whose fp32 quotient floors differently from the fp64 one (`fp64_def_rows` for coord / gs on the x axis,
            `fp64_exp_rows` for (coord - min) / gs on the y axis)
  one       one point
  onevoxel  500 points in one voxel under both origins (500 test-mode parts of one voxel)
  range     explicit origin zero, grid 1.0: +-inf, +-3e30, +-fp32(2^63 - 2^39) (the largest fp32 below 2^63), +-2^63, +-2^62 and
            ordinary points; numpy's fp32 -> int64 conversion on x86 (out of range gives INT64_MIN).  No default-origin record
            and no NaN (coord.min(0) and the device's fminf treat NaN differently; not pinned here)
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
GS = np.float32(0.02)


def _rand(n, seed, spread, shift=0.0):
    return (np.random.default_rng(seed).random((n, 3), dtype=np.float32) * np.float32(spread) + np.float32(shift)).astype(np.float32)


def _fp64_disagreeing(m, ks, want=8):
    """fp32 x near m + k * 0.02 whose cell floor(fp32(x - m) / fp32(0.02)) differs between the fp32 and the fp64 division."""
    out = []
    m = np.float32(m)
    for k in ks:
        x0 = np.float32(m + np.float32(k * GS))
        for u in range(-4, 5):
            x = np.float32(x0 + np.float32(u) * np.spacing(x0))
            d = np.float32(x - m)
            if np.floor(d / GS) != np.floor(np.float64(d) / 0.02):
                out.append(x)
                break
        if len(out) >= want:
            break
    assert len(out) >= 4, len(out)
    return np.array(out, np.float32)


def clouds():
    """-> list of (name, coord (N,3) fp32, explicit min_coord (3,) fp32, grid_size fp32, has a default-origin record), extras"""
    out, extra = [], {}
    c = _rand(500, 1, 0.3, 0.013)
    out.append(("shift", c, c.min(0), GS, True))
    c = _rand(500, 2, 0.1, -1.237)
    out.append(("neg", c, c.min(0) - np.array([0.003, 0.011, 0.017], np.float32), GS, True))
    c = _rand(500, 3, 0.3, -0.15)
    out.append(("straddle", c, np.zeros(3, np.float32), GS, True))

    # on the cell boundaries of both origins, and one fp32 step either side of them
    c = _rand(400, 4, 0.3, -0.107)
    rows = np.random.default_rng(40).permutation(400)
    for p in rows[:120]:
        for a in range(3):
            c[p, a] = np.float32(int(np.floor(c[p, a] / GS)) * GS)      # fp32(k * 0.02), k of either sign
    for j, p in enumerate(rows[240:300]):                               # their fp32 neighbours
        c[p] = np.nextafter(c[rows[j]], np.float32(np.inf if j % 2 else -np.inf))
    m = c.min(0)
    for p in rows[120:240]:
        for a in range(3):
            k = int(np.floor((c[p, a] - m[a]) / GS))
            c[p, a] = np.float32(m[a] + np.float32(k * GS))              # fp32(min + fp32(k * 0.02))
    for j, p in enumerate(rows[300:360]):                               # their fp32 neighbours (none below the minimum)
        c[p] = np.maximum(np.nextafter(c[rows[120 + j]], np.float32(np.inf if j % 2 else -np.inf)), m)
    assert np.array_equal(c.min(0), m)
    out.append(("boundary", c, m, GS, True))

    c = _rand(300, 5, 0.5, -0.21)
    m = c.min(0)
    xs = np.concatenate([_fp64_disagreeing(0.0, range(1, 400), 6), _fp64_disagreeing(0.0, range(-1, -400, -1), 6)])
    xs = xs[(xs > m[0]) & (xs < c[:, 0].max())]
    ys = _fp64_disagreeing(m[1], range(1, 400), 8)
    ys = ys[ys < c[:, 1].max()]
    assert len(xs) >= 4 and len(ys) >= 4, (len(xs), len(ys))
    c[10:10 + len(xs), 0] = xs
    c[100:100 + len(ys), 1] = ys
    assert np.array_equal(c.min(0), m)
    extra["fp64_def_rows"] = np.arange(10, 10 + len(xs))
    extra["fp64_exp_rows"] = np.arange(100, 100 + len(ys))
    out.append(("fp64", c, m, GS, True))

    c = np.array([[0.37, -1.21, 2.5]], np.float32)
    out.append(("one", c, np.array([0.3, -1.3, 2.5], np.float32), GS, True))
    c = _rand(500, 6, 0.004, 0.501)
    out.append(("onevoxel", c, np.full(3, 0.5, np.float32), GS, True))

    big = np.float32(2.0 ** 63 - 2.0 ** 39)
    assert float(big) == 2.0 ** 63 - 2.0 ** 39 and np.nextafter(big, np.float32(np.inf)) == np.float32(2.0 ** 63)
    special = [np.inf, -np.inf, 3e30, -3e30, big, -big, 2.0 ** 63, -2.0 ** 63, 2.0 ** 62, -2.0 ** 62, 2.0 ** 63 - 2.0 ** 40, 2.0 ** 64]
    c = np.floor(_rand(len(special) + 20, 7, 6.0, -3.0) * 2) / 2                                # ordinary points, several per voxel
    c = c.astype(np.float32)
    for j, v in enumerate(special):
        c[j, j % 3] = np.float32(v)
    c[len(special)] = [big, -big, np.float32(2.0 ** 63)]
    c[len(special) + 1] = c[4]                                                                   # two points in an out-of-range voxel
    out.append(("range", c, np.zeros(3, np.float32), np.float32(1.0), False))
    return out, extra


def record(GridSample, coord, min_coord, grid_size, seed):
    """One origin of one cloud through the reference class, train and test mode."""
    draws = []
    orig = (np.random.randint, np.argsort)

    def randint(*a, **k):
        r = orig[0](*a, **k)
        draws.append(np.array(r))
        return r

    np.random.randint = randint
    np.argsort = lambda a, *x, **k: orig[1](a, kind="stable")
    np.random.seed(seed)
    kw = dict(grid_size=grid_size, hash_type="fnv", return_inverse=True, return_grid_coord=True, min_coord=min_coord)
    try:
        with np.errstate(invalid="ignore"):
            tr = GridSample(mode="train", keys=("coord", "index"), **kw)({"coord": coord.copy(), "index": np.arange(len(coord))})
            parts = GridSample(mode="test", keys=("coord",), **kw)({"coord": coord.copy()})
    finally:
        np.random.randint, np.argsort = orig
    assert len(draws) == 1, len(draws)
    assert np.array_equal(tr["coord"], coord[tr["index"]])
    return {"draws": draws[0].astype(np.int64), "train_index": tr["index"].astype(np.int64),
            "train_grid_coord": tr["grid_coord"].astype(np.int64), "train_inverse": tr["inverse"].astype(np.int64),
            "test_index": np.stack([p["index"] for p in parts]).astype(np.int64),
            "test_grid_coord": np.stack([p["grid_coord"] for p in parts]).astype(np.int64),
            "test_inverse": parts[0]["inverse"].astype(np.int64)}


def main():
    from make_g11_point_fusion import _reference_modules
    _reference_modules()
    GridSample = sys.modules["pointcept.datasets.transform_with_extrinsic"].GridSample
    cl, arrays = clouds()
    arrays["names"] = np.array([c[0] for c in cl])
    arrays["names_def"] = np.array([c[0] for c in cl if c[4]])
    for i, (name, coord, min_coord, gs, has_def) in enumerate(cl):
        assert coord.dtype == np.float32 and min_coord.dtype == np.float32 and not np.isnan(coord).any()
        arrays[f"{name}_coord"], arrays[f"{name}_min_coord"], arrays[f"{name}_grid_size"] = coord, min_coord, np.float32(gs)
        for origin in ("def", "exp") if has_def else ("exp",):
            rec = record(GridSample, coord, None if origin == "def" else min_coord, np.float32(gs), 170 + 2 * i + (origin == "exp"))
            for k, v in rec.items():
                arrays[f"{name}_{origin}_{k}"] = v
            print(f"g17 {name:9s} {origin}: {len(coord)} points, {len(rec['draws'])} voxels, {len(rec['test_index'])} parts")
    path = os.path.join(OUT, "g17_grid_sample.npz")
    np.savez_compressed(path, **arrays)
    print(f"g17: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
