#!/usr/bin/env python3
"""Furthest point sampling of large clouds: the grid kernel (u3d_furthest_point_sampling_grid, one cloud over several workgroups,
csrc/u3d_fps_grid.h) against the one-workgroup-per-cloud path (u3d_furthest_point_sampling, which runs fps_kernel_large above 8192
points), at the scene-level loader's shapes and around the routing threshold of unipre3d_amd.pointops.furthest_point_sample:

  loader_100k   the loader's FPS(max_points=80000) on a 100 000-point scene                (B 1, N 100 000, M 80 000)
  loader_200k   ... on a 200 000-point scene                                               (B 1, N 200 000, M 80 000)
  n16k          just above the dense kernels' 8192                                          (B 1, N 16 384,  M 1024)
  n32k                                                                                      (B 1, N 32 768,  M 2048)
  batch4_50k    four clouds, four independent meeting groups                                (B 4, N 50 000,  M 10 000)
  ragged_60k_140k   offset_ops.furthestsampling on offset = [60 000, 200 000], new_offset = [24 000, 80 000] (grid kernel only)

Method.  Both paths are called through the raw C ABI on the same device buffers.  `--parent-lib` names a libunipre3d_pointops.so
built from the commit before the grid kernel; without it the one-workgroup path is this library's own u3d_furthest_point_sampling
(the same source).  Device events around one call give one sample; the two paths are sampled in turn, `samples` times each after
`warmup` calls each; the median, minimum and maximum are kept, and the median per selection in microseconds.  `same_indices`: the two
paths returned identical indices.  ratio = median(one workgroup) / median(grid): above 1 the grid kernel is faster.  One JSON line
per shape to --out (default profiles/fps/fps_bench.jsonl).  Recorded, not gated: DESIGN.md's routing rule reads these lines."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("loader_100k", 1, 100000, 80000), ("loader_200k", 1, 200000, 80000), ("n16k", 1, 16384, 1024), ("n32k", 1, 32768, 2048),
          ("batch4_50k", 4, 50000, 10000)]
RAGGED = ("ragged_60k_140k", [60000, 200000], [24000, 80000])


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(prefix, ms, selections):
    med = statistics.median(ms)
    return {f"{prefix}_ms": round(med, 3), f"{prefix}_ms_min": round(min(ms), 3), f"{prefix}_ms_max": round(max(ms), 3),
            f"{prefix}_us_per_selection": round(med * 1e3 / selections, 3)}


def _cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N, 3, generator=g) * 2 - 1).cuda()


def bench_dense(name, B, N, M, samples, warmup, parent):
    from unipre3d_amd import _lib, pointops
    lib = pointops.load()
    xyz = _cloud(B, N, N + M)
    ws = pointops.grid_workspace(B, xyz.device)
    temp = torch.empty(B, N, dtype=torch.float32, device=xyz.device)
    out_g = torch.empty(B, M, dtype=torch.int32, device=xyz.device)
    out_p = torch.empty(B, M, dtype=torch.int32, device=xyz.device)
    st = _lib.stream_ptr(xyz.device)

    def grid():
        pointops.check(lib.u3d_furthest_point_sampling_grid(B, N, M, _lib.ptr(xyz), _lib.ptr(ws), _lib.ptr(out_g), st), "grid", named=False)

    def one():
        pointops.check(parent.u3d_furthest_point_sampling(B, N, M, _lib.ptr(xyz), _lib.ptr(temp), _lib.ptr(out_p), st), "parent", named=False)

    for _ in range(warmup):
        grid()
        one()
    torch.cuda.synchronize()
    tg, tp = [], []
    for _ in range(samples):
        tp.append(_timed(one))
        tg.append(_timed(grid))
    row = {"shape": name, "B": B, "N": N, "M": M, "samples": samples, "same_indices": bool(torch.equal(out_g, out_p)),
           "status_word": pointops.grid_status(xyz.device)}
    row.update(_stats("one_workgroup", tp, M))
    row.update(_stats("grid", tg, M))
    row["ratio"] = round(row["one_workgroup_ms"] / row["grid_ms"], 2)
    return row


def bench_ragged(name, offset, new_offset, samples, warmup):
    from unipre3d_amd import offset_ops, pointops
    n, m = offset[-1], new_offset[-1]
    xyz = _cloud(1, n, n)[0].contiguous()
    off = torch.tensor(offset, dtype=torch.int32, device=xyz.device)
    noff = torch.tensor(new_offset, dtype=torch.int32, device=xyz.device)
    for _ in range(warmup):
        offset_ops.furthestsampling(xyz, off, noff, m=m)
    torch.cuda.synchronize()
    ms = [_timed(lambda: offset_ops.furthestsampling(xyz, off, noff, m=m)) for _ in range(samples)]
    longest = max(b - a for a, b in zip([0] + new_offset[:-1], new_offset))
    row = {"shape": name, "offset": offset, "new_offset": new_offset, "samples": samples, "status_word": pointops.grid_status(xyz.device)}
    row.update(_stats("grid", ms, longest))        # the segments run side by side: the longest request is the dependent chain
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--parent-lib", default="", help="libunipre3d_pointops.so of the parent commit (default: this library's own one-workgroup path)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps", "fps_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_bench.py needs an MI355X: nothing is timed without one")
    from unipre3d_amd import pointops
    parent = pointops.load()
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.u3d_furthest_point_sampling.restype, parent.u3d_furthest_point_sampling.argtypes = pointops.SIGNATURES["u3d_furthest_point_sampling"]
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, B, N, M in SHAPES:
            if only and name not in only:
                continue
            row = bench_dense(name, B, N, M, a.samples, a.warmup, parent)
            row["one_workgroup_library"] = "parent commit" if a.parent_lib else "this build"
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
        if not only or RAGGED[0] in only:
            row = bench_ragged(*RAGGED, a.samples, a.warmup)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
