#!/usr/bin/env python3
"""Scene-level PointFusion: forward (filter + grid sample + feature gather, unipre3d_amd.pointfusion.fuse_pixels) and
backward (gather-form feature gradient) timed on the device at the scene configs' training resolution (8 x 120 x 160) and at the full
8 x 480 x 640, C = 32, on unipre3d_amd.synthetic.point_fusion_scene; next to the numpy restatement's host time on the same input
(tests/pointfusion_ref.py, the reference's arithmetic without its torch plumbing).

Bytes are the kernels' own traffic by design, with no cache reuse counted: compaction reads the (P,4) pixels twice and writes n kept
rows (16 B), keys read 12 B and write 12 B per point, each of the 8 radix passes reads 12 B (histogram) + 12 B and writes 12 B
(scatter), segment heads read 12 B and write 4 B per point, the pick reads its voxel's bounds and writes 44 B, the gather reads and
writes 4 B per feature.  Backward: the (V,P/V) pixel map written twice and read once per channel plane, the gradient written once,
the picked rows read.  One JSON line per shape; --out also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 8.0e12


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e6


def run(V, H, W, C, iters, warmup, host_reps):
    import pointfusion_ref as R
    from unipre3d_amd import synthetic
    from unipre3d_amd.pointfusion import fuse_pixels
    dev = torch.device("cuda:0")
    s = synthetic.point_fusion_scene(V, H, W, C=C, seed=1)
    feat = s["feat_2d_all"].to(dev).requires_grad_(True)
    uc, init = s["unprojected_coord"].to(dev), s["init_coord"].to(dev)
    torch.manual_seed(0)
    out = fuse_pixels(feat, uc, init, 0.02)
    n, M, P = out["n"], out["feat"].shape[0], V * H * W
    g = torch.randn_like(out["feat"])

    fwd_us = _time(lambda: fuse_pixels(feat.detach(), uc, init, 0.02), iters, warmup)
    bwd_us = _time(lambda: torch.autograd.grad(out["feat"], feat, g, retain_graph=True), iters, warmup)

    fwd_bytes = 2 * P * 16 + n * 16 + n * 24 + 8 * n * 36 + n * 16 + M * (8 + 4 + 44) + M * C * 8
    bwd_bytes = P * 4 * 2 + M * 8 + V * C * H * W * 8 + M * C * 4

    ucn, initn, featn = s["unprojected_coord"].numpy(), s["init_coord"].numpy(), s["feat_2d_all"].numpy()
    coord, _ = R.filter_pixels(ucn, initn)
    count = R.voxelize(coord, initn.min(0), 0.02)["count"]
    draws = np.random.default_rng(0).integers(0, count.max(), len(count))
    host = []
    for _ in range(host_reps):
        t = time.perf_counter()
        R.point_fusion(featn, ucn, initn, 0.02, draws=draws)
        host.append(time.perf_counter() - t)
    return {"shape": f"{V}x{H}x{W}", "C": C, "P": P, "N": n, "M": M, "fwd_us": round(fwd_us, 1), "bwd_us": round(bwd_us, 1),
            "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes, "fwd_roofline": round(fwd_bytes / (fwd_us * 1e-6) / HBM, 3),
            "bwd_roofline": round(bwd_bytes / (bwd_us * 1e-6) / HBM, 3), "host_numpy_ms": round(min(host) * 1e3, 1),
            "speedup_fwd_vs_host": round(min(host) * 1e6 / fwd_us, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lines = []
    for V, H, W in ((8, 120, 160), (8, 480, 640)):
        r = run(V, H, W, 32, a.iters, a.warmup, a.host_reps)
        r["device"] = torch.cuda.get_device_name(0)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
