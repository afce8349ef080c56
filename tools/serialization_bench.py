#!/usr/bin/env python3
"""PTv3's index plumbing (unipre3d_amd.serialization) at scene sizes: microseconds per call of serialize, patch_padding (host offset
and device offset) and pool_clusters, next to the torch RESTATEMENT of the same work (tests/serialization_ref.py: torch.argsort,
scatter_, torch.unique and the per-item Python loop) on the same device in the same run.  The restatement is not the reference:
the reference's Hilbert code works on (N, 3, depth) bit planes and is heavier.

Timing as tools/attention_bench.py: warm-up calls, then wall time of `iters` back-to-back calls between two synchronisations,
repeated `repeats` times; the median is reported (calls that read the device, pool_clusters and the restatement's, synchronise
inside every call, which is part of what they cost).  Outputs are compared before timing.  One JSON line per row to --out
(default profiles/serialization/serialization_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")


def _time(fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t) / iters * 1e6)
    return statistics.median(runs)


def _scene(N, B, depth, dev):
    """B items of N / B points on a surface-like set of sites (two coordinates free, the third a function of them), about
    a tenth of the points on a repeated site, as fused voxels are."""
    g = torch.Generator().manual_seed(N + depth)
    side = min(1 << depth, 1024)
    a, b = torch.randint(0, side, (N,), generator=g), torch.randint(0, side, (N,), generator=g)
    coord = torch.stack([a, b, (a * 3 + b * 5) // 8 % side], 1).int()
    rep = torch.randint(0, N, (N // 10,), generator=g)
    coord[rep] = coord[(rep + 1) % N]
    batch = torch.arange(N) * B // N
    offset = torch.tensor([(i + 1) * N // B for i in range(B)])
    return coord.to(dev), batch.to(dev), offset


def bench(N, B, depth, patch, pooling_depth, a, dev):
    import serialization_ref as R
    from unipre3d_amd import serialization as S
    coord, batch, offset = _scene(N, B, depth, dev)
    off_host, off_dev = offset.tolist(), offset.to(dev)
    ours = S.serialize(coord, batch, depth, ORDERS, batch_size=B)
    ref = R.serialize(coord, batch, depth, ORDERS)
    code = ours[0]
    checks = list(zip(ours, ref)) + list(zip(S.patch_padding(off_dev, patch), R.patch_padding(off_dev, patch)))
    checks += list(zip(S.pool_clusters(code, pooling_depth, depth=depth, batch_size=B), R.pool_clusters(code, pooling_depth)))
    if not all(torch.equal(x, y) for x, y in checks):
        raise SystemExit(f"N={N} depth={depth}: the library and the restatement disagree")
    t = lambda fn: _time(fn, a.iters, a.warmup, a.repeats)
    row = {"row": f"N{N}_B{B}_d{depth}", "N": N, "B": B, "depth": depth, "orders": len(ORDERS), "patch": patch,
           "pooling_depth": pooling_depth, "clusters": int(checks[-4][0].shape[0]), "baseline": "torch restatement (tests/serialization_ref.py)"}
    for name, fn, base in (
            ("serialize", lambda: S.serialize(coord, batch, depth, ORDERS, batch_size=B), lambda: R.serialize(coord, batch, depth, ORDERS)),
            ("encode", lambda: S.encode(coord, batch, depth, ORDERS), lambda: [R.encode(coord, batch, depth, o) for o in ORDERS]),
            ("sort", lambda: S.sort_codes(code, key_bits=3 * depth + (B - 1).bit_length()), lambda: R.order_inverse(code)),
            ("patch_padding_host_offset", lambda: S.patch_padding(off_host, patch, device=dev), lambda: R.patch_padding(off_host, patch, device=dev)),
            ("patch_padding_device_offset", lambda: S.patch_padding(off_dev, patch), lambda: R.patch_padding(off_dev, patch)),
            ("pool_clusters", lambda: S.pool_clusters(code, pooling_depth, depth=depth, batch_size=B), lambda: R.pool_clusters(code, pooling_depth))):
        us, base_us = t(fn), t(base)
        row.update({f"{name}_us": round(us, 1), f"{name}_torch_us": round(base_us, 1), f"{name}_speedup": round(base_us / us, 2)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[40_000, 120_000, 350_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serialization", "serialization_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("serialization_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    rows = [bench(N, 2, depth, 1024, 1, a, dev) for N in a.sizes for depth in (10, 16)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
