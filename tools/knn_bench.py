#!/usr/bin/env python3
"""k-nearest-neighbour search (unipre3d_amd.knn.knn_query) against torch's own on-device forms of the same call, at the shapes the three
backbones that need it use (model/point_predictor.py:136-218 and the backbone constructors of the reference):

  mamba3d_group        Mamba3D `Group`: 128 FPS centres query the cloud for group_size = 32 neighbours      (B 32, N 1024, M 128, k 32)
  mamba3d_group_2048   the same on a 2048-point cloud                                                       (B 32, N 2048, M 128, k 32)
  mamba3d_feature_k4   Mamba3D `GroupFeature`: the 128 centres among themselves, center_local_k = 4         (B 32, N 128, M 128, k 4)
  mamba3d_feature_k8   ... with the constructor's default k_group_size = 8                                  (B 32, N 128, M 128, k 8)
  pcm_stage{1..4}      PCM's PointMambaEncoder: k_neighbors 12, reducers 2 at every stage                    (B 16, N 2048 >> (i-1), M N/2, k 12)
  pointmlp_stage{1..4} PointMLP: k_neighbors 24, reducers 2, at config C3's B 16, N 2048                    (B 16, N 2048 >> (i-1), M N/2, k 24)

The two torch forms are written out here, as the reference's groupers write them:
  direct   ((q.unsqueeze(2) - s.unsqueeze(1)) ** 2).sum(-1).topk(k, largest=False, sorted=True)                 (PCM)
  matmul   -2 q s^T + |q|^2 + |s|^2, then the same topk                                                         (PointMLP)

Method.  Device events around `iters` back-to-back calls give one sample (microseconds per call); the three forms are sampled in
turn, `samples` times each after `warmup` calls, and the median, the minimum and the maximum of the samples are kept.  ratio_* is
median(torch form) / median(HIP): above 1 the HIP kernel is faster.  `same_indices` says whether the HIP indices equal the direct
form's on this input (seeded uniform clouds, queries a subset of the support).  One JSON line per shape to --out (default
profiles/knn/knn_bench.jsonl).  Recorded, not gated; INTEGRATION.md's switch-over rule for PCM / PointMLP reads these lines."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("mamba3d_group", 32, 1024, 128, 32), ("mamba3d_group_2048", 32, 2048, 128, 32), ("mamba3d_feature_k4", 32, 128, 128, 4),
          ("mamba3d_feature_k8", 32, 128, 128, 8)]
SHAPES += [(f"pcm_stage{i + 1}", 16, 2048 >> i, 1024 >> i, 12) for i in range(4)]
SHAPES += [(f"pointmlp_stage{i + 1}", 16, 2048 >> i, 1024 >> i, 24) for i in range(4)]


def direct(k, s, q):
    return ((q.unsqueeze(2) - s.unsqueeze(1)) ** 2).sum(-1).topk(k, dim=-1, largest=False, sorted=True)


def matmul(k, s, q):
    d = -2 * torch.matmul(q, s.permute(0, 2, 1))
    d += torch.sum(q ** 2, -1).unsqueeze(2)
    d += torch.sum(s ** 2, -1).unsqueeze(1)
    return d.topk(k, dim=-1, largest=False, sorted=True)


def _sample(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench(name, B, N, M, k, iters, samples, warmup, dev):
    from unipre3d_amd import knn
    g = torch.Generator().manual_seed(N * 31 + k)
    s = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    q = s[:, torch.randperm(N, generator=g)[:M].to(dev)].contiguous()
    forms = {"hip": lambda: knn.knn_query(k, s, q), "direct": lambda: direct(k, s, q), "matmul": lambda: matmul(k, s, q)}
    with torch.no_grad():
        same = bool(torch.equal(forms["hip"]()[1].long(), forms["direct"]()[1]))
        for fn in forms.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        got = {f: [] for f in forms}
        for _ in range(samples):
            for f, fn in forms.items():
                got[f].append(_sample(fn, iters))
    row = {"shape": name, "B": B, "N": N, "M": M, "k": k, "iters": iters, "samples": samples, "same_indices": same}
    for f, v in got.items():
        row.update({f"{f}_us": round(statistics.median(v), 2), f"{f}_us_min": round(min(v), 2), f"{f}_us_max": round(max(v), 2)})
    row["ratio_direct"] = round(row["direct_us"] / row["hip_us"], 2)
    row["ratio_matmul"] = round(row["matmul_us"] / row["hip_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--samples", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn", "knn_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, B, N, M, k in SHAPES:
            if only and name not in only:
                continue
            row = bench(name, B, N, M, k, a.iters, a.samples, a.warmup, dev)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
