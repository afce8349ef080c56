#!/usr/bin/env python3
"""The offset-batched point operators (unipre3d_amd.offset_ops) against torch's own on-device forms of the same calls.

  evaluator_b1 / _b4   the evaluator's call (pointcept/engines/hooks/evaluator.py:125-132): nearest voxel of every original point,
                       b scenes of n = 100 000 voxels and m = 200 000 points each, k = 1.  torch form: the best chunk size of a
                       loop of torch.cdist(query chunk, scene) + min over the scene's queries (a full distance matrix is 80 GB).
  ptv1_*               a PTv1-style layer, one scene, n = m = 100 000, k = 16, c = 64 (weights shared over 8 channels):
                       knn        HIP only (no torch form fits: recorded for the sum of the layer)
                       grouping / subtraction / aggregation, forward and backward, against torch indexing (`x[idx]`, broadcast
                       arithmetic, sum) whose backward is torch's own index_add_-style scatter.

Method (tools/knn_bench.py): device events around `iters` back-to-back calls give one sample (microseconds per call); the forms
are sampled in turn, `samples` times each after `warmup` calls; median, minimum and maximum are kept.  ratio = median(torch) /
median(HIP): above 1 the HIP kernel is faster.  One JSON line per row to --out (default profiles/offsetops/offsetops_bench.jsonl).
Recorded, not gated."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sample(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _measure(forms, iters, samples, warmup):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {f: [] for f in forms}
    for _ in range(samples):
        for f, fn in forms.items():
            got[f].append(_sample(fn, iters))
    row = {}
    for f, v in got.items():
        row.update({f"{f}_us": round(statistics.median(v), 2), f"{f}_us_min": round(min(v), 2), f"{f}_us_max": round(max(v), 2)})
    return row


def cdist_nearest(xyz, offsets, new_xyz, new_offsets, chunk):
    """Nearest support row per query, scene by scene, `chunk` queries at a time (host-side offsets: the torch form needs them)."""
    out = torch.empty(new_xyz.size(0), dtype=torch.int64, device=xyz.device)
    a = qa = 0
    for e, qe in zip(offsets, new_offsets):
        scene = xyz[a:e]
        for q0 in range(qa, qe, chunk):
            q1 = min(qe, q0 + chunk)
            out[q0:q1] = torch.cdist(new_xyz[q0:q1], scene).argmin(1) + a
        a, qa = e, qe
    return out


def evaluator(b, n, m, a, dev):
    from unipre3d_amd import offset_ops
    g = torch.Generator().manual_seed(b)
    xyz, new_xyz = torch.rand(b * n, 3, generator=g).to(dev), torch.rand(b * m, 3, generator=g).to(dev)
    off, new_off = [n * (i + 1) for i in range(b)], [m * (i + 1) for i in range(b)]
    t_off, t_new = torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(new_off, dtype=torch.int32, device=dev)
    hip = lambda: offset_ops.knn_query(1, xyz, t_off, new_xyz, t_new)
    row = {"shape": f"evaluator_b{b}", "b": b, "n": n, "m": m, "k": 1, "iters": a.iters_search, "samples": a.samples}
    with torch.no_grad():
        same = hip()[0].flatten().long() == cdist_nearest(xyz, off, new_xyz, new_off, 8192)
        row["same_indices_fraction"] = round(float(same.float().mean()), 6)      # cdist's |a|^2 + |b|^2 - 2ab rounds differently
        row.update(_measure({"hip": hip}, a.iters_search, a.samples, a.warmup))
        best = None
        for chunk in (2048, 8192, 32768):
            r = _measure({"cdist": lambda: cdist_nearest(xyz, off, new_xyz, new_off, chunk)}, 1, max(3, a.samples // 3), 1)
            row[f"cdist_chunk{chunk}_us"] = r["cdist_us"]
            if best is None or r["cdist_us"] < best["cdist_us"]:
                best, row["cdist_best_chunk"] = r, chunk
        row.update(best)
    row["ratio_cdist"] = round(row["cdist_us"] / row["hip_us"], 2)
    return [row]


def ptv1(n, k, c, w_c, a, dev):
    from unipre3d_amd import offset_ops as ops
    g = torch.Generator().manual_seed(n)
    xyz = torch.rand(n, 3, generator=g).to(dev)
    off = torch.tensor([n], dtype=torch.int32, device=dev)
    base = {"n": n, "m": n, "k": k, "c": c, "w_c": w_c, "samples": a.samples}
    rows = []
    with torch.no_grad():
        rows.append({"shape": "ptv1_knn", **base, "iters": a.iters_search,
                     **_measure({"hip": lambda: ops.knn_query_raw(k, xyz, None, off, None)}, a.iters_search, a.samples, a.warmup)})
        idx = ops.knn_query_raw(k, xyz, None, off, None)[1]
    long = idx.long()
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    x, x2, p, w = r(n, c), r(n, c), r(n, k, c), r(n, k, w_c)
    g3, g2 = r(n, k, c), r(n, c)

    def pair(name, hip_fn, torch_fn, inputs, cot):
        """forward and forward+backward of both forms on leaf copies of `inputs`"""
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        with torch.no_grad():
            fwd = _measure({"hip": lambda: hip_fn(*leaves), "torch": lambda: torch_fn(*leaves)}, a.iters, a.samples, a.warmup)
        step = lambda fn: torch.autograd.grad(fn(*leaves), leaves, cot)
        both = _measure({"hip": lambda: step(hip_fn), "torch": lambda: step(torch_fn)}, a.iters, a.samples, a.warmup)
        for tag, m in (("forward", fwd), ("forward_backward", both)):
            rows.append({"shape": f"ptv1_{name}_{tag}", **base, "iters": a.iters, **m, "ratio_torch": round(m["torch_us"] / m["hip_us"], 2)})

    pair("grouping", lambda t: ops.grouping(t, idx), lambda t: t[long], [x], g3)
    pair("subtraction", lambda s, t: ops.subtraction(s, t, idx), lambda s, t: s.unsqueeze(1) - t[long], [x, x2], g3)
    pair("aggregation", lambda t, q, v: ops.aggregation(t, q, v, idx),
         lambda t, q, v: ((t[long] + q).view(n, k, c // w_c, w_c) * v.unsqueeze(2)).sum(1).view(n, c), [x, p, w], g2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--iters-search", dest="iters_search", type=int, default=3)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated groups: evaluator_b1, evaluator_b4, ptv1 (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offsetops", "offsetops_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("offsetops_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    only = set(filter(None, a.only.split(",")))
    groups = [("evaluator_b1", lambda: evaluator(1, 100000, 200000, a, dev)), ("evaluator_b4", lambda: evaluator(4, 100000, 200000, a, dev)),
              ("ptv1", lambda: ptv1(100000, 16, 64, 8, a, dev))]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, run in groups:
            if only and name not in only:
                continue
            for row in run():
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
