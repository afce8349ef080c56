#!/usr/bin/env python3
"""The decoder's feature propagation of PointMLP and PCM (unipre3d_amd.feature_propagation.propagate) against the two other ways to get
the (B, D1 + D2, N) tensor the `fuse` convolution reads, at (B, N, S, D1, D2):

  pointmlp_1 .. 4   (16, 256, 128, 512, 1024), (16, 512, 256, 256, 512), (16, 1024, 512, 128, 256), (16, 2048, 1024, 64, 128): PointMLP's four
                    decoder stages at configuration C3's per-GPU batch
  pcm_first, pcm_last   (16, 256, 128, 768, 768) and (16, 2048, 1024, 384, 384): the first and the last decoder stage of PCM.py's defaults
                    (encoder channels 384, 384, 384, 768, 768, decoder channels 768, 384, 384, 384, reducers of 2 from 2048 points)

  hip        propagate(xyz1, xyz2, points1, points2): search, forward, and with a gradient the lists and the backward
  reference  the reference's lines in torch on the device (tests/feature_propagation_ref.py: reference_form): the (B, N, S) matrix in the
             matmul form, the full sort, the (B, N, 3, D2) gather, sum, cat, permute, then .contiguous(), which the convolution would do
  composed   what the project had before: knn.knn_query(3, xyz2, xyz1), the weights in torch, pointops.three_interpolate, torch.cat

xyz2 is a subset of xyz1, as every stage's sampling makes it.  `forward` runs under no_grad; `fwd_bwd` is the forward and its backward to
points1 and points2 from a fixed gradient.  Every figure is taken in two modes: `eager`, a Python loop of `iters` calls between two device
events (the host's cost per call is in it), and `graph`, the same `iters` calls captured once into one graph on one stream and replayed
between the events (the device's cost).  A sample is microseconds per call; the forms are sampled in turn, `samples` times each after
`warmup` calls (or replays), and the median, the minimum and the maximum are kept.  ratio_<mode>_<what>_<form> = form / hip on the medians:
at or above 1 the HIP kernels are at or below that form.  kept_mb: what one forward leaves allocated above the starting level while its
result is alive (the result itself included, out_mb); peak_mb: the peak of one forward + backward above the same level.  max_rel_*: hip
against the other form on this input, max|difference| / max|other|.  hip_forward_gbs: the bytes the forward has to move (points1 and
points2 read, out written, both clouds read, idx and weight written and read) over the graph-mode time.

One JSON line per shape to --out (default profiles/feature_propagation/feature_propagation_bench.jsonl).  Recorded, not gated; DESIGN.md
and INTEGRATION.md 5.13 read these lines."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("pointmlp_1", 16, 256, 128, 512, 1024), ("pointmlp_2", 16, 512, 256, 256, 512), ("pointmlp_3", 16, 1024, 512, 128, 256),
          ("pointmlp_4", 16, 2048, 1024, 64, 128), ("pcm_first", 16, 256, 128, 768, 768), ("pcm_last", 16, 2048, 1024, 384, 384)]


def composed(xyz1, xyz2, points1, points2):
    from unipre3d_amd import knn, pointops
    d2, idx = knn.knn_query(3, xyz2, xyz1)
    r = 1.0 / (d2 + 1e-8)
    w = r / torch.sum(r, dim=2, keepdim=True)
    return torch.cat([points1, pointops.three_interpolate(points2, idx, w)], dim=1)


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _captured(body, iters):
    """`iters` calls of body captured into one graph on one stream, after the side-stream warm-up capture needs."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            body()
    return graph


def bench(name, B, N, S, D1, D2, iters, samples, warmup, dev):
    import feature_propagation_ref as FR
    from unipre3d_amd import feature_propagation as fp
    g = torch.Generator().manual_seed(N * 31 + D1 + D2)
    xyz1 = torch.rand(B, N, 3, generator=g)
    xyz2 = torch.stack([xyz1[b, torch.randperm(N, generator=g)[:S].sort()[0]] for b in range(B)]).to(dev)
    xyz1 = xyz1.to(dev)
    p1d, p2d = torch.randn(B, D1, N, generator=g).to(dev), torch.randn(B, D2, S, generator=g).to(dev)
    dout = torch.randn(B, D1 + D2, N, generator=g).to(dev)
    p1, p2 = p1d.clone().requires_grad_(True), p2d.clone().requires_grad_(True)
    forms = {"hip": lambda a, b: fp.propagate(xyz1, xyz2, a, b),
             "reference": lambda a, b: FR.reference_form(xyz1, xyz2, a, b).contiguous(),
             "composed": lambda a, b: composed(xyz1, xyz2, a, b)}

    def fwd(form):
        def body():
            with torch.no_grad():
                return forms[form](p1d, p2d)
        return body

    def fb(form):
        def body():
            return torch.autograd.grad(forms[form](p1, p2), (p1, p2), dout)
        return body

    row = {"shape": name, "B": B, "N": N, "S": S, "D1": D1, "D2": D2, "iters": iters, "samples": samples,
           "out_mb": round(B * (D1 + D2) * N * 4 / 2 ** 20, 1)}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    o_hip = fwd("hip")()
    g_hip = fb("hip")()
    for other in ("reference", "composed"):
        row[f"max_rel_out_{other}"] = rel(o_hip, fwd(other)())
        row[f"max_rel_dpoints2_{other}"] = rel(g_hip[1], fb(other)()[1])
    del o_hip, g_hip
    for form in forms:                           # memory: one forward kept alive, then one forward + backward
        for _ in range(2):                       # (the second pass is the measured one)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y = forms[form](p1, p2)
            torch.cuda.synchronize()
            kept = torch.cuda.memory_allocated() - base
            grads = torch.autograd.grad(y, (p1, p2), dout)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del y, grads
        row[f"{form}_kept_mb"], row[f"{form}_peak_mb"] = round(kept / 2 ** 20, 1), round(peak / 2 ** 20, 1)
    bodies = {f"{form}_{what}": mk(form) for what, mk in (("forward", fwd), ("fwd_bwd", fb)) for form in forms}
    run = {}
    for key, body in bodies.items():
        run[f"eager_{key}"] = (lambda body=body: [body() for _ in range(iters)])
        run[f"graph_{key}"] = _captured(body, iters).replay      # (the bound method keeps the graph, which owns its memory, alive)
    for fn in run.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in run}
    for _ in range(samples):
        for k, fn in run.items():
            got[k].append(_events(fn) / iters)
    for k, v in got.items():
        row.update({f"{k}_us": round(statistics.median(v), 2), f"{k}_us_min": round(min(v), 2), f"{k}_us_max": round(max(v), 2)})
    for m in ("eager", "graph"):
        for what in ("forward", "fwd_bwd"):
            for other in ("reference", "composed"):
                row[f"ratio_{m}_{what}_{other}"] = round(row[f"{m}_{other}_{what}_us"] / row[f"{m}_hip_{what}_us"], 2)
    moved = 4 * (B * D1 * N + B * D2 * S + B * (D1 + D2) * N + 3 * B * (N + S) + 4 * 3 * B * N)
    row["hip_forward_gbs"] = round(moved / row["graph_hip_forward_us"] / 1e3, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_propagation", "feature_propagation_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_propagation_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, *shape in SHAPES:
            if only and name not in only:
                continue
            row = bench(name, *shape, a.iters, a.samples, a.warmup, dev)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
