#!/usr/bin/env python3
"""PCM's order serialization (unipre3d_amd.pcm_order.serialization) at the backbone's four stages and one larger shape: microseconds
per call next to the torch RESTATEMENT of the same work (tests/pcm_order_ref.py) on the same device in the same run, forward and forward
+ backward, in an eager loop and replayed from a graph.  The restatement is timed twice: with the reference's host read
(`int(grid.max())`, which the reference makes before every order; it cannot be captured) and without it (the depth passed in as a known int), which is also the
form that captures into a graph.  The restatement is not the reference: the reference's Hilbert code works on bit planes and is heavier.

Timing as tools/serialization_bench.py: warm-up calls, then wall time of `iters` back-to-back calls between two synchronisations,
repeated `repeats` times, the two sides alternating inside each repeat; the median is reported with the spread (min, max) of the
repeats.  Outputs and gradients are compared bit for bit before timing.  One JSON line per (shape, order) to --out
(default profiles/pcm_order/pcm_order_bench.jsonl)."""
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
SHAPES = ((16, 512, 384), (16, 256, 384), (16, 128, 768), (16, 64, 768), (16, 4096, 384))      # (B, N, C): PCM's stages, one larger
ORDERS = ("xyz", "hilbert")
GRID = 0.02


def _window(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e6


def _time_all(fns, iters, warmup, repeats):
    """{name: (median, min, max) us}; the candidates alternate inside every repeat."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            runs[k].append(_window(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def _graph(fn):
    """fn captured after a warm-up on a side stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def bench(B, N, C, order, a, dev):
    import pcm_order_ref as R
    from unipre3d_amd import pcm_order as P
    g = torch.Generator().manual_seed(B * N + C)
    pos = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)                  # the unit cube PCM's clouds are normalised to
    feat, x_res = torch.randn(B, N, C, generator=g).to(dev), torch.randn(B, N, C, generator=g).to(dev)
    dy = torch.randn(B, N, C, generator=g).to(dev)
    depth = int(R.grid_cells(pos, GRID).max()).bit_length()

    def run(ser, backward, **kw):
        # fresh leaves per call, as a layer's activations are: a leaf first used on another stream keeps a gradient accumulator bound
        # to that stream, and a backward captured on a side stream would then synchronise with it inside the capture
        fi, xi = feat.detach().requires_grad_(backward), x_res.detach().requires_grad_(backward)
        p, f, x = ser(pos, fi, xi, order, [], GRID, **kw)
        return (p, f, x) + (torch.autograd.grad([f, x], [fi, xi], [dy, dy]) if backward else ())

    ours, ref = run(P.serialization, True), run(R.serialization, True)
    if not all(torch.equal(u.view(torch.int32), r.view(torch.int32)) for u, r in zip(ours, ref)):
        raise SystemExit(f"B={B} N={N} C={C} {order}: the library and the restatement disagree")
    row = {"row": f"B{B}_N{N}_C{C}_{order}", "B": B, "N": N, "C": C, "order": order, "grid_size": GRID, "depth": depth,
           "baseline": "torch restatement (tests/pcm_order_ref.py)", "iters": a.iters, "repeats": a.repeats}
    for tag, backward in (("fwd", False), ("fwdbwd", True)):
        fns = {"hip": lambda: run(P.serialization, backward),
               "torch_host_read": lambda: run(R.serialization, backward),
               "torch_no_read": lambda: run(R.serialization, backward, depth=depth)}
        print(f"{row['row']} {tag}: capturing the HIP form", file=sys.stderr, flush=True)
        fns["hip_graph"] = _graph(fns["hip"])
        print(f"{row['row']} {tag}: capturing the torch form", file=sys.stderr, flush=True)
        fns["torch_no_read_graph"] = _graph(fns["torch_no_read"])
        print(f"{row['row']} {tag}: timing", file=sys.stderr, flush=True)
        row[f"{tag}_launches_hip"] = 4 + (N * B > P.SMALL_SORT) * 23 + (2 if backward else 1)
        for k, (med, lo, hi) in _time_all(fns, a.iters, a.warmup, a.repeats).items():
            row.update({f"{tag}_{k}_us": round(med, 1), f"{tag}_{k}_min_us": round(lo, 1), f"{tag}_{k}_max_us": round(hi, 1)})
        row[f"{tag}_speedup_eager"] = round(row[f"{tag}_torch_host_read_us"] / row[f"{tag}_hip_us"], 2)
        row[f"{tag}_speedup_graph"] = round(row[f"{tag}_torch_no_read_graph_us"] / row[f"{tag}_hip_graph_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=0, help="only the first ROWS (shape, order) rows; 0 = all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_order", "pcm_order_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcm_order_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        todo = [(s, o) for s in SHAPES for o in ORDERS]
        for (B, N, C), order in todo[:a.rows or None]:
            r = bench(B, N, C, order, a, dev)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
