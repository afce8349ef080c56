#!/usr/bin/env python3
"""The object-level image branch, dense against pixel-sparse, on the same device, in the same process, with the same weights:

  dense   torch's GroupNorm and 1x1 Conv2d over the whole decoder map (ImageConv.forward), then fusion.FeatureFusion's z-buffer gather
  sparse  image_fusion.sample_at_points, which is what image_fusion.FeatureFusion runs for ImageConv.deferred(map): one statistics pass
          over the map, the z-buffer gather of the raw map, then normalisation and convolution on the B N gathered rows
          (libunipre3d_image_fusion.so)

Both end in the (B, N, 2 Cout) tensor the fusion MLP reads (x is (B, N, Cout); the camera-space points are computed once, outside), at
(B, Cin, Cout, H, N):

  transformer (32, 128, 384, 128, 128)   the reference's object config
  c2          (32, 128, 384, 256, 128)   BASELINE C2
  pointmlp    (16, 128, 128, 256, 1024)  PointMLP fuses after its LAST decoder stage (pointmlp.py:599-615), which is back at the input
                                         resolution: the 1024 points of the ShapeNet object config
  eval        (1, 128, 384, 128, 128)    evaluation: every group of the single image is cut over 8 workgroups

`forward` runs under no_grad; `fwd_bwd` is the forward and its backward to the four parameters of image_conv from a fixed cotangent (the
map is frozen, as the VAE is).  Every figure is taken in two modes: `eager`, a Python loop of `iters` calls between two device events, and
`graph`, the same calls captured once into one graph on one stream and replayed between the events.  A sample is microseconds per call;
the forms are sampled in turn, `samples` times each after `warmup` calls, and the median, minimum and maximum are kept.
ratio_<mode>_<what> = dense / sparse on the medians.  peak_mb_*: torch.cuda.max_memory_allocated across one forward + backward above what
was allocated before it (the map itself is allocated before).  stats_bytes: the bytes the statistics kernel reads, from the shape;
--stats-only runs nothing but group_stats a few times, for a kernel trace of its own to take the kernel's time from.

One JSON line per shape to --out (default profiles/image_fusion/image_fusion_bench.jsonl).  Recorded, not gated."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("transformer", 32, 128, 384, 128, 128), ("c2", 32, 128, 384, 256, 128), ("pointmlp", 16, 128, 128, 256, 1024),
          ("eval", 1, 128, 384, 128, 128)]


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _captured(body, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            body()
    return graph


def scene(B, N, H, dev):
    """points in a cube in front of a camera two units away, the reference's field of view: most land inside the image"""
    g = torch.Generator().manual_seed(N + H)
    center = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev)
    c2w = torch.eye(4).repeat(B, 1, 1)
    c2w[:, :3, 3] = torch.tensor([0.0, 0.0, -2.0])
    focal = (H / 2.0) / math.tan(math.radians(49.13434264120263 / 2.0))
    intr = [[focal, 0.0, H / 2.0, 0.0], [0.0, focal, H / 2.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    return center, c2w.transpose(1, 2).contiguous().to(dev), intr


def bench(name, B, Cin, Cout, H, N, iters, samples, warmup, dev):
    from unipre3d_amd import fusion, image_fusion
    torch.manual_seed(0)
    conv = image_fusion.ImageConv(Cin, Cout).to(dev)
    with torch.no_grad():
        conv[0].weight.uniform_(0.5, 1.5)
        conv[0].bias.uniform_(-0.5, 0.5)
    params = list(conv.parameters())
    g = torch.Generator().manual_seed(B + H)
    xmap = torch.randn(B, Cin, H, H, generator=g).to(dev)
    x = torch.randn(B, N, Cout, generator=g).to(dev)
    cot = torch.randn(B, N, 2 * Cout, generator=g).to(dev)
    center, c2w, intr = scene(B, N, H, dev)
    # the world-to-camera product is shared and done once: torch.linalg.inv reads its status back on the host and cannot be captured
    cp = fusion.FeatureFusion.camera_points(center, c2w).contiguous()
    fxy = (intr[0][0], intr[1][1], intr[0][2], intr[1][2])
    forms = {"dense": lambda: torch.cat([x, fusion._ZBufferGather.apply(cp, conv(xmap), *fxy)[0]], dim=-1),
             "sparse": lambda: torch.cat([x, image_fusion.sample_at_points(conv, xmap, cp, *fxy)[0]], dim=-1)}

    def fwd(form):
        def body():
            with torch.no_grad():
                return forms[form]()
        return body

    def fb(form):
        return lambda: torch.autograd.grad(forms[form](), params, cot)

    row = {"shape": name, "B": B, "Cin": Cin, "Cout": Cout, "H": H, "N": N, "iters": iters, "samples": samples,
           "stats_bytes": B * Cin * H * H * 4, "dense_output_bytes": B * Cout * H * H * 4}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    yd, ys = fwd("dense")(), fwd("sparse")()
    row["winner_rows"] = int((ys[..., Cout:] != 0).any(-1).sum())
    row["max_rel_out"] = rel(ys, yd)
    row["max_rel_dparams"] = max(rel(a, b) for a, b in zip(fb("sparse")(), fb("dense")()))
    del yd, ys
    for form in forms:
        for _ in range(2):                   # the second pass is the measured one
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            grads = fb(form)()
            torch.cuda.synchronize()
            row[f"peak_mb_{form}"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            del grads
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
        row.update({f"{k}_us": round(statistics.median(v), 1), f"{k}_us_min": round(min(v), 1), f"{k}_us_max": round(max(v), 1)})
    for mode in ("eager", "graph"):
        for what in ("forward", "fwd_bwd"):
            row[f"ratio_{mode}_{what}"] = round(row[f"{mode}_dense_{what}_us"] / row[f"{mode}_sparse_{what}_us"], 2)
    return row


def stats_only(dev, reps):
    from unipre3d_amd import image_fusion
    for name, B, Cin, _, H, _ in SHAPES:
        xmap = torch.randn(B, Cin, H, H, device=dev)
        for _ in range(reps):
            image_fusion.group_stats(xmap, 32, 1e-6)
        torch.cuda.synchronize()
        print(json.dumps({"shape": name, "stats_bytes": B * Cin * H * H * 4, "launches": reps}), flush=True)
        del xmap
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--stats-only", type=int, default=0, metavar="REPS", help="run only the statistics pass REPS times per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_fusion", "image_fusion_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_fusion_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    if a.stats_only:
        return stats_only(dev, a.stats_only)
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, B, Cin, Cout, H, N in SHAPES:
            if only and name not in only:
                continue
            line = json.dumps(bench(name, B, Cin, Cout, H, N, a.iters, a.samples, a.warmup, dev))
            print(line, flush=True)
            f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
