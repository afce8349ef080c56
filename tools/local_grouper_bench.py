#!/usr/bin/env python3
"""The LocalGrouper of PointMLP and PCM (unipre3d_amd.local_grouper.local_group) against the reference's op-by-op form on the device, from
points held as (B, D, N) to the (B S, C, K) tensor PreExtraction's first convolution reads, at (B, N, S, D, K):

  pointmlp_1 .. 4   (16, 2048, 1024, 64, 32), (16, 1024, 512, 128, 32), (16, 512, 256, 256, 32), (16, 256, 128, 512, 32): PointMLP's four
                    stages at configuration C3's per-GPU batch, normalize = anchor, use_xyz
  pcm_a, pcm_b      (16, 2048, 1024, 48, 24) and (16, 1024, 1024, 96, 24) (S == N, no sampling): PCM-like, normalize = center, no xyz

  hip      local_group(xyz, x.permute(0, 2, 1), fps_idx, idx, alpha, beta, ...) with channels_first=True, then permute(0, 1, 3, 2).reshape
           (-1, C, K), which is a view
  opbyop   LocalGrouper.forward after the search line by line in torch (the two index_points gathers, cat, subtraction, std per batch
           element, division, affine, repeat, cat), then PreExtraction's permute(0, 1, 3, 2).reshape(-1, d, s), which copies

Anchors and neighbours are given to both (the search is not timed).  `forward` runs under no_grad; `fwd_bwd` is the forward and its backward
to x, alpha and beta from a fixed gradient of the (B S, C, K) tensor.  Every figure is taken in two modes: `eager`, a Python loop of `iters`
calls between two device events (the host's cost per call is in it), and `graph`, the same `iters` calls captured once into one graph on
one stream and replayed between the events (the device's cost).  A sample is microseconds per call; the forms are sampled in turn,
`samples` times each after `warmup` calls (or replays), and the median, the minimum and the maximum are kept.
ratio_<mode>_<what> = opbyop / hip on the medians: at or above 1 the HIP kernels are at or below torch's form.
kept_mb: what one forward leaves allocated above the starting level while its result is alive (the result itself included, out_mb);
peak_mb: the peak of one forward + backward above the same level.  max_rel_*: hip against opbyop on this input, max|difference| / max|opbyop|.

One JSON line per shape to --out (default profiles/local_grouper/local_grouper_bench.jsonl).  Recorded, not gated; DESIGN.md and
INTEGRATION.md 5.12 read these lines."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("pointmlp_1", 16, 2048, 1024, 64, 32, "anchor", True), ("pointmlp_2", 16, 1024, 512, 128, 32, "anchor", True),
          ("pointmlp_3", 16, 512, 256, 256, 32, "anchor", True), ("pointmlp_4", 16, 256, 128, 512, 32, "anchor", True),
          ("pcm_a", 16, 2048, 1024, 48, 24, "center", False), ("pcm_b", 16, 1024, 1024, 96, 24, "center", False)]


def opbyop(xyz, points, fps, idx, alpha, beta, mode, use_xyz):
    """The block op by op, as pointmlp.py:160-195 and PreExtraction.forward's first lines (:312-314) run it, on given fps (B, S) and
    idx (B, S, K) int64: advanced-index gathers, cat, subtraction, one std per batch element, division, affine, repeat, cat, and the
    permute + reshape that copies."""
    B, S, K = idx.shape
    b1, b2 = torch.arange(B, device=xyz.device)[:, None], torch.arange(B, device=xyz.device)[:, None, None]
    anchor_xyz, anchor_feat = xyz[b1, fps], points[b1, fps]
    g = points[b2, idx]
    if use_xyz:
        g = torch.cat([g, xyz[b2, idx]], dim=-1)
    if mode == "center":
        m = g.mean(dim=2, keepdim=True)
    else:
        m = (torch.cat([anchor_feat, anchor_xyz], dim=-1) if use_xyz else anchor_feat).unsqueeze(-2)
    sd = torch.std((g - m).reshape(B, -1), dim=-1, keepdim=True).view(B, 1, 1, 1)
    y = alpha * ((g - m) / (sd + 1e-5)) + beta
    out = torch.cat([y, anchor_feat.view(B, S, 1, -1).repeat(1, 1, K, 1)], dim=-1)
    return out.permute(0, 1, 3, 2).reshape(B * S, out.shape[3], K)


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


def bench(name, B, N, S, D, K, mode, use_xyz, iters, samples, warmup, dev):
    from unipre3d_amd import knn, local_grouper as lg, pointops
    g = torch.Generator().manual_seed(N * 31 + D + K)
    Cn = D + (3 if use_xyz else 0)
    C = D + Cn
    xyz = torch.rand(B, N, 3, generator=g).to(dev)
    xd = torch.randn(B, D, N, generator=g).to(dev)
    dout = torch.randn(B * S, C, K, generator=g).to(dev)
    x = xd.clone().requires_grad_(True)
    alpha = (1 + 0.1 * torch.randn(1, 1, 1, Cn, generator=g)).to(dev).requires_grad_(True)
    beta = (0.1 * torch.randn(1, 1, 1, Cn, generator=g)).to(dev).requires_grad_(True)
    if S == N:
        fps, fps64, anchors = None, torch.arange(N, device=dev).expand(B, N).contiguous(), xyz
    else:
        fps = pointops.furthest_point_sample(xyz, S)
        fps64 = fps.long()
        anchors = torch.gather(xyz, 1, fps64.unsqueeze(-1).expand(-1, -1, 3))
    idx = knn.knn_query(K, xyz, anchors)[1]
    idx64 = idx.long()
    forms = {"hip": lambda p: lg.local_group(xyz, p.permute(0, 2, 1), fps, idx, alpha, beta, mode, use_xyz)[1].permute(0, 1, 3, 2).reshape(-1, C, K),
             "opbyop": lambda p: opbyop(xyz, p.permute(0, 2, 1), fps64, idx64, alpha, beta, mode, use_xyz)}

    def fwd(form):
        def body():
            with torch.no_grad():
                return forms[form](xd)
        return body

    def fb(form):
        def body():
            return torch.autograd.grad(forms[form](x), (x, alpha, beta), dout)
        return body

    row = {"shape": name, "B": B, "N": N, "S": S, "D": D, "K": K, "normalize": mode, "use_xyz": use_xyz, "iters": iters, "samples": samples,
           "out_mb": round(B * S * K * C * 4 / 2 ** 20, 1)}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    o_hip, o_ref = fwd("hip")(), fwd("opbyop")()
    assert o_hip.data_ptr() % 16 == 0 and o_hip.is_contiguous()              # the reshape was a view of the (B, S, C, K) storage
    row["max_rel_out"] = rel(o_hip, o_ref)
    for n, a, b in zip(("dpoints", "dalpha", "dbeta"), fb("hip")(), fb("opbyop")()):
        row[f"max_rel_{n}"] = rel(a, b)
    del o_hip, o_ref
    for form in forms:                           # memory: one forward kept alive, then one forward + backward
        for _ in range(2):                       # (the second pass is the measured one)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y = forms[form](x)
            torch.cuda.synchronize()
            kept = torch.cuda.memory_allocated() - base
            grads = torch.autograd.grad(y, (x, alpha, beta), dout)
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
            row[f"ratio_{m}_{what}"] = round(row[f"{m}_opbyop_{what}_us"] / row[f"{m}_hip_{what}_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_grouper", "local_grouper_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("local_grouper_bench.py needs an MI355X: nothing is timed without one")
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
