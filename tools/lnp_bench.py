#!/usr/bin/env python3
"""Mamba3D's local norm pooling (unipre3d_amd.lnp.local_norm_pool) against the reference's op-by-op form on the device, x (B, G, C) ->
(B, G, 2C), at (B, G, C, K):

  c2_k4     (32, 128, 384, 4)    config C2's per-GPU batch at the reference's center_local_k
  c2_k8     (32, 128, 384, 8)
  small_k4  (8, 128, 384, 4)

  hip          local_norm_pool(x, nb, alpha, beta) with nb = lnp.neighbours(center, K) built once, outside the timed call
  opbyop       GroupFeature's gather, K_Norm and K_Pool line by line in torch (the reference's permutes included), neighbour indices given
  opbyop_knn   the same with the search inside, as the reference runs it in every block (the search is unipre3d_amd.knn's: knn_cuda is
               not part of the reference tree)

`forward` runs under no_grad; `fwd_bwd` is the forward and its backward to x, alpha and beta from a fixed dout.  Every figure is taken in
two modes: `eager`, a Python loop of `iters` calls between two device events (the host's cost per call is in it), and `graph`, the same
`iters` calls captured once into one graph on one stream and replayed between the events (the device's cost).  A sample is microseconds
per call; the forms are sampled in turn, `samples` times each after `warmup` calls (or replays), and the median, the minimum and the
maximum are kept.  ratio_<mode>_<what> = opbyop / hip and ratio_knn_<mode>_<what> = opbyop_knn / hip on the medians: at or above 1 the
HIP kernels are at or below torch's form.  neighbours_us: one lnp.neighbours(center, K) call (search + inverse lists), eager, which the
hip form pays once per model forward.  max_rel_*: hip against opbyop on this input, max|difference| / max|opbyop|.

peak_mb_16_blocks (c2_k8 only): peak allocated memory, above what is allocated before, of 16 chained blocks forward + backward -- each block
the form and a Linear(2C, C) -- for hip and opbyop: what is kept between forward and backward.

One JSON line per shape to --out (default profiles/lnp/lnp_bench.jsonl).  Recorded, not gated; INTEGRATION.md 5.11 reads these lines."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("c2_k4", 32, 128, 384, 4), ("c2_k8", 32, 128, 384, 8), ("small_k4", 8, 128, 384, 4)]


def opbyop(x, idx, alpha, beta):
    """Mamba3D.py:148-259 on a given idx (B, G, K) int64."""
    B, G, C = x.shape
    K = idx.shape[2]
    flat = (idx + torch.arange(0, B, device=x.device).view(-1, 1, 1) * G).view(-1)
    knn_x = x.contiguous().view(-1, C)[flat, :].view(B, G, K, C).contiguous()
    mean_x = x.unsqueeze(dim=-2)
    std_x = torch.std(knn_x - mean_x)
    knn_x = (knn_x - mean_x) / (std_x + 1e-5)
    knn_x = torch.cat([knn_x, x.reshape(B, G, 1, -1).repeat(1, 1, K, 1)], dim=-1)
    w = (alpha.view(1, 1, 1, -1) * knn_x + beta.view(1, 1, 1, -1)).permute(0, 3, 1, 2)
    e_x = torch.exp(w)
    return torch.div((w * e_x).mean(-1), e_x.mean(-1)).permute(0, 2, 1)


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


def make_forms(center, K):
    from unipre3d_amd import knn, lnp
    nb = lnp.neighbours(center, K)
    idx64 = nb.idx.long()
    search = knn.KNN(k=K, transpose_mode=True)
    return {"hip": lambda x, a, b: lnp.local_norm_pool(x, nb, a, b),
            "opbyop": lambda x, a, b: opbyop(x, idx64, a, b),
            "opbyop_knn": lambda x, a, b: opbyop(x, search(center, center)[1], a, b)}


def bench(name, B, G, C, K, iters, samples, warmup, dev):
    from unipre3d_amd import lnp
    g = torch.Generator().manual_seed(G * 31 + B + K)
    center = torch.rand(B, G, 3, generator=g).to(dev)
    xd = torch.randn(B, G, C, generator=g).to(dev)
    dout = torch.randn(B, G, 2 * C, generator=g).to(dev)
    x = xd.clone().requires_grad_(True)
    alpha = (1 + 0.1 * torch.randn(2 * C, generator=g)).to(dev).requires_grad_(True)
    beta = (0.1 * torch.randn(2 * C, generator=g)).to(dev).requires_grad_(True)
    forms = make_forms(center, K)

    def fwd(form):
        def body():
            with torch.no_grad():
                return forms[form](xd, alpha, beta)
        return body

    def fb(form):
        def body():
            return torch.autograd.grad(forms[form](x, alpha, beta), (x, alpha, beta), dout)
        return body

    row = {"shape": name, "B": B, "G": G, "C": C, "K": K, "iters": iters, "samples": samples}
    o_ref, g_ref = fwd("opbyop")(), fb("opbyop")()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    row["max_rel_out"] = rel(fwd("hip")(), o_ref)
    for n, a, b in zip(("dx", "dalpha", "dbeta"), fb("hip")(), g_ref):
        row[f"max_rel_{n}"] = rel(a, b)
    bodies = {f"{form}_{what}": mk(form) for what, mk in (("forward", fwd), ("fwd_bwd", fb)) for form in forms}
    run = {"eager_neighbours": lambda: [lnp.neighbours(center, K) for _ in range(iters)]}
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
    for mode in ("eager", "graph"):
        for what in ("forward", "fwd_bwd"):
            row[f"ratio_{mode}_{what}"] = round(row[f"{mode}_opbyop_{what}_us"] / row[f"{mode}_hip_{what}_us"], 2)
            row[f"ratio_knn_{mode}_{what}"] = round(row[f"{mode}_opbyop_knn_{what}_us"] / row[f"{mode}_hip_{what}_us"], 2)
    return row


def peak_16_blocks(B, G, C, K, dev):
    """Peak allocated MB above the starting level of 16 chained blocks (the form, then a Linear(2C, C)), forward + backward."""
    out = {}
    torch.manual_seed(0)
    lin = [torch.nn.Linear(2 * C, C).to(dev) for _ in range(16)]
    par = [(torch.ones(2 * C, device=dev, requires_grad=True), torch.zeros(2 * C, device=dev, requires_grad=True)) for _ in range(16)]
    x0 = torch.randn(B, G, C, device=dev)
    forms = make_forms(torch.rand(B, G, 3, device=dev), K)
    for form in ("hip", "opbyop"):
        for _ in range(2):                       # the second pass is the measured one
            for p in [p for m in lin for p in m.parameters()] + [p for ab in par for p in ab]:
                p.grad = None
            x = x0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y = x
            for m, (a, b) in zip(lin, par):
                y = m(forms[form](y, a, b))
            y.sum().backward()
            torch.cuda.synchronize()
            out[form] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            del y, x
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lnp", "lnp_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lnp_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, B, G, C, K in SHAPES:
            if only and name not in only:
                continue
            row = bench(name, B, G, C, K, a.iters, a.samples, a.warmup, dev)
            if name == "c2_k8":
                row["peak_mb_16_blocks"] = peak_16_blocks(B, G, C, K, dev)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
