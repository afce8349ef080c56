#!/usr/bin/env python3
"""Dense fp32 attention (unipre3d_amd.mha.attention_qkvpacked) against torch's two on-device forms of the same core, on the packed qkv a
Linear produces, at (B, N, H, 64):

  c2        (32, 129, 6, 64)    config C2's per-GPU batch: 128 groups + cls per object
  small     (8, 129, 6, 64)
  n257      (32, 257, 6, 64)

  hip       attention_qkvpacked(qkv)                                   (B, N, 3, H, 64) -> (B, N, H, 64)
  opbyop    the reference's form: permute, q @ k^T, * scale, softmax, attn @ v, transpose(1, 2).reshape
  sdpa      F.scaled_dot_product_attention on the permuted views, then transpose(1, 2).reshape (what standin.py runs)

`forward` runs under no_grad; `fwd_bwd` is the forward and its backward to qkv from a fixed dout.  Every figure is taken in two modes:
`eager`, a Python loop of `iters` calls between two device events (the host's cost per call is in it: autograd.Function over ctypes
for hip, the dispatcher for torch), and `graph`, the same `iters` calls captured once into one graph on one stream and replayed between
the events (the device's cost).  A sample is microseconds per call; the forms are sampled in turn, `samples` times each after `warmup`
calls (or replays), and the median, the minimum and the maximum are kept.  ratio_<mode>_<what> = min(opbyop, sdpa) / hip on the
medians: at or above 1 the HIP kernels are at or below torch's better form.  max_rel_out / max_rel_dqkv: hip against opbyop on this
input, max|difference| / max|opbyop|.

peak_mb_16_blocks (c2 only): peak allocated memory, above what is allocated before, of 16 chained blocks forward + backward -- each
block a Linear(384, 1152), the attention form and a Linear(384, 384) -- for the three forms: what is kept between forward and backward.

One JSON line per shape to --out (default profiles/mha/mha_bench.jsonl).  Recorded, not gated; INTEGRATION.md 5.10 reads these lines."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("c2", 32, 129, 6), ("small", 8, 129, 6), ("n257", 32, 257, 6)]
D = 64


def opbyop(qkv):
    B, N, _, H, _ = qkv.shape
    p = qkv.permute(2, 0, 3, 1, 4)
    attn = ((p[0] @ p[1].transpose(-2, -1)) * D ** -0.5).softmax(dim=-1)
    return (attn @ p[2]).transpose(1, 2).reshape(B, N, H * D)


def sdpa(qkv):
    B, N, _, H, _ = qkv.shape
    p = qkv.permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(p[0], p[1], p[2]).transpose(1, 2).reshape(B, N, H * D)


def hip(qkv):
    from unipre3d_amd import mha
    B, N, _, H, _ = qkv.shape
    return mha.attention_qkvpacked(qkv).view(B, N, H * D)


FORMS = {"hip": hip, "opbyop": opbyop, "sdpa": sdpa}


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


def bench(name, B, N, H, iters, samples, warmup, dev):
    g = torch.Generator().manual_seed(N * 31 + B)
    qkv = torch.randn(B, N, 3, H, D, generator=g).to(dev)
    dout = torch.randn(B, N, H * D, generator=g).to(dev)
    x = qkv.clone().requires_grad_(True)

    def fwd(form):
        def body():
            with torch.no_grad():
                return FORMS[form](qkv)
        return body

    def fb(form):
        def body():
            return torch.autograd.grad(FORMS[form](x), x, dout)[0]
        return body

    row = {"shape": name, "B": B, "N": N, "H": H, "D": D, "iters": iters, "samples": samples}
    o_ref, g_ref = fwd("opbyop")(), fb("opbyop")()
    row["max_rel_out"] = float((fwd("hip")() - o_ref).abs().max() / o_ref.abs().max())
    row["max_rel_dqkv"] = float((fb("hip")() - g_ref).abs().max() / g_ref.abs().max())
    bodies = {f"{form}_{what}": mk(form) for what, mk in (("forward", fwd), ("fwd_bwd", fb)) for form in FORMS}
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
    for mode in ("eager", "graph"):
        for what in ("forward", "fwd_bwd"):
            best = min(row[f"{mode}_opbyop_{what}_us"], row[f"{mode}_sdpa_{what}_us"])
            row[f"ratio_{mode}_{what}"] = round(best / row[f"{mode}_hip_{what}_us"], 2)
    return row


def peak_16_blocks(B, N, H, dev):
    """Peak allocated MB above the starting level of 16 chained blocks (qkv Linear, the form, proj Linear), forward + backward."""
    C, out = H * D, {}
    torch.manual_seed(0)
    lin = [(torch.nn.Linear(C, 3 * C, bias=False).to(dev), torch.nn.Linear(C, C).to(dev)) for _ in range(16)]
    x0 = torch.randn(B, N, C, device=dev)
    for form, fn in FORMS.items():
        for _ in range(2):                       # the second pass is the measured one
            for p in (p for pair in lin for m in pair for p in m.parameters()):
                p.grad = None
            x = x0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y = x
            for qkv_l, proj_l in lin:
                y = proj_l(fn(qkv_l(y).view(B, N, 3, H, D)))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mha", "mha_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mha_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, B, N, H in SHAPES:
            if only and name not in only:
                continue
            row = bench(name, B, N, H, a.iters, a.samples, a.warmup, dev)
            if name == "c2":
                row["peak_mb_16_blocks"] = peak_16_blocks(B, N, H, dev)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
