#!/usr/bin/env python3
"""The group tokenizer (unipre3d_amd.tokenizer.Encoder) against the op-by-op form of unipre3d_amd.standin._Tokenizer (the reference's
lines: Conv1d, BatchNorm1d, ReLU, max, cat through torch) on the same device, in the same process, with the same weights, in training
mode, point_groups (B, G, n, 3) -> (B, G, C), at (B, G, n, C):

  headline  (32, 128, 32, 384)    config C2's per-GPU batch
  half_b    (16, 128, 32, 384)
  half_g    (32, 64, 32, 384)

`forward` runs under no_grad (both forms still take batch statistics and update the running ones); `fwd_bwd` is the forward and its
backward to the twelve parameters from a fixed dout.  Every figure is taken in two modes: `eager`, a Python loop of `iters` calls between
two device events (the host's cost per call is in it), and `graph`, the same `iters` calls captured once into one graph on one stream
and replayed between the events (the device's cost).  A sample is microseconds per call; the forms are sampled in turn, `samples` times
each after `warmup` calls (or replays), and the median, the minimum and the maximum are kept.  ratio_<mode>_<what> = opbyop / hip on the
medians: at or above 1 the HIP kernels are at or below torch's form.  peak_mb_{hip,opbyop}: torch.cuda.max_memory_allocated across one
forward + backward above what was allocated before it.  max_rel_*: hip against opbyop on this input, max|difference| / max|opbyop|.

One JSON line per shape to --out (default profiles/tokenizer/tokenizer_bench.jsonl).  Recorded, not gated; INTEGRATION.md 5.15 reads
these lines."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("headline", 32, 128, 32, 384), ("half_b", 16, 128, 32, 384), ("half_g", 32, 64, 32, 384)]


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
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            body()
    return graph


def make_forms(C, dev):
    from unipre3d_amd import standin, tokenizer
    torch.manual_seed(0)
    hip = tokenizer.Encoder(C).to(dev).train()
    ref = standin._Tokenizer(C).to(dev).train()
    with torch.no_grad():
        for bn in (hip.first_conv[1], hip.second_conv[1]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    ref.first.load_state_dict(hip.first_conv.state_dict())
    ref.second.load_state_dict(hip.second_conv.state_dict())
    return {"hip": hip, "opbyop": ref}


def peak_mb(module, x, dout):
    for _ in range(2):                       # the second pass is the measured one
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        grads = torch.autograd.grad(module(x), list(module.parameters()), dout)
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        del grads
    return round(peak, 1)


def bench(name, B, G, n, C, iters, samples, warmup, dev):
    g = torch.Generator().manual_seed(G * 31 + B + n)
    x = (0.2 * torch.randn(B, G, n, 3, generator=g)).to(dev)
    dout = torch.randn(B, G, C, generator=g).to(dev)
    forms = make_forms(C, dev)

    def fwd(form):
        def body():
            with torch.no_grad():
                return forms[form](x)
        return body

    def fb(form):
        params = list(forms[form].parameters())

        def body():
            return torch.autograd.grad(forms[form](x), params, dout)
        return body

    row = {"shape": name, "B": B, "G": G, "n": n, "C": C, "iters": iters, "samples": samples}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    row["max_rel_out"] = rel(fwd("hip")(), fwd("opbyop")())
    worst = 0.0
    for (k, _), a, b in zip(forms["hip"].named_parameters(), fb("hip")(), fb("opbyop")()):
        if not k.endswith(".bias") or k.endswith("1.bias") or k.endswith("second_conv.3.bias"):   # (the other biases' gradients are zero)
            worst = max(worst, rel(a, b))
    row["max_rel_dparams"] = worst
    for form in forms:
        row[f"peak_mb_{form}"] = peak_mb(forms[form], x, dout)
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
            row[f"ratio_{mode}_{what}"] = round(row[f"{mode}_opbyop_{what}_us"] / row[f"{mode}_hip_{what}_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokenizer", "tokenizer_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tokenizer_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, B, G, n, C in SHAPES:
            if only and name not in only:
                continue
            line = json.dumps(bench(name, B, G, n, C, a.iters, a.samples, a.warmup, dev))
            print(line, flush=True)
            f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
