#!/usr/bin/env python3
"""The fused BatchNorm + activation (+ residual) of unipre3d_amd.batchnorm against torch's own modules (nn.BatchNorm1d(eps=1e-3,
momentum=0.01), then nn.ReLU / nn.GELU, with `+ residual` before the activation for the BasicBlock tail) on the same device, in the
same run, in training mode, on (N, C) fp32 rows:

  relu   (120000, 32) (350000, 32) (60000, 64) (30000, 128) (8000, 256) (120000, 96)
  tail   bn2 + add + relu at (120000, 32) and (350000, 32)
  gelu   (120000, 32)

`forward` runs under no_grad (both forms still take batch statistics and move the running ones); `fwd_bwd` is the forward and its
backward to x, weight, bias (and the residual) from a fixed dy.  Every figure is taken in two modes: `eager`, a Python loop of `iters`
calls between two device events (the host's cost per call is in it), and `graph`, the same calls captured once and replayed (the
device's cost).  A sample is microseconds per call; the forms are sampled in turn, `samples` times each after `warmup` calls, and the
median, minimum and maximum are kept.  ratio_<mode>_<what> = torch / hip on the medians: at or above 1 the HIP kernels are at or below
torch's.  peak_mb_{hip,torch}: torch.cuda.max_memory_allocated across one forward + backward above what was allocated before it.
copy_gbs: a device copy of a 256 MiB fp32 tensor measured in the same process (read + write bytes per second);
fwd_share_of_copy = (x twice + y [+ residual]) bytes / graph forward time / copy_gbs, the share of the copy bandwidth the forward's
unavoidable traffic reaches.  max_rel_*: hip against torch on this input.

Each case runs in a child process of its own under a time limit (--limit seconds); the first one that fails or runs out ends the run.
One JSON line per case to --out (default profiles/batchnorm/batchnorm_bench.jsonl).  Recorded, not gated."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("relu_120k_32", 120000, 32, "relu", False), ("relu_350k_32", 350000, 32, "relu", False), ("relu_60k_64", 60000, 64, "relu", False),
         ("relu_30k_128", 30000, 128, "relu", False), ("relu_8k_256", 8000, 256, "relu", False), ("relu_120k_96", 120000, 96, "relu", False),
         ("tail_120k_32", 120000, 32, "relu", True), ("tail_350k_32", 350000, 32, "relu", True), ("gelu_120k_32", 120000, 32, "gelu", False)]


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


def _copy_gbs(dev):
    a = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    us = statistics.median(_events(lambda: b.copy_(a)) for _ in range(9))
    return 2 * a.numel() * 4 / us / 1e3


def bench(name, N, C, act, residual, iters, samples, warmup, dev):
    from unipre3d_amd import batchnorm
    g = torch.Generator().manual_seed(N + C)
    x = (torch.randn(N, C, generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
    res = torch.randn(N, C, generator=g).to(dev).requires_grad_(True) if residual else None
    dy = torch.randn(N, C, generator=g).to(dev)
    forms = {"hip": batchnorm.BatchNormAct(C, eps=1e-3, momentum=0.01, act=act).to(dev).train(),
             "torch": torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).to(dev).train()}
    with torch.no_grad():
        forms["hip"].weight.uniform_(0.5, 1.5)
        forms["hip"].bias.uniform_(-0.5, 0.5)
    forms["torch"].load_state_dict(forms["hip"].state_dict())
    fn_act = F.relu if act == "relu" else F.gelu

    def call(form):
        if form == "hip":
            return forms["hip"](x, res)
        z = forms["torch"](x)
        return fn_act(z if res is None else z + res)

    def fwd(form):
        def body():
            with torch.no_grad():
                return call(form)
        return body

    def fb(form):
        wrt = [x] + list(forms[form].parameters()) + ([res] if residual else [])
        return lambda: torch.autograd.grad(call(form), wrt, dy)

    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    row = {"case": name, "N": N, "C": C, "act": act, "residual": residual, "iters": iters, "samples": samples}
    row["max_rel_y"] = rel(fwd("hip")(), fwd("torch")())
    row["max_rel_grads"] = max(rel(a, b) for a, b in zip(fb("hip")(), fb("torch")()))
    for form in forms:
        for _ in range(2):
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
        run[f"graph_{key}"] = _captured(body, iters).replay
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
            row[f"ratio_{mode}_{what}"] = round(row[f"{mode}_torch_{what}_us"] / row[f"{mode}_hip_{what}_us"], 2)
    row["copy_gbs"] = round(_copy_gbs(dev), 1)
    nbytes = N * C * 4 * (3 + int(residual))
    for form in forms:
        row[f"fwd_share_of_copy_{form}"] = round(nbytes / row[f"graph_{form}_forward_us"] / 1e3 / row["copy_gbs"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds one case may take")
    ap.add_argument("--only", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--case", default="", help="(internal) run this one case in this process and print its line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batchnorm", "batchnorm_bench.jsonl"))
    a = ap.parse_args()
    if a.case:
        if not torch.cuda.is_available():
            raise SystemExit("batchnorm_bench.py needs an MI355X: nothing is timed without one")
        name, N, C, act, residual = next(c for c in CASES if c[0] == a.case)
        print(json.dumps(bench(name, N, C, act, residual, a.iters, a.samples, a.warmup, torch.device("cuda:0"))), flush=True)
        return
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for case in CASES:
            if only and case[0] not in only:
                continue
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case[0], "--iters", str(a.iters),
                   "--samples", str(a.samples), "--warmup", str(a.warmup)]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                raise SystemExit(f"{case[0]}: exit status {res.returncode}; nothing more is started\n{res.stdout[-2000:]}{res.stderr[-2000:]}")
            line = res.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
