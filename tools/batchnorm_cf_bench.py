#!/usr/bin/env python3
"""The channels-first fused BatchNorm + activation (+ residual) (+ max over the neighbours) of unipre3d_amd.batchnorm_cf against torch's
own modules (nn.BatchNorm1d, `+ residual`, nn.ReLU, F.adaptive_max_pool1d) on the same device, in the same run, in training mode, fp32:

  pre<i>_relu | pre<i>_tail | pre<i>_tail_max   the (B S, C, K) tensor of PreExtraction at pointmlp_<i> of tools/local_grouper_bench.py with
                                                C = 2 D: (16384, 128, 32), (8192, 256, 32), (4096, 512, 32), (2048, 1024, 32);
                                                BN + relu, BN + residual + relu, BN + residual + relu + max over K
  pos<i>_tail                                   the matching PosExtraction tensor (B, C, S): (16, 128, 1024) ... (16, 1024, 128)
  embed_relu                                    the embedding (16, 64, 2048)
  module_pre | module_pos                       one whole PreExtraction(64, 128, blocks=2, bias=False, use_xyz=False) on (16, 1024, 32, 128)
                                                and one whole PosExtraction(128, blocks=2, bias=False) on (16, 128, 1024), convolutions
                                                included: the op-by-op classes against the same module after fuse_pointmlp_blocks

`forward` runs under no_grad (both forms still take batch statistics and move the running ones); `fwd_bwd` is the forward and its
backward to the input and every parameter (and the residual) from a fixed gradient.  Every figure is taken in two modes: `eager`, a
Python loop of `iters` calls between two device events (the host's cost per call is in it), and `graph`, the same calls captured once
and replayed (the device's cost).  A sample is microseconds per call; the forms are sampled in turn, `samples` times each after
`warmup` calls, and the median, minimum and maximum are kept.  ratio_<mode>_<what> = torch / hip on the medians: at or above 1 the HIP
kernels are at or below torch's.  peak_mb_{hip,torch}: torch.cuda.max_memory_allocated across one forward + backward above what was
allocated before it.  max_rel_*: hip against torch on this input.

Each case runs in a child process of its own under a time limit (--limit seconds); the first one that fails or runs out ends the run.
One JSON line per case to --out (default profiles/batchnorm_cf/batchnorm_cf_bench.jsonl).  Recorded, not gated."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batchnorm_bench import _captured, _events  # noqa: E402  (the protocol is that tool's)

PRE = [(16384, 128, 32), (8192, 256, 32), (4096, 512, 32), (2048, 1024, 32)]
POS = [(16, 128, 1024), (16, 256, 512), (16, 512, 256), (16, 1024, 128)]
# name: (shape (B, C, L), residual, pool, pool_groups)
CASES = {}
for i, (shape, pos) in enumerate(zip(PRE, POS), 1):
    CASES[f"pre{i}_relu"] = (shape, False, False, 1)
    CASES[f"pre{i}_tail"] = (shape, True, False, 1)
    CASES[f"pre{i}_tail_max"] = (shape, True, True, pos[2])
    CASES[f"pos{i}_tail"] = (pos, True, False, 1)
CASES["embed_relu"] = ((16, 64, 2048), False, False, 1)
MODULES = {"module_pre": ("PreExtraction", (128, 128), (16, 1024, 32, 128)), "module_pos": ("PosExtraction", (128,), (16, 128, 1024))}


def _norm_forms(name, dev):
    from unipre3d_amd import batchnorm_cf
    (B, C, L), residual, pool, S = CASES[name]
    g = torch.Generator().manual_seed(B + C + L)
    x = (torch.randn(B, C, L, generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
    res = torch.randn(B, C, L, generator=g).to(dev).requires_grad_(True) if residual else None
    dy = torch.randn((B // S, C, S) if pool else (B, C, L), generator=g).to(dev)
    norms = {"hip": batchnorm_cf.BatchNormActCF(C, act="relu").to(dev).train(), "torch": torch.nn.BatchNorm1d(C).to(dev).train()}
    with torch.no_grad():
        norms["hip"].weight.uniform_(0.5, 1.5)
        norms["hip"].bias.uniform_(-0.5, 0.5)
    norms["torch"].load_state_dict(norms["hip"].state_dict())

    def call(form):
        if form == "hip":
            return norms["hip"](x, res, "max" if pool else None, S)
        z = norms["torch"](x)
        z = F.relu(z if res is None else z + res)
        if pool:                                                  # the reference's lines: max over K, then (b, n, d) -> (b, d, n)
            z = F.adaptive_max_pool1d(z, 1).view(B, -1).reshape(B // S, S, -1).permute(0, 2, 1)
        return z
    wrt = {form: [x] + list(norms[form].parameters()) + ([res] if residual else []) for form in norms}
    return call, wrt, dy, dict(shape=[B, C, L], residual=residual, pool=pool, pool_groups=S)


def _module_forms(name, dev):
    import batchnorm_cf_ref
    from unipre3d_amd import batchnorm_cf
    kind, args, shape = MODULES[name]
    torch.manual_seed(7)
    plain = batchnorm_cf_ref.reference_classes()[kind](*args, blocks=2, bias=False).to(dev).train()
    holder = torch.nn.Sequential(copy.deepcopy(plain))
    assert batchnorm_cf.fuse_pointmlp_blocks(holder) == 1
    mods = {"hip": holder[0], "torch": plain}
    g = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
    with torch.no_grad():
        dy = torch.randn(plain(x).shape, generator=g).to(dev)
    plain.load_state_dict(holder[0].state_dict())                 # (the probe call moved the op-by-op form's buffers)
    wrt = {form: [x] + list(mods[form].parameters()) for form in mods}
    return (lambda form: mods[form](x)), wrt, dy, dict(shape=list(shape), kind=kind)


def bench(name, iters, samples, warmup, dev):
    call, wrt, dy, row = (_module_forms if name in MODULES else _norm_forms)(name, dev)
    row = dict(case=name, iters=iters, samples=samples, **row)
    forms = ("hip", "torch")

    def fwd(form):
        def body():
            with torch.no_grad():
                return call(form)
        return body

    def fb(form):
        return lambda: torch.autograd.grad(call(form), wrt[form], dy)

    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
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
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds one case may take")
    ap.add_argument("--only", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--case", default="", help="(internal) run this one case in this process and print its line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batchnorm_cf", "batchnorm_cf_bench.jsonl"))
    a = ap.parse_args()
    names = list(CASES) + list(MODULES)
    if a.case:
        if not torch.cuda.is_available():
            raise SystemExit("batchnorm_cf_bench.py needs an MI355X: nothing is timed without one")
        print(json.dumps(bench(a.case, a.iters, a.samples, a.warmup, torch.device("cuda:0"))), flush=True)
        return
    only = set(filter(None, a.only.split(",")))
    assert only <= set(names), sorted(only - set(names))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for case in names:
            if only and case not in only:
                continue
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case, "--iters", str(a.iters),
                   "--samples", str(a.samples), "--warmup", str(a.warmup)]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                raise SystemExit(f"{case}: exit status {res.returncode}; nothing more is started\n{res.stdout[-2000:]}{res.stderr[-2000:]}")
            line = res.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
