#!/usr/bin/env python3
"""Selective scan (unipre3d_amd.selective_scan) at Mamba3D's shape (B 32, D 768, L 129) and a PCM-like one (B 8, D 768, L 4096):
forward and backward microseconds (wall time of `iters` back-to-back calls between two synchronisations, as tools/attention_bench.py;
backward = (forward + backward) - forward), and for scale the same inputs through the step loop of the restatement
(tests/selective_scan_ref.py) on the same device (forward only above L 1024: its autograd graph over 4096 steps is not a fair cost).
frac_hbm is the achieved fraction of 8 TB/s on the algorithmic bytes: forward reads u, delta, z, B, C and writes out
(4 (4 B D L + 2 B G N L)); backward reads those and dout and writes du, ddelta, dz, dB, dC (4 (7 B D L + 4 B G N L)).
One JSON line per shape to --out (default profiles/selective_scan/selective_scan_bench.jsonl).  Recorded, not gated."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12
N = 16


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e6


def bench(name, B, D, L, iters, warmup, dev):
    from unipre3d_amd.selective_scan import selective_scan_fn
    import selective_scan_ref as R
    g = lambda *s: torch.randn(*s, device=dev)
    t = {"u": g(B, D, L), "delta": g(B, D, L) - 1.5, "A": -torch.exp(0.3 * g(D, N)) * torch.arange(1, N + 1, device=dev),
         "B": g(B, 1, N, L), "C": g(B, 1, N, L), "D": g(D), "z": g(B, D, L), "delta_bias": 0.5 * g(D)}
    for v in t.values():
        v.requires_grad_(True)
    leaves, dout = list(t.values()), g(B, D, L)
    ours = lambda: selective_scan_fn(**t, delta_softplus=True)
    loop = lambda: R.selective_scan(**t, delta_softplus=True)
    with torch.no_grad():
        t_f = _time(ours, iters, warmup)
        r_f = _time(loop, max(1, iters // 10), 1)
    t_b = _time(lambda: torch.autograd.grad(ours(), leaves, dout), iters, warmup) - t_f
    r_b = _time(lambda: torch.autograd.grad(loop(), leaves, dout), max(1, iters // 10), 1) - r_f if L <= 1024 else None
    row = {"row": name, "B": B, "D": D, "L": L, "G": 1, "N": N}
    for part, us, ref, nbytes in (("fwd", t_f, r_f, 4.0 * (4 * B * D * L + 2 * B * N * L)), ("bwd", t_b, r_b, 4.0 * (7 * B * D * L + 4 * B * N * L))):
        row.update({f"{part}_us": round(us, 2), f"{part}_step_loop_us": None if ref is None else round(ref, 1),
                    f"{part}_frac_hbm": round(nbytes / (us * 1e-6) / HBM, 4)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selective_scan", "selective_scan_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = [bench("mamba3d_B32_D768_L129", 32, 768, 129, a.iters, a.warmup, dev),
            bench("pcm_like_B8_D768_L4096", 8, 768, 4096, a.iters, a.warmup, dev)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
