#!/usr/bin/env python3
"""Causal conv1d (unipre3d_amd.causal_conv1d) and fused add + norm (unipre3d_amd.layernorm) at Mamba3D's shapes (conv B 32, D 768,
L 129, W 4; norm M 4128, N 384) and PCM-like ones (conv B 8, D 768, L 4096; norm M 32768, N 384): forward and backward microseconds
(wall time of `iters` back-to-back calls between two synchronisations, as tools/selective_scan_bench.py; backward = (forward +
backward) - forward), and in the same run on the same device the torch composition each one replaces:
  conv: x = xz.chunk(2, dim=1)[0]; F.silu(F.conv1d(x.contiguous(), w, b, padding=W-1, groups=D)[..., :L]), the composition
        mamba_inner_fn_no_out_proj ran before (dense copy of the view, padded grouped conv, slice, SiLU);
  norm: r = x + residual, then F.layer_norm(r), or r * rsqrt(mean(r^2) + eps) * w for RMSNorm; returns (y, r) as the blocks use it.
frac_hbm is the achieved fraction of 8 TB/s on the algorithmic bytes: conv forward reads x and writes out (8 B D L), backward reads x
and dout and writes dx (12 B D L); norm forward reads x and residual and writes y and r (16 M N), backward reads dy, dr and r and writes
dx (16 M N).  One JSON line per shape ({"row", "conv", "rms_norm", "layer_norm"}) to --out (default
profiles/mambaops/mambaops_bench.jsonl).  Recorded, not gated; the conv entries decide whether mamba_inner_fn* calls the HIP conv
(DESIGN.md)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e6


def _pair(ours, torch_fn, leaves, douts, iters, warmup):
    """(ours fwd, ours bwd, torch fwd, torch bwd) in microseconds; the two are timed alternately, twice, and the lower figure kept."""
    def both(fn):
        outs = fn()
        return torch.autograd.grad(outs if isinstance(outs, tuple) else (outs,), leaves, douts)
    best = [float("inf")] * 4
    for _ in range(2):
        with torch.no_grad():
            f_o, f_t = _time(ours, iters, warmup), _time(torch_fn, iters, warmup)
        fb_o, fb_t = _time(lambda: both(ours), iters, warmup), _time(lambda: both(torch_fn), iters, warmup)
        best = [min(a, b) for a, b in zip(best, (f_o, fb_o - f_o, f_t, fb_t - f_t))]
    return best


def _row(row, times, fwd_bytes, bwd_bytes):
    f_o, b_o, f_t, b_t = times
    row.update({"fwd_us": round(f_o, 2), "bwd_us": round(b_o, 2), "fwd_torch_us": round(f_t, 2), "bwd_torch_us": round(b_t, 2),
                "fwd_frac_hbm": round(fwd_bytes / (f_o * 1e-6) / HBM, 4), "bwd_frac_hbm": round(bwd_bytes / (b_o * 1e-6) / HBM, 4),
                "fwd_bwd_us": round(f_o + b_o, 2), "fwd_bwd_torch_us": round(f_t + b_t, 2)})
    return row


def bench_conv(B, D, L, W, iters, warmup, dev):
    from unipre3d_amd.causal_conv1d import causal_conv1d_fn
    xz = torch.randn(B, 2 * D, L, device=dev, requires_grad=True)
    w = (0.5 * torch.randn(D, 1, W, device=dev)).requires_grad_(True)
    b = (0.1 * torch.randn(D, device=dev)).requires_grad_(True)
    dout = torch.randn(B, D, L, device=dev)
    ours = lambda: causal_conv1d_fn(xz.chunk(2, dim=1)[0], w.reshape(D, W), b, "silu")
    comp = lambda: F.silu(F.conv1d(xz.chunk(2, dim=1)[0].contiguous(), w, b, padding=W - 1, groups=D)[..., :L])
    with torch.no_grad():
        err = float((ours() - comp()).abs().max())
    n = 4.0 * B * D * L
    return _row({"op": "causal_conv1d_silu", "B": B, "D": D, "L": L, "W": W, "max_abs_diff_vs_torch": err},
                _pair(ours, comp, (xz, w, b), (dout,), iters, warmup), 2 * n, 3 * n)


def bench_norm(M, N, is_rms, iters, warmup, dev):
    from unipre3d_amd.layernorm import layer_norm_fn
    x = torch.randn(M, N, device=dev, requires_grad=True)
    res = torch.randn(M, N, device=dev, requires_grad=True)
    w = (1.0 + 0.1 * torch.randn(N, device=dev)).requires_grad_(True)
    b = None if is_rms else (0.1 * torch.randn(N, device=dev)).requires_grad_(True)
    eps = 1e-5
    dy, dr = torch.randn(M, N, device=dev), torch.randn(M, N, device=dev)
    ours = lambda: layer_norm_fn(x, w, b, res, eps, True, True, is_rms)

    def comp():
        r = x + res
        return (r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w if is_rms else F.layer_norm(r, (N,), w, b, eps)), r
    with torch.no_grad():
        err = float((ours()[0] - comp()[0]).abs().max())
    n = 4.0 * M * N
    leaves = (x, res, w) if is_rms else (x, res, w, b)
    return _row({"op": "add_rms_norm" if is_rms else "add_layer_norm", "M": M, "N": N, "max_abs_diff_vs_torch": err},
                _pair(ours, comp, leaves, (dy, dr), iters, warmup), 4 * n, 4 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mambaops", "mambaops_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mambaops_bench.py needs an MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    for name, conv, norm in (("mamba3d", (32, 768, 129, 4), (4128, 384)), ("pcm_like", (8, 768, 4096, 4), (32768, 384))):
        rows.append({"row": name, "conv": bench_conv(*conv, a.iters, a.warmup, dev),
                     "rms_norm": bench_norm(*norm, True, a.iters, a.warmup, dev),
                     "layer_norm": bench_norm(*norm, False, a.iters, a.warmup, dev)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
