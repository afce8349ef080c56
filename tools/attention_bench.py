#!/usr/bin/env python3
"""Varlen patch attention (unipre3d_amd.attention) and segment_csr (unipre3d_amd.scatter) at PTv3's shapes: forward and backward
microseconds (wall time of `iters` back-to-back calls between two synchronisations, as tools/sparseconv_bench.py; backward = (forward +
backward) - forward), next to the same work done by torch on the same device in the same run: fp16 softmax(q k^T * scale) v on the
patch-reshaped tensor (whole patches only; torch has no ragged form), its gradient by autograd; for segment_csr, torch.segment_reduce.
frac_hbm is the achieved fraction of 8 TB/s on the algorithmic bytes: forward 8 T H D (read qkv, write out), backward 16 T H D (read
qkv, out, dout; write dqkv).  One JSON line per row to --out (default profiles/attention/attention_bench.jsonl)."""
import argparse
import json
import os
import sys
import time

import torch

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


def _torch_attention(qkv, patch, scale):
    T, _, H, D = qkv.shape
    q, k, v = qkv.reshape(T // patch, patch, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    p = torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1)
    return (p @ v).transpose(1, 2).reshape(T, H, D)


def bench_attention(tokens, H, patch, iters, warmup, dev):
    from unipre3d_amd.attention import flash_attn_varlen_qkvpacked_func as fa
    T, D = tokens // patch * patch, 16
    qkv = torch.randn(T, 3, H, D, device=dev).half().requires_grad_(True)
    dout = torch.randn(T, H, D, device=dev).half()
    cu = torch.arange(0, T + 1, patch, dtype=torch.int32, device=dev)
    scale = D ** -0.5
    with torch.no_grad():
        t_f = _time(lambda: fa(qkv, cu, patch), iters, warmup)
        r_f = _time(lambda: _torch_attention(qkv, patch, scale), iters, warmup)
    t_b = _time(lambda: torch.autograd.grad(fa(qkv, cu, patch), qkv, dout), iters, warmup) - t_f
    r_b = _time(lambda: torch.autograd.grad(_torch_attention(qkv, patch, scale), qkv, dout), iters, warmup) - r_f
    row = {"row": f"attn_T{T}_H{H}_p{patch}", "T": T, "H": H, "D": D, "patch": patch}
    for part, t, r, nbytes in (("fwd", t_f, r_f, 8.0 * T * H * D), ("bwd", t_b, r_b, 16.0 * T * H * D)):
        row.update({f"{part}_us": round(t, 2), f"{part}_torch_us": round(r, 2), f"{part}_speedup": round(r / t, 2),
                    f"{part}_frac_hbm": round(nbytes / (t * 1e-6) / HBM, 4)})
    return row


def bench_segment(N, C, reduce, iters, warmup, dev):
    from unipre3d_amd.scatter import segment_csr
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(1, 9, (N,), generator=g)
    lens = lens[: int((torch.cumsum(lens, 0) <= N).sum())]
    indptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(lens, 0)]).to(dev)
    lens_d = lens.to(dev)
    src = torch.randn(N, C, device=dev, requires_grad=True)
    dout = torch.randn(len(lens), C, device=dev)
    n_cov = int(indptr[-1])
    src_cov = src[:n_cov]
    ref = lambda: torch.segment_reduce(src_cov, reduce, lengths=lens_d, axis=0, unsafe=True)
    with torch.no_grad():
        t_f = _time(lambda: segment_csr(src, indptr, reduce=reduce), iters, warmup)
        r_f = _time(ref, iters, warmup)
    t_b = _time(lambda: torch.autograd.grad(segment_csr(src, indptr, reduce=reduce), src, dout), iters, warmup) - t_f
    r_b = _time(lambda: torch.autograd.grad(ref(), src, dout), iters, warmup) - r_f
    row = {"row": f"segment_csr_{reduce}_N{N}_C{C}", "N": N, "C": C, "segments": len(lens), "reduce": reduce}
    nbytes = 4.0 * C * (N + len(lens))
    for part, t, r in (("fwd", t_f, r_f), ("bwd", t_b, r_b)):
        row.update({f"{part}_us": round(t, 2), f"{part}_torch_us": round(r, 2), f"{part}_speedup": round(r / t, 2),
                    f"{part}_frac_hbm": round(nbytes / (t * 1e-6) / HBM, 4)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention", "attention_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    for tokens in (40_000, 240_000):
        for H, patch in ((2, 48), (4, 48), (8, 48), (16, 48), (32, 48)):
            rows.append(bench_attention(tokens, H, patch, a.iters, a.warmup, dev))
    rows.append(bench_attention(240_000, 4, 1024, a.iters, a.warmup, dev))
    for reduce in ("max", "mean"):
        rows.append(bench_segment(240_000, 64, reduce, a.iters, a.warmup, dev))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
