#!/usr/bin/env python3
"""PSNR / SSIM (unipre3d_amd.metrics) against torch's own on-device form of the same call, at the image stacks the evaluation loop sees:

  object_eval    128 x (3, 128, 128)    object-level validation batch
  c2             128 x (3, 256, 256)    config C2
  scene          8 x (3, 120, 160)      scene-level config
  c4_c5          16 x (3, 480, 640)     configs C4 / C5

The torch form is the reference's `_ssim` written out here (utils/loss_utils.py:47-87: five grouped conv2d calls with the 121-tap 2-D
window, per-image mean) plus the PSNR line of eval.py:28-30 per image; `forward` is what image_metrics computes (SSIM and PSNR per
image, no gradient), `fwd_bwd` is ssim(img1, img2) and its backward to img1.

Method.  Device events around `iters` back-to-back calls give one sample (microseconds per call); the forms are sampled in turn,
`samples` times each after `warmup` calls, and the median, the minimum and the maximum of the samples are kept.  ratio_* is
median(torch form) / median(HIP): above 1 the HIP kernels are faster.  hbm_fraction_forward is the least traffic of the forward,
2 * N * C * H * W * 4 bytes (both stacks read once), over the HIP forward's median time, as a share of the 8.0 TB/s HBM3E peak:
a whole-call figure (tile kernel, reduce kernel and the PSNR arithmetic in torch), not a kernel's share.  max_abs_ssim / max_abs_psnr:
the two forms' results on this input, compared.  One JSON line per stack to --out (default profiles/metrics/metrics_bench.jsonl).
Recorded, not gated; INTEGRATION.md's switch-over note reads these lines."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("object_eval", 128, 3, 128, 128), ("c2", 128, 3, 256, 256), ("scene", 8, 3, 120, 160), ("c4_c5", 16, 3, 480, 640)]
HBM_PEAK = 8.0e12


def window(channel, dev):
    g = torch.Tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().expand(channel, 1, 11, 11).contiguous().to(dev)


def torch_ssim(a, b, win):
    c = a.size(1)
    mu1, mu2 = F.conv2d(a, win, padding=5, groups=c), F.conv2d(b, win, padding=5, groups=c)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(a * a, win, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(b * b, win, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(a * b, win, padding=5, groups=c) - mu12
    m = ((2 * mu12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m.mean((1, 2, 3))


def torch_psnr(a, b):
    return -10 * torch.log10(((a - b) ** 2).mean((1, 2, 3)))


def _sample(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench(name, N, C, H, W, iters, samples, warmup, dev):
    from unipre3d_amd import metrics
    g = torch.Generator().manual_seed(H * 31 + N)
    a = torch.rand(N, C, H, W, generator=g).to(dev)
    b = (a + 0.05 * torch.randn(N, C, H, W, generator=g).to(dev)).clamp(0, 1)
    win = window(C, dev)
    x = a.clone().requires_grad_(True)

    def hip_fwd():
        return metrics.image_metrics(a, b)

    def torch_fwd():
        with torch.no_grad():
            return {"ssim": torch_ssim(a, b, win), "psnr": torch_psnr(a, b)}

    def hip_fb():
        x.grad = None
        metrics.ssim(x, b).backward()

    def torch_fb():
        x.grad = None
        torch_ssim(x, b, win).mean().backward()

    forms = {"hip_forward": hip_fwd, "torch_forward": torch_fwd, "hip_fwd_bwd": hip_fb, "torch_fwd_bwd": torch_fb}
    h, t = hip_fwd(), torch_fwd()
    row = {"stack": name, "N": N, "C": C, "H": H, "W": W, "iters": iters, "samples": samples,
           "max_abs_ssim": float((h["ssim"] - t["ssim"]).abs().max()), "max_abs_psnr": float((h["psnr"] - t["psnr"]).abs().max())}
    hip_fb()
    gh = x.grad.clone()
    torch_fb()
    row["grad_rel_l2"] = float((gh - x.grad).norm() / x.grad.norm())
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {f: [] for f in forms}
    for _ in range(samples):
        for f, fn in forms.items():
            got[f].append(_sample(fn, iters))
    for f, v in got.items():
        row.update({f"{f}_us": round(statistics.median(v), 2), f"{f}_us_min": round(min(v), 2), f"{f}_us_max": round(max(v), 2)})
    row["ratio_forward"] = round(row["torch_forward_us"] / row["hip_forward_us"], 2)
    row["ratio_fwd_bwd"] = round(row["torch_fwd_bwd_us"] / row["hip_fwd_bwd_us"], 2)
    row["hbm_fraction_forward"] = round(2 * N * C * H * W * 4 / (row["hip_forward_us"] * 1e-6) / HBM_PEAK, 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated stack names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics", "metrics_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda:0")
    only = set(filter(None, a.only.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for name, N, C, H, W in SHAPES:
            if only and name not in only:
                continue
            row = bench(name, N, C, H, W, a.iters, a.samples, a.warmup, dev)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
