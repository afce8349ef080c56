#!/usr/bin/env python3
"""Generates tests/golden/g18_metrics.npz: what the reference's OWN `utils.loss_utils.ssim` (loaded by path, as it is) and the PSNR line of
eval.py:28-30 return on the CPU, in fp32 and again in fp64, for unipre3d_amd/metrics.py and tests/metrics_ref.py.  Only inputs and
recorded results are stored.

  names                 the case names, in order
  window                (11,) fp32: the reference's gaussian(11, 1.5)
  {case}_img1, _img2    (N, C, H, W) fp32 inputs (the fp64 runs take the same values cast to fp64)
  {case}_ssim32, _ssim64    (N,) ssim(img1, img2, size_average=False)
  {case}_grad32, _grad64    (N, C, H, W) autograd gradient of ssim(..., size_average=False).sum() with respect to img1
  {case}_psnr32, _psnr64    (N,) -10 * log10(mean((img1[i] - img2[i]) ** 2, dim=[0, 1, 2])) per image

Cases: noise (uniform noise against noise), smooth (a smooth image against itself plus noise), render (a hard-edged silhouette on a
black background against itself shifted by a pixel and slightly dimmed), identical, constant_constant (0.5 against 0.5),
constant_zero (0.5 against an all-zero target), one_channel (C = 1), small (9 x 7: smaller than the window) and pixel (1 x 1).

With --tolerance it also measures the yardsticks (reference fp32 against reference fp64) and the floors (the fp32 restatement of
tests/metrics_ref.py against the reference's fp64) and writes profiles/metrics/tolerance.json, keeping the kernel's recorded worst
figures if the file already has them.  A seed on which main()'s assertions fail is replaced by another seed, never excused."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import metrics_ref as MR  # noqa: E402


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _smooth(rng, n, c, h, w):
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    f = rng.uniform(1, 4, (n, c, 1, 1))
    ph = rng.uniform(0, 6.28, (n, c, 1, 1))
    return 0.5 + 0.4 * np.sin(f * 3.0 * x + ph) * np.cos(f * 2.0 * y - ph)


def _render(rng, n, c, h, w):
    """A disc and a box of flat colour with hard edges on black; the target is the same shifted by one pixel, slightly dimmed."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.zeros((n, c, h, w))
    for i in range(n):
        cy, cx, rad = rng.uniform(0.35, 0.65) * h, rng.uniform(0.35, 0.65) * w, 0.3 * min(h, w)
        disc = (y - cy) ** 2 + (x - cx) ** 2 < rad ** 2
        box = (abs(y - 0.25 * h) < 0.12 * h) & (abs(x - 0.7 * w) < 0.2 * w)
        for k in range(c):
            img[i, k][disc] = rng.uniform(0.3, 0.9)
            img[i, k][box] = rng.uniform(0.3, 0.9)
    return img, 0.97 * np.roll(img, (1, 1), (2, 3))


def cases():
    out = {}
    rng = np.random.default_rng(18)
    out["noise"] = (rng.uniform(0, 1, (2, 3, 37, 53)), rng.uniform(0, 1, (2, 3, 37, 53)))
    s = _smooth(rng, 1, 3, 37, 53)
    out["smooth"] = (s, np.clip(s + rng.normal(0, 0.05, s.shape), 0, 1))
    out["render"] = _render(rng, 2, 3, 33, 41)
    s = _smooth(rng, 1, 3, 19, 23) * rng.uniform(0.8, 1, (1, 3, 19, 23))
    out["identical"] = (s, s.copy())
    out["constant_constant"] = (np.full((1, 3, 16, 18), 0.5), np.full((1, 3, 16, 18), 0.5))
    out["constant_zero"] = (np.full((1, 3, 16, 18), 0.5), np.zeros((1, 3, 16, 18)))
    out["one_channel"] = (rng.uniform(0, 1, (2, 1, 21, 17)), rng.uniform(0, 1, (2, 1, 21, 17)))
    out["small"] = (rng.uniform(0, 1, (2, 3, 9, 7)), rng.uniform(0, 1, (2, 3, 9, 7)))
    out["pixel"] = (rng.uniform(0.2, 1, (3, 3, 1, 1)), rng.uniform(0.2, 1, (3, 3, 1, 1)))
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in out.items()}


def record(lu, a, b, dtype):
    x = torch.from_numpy(a).to(dtype).requires_grad_(True)
    y = torch.from_numpy(b).to(dtype)
    s = lu.ssim(x, y, size_average=False)
    s.sum().backward()
    with torch.no_grad():
        p = torch.stack([-10 * torch.log10(torch.mean((x[i] - y[i]) ** 2, dim=[0, 1, 2])) for i in range(x.size(0))])
    return s.detach().numpy(), x.grad.numpy(), p.numpy()


def main():
    lu = _load("g18_loss_utils", "utils/loss_utils.py")
    window = lu.gaussian(11, 1.5).numpy()
    assert window.dtype == np.float32 and np.array_equal(window, MR.WINDOW), "the restatement's taps are the reference's"
    out = {"window": window}
    names = []
    for name, (a, b) in cases().items():
        names.append(name)
        out[f"{name}_img1"], out[f"{name}_img2"] = a, b
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            s, g, p = record(lu, a, b, dtype)
            assert s.shape == (a.shape[0],) and g.shape == a.shape and p.shape == (a.shape[0],)
            out[f"{name}_ssim{tag}"], out[f"{name}_grad{tag}"], out[f"{name}_psnr{tag}"] = s, g, p
        assert np.isfinite(out[f"{name}_ssim64"]).all() and np.isfinite(out[f"{name}_grad64"]).all()
        # the fp64 restatement IS the reference's fp64 arithmetic (2-D window), forward and gradient
        assert np.abs(MR.ssim_f64(a, b) - out[f"{name}_ssim64"]).max() < 1e-12, name
        g64 = MR.ssim_grad(a, b)
        assert np.abs(g64 - out[f"{name}_grad64"]).max() < 1e-12 * max(1.0, np.abs(g64).max()), name
    out["names"] = np.asarray(names)
    path = os.path.join(OUT, "g18_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "keys")
    if "--tolerance" in sys.argv:
        write_tolerance(np.load(path, allow_pickle=False))


def write_tolerance(z):
    old = {}
    if os.path.exists(MR.TOLERANCE):
        with open(MR.TOLERANCE) as f:
            old = {c["case"]: c for c in json.load(f).get("cases", [])}
    rows, floors = [], {"ssim": 0.0, "psnr": 0.0, "grad_rel_l2": 0.0, "grad_max_abs_degenerate": 0.0}
    for name in MR.case_names(z):
        y, d = MR.yardsticks(name, z), MR.restatement_distances(name, z)
        gk = "grad_max_abs_degenerate" if name in MR.DEGENERATE else "grad_rel_l2"
        floors["ssim"], floors["psnr"], floors[gk] = max(floors["ssim"], d["ssim"]), max(floors["psnr"], d["psnr"]), max(floors[gk], d["grad"])
        rows.append({"case": name, "grad_measure": "max_abs" if name in MR.DEGENERATE else "rel_l2",
                     "ssim_yardstick": y["ssim"], "psnr_yardstick": y["psnr"], "grad_yardstick": y["grad"],
                     "ssim_restatement_f32": d["ssim"], "psnr_restatement_f32": d["psnr"], "grad_restatement_f32": d["grad"],
                     "ssim_kernel_worst": old.get(name, {}).get("ssim_kernel_worst"),
                     "psnr_kernel_worst": old.get(name, {}).get("psnr_kernel_worst"),
                     "grad_kernel_worst": old.get(name, {}).get("grad_kernel_worst")})
    doc = {"unit": "ssim, psnr: max over images of |value - reference fp64|; grad: relative L2 against the reference's fp64 gradient "
                   "(max-abs for the degenerate pairs, whose true gradient is 0)",
           "rule": "bar = 2 x yardstick + floor.  yardstick: the reference's own fp32 result against its fp64 record, per case.  floor: "
                   "the largest distance of the fp32 restatement (tests/metrics_ref.py, separable order) from the fp64 record over the "
                   "golden cases, per quantity, measured on the CPU -- the separable order and fused multiply-adds round differently "
                   "from the reference's 2-D window.  Shapes without a recorded case (tile classes, full shapes) are compared with "
                   "the fp64 restatement and held to the largest bar of the non-degenerate golden cases.",
           "floors": floors, "cases": rows,
           "kernel_worst_source": "tests/test_gpu_metrics.py::test_golden_cases on one MI355X (the figures it prints), same measures "
                                  "as the yardsticks"}
    os.makedirs(os.path.dirname(MR.TOLERANCE), exist_ok=True)
    with open(MR.TOLERANCE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", MR.TOLERANCE)
    for r in rows:
        print(r)
    print(floors)


if __name__ == "__main__":
    main()
