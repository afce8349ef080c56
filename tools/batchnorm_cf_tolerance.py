#!/usr/bin/env python3
"""Writes profiles/batchnorm_cf/tolerance.json (CPU only): per norm case of tests/golden/g27_pointmlp_blocks.npz and per quantity, the
floor (the fp32 restatement of tests/batchnorm_cf_ref.py against the fp64 record), the bar (2 x floor) and the yardstick (torch's own
fp32 BatchNorm1d + add + activation + adaptive_max_pool1d on the CPU against the record, which sets no bar); per module case the same
floors for the module's output, input gradient, parameter gradients and buffers.  `--kernel FILE` merges the figures that
tests/test_gpu_batchnorm_cf.py::test_golden_norm_cases wrote on the GPU (U3D_BNCF_FIGURES=FILE) as <quantity>_kernel_worst; without it
the figures already in the file are kept."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batchnorm_cf_ref as R  # noqa: E402
from batchnorm_cf_ref import module_case, norm_case, residual_of, wanted  # noqa: E402

RULE = ("The rule of profiles/batchnorm/tolerance.json, unchanged: bar = 2 x floor, per case and per quantity.  floor: the distance of the "
        "fp32 restatement in the kernels' order (tests/batchnorm_cf_ref.py) from the fp64 record (tests/golden/g27_pointmlp_blocks.npz: the "
        "reference's own ConvBNReLU1D, ConvBNReLURes1D, PreExtraction and PosExtraction), measured on the CPU.  For a pooled case `y` is the "
        "pooled tensor, and arg and mask must equal the record everywhere (the record's inputs keep every decision 64 x the fp32 deviation "
        "away from a tie).  The yardsticks (torch's own fp32 lines on the CPU against the record) are written down and set no bar.  A "
        "shape without a recorded case is held to the fp64 restatement by the same rule: its floor is the fp32 restatement's distance from "
        "the fp64 restatement on that very input, computed on the CPU by the test, and not less than the largest recorded floor of the "
        "quantity (`floors`).  Module cases: the restatement's floors are recorded; on the device a module's convolutions are torch's in "
        "the fused and in the op-by-op form alike, so the fused form is held to 2 x the op-by-op form's distance from the record + the "
        "recorded floor of y, the module rule of tests/test_gpu_batchnorm.py.  The gradient of a Conv1d bias in front of a norm is zero in "
        "the record (`zero_in_the_record`: the restatement's largest absolute value there); it has no relative unit.")


def _torch_f32(g, c):
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    x, gamma, beta = t(g[c + "_x"]).requires_grad_(True), t(g[c + "_gamma"]).requires_grad_(True), t(g[c + "_beta"]).requires_grad_(True)
    rm, rv = t(g[c + "_rm0"]), t(g[c + "_rv0"])
    r = residual_of(g, c)
    res = t(r).requires_grad_(True) if r is not None else None
    z = F.batch_norm(x, rm, rv, gamma, beta, bool(g[c + "_training"]), float(g["momentum"]), float(g["eps"]))
    if res is not None:
        z = z + res
    act = str(g[c + "_act"])
    y = F.relu(z) if act == "relu" else F.gelu(z) if act == "gelu" else z
    if bool(g[c + "_pool"]):
        y = F.adaptive_max_pool1d(y, 1)[:, :, 0]
        y.backward(t(g[c + "_dpooled"]))
    else:
        y.backward(t(g[c + "_dy"]))
    out = dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)
    if res is not None:
        out["dresidual"] = res.grad
    return {k: v.numpy() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default=None)
    args = ap.parse_args()
    g = np.load(R.GOLDEN)
    old = {}
    if os.path.exists(R.TOLERANCE):
        old = {c["case"]: c for c in json.load(open(R.TOLERANCE)).get("cases", [])}
    kernel = json.load(open(args.kernel)) if args.kernel else {}
    cases, floors = [], {}
    for c in map(str, g["cases"]):
        got, f = norm_case(g, c, np.float32)
        yard = _torch_f32(g, c)
        row = {"case": c, "shape_BCL": [int(v) for v in g[c + "_x"].shape], "act": str(g[c + "_act"]), "training": bool(g[c + "_training"]),
               "residual": residual_of(g, c) is not None, "pool": bool(g[c + "_pool"])}
        if row["pool"]:
            row["arg_and_mask_reproduced"] = bool(np.array_equal(f["arg"], g[c + "_arg"]) and np.array_equal(f["mask"], g[c + "_mask"]))
            row["preactivation_deviation"], row["margin_kept"] = float(g[c + "_dev"]), float(g[c + "_margin"])
        for q in R.QUANTITIES:
            want = wanted(g, c, q)
            if want is None:
                continue
            row[q + "_floor"] = R.rel(got[q], want)
            row[q + "_bar"] = 2 * row[q + "_floor"]
            row[q + "_yardstick"] = R.rel(yard[q], want)
            worst = kernel.get(c, {}).get(q, old.get(c, {}).get(q + "_kernel_worst"))
            if worst is not None:
                row[q + "_kernel_worst"] = worst
            floors[q] = max(floors.get(q, 0.0), row[q + "_floor"])
        cases.append(row)
    modules = []
    for m in map(str, g["modules"]):
        res, _ = module_case(g, m, np.float32)
        res = {k: v for k, v in res.items() if not k.endswith("num_batches_tracked")}
        zero = sorted(k for k in res if np.abs(g[f"{m}_{k}"]).max() < 1e-12)     # a Conv1d bias in front of a norm: no gradient
        modules.append({"case": m, "kind": str(g[f"{m}_kind"]), "shape": [int(v) for v in g[f"{m}_x"].shape],
                        "floors": {k: R.rel(v, g[f"{m}_{k}"]) for k, v in res.items() if k not in zero},
                        "zero_in_the_record": {k: float(np.abs(res[k]).max()) for k in zero}})
    doc = {"unit": "max|x - fp64 record| / max|fp64 record|, per case, for y (pooled for a pooled case), dx, dresidual, dgamma, dbeta, "
                   "running_mean, running_var",
           "rule": RULE, "floors": floors, "cases": cases, "module_cases": modules,
           "kernel_worst_source": "tests/test_gpu_batchnorm_cf.py::test_golden_norm_cases on one MI355X (the figures it prints), same unit"}
    os.makedirs(os.path.dirname(R.TOLERANCE), exist_ok=True)
    with open(R.TOLERANCE, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", R.TOLERANCE, {k: f"{v:.3e}" for k, v in floors.items()})


if __name__ == "__main__":
    main()
