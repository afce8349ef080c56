#!/usr/bin/env python3
"""Writes profiles/batchnorm/tolerance.json (CPU only): per golden case of tests/golden/g26_batchnorm.npz and per quantity, the floor (the
fp32 restatement of tests/batchnorm_ref.py against the fp64 record), the bar (2 x floor) and the yardstick (torch's own fp32
BatchNorm1d + add + activation on the CPU against the record, which sets no bar).  `--kernel FILE` merges the figures that
tests/test_gpu_batchnorm.py::test_golden_cases wrote on the GPU (U3D_BN_FIGURES=FILE) as <quantity>_kernel_worst; without it the
figures already in the file are kept."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batchnorm_ref as R  # noqa: E402

WANT = {"y": "_y", "dx": "_dx", "dresidual": "_dresidual", "dgamma": "_dgamma", "dbeta": "_dbeta", "running_mean": "_rm1", "running_var": "_rv1"}
RULE = ("bar = 2 x floor, per case and per quantity.  floor: the distance of the fp32 restatement in the kernels' order "
        "(tests/batchnorm_ref.py) from the fp64 record (tests/golden/g26_batchnorm.npz: the reference's own BasicBlock and stems), measured "
        "on the CPU; 2 x is the margin profiles/feature_propagation/tolerance.json gives a reordered fp32 evaluation.  The yardsticks "
        "(torch's own fp32 BatchNorm1d + add + activation on the CPU against the record) are written down and set no bar.  A shape "
        "without a recorded case is held to the fp64 restatement by the same rule: its floor is the fp32 restatement's distance from the "
        "fp64 restatement on that very input, computed on the CPU by the test, and not less than the largest recorded floor of the "
        "quantity (`floors`) -- a case of a few hundred values samples the rounding error of a quantity less widely than the record does.")


def _torch_f32(g, c):
    t = lambda k: torch.tensor(g[c + k].astype(np.float32))
    x, gamma, beta = t("_x").requires_grad_(True), t("_gamma").requires_grad_(True), t("_beta").requires_grad_(True)
    rm, rv = t("_rm0"), t("_rv0")
    res = t("_residual").requires_grad_(True) if c + "_residual" in g.files else None
    z = F.batch_norm(x, rm, rv, gamma, beta, bool(g[c + "_training"]), float(g["momentum"]), float(g["eps"]))
    if res is not None:
        z = z + res
    act = str(g[c + "_act"])
    y = F.relu(z) if act == "relu" else F.gelu(z) if act == "gelu" else z
    y.backward(t("_dy"))
    out = dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)
    if c + "_dresidual" in g.files:
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
        res = g[c + "_residual"] if c + "_residual" in g.files else None
        f = R.forward(g[c + "_x"], g[c + "_gamma"], g[c + "_beta"], g[c + "_rm0"], g[c + "_rv0"], int(g[c + "_nbt0"]),
                      training=bool(g[c + "_training"]), momentum=float(g["momentum"]), eps=float(g["eps"]), act=str(g[c + "_act"]),
                      residual=res, dtype=np.float32)
        b = R.backward(f, g[c + "_dy"])
        got = dict(y=f["y"], dx=b["dx"], dresidual=b["dresidual"], dgamma=b["dgamma"], dbeta=b["dbeta"], running_mean=f["running_mean"],
                   running_var=f["running_var"])
        yard = _torch_f32(g, c)
        row = {"case": c, "shape_NC": [int(v) for v in g[c + "_x"].shape], "act": str(g[c + "_act"]), "training": bool(g[c + "_training"]),
               "residual": res is not None}
        for q in R.QUANTITIES:
            if c + WANT[q] not in g.files:
                continue
            want = g[c + WANT[q]]
            row[q + "_floor"] = R.rel(got[q], want)
            row[q + "_bar"] = 2 * row[q + "_floor"]
            row[q + "_yardstick"] = R.rel(yard[q], want)
            worst = kernel.get(c, {}).get(q, old.get(c, {}).get(q + "_kernel_worst"))
            if worst is not None:
                row[q + "_kernel_worst"] = worst
            floors[q] = max(floors.get(q, 0.0), row[q + "_floor"])
        cases.append(row)
    doc = {"unit": "max|x - fp64 record| / max|fp64 record|, per case, for y, dx, dresidual, dgamma, dbeta, running_mean, running_var",
           "rule": RULE, "floors": floors, "cases": cases,
           "kernel_worst_source": "tests/test_gpu_batchnorm.py::test_golden_cases on one MI355X (the figures it prints), same unit"}
    os.makedirs(os.path.dirname(R.TOLERANCE), exist_ok=True)
    with open(R.TOLERANCE, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", R.TOLERANCE, {k: f"{v:.3e}" for k, v in floors.items()})


if __name__ == "__main__":
    main()
