#!/usr/bin/env python3
"""Generates tests/golden/g19_dense_attention.npz: what the reference's OWN Attention.forward (openpoints/models/backbone/transformer.py,
loaded by path under stub packages, as it is) computes between its qkv Linear and its proj on the CPU, in fp32 and again in fp64, for
unipre3d_amd/mha.py and tests/mha_ref.py.  The module's qkv is replaced by a module that returns a fixed leaf tensor and its proj by
nn.Identity(), so its forward runs exactly the core and autograd gives d(qkv).  Only inputs and recorded results are stored.

  names                 the case names, in order
  {case}_qkv            (B, N, 3, H, 64) fp32: uniform in [-1, 1] on a 2^-8 grid, q and k times the case's gain
  {case}_dout           (B, N, H, 64) fp32, uniform in [-1, 1] on the same grid
  {case}_out64          (B, N, H, 64) fp64: the module's fp64 output, viewed per head
  {case}_dqkv64         (B, N, 3, H, 64) fp64: its autograd gradient of sum(out * dout)
  {case}_yard_out, _yard_dqkv   the yardsticks: max|fp32 - fp64| / max|fp64| of the module's own fp32 run (the fp32 tensors are not stored)

Cases (B, N, H) x gain: object (1, 129, 1) x 1; one (2, 1, 2) x 1; odd17 (2, 17, 2) x 1; sharp17 (1, 17, 1) x 4 (largest probability
about 1); huge9 (1, 9, 1) x 12 (scores of several tens: only the max subtraction keeps the softmax finite).

With --tolerance it also measures the floors (the fp32 restatement in the kernel's order, tests/mha_ref.py, against the fp64 record)
and writes profiles/mha/tolerance.json, keeping the kernel's recorded worst figures if the file already has them."""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import mha_ref as MR  # noqa: E402
import make_g12_ptv3_boundary as g12  # noqa: E402

SHAPES = {"object": ((1, 129, 1), 1.0), "one": ((2, 1, 2), 1.0), "odd17": ((2, 17, 2), 1.0), "sharp17": ((1, 17, 1), 4.0),
          "huge9": ((1, 9, 1), 12.0)}
D = 64


class _Registry:
    def register_module(self, *a, **k):
        return lambda c: c


class _Fixed(nn.Module):
    def __init__(self, leaf):
        super().__init__()
        self.leaf = leaf

    def forward(self, x):
        return self.leaf


def load_reference():
    g12._stub("timm")
    g12._stub("timm.models")
    g12._stub("timm.models.layers", DropPath=nn.Identity)
    g12._stub("openpoints")
    g12._stub("openpoints.models")
    g12._stub("openpoints.models.build", MODELS=_Registry())
    g12._stub("openpoints.models.layers", SubsampleGroup=None)
    g12._stub("fusion", FeatureFusion=None)
    return g12._load("g19_transformer", "openpoints/models/backbone/transformer.py")


def cases():
    rng = np.random.default_rng(19)
    out = {}
    for name, ((B, N, H), gain) in SHAPES.items():
        qkv = np.round(rng.uniform(-1, 1, (B, N, 3, H, D)) * 256) / 256    # (a 2^-8 grid: the fp32 inputs compress)
        qkv[:, :, :2] *= gain
        out[name] = (qkv.astype(np.float32), (np.round(rng.uniform(-1, 1, (B, N, H, D)) * 256) / 256).astype(np.float32))
    return out


def record(tf, qkv, dout, dtype):
    B, N, _, H, _ = qkv.shape
    a = tf.Attention(H * D, num_heads=H)
    leaf = torch.from_numpy(qkv).to(dtype).reshape(B, N, 3 * H * D).requires_grad_(True)
    a.qkv, a.proj = _Fixed(leaf), nn.Identity()
    y = a(torch.zeros(B, N, H * D, dtype=dtype))
    assert y.shape == (B, N, H * D) and y.dtype == dtype
    (y * torch.from_numpy(dout).to(dtype).reshape(B, N, H * D)).sum().backward()
    return y.detach().numpy().reshape(B, N, H, D), leaf.grad.numpy().reshape(B, N, 3, H, D)


def main():
    tf = load_reference()
    out, names = {}, []
    for name, (qkv, dout) in cases().items():
        names.append(name)
        o32, g32 = record(tf, qkv, dout, torch.float32)
        o64, g64 = record(tf, qkv, dout, torch.float64)
        assert np.isfinite(o64).all() and np.isfinite(g64).all() and np.isfinite(o32).all() and np.isfinite(g32).all()
        # the fp64 restatement IS the reference's fp64 arithmetic, forward and gradient
        assert MR.dist(MR.forward_f64(qkv)[0], o64) < 1e-12 and MR.dist(MR.backward_f64(qkv, dout), g64) < 1e-12, name
        out[f"{name}_qkv"], out[f"{name}_dout"], out[f"{name}_out64"], out[f"{name}_dqkv64"] = qkv, dout, o64, g64
        out[f"{name}_yard_out"], out[f"{name}_yard_dqkv"] = np.float64(MR.dist(o32, o64)), np.float64(MR.dist(g32, g64))
        p = np.exp(MR.forward_f64(qkv)[1])   # not stored: the scale of the case
        s = np.einsum("bnhd,bmhd->bhnm", qkv[:, :, 0].astype(np.float64), qkv[:, :, 1].astype(np.float64)) * MR.default_scale(D)
        print(f"{name}: yardstick out {out[f'{name}_yard_out']:.3g} dqkv {out[f'{name}_yard_dqkv']:.3g}; largest |score| "
              f"{np.abs(s).max():.1f}, largest probability {np.exp(s - np.log(p)[..., None]).max():.6f}")
    out["names"] = np.asarray(names)
    path = MR.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "keys")
    if "--tolerance" in sys.argv:
        write_tolerance(np.load(path, allow_pickle=False))


def write_tolerance(z):
    old = {}
    if os.path.exists(MR.TOLERANCE):
        with open(MR.TOLERANCE) as f:
            old = {c["case"]: c for c in json.load(f).get("cases", [])}
    rows, floors = [], {"out": 0.0, "dqkv": 0.0}
    for name in (str(n) for n in z["names"]):
        qkv, dout = z[f"{name}_qkv"], z[f"{name}_dout"]
        d_out = MR.dist(MR.forward_kernel_f32(qkv)[0], z[f"{name}_out64"])
        d_g = MR.dist(MR.backward_kernel_f32(qkv, dout), z[f"{name}_dqkv64"])
        floors["out"], floors["dqkv"] = max(floors["out"], d_out), max(floors["dqkv"], d_g)
        rows.append({"case": name, "shape_BNH": [int(qkv.shape[0]), int(qkv.shape[1]), int(qkv.shape[3])],
                     "out_yardstick": float(z[f"{name}_yard_out"]), "dqkv_yardstick": float(z[f"{name}_yard_dqkv"]),
                     "out_restatement_f32": d_out, "dqkv_restatement_f32": d_g,
                     "out_kernel_worst": old.get(name, {}).get("out_kernel_worst"),
                     "dqkv_kernel_worst": old.get(name, {}).get("dqkv_kernel_worst")})
    for r in rows:
        r["out_bar"], r["dqkv_bar"] = 2.0 * r["out_yardstick"] + floors["out"], 2.0 * r["dqkv_yardstick"] + floors["dqkv"]
    doc = {"unit": "max|x - reference fp64| / max|reference fp64|, per case, for out and for d(qkv)",
           "rule": "bar = 2 x yardstick + floor.  yardstick: the reference's own fp32 run of Attention.forward's core against its fp64 run, "
                   "per case.  floor: the largest distance of the fp32 restatement in the kernel's order (tests/mha_ref.py: k-ordered fma "
                   "chains, online softmax over blocks of 64 keys, exp2 with the folded scale, P recomputed from lse) from the fp64 record "
                   "over the golden cases, per quantity, measured on the CPU.  A shape without a recorded case takes its yardstick on "
                   "the spot: the reference's four lines in fp32 against the fp64 restatement.",
           "floors": floors, "cases": rows,
           "kernel_worst_source": "tests/test_gpu_mha.py::test_golden_cases on one MI355X (the figures it prints), same unit"}
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
