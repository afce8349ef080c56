#!/usr/bin/env python3
"""Generates tests/golden/g20_lnp.npz: what the reference's OWN K_Norm + K_Pool and LNPBlock (openpoints/models/Mamba3D/Mamba3D.py, loaded
by path under stub packages, as it is) compute on the CPU, in fp64, with autograd's gradients, for unipre3d_amd/lnp.py and tests/lnp_ref.py.
`knn_cuda.KNN` is a brute-force search here (distances in fp64, ties to the lower index); the recipe asserts that no cloud has a distance
tie among a centre's first k + 1 neighbours, so the choice of the search cannot matter.  Only inputs and recorded results are stored.

  names                          the case names, in order
  {case}_center                  (B, G, 3) fp32
  {case}_idx                     (B, G, K) int32: what the stubbed KNN returned inside the reference's forward
  {case}_x, _dout                (B, G, C) fp32 on a 2^-5 grid and (B, G, 2C) fp32 on a 2^-4 grid; _alpha, _beta (2C,) fp32
  {case}_out64, _dx64            fp64: K_Pool(K_Norm(center, x)) as (B, G, 2C) and autograd's d(x) of sum(out * dout)
  {case}_dalpha64, _dbeta64      (2C,) fp64
  {case}_yard_{out,dx,dalpha,dbeta}   the yardsticks: max|fp32 - fp64| / max|fp64| of the reference's own fp32 run (huge: of the
                                 max-subtracted form in torch, tests/lnp_ref.py reference_form(stable=True); the reference's fp32 run is NaN)
  object_cols                    object keeps out64 at channels cols and C + cols and dx64 at cols (48 of 384, every residue mod 8), and its
                                 yardsticks are measured there, so that the file stays small
  block_*                        the whole LNPBlock on the tiny case: block_feat (B, G+1, C), block_dy, block_w_{state_dict key},
                                 block_y64, block_dfeat64, block_g64_{key}, block_yard_{y, dfeat, key}

Cases (B, G, C, K): object (2, 128, 384, 4); kg (1, 5, 8, 5); tiny (2, 16, 8, 4); k8 (1, 16, 12, 8); sharp (1, 16, 12, 4) with alpha of
about 30 in three channels; huge (1, 16, 12, 4) with alpha of 80 in three channels (|v| up to about 200: the plain exp of fp32 overflows).

With --tolerance it also measures the floors (the fp32 restatement in the kernels' order against the fp64 record) and writes
profiles/lnp/tolerance.json, keeping the kernels' recorded worst figures if the file already has them."""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import lnp_ref as LR  # noqa: E402
import make_g12_ptv3_boundary as g12  # noqa: E402

SHAPES = {"object": (2, 128, 384, 4), "kg": (1, 5, 8, 5), "tiny": (2, 16, 8, 4), "k8": (1, 16, 12, 8), "sharp": (1, 16, 12, 4),
          "huge": (1, 16, 12, 4)}
GAIN = {"sharp": 30.0, "huge": 80.0}
SEEN = []          # the index tensors the stubbed KNN returned, in call order


class _Registry:
    def register_module(self, *a, **k):
        return lambda c: c


class BruteKNN(nn.Module):
    """knn_cuda.KNN(k, transpose_mode=True)(ref, query) -> (dist, idx int64), by sorting all distances; ties go to the lower index."""

    def __init__(self, k, transpose_mode=False):
        super().__init__()
        assert transpose_mode
        self.k = k

    def forward(self, ref, query):
        r, q = ref.detach().double().numpy(), query.detach().double().numpy()
        d2 = ((q[:, :, None, :] - r[:, None, :, :]) ** 2).sum(-1)
        order = np.argsort(d2, axis=-1, kind="stable")
        srt = np.take_along_axis(d2, order, -1)[:, :, :min(self.k + 1, d2.shape[-1])]
        assert (np.diff(srt, axis=-1) > 0).all(), "a distance tie among the first k + 1 neighbours"
        idx = torch.from_numpy(order[:, :, :self.k].copy())
        SEEN.append(idx)
        return torch.from_numpy(np.sqrt(np.take_along_axis(d2, order[:, :, :self.k], -1))).to(ref.dtype), idx


def load_reference():
    g12._stub("timm")
    g12._stub("timm.models")
    g12._stub("timm.models.layers", DropPath=nn.Identity, trunc_normal_=None, PatchEmbed=None)
    g12._stub("timm.models.vision_transformer", VisionTransformer=None, _cfg=None, _load_weights=None)
    g12._stub("timm.models.registry", register_model=lambda f: f)
    g12._stub("knn_cuda", KNN=BruteKNN)
    g12._stub("fusion", FeatureFusion=None)
    g12._stub("g20")
    g12._stub("g20.backbone")
    g12._stub("g20.backbone.pointmlp", PointNetFeaturePropagation=None)
    g12._stub("g20.Mamba3D")
    g12._stub("g20.Mamba3D.build_fn", MODELS=_Registry())
    g12._stub("g20.Mamba3D.Mamba3D_utils", misc=None)
    g12._stub("g20.Mamba3D.Mamba3D_utils.checkpoint", get_missing_parameters_message=None, get_unexpected_parameters_message=None)
    g12._stub("g20.Mamba3D.Mamba3D_utils.logger")
    g12._stub("g20.Mamba3D.bimamba_ssm")
    g12._stub("g20.Mamba3D.bimamba_ssm.modules")
    g12._stub("g20.Mamba3D.bimamba_ssm.modules.mamba_simple", Mamba=None)
    g12._stub("g20.Mamba3D.bimamba_ssm.utils")
    g12._stub("g20.Mamba3D.bimamba_ssm.utils.generation", GenerationMixin=None)
    g12._stub("g20.Mamba3D.bimamba_ssm.utils.hf", load_config_hf=None, load_state_dict_hf=None)
    g12._stub("g20.Mamba3D.bimamba_ssm.ops")           # (no .triton below it: the reference's own ImportError branch)
    g12._stub("g20.Mamba3D.rope")
    g12._stub("g20.Mamba3D.z_order")
    return g12._load("g20.Mamba3D.Mamba3D", "openpoints/models/Mamba3D/Mamba3D.py")


def grid(rng, shape, step, lo=-1.0, hi=1.0):
    return (np.round(rng.uniform(lo, hi, shape) / step) * step).astype(np.float32)


def cases():
    rng = np.random.default_rng(20)
    out = {}
    for name, (B, G, C, K) in SHAPES.items():
        center = rng.uniform(-1, 1, (B, G, 3)).astype(np.float32)
        x, dout = grid(rng, (B, G, C), 2.0 ** -5), grid(rng, (B, G, 2 * C), 2.0 ** -4)
        alpha = grid(rng, (2 * C,), 2.0 ** -6, 0.5, 1.5) * np.where(rng.uniform(size=2 * C) < 0.25, -1, 1).astype(np.float32)
        beta = grid(rng, (2 * C,), 2.0 ** -6, -0.5, 0.5)
        if name in GAIN:
            alpha[[1, 6, 10]] = np.float32(GAIN[name]) * np.array([1, -1, 1], np.float32)
        out[name] = (center, x, alpha, beta, dout, K)
    return out


def record(ref, center, x, alpha, beta, dout, K, dtype):
    """The reference's K_Norm and K_Pool modules -> out (B, G, 2C), (dx, dalpha, dbeta), and the idx its KNN returned."""
    C = x.shape[2]
    lga = ref.K_Norm(2 * C, K, 100, 1000).to(dtype)
    with torch.no_grad():
        lga.affine_alpha_feat.copy_(torch.from_numpy(alpha).view(1, 1, 1, -1))
        lga.affine_beta_feat.copy_(torch.from_numpy(beta).view(1, 1, 1, -1))
    t = torch.from_numpy(x).to(dtype).requires_grad_(True)
    del SEEN[:]
    out = ref.K_Pool()(lga(torch.from_numpy(center).to(dtype), t)).permute(0, 2, 1)
    (out * torch.from_numpy(dout).to(dtype)).sum().backward()
    g = (t.grad.numpy(), lga.affine_alpha_feat.grad.numpy().reshape(-1), lga.affine_beta_feat.grad.numpy().reshape(-1))
    return out.detach().numpy(), g, SEEN[0].numpy().astype(np.int32)


def record_block(ref, center, feat, dy, state, K, dtype):
    C = feat.shape[2]
    blk = ref.LNPBlock(lga_out_dim=2 * C, k_group_size=K, alpha=100, beta=1000, mlp_in_dim=2 * C, mlp_out_dim=C, num_group=center.shape[1])
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    blk = blk.to(dtype)
    f = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    y = blk(torch.from_numpy(center).to(dtype), f)
    (y * torch.from_numpy(dy).to(dtype)).sum().backward()
    return y.detach().numpy(), f.grad.numpy(), {k: p.grad.numpy() for k, p in blk.named_parameters()}


def main():
    ref = load_reference()
    out, names = {}, []
    for name, (center, x, alpha, beta, dout, K) in cases().items():
        names.append(name)
        o64, g64, idx = record(ref, center, x, alpha, beta, dout, K, torch.float64)
        o32, g32, idx32 = record(ref, center, x, alpha, beta, dout, K, torch.float32)
        assert np.array_equal(idx, idx32) and np.isfinite(o64).all() and all(np.isfinite(g).all() for g in g64)
        if name == "huge":
            assert not np.isfinite(o32).all(), "the reference's fp32 run was expected to overflow"
            o32, g32 = LR.reference_form(x, idx, alpha, beta, dout, stable=True)
        assert np.isfinite(o32).all() and all(np.isfinite(g).all() for g in g32)
        # the fp64 restatement IS the reference's fp64 arithmetic, forward and gradient
        r64 = dict(zip(LR.QUANTITIES, (LR.forward_f64(x, idx, alpha, beta)[0],) + LR.backward_f64(x, idx, alpha, beta, dout)))
        ref64 = dict(zip(LR.QUANTITIES, (o64,) + g64))
        for q in LR.QUANTITIES:
            assert LR.dist(r64[q], ref64[q]) < 1e-12, (name, q, LR.dist(r64[q], ref64[q]))
        cols = None
        if name == "object":
            cols = (np.arange(0, x.shape[2], 8) + np.arange(x.shape[2] // 8) % 8).astype(np.int32)
            out["object_cols"] = cols
        ref64, got32 = LR.recorded(ref64, cols), LR.recorded(dict(zip(LR.QUANTITIES, (o32,) + g32)), cols)
        out.update({f"{name}_center": center, f"{name}_idx": idx, f"{name}_x": x, f"{name}_dout": dout, f"{name}_alpha": alpha,
                    f"{name}_beta": beta, f"{name}_out64": ref64["out"], f"{name}_dx64": ref64["dx"], f"{name}_dalpha64": ref64["dalpha"],
                    f"{name}_dbeta64": ref64["dbeta"]})
        for q in LR.QUANTITIES:
            out[f"{name}_yard_{q}"] = np.float64(LR.dist(got32[q], ref64[q]))
        v = np.asarray(alpha[:x.shape[2]], np.float64) * (LR._gather(x.astype(np.float64), idx) - x[:, :, None, :]) \
            / (np.std(LR._gather(x.astype(np.float64), idx) - x[:, :, None, :], ddof=1) + 1e-5) + beta[:x.shape[2]]
        p = np.exp(v - LR.forward_f64(x, idx, alpha, beta)[1][:, :, None, :])
        print(f"{name}: yardsticks " + " ".join(f"{q} {out[f'{name}_yard_{q}']:.3g}" for q in LR.QUANTITIES)
              + f"; largest |v| {np.abs(v).max():.1f}, largest probability {p.max():.6f}")
    # the whole block on the tiny case
    rng = np.random.default_rng(120)
    center, _, alpha, beta, _, K = cases()["tiny"]
    B, G, C, _ = SHAPES["tiny"]
    feat, dy = grid(rng, (B, G + 1, C), 2.0 ** -6), grid(rng, (B, G + 1, C), 2.0 ** -6)
    state = {"lga.affine_alpha_feat": alpha.reshape(1, 1, 1, -1), "lga.affine_beta_feat": beta.reshape(1, 1, 1, -1),
             "mlp.share_mlp.weight": grid(rng, (C, 2 * C, 1), 2.0 ** -6), "mlp.share_mlp.bias": grid(rng, (C,), 2.0 ** -6),
             "pre_norm_ft.weight": grid(rng, (2 * C,), 2.0 ** -6, 0.5, 1.5), "pre_norm_ft.bias": grid(rng, (2 * C,), 2.0 ** -6)}
    y64, df64, gp64 = record_block(ref, center, feat, dy, state, K, torch.float64)
    y32, df32, gp32 = record_block(ref, center, feat, dy, state, K, torch.float32)
    assert set(gp64) == set(state)
    out.update({"block_feat": feat, "block_dy": dy, "block_y64": y64, "block_dfeat64": df64,
                "block_yard_y": np.float64(LR.dist(y32, y64)), "block_yard_dfeat": np.float64(LR.dist(df32, df64))})
    for k in state:
        out[f"block_w_{k}"], out[f"block_g64_{k}"] = state[k], gp64[k]
        out[f"block_yard_{k}"] = np.float64(LR.dist(gp32[k], gp64[k]))
    out["names"] = np.asarray(names)
    np.savez_compressed(LR.GOLDEN, **out)
    print("wrote", LR.GOLDEN, os.path.getsize(LR.GOLDEN), "bytes;", len(out), "keys")
    if "--tolerance" in sys.argv:
        write_tolerance(np.load(LR.GOLDEN, allow_pickle=False))


def write_tolerance(z):
    old = {}
    if os.path.exists(LR.TOLERANCE):
        with open(LR.TOLERANCE) as f:
            old = {c["case"]: c for c in json.load(f).get("cases", [])}
    rows, floors = [], {q: 0.0 for q in LR.QUANTITIES}
    for name in (str(n) for n in z["names"]):
        x, idx, alpha, beta, dout, cols = LR.golden_case(z, name)
        saved = LR.forward_kernel_f32(x, idx, alpha, beta)
        got = LR.recorded(dict(zip(LR.QUANTITIES, (saved[0],) + LR.backward_kernel_f32(x, idx, alpha, beta, dout, saved=saved))), cols)
        row = {"case": name, "shape_BGCK": [int(s) for s in x.shape] + [int(idx.shape[2])]}
        for q in LR.QUANTITIES:
            d = LR.dist(got[q], z[f"{name}_{q}64"])
            floors[q] = max(floors[q], d)
            row[f"{q}_yardstick"], row[f"{q}_restatement_f32"] = float(z[f"{name}_yard_{q}"]), d
            row[f"{q}_kernel_worst"] = old.get(name, {}).get(f"{q}_kernel_worst")
        rows.append(row)
    for r in rows:
        for q in LR.QUANTITIES:
            r[f"{q}_bar"] = 2.0 * r[f"{q}_yardstick"] + floors[q]
    doc = {"unit": "max|x - reference fp64| / max|reference fp64|, per case, for out, d(x), d(alpha) and d(beta)",
           "rule": "bar = 2 x yardstick + floor.  yardstick: the reference's own fp32 run of K_Norm + K_Pool against its fp64 run, per case "
                   "(huge: the max-subtracted form in torch, the reference's fp32 run being NaN).  floor: the largest distance of the fp32 "
                   "restatement in the kernels' order (tests/lnp_ref.py) from the fp64 record over the golden cases, per quantity, measured on "
                   "the CPU.  A shape without a recorded case takes its yardstick on the spot: the reference's lines in torch in fp32 against "
                   "the fp64 restatement.",
           "floors": floors, "cases": rows,
           "kernel_worst_source": "tests/test_gpu_lnp.py::test_golden_cases on one MI355X (the figures it prints), same unit"}
    os.makedirs(os.path.dirname(LR.TOLERANCE), exist_ok=True)
    with open(LR.TOLERANCE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", LR.TOLERANCE)
    for r in rows:
        print(r)
    print(floors)


if __name__ == "__main__":
    main()
