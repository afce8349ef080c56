"""Golden G25: the reference's image branch at the fused pixels.  Run where the reference checkout is (REF, default /root/reference); the
tests only read tests/golden/g25_image_fusion.npz.

The reference's FeatureFusion (fusion/feat_fusion.py, loaded by file path, Identity MLP, x of width 0) is applied to the output of the two
modules of model/gaussian_predictor.py:210-214, nn.Sequential(nn.GroupNorm(G, Cin, eps=1e-6), nn.Conv2d(Cin, Cout, 1)), once in fp64 (the
record) and once in fp32 (the yardstick), and the loss sum(mapped * cot) is differentiated to the four parameters.  The large inputs come
from tests/image_fusion_ref.py::case_inputs (numpy's frozen RandomState), so the file holds per case: the scene (center, c2w, intr), the
camera-space points and sel of the fp32 run, a checksum of the inputs, and out / dW / dbias / dgamma / dbeta in fp64 and fp32.  The fp64
run must select the same winners as the fp32 run (asserted): the record is the arithmetic on those rows, not another projection."""
import importlib.util
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fusion_ref  # noqa: E402
import image_fusion_ref as IR  # noqa: E402
from unipre3d_amd.fusion import FeatureFusion as ProjectFusion  # noqa: E402

REF = os.environ.get("REF", "/root/reference")


def scene(tag, B, N, H, W):
    """G7's scene: a duplicated point (tie), one behind the camera, one outside; nowin: every point of item 1 behind the camera"""
    g = torch.Generator().manual_seed(2500 + H * 31 + W)
    center = torch.randn(B, N, 3, generator=g) * 0.4
    center[:, 5] = center[:, 4]
    center[:, 9, 2] = -5.0
    center[:, 11, 0] = 30.0
    if tag == "nowin":
        center[1, :, 2] = -5.0 - center[1, :, 2].abs()
    A = torch.eye(3).repeat(B, 1, 1) + 0.15 * torch.randn(B, 3, 3, generator=g)
    Q, Rr = torch.linalg.qr(A)
    Q = Q * torch.sign(torch.diagonal(Rr, dim1=1, dim2=2)).unsqueeze(1)
    c2w = torch.eye(4).repeat(B, 1, 1)
    c2w[:, :3, :3] = Q
    c2w[:, :3, 3] = torch.tensor([0.0, 0.0, -2.0]) + 0.1 * torch.randn(B, 3, generator=g)
    focal = (H / 2.0) / math.tan(math.radians(49.13434264120263 / 2.0))
    intr = np.zeros((3, 4))
    intr[2, 2] = 1
    intr[0, 0] = intr[1, 1] = focal
    intr[0, 2], intr[1, 2] = H / 2.0, W / 2.0
    return center, c2w.transpose(1, 2).contiguous(), intr


def run(mod, inp, center, c2w, intr, cfg, dtype):
    B, N, Cin, G, Cout = (cfg[k] for k in ("B", "N", "Cin", "G", "Cout"))
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                           # the reference allocates mapped_features in the default dtype
    try:
        conv = torch.nn.Sequential(torch.nn.GroupNorm(G, Cin, eps=1e-06), torch.nn.Conv2d(Cin, Cout, kernel_size=1)).to(dtype)
        with torch.no_grad():
            conv[0].weight.copy_(torch.from_numpy(inp["gamma"]))
            conv[0].bias.copy_(torch.from_numpy(inp["beta"]))
            conv[1].weight.copy_(torch.from_numpy(inp["weight"]).reshape(Cout, Cin, 1, 1))
            conv[1].bias.copy_(torch.from_numpy(inp["bias"]))
        feats = conv.forward(torch.from_numpy(inp["map"]).to(dtype))
        cls = 1 if cfg.get("cls") else 0
        x = torch.zeros(B, N + cls, 0, dtype=dtype)
        y = mod.FeatureFusion(torch.nn.Identity())(x, center.to(dtype), feats, c2w.to(dtype), intr)
        assert y.shape == (B, N + cls, Cout) and y.dtype == dtype
        if cls:
            assert not y[:, 0].any()
        mapped = y[:, cls:]
        grads = torch.autograd.grad((mapped * torch.from_numpy(inp["cot"]).to(dtype)).sum(), list(conv.parameters()), allow_unused=True)
        grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, conv.parameters())]
    finally:
        torch.set_default_dtype(old)
    dgamma, dbeta, dW, dbias = (g.detach().numpy() for g in grads)
    return {"out": mapped.detach().numpy(), "dW": dW.reshape(Cout, Cin), "dbias": dbias, "dgamma": dgamma, "dbeta": dbeta}


def main():
    spec = importlib.util.spec_from_file_location("ref_feat_fusion", os.path.join(REF, "fusion/feat_fusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for tag, cfg in IR.CASES.items():
        B, N, H, W = cfg["B"], cfg["N"], cfg["H"], cfg["W"]
        inp = IR.case_inputs(tag)
        center, c2w, intr = scene(tag, B, N, H, W)
        r64 = run(mod, inp, center, c2w, intr, cfg, torch.float64)
        r32 = run(mod, inp, center, c2w, intr, cfg, torch.float32)
        cam = ProjectFusion.camera_points(center, c2w).numpy()
        fx, fy, cx, cy = float(intr[0][0]), float(intr[1][1]), float(intr[0][2]), float(intr[1][2])
        _, sel, _ = fusion_ref.zbuffer_loop(cam, inp["map"], fx, fy, cx, cy)
        for r in (r64, r32):                                  # a winner's row holds the bias at least; every other row is zero
            assert np.array_equal(np.any(r["out"] != 0, axis=2), sel >= 0), tag
        if tag == "nowin":
            assert not (sel[1] >= 0).any() and (sel[0] >= 0).any()
        print(tag, "winners", int((sel >= 0).sum()), "of", sel.size,
              {q: f"{IR.distance(r32[q], r64[q]):.2e}" for q in IR.QUANTITIES})
        out.update({f"{tag}_center": center.numpy(), f"{tag}_c2w": c2w.numpy(), f"{tag}_intr": intr, f"{tag}_cam": cam, f"{tag}_sel": sel,
                    f"{tag}_checksum": IR.checksum(inp)})
        for q in IR.QUANTITIES:
            out[f"{tag}_{q}_f64"] = r64[q].astype(np.float64)
            out[f"{tag}_{q}_f32"] = r32[q].astype(np.float32)
    path = os.path.join(HERE, "g25_image_fusion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    write_tolerance(out)


def write_tolerance(g):
    """profiles/image_fusion/tolerance.json: floors from the fp32 restatement in the kernels' order, bars = 2 x floor, the yardsticks next
    to them; the `kernel_worst` figures a GPU run added before are kept."""
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "image_fusion", "tolerance.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    old = {c["case"]: c for c in json.load(open(path)).get("cases", [])} if os.path.exists(path) else {}
    old_edges = json.load(open(path)).get("edge_cases", {}) if os.path.exists(path) else {}
    cases, floors = [], {q: 0.0 for q in IR.QUANTITIES}
    for tag, cfg in IR.CASES.items():
        inp, sel = IR.case_inputs(tag), g[f"{tag}_sel"]
        got = {"out": IR.forward32(inp["map"], sel, inp, cfg["G"]), **IR.backward32(inp["map"], sel, inp, cfg["G"], inp["cot"])}
        row = {"case": tag, "shape_BNCinGCoutHW": [cfg[k] for k in ("B", "N", "Cin", "G", "Cout", "H", "W")]}
        for q in IR.QUANTITIES:
            row[f"{q}_yardstick"] = IR.distance(g[f"{tag}_{q}_f32"], g[f"{tag}_{q}_f64"])
            row[f"{q}_restatement_f32"] = IR.distance(got[q], g[f"{tag}_{q}_f64"])
            floors[q] = max(floors[q], row[f"{q}_restatement_f32"])
            if f"{q}_kernel_worst" in old.get(tag, {}):
                row[f"{q}_kernel_worst"] = old[tag][f"{q}_kernel_worst"]
        cases.append(row)
    edges = {}
    for name, shape in IR.EDGE_SHAPES.items():
        inp, _, sel = IR.edge_inputs(name)
        G = shape[3]
        f64 = {"out": IR.forward(inp["map"], sel, inp, G), **IR.backward(inp["map"], sel, inp, G, inp["cot"])}
        f32 = {"out": IR.forward32(inp["map"], sel, inp, G), **IR.backward32(inp["map"], sel, inp, G, inp["cot"])}
        own = {q: IR.distance(f32[q], f64[q]) for q in IR.QUANTITIES}
        edges[name] = {"shape_BNCinGCoutHW": list(shape[:7]), "winners": int((sel >= 0).sum()), "floors": own,
                       "bars": {q: 2 * max(floors[q], own[q]) for q in IR.QUANTITIES}}
        if name in old_edges and "kernel_worst" in old_edges[name]:
            edges[name]["kernel_worst"] = old_edges[name]["kernel_worst"]
    rec = {"unit": "max|x - reference fp64| / max|reference fp64|, per case, for out, dW, dbias, dgamma and dbeta",
           "rule": "bar = 2 x floor per quantity.  floor: the largest distance of the fp32 restatement in the kernels' order "
                   "(tests/image_fusion_ref.py) from the fp64 record over the cases of golden G25, measured on the CPU.  The factor 2 covers "
                   "the MFMA's order of summation and the device's rounding of the statistics.  The yardsticks (the reference's own fp32 run "
                   "against its fp64 run) are recorded and set no bar for the kernels.  A shape without a recorded case (edge_cases: the seeded "
                   "inputs of tests/image_fusion_ref.py::edge_inputs) is held to the fp64 restatement with bar = 2 x max(floor of the golden "
                   "cases, floor of the shape), written out per shape under edge_cases: sums over more rows round more.  "
                   "dense32_against_sparse_bars: torch's fp32 dense path against the sparse path are two fp32 evaluations, whose errors "
                   "add; at the dims shape the bar is the sparse bar + 2 x the dims case's yardstick (the dense path's own recorded distance "
                   "from fp64, with the same factor 2).",
           "floors": floors, "bars": {q: 2 * v for q, v in floors.items()},
           "dense32_against_sparse_bars": {q: 2 * floors[q] + 2 * [c for c in cases if c["case"] == "dims"][0][f"{q}_yardstick"]
                                           for q in IR.QUANTITIES},
           "cases": cases,
           "edge_cases": edges,
           "kernel_worst_source": "tests/test_gpu_image_fusion.py::test_golden_cases on one MI355X (the figures it prints), same unit"}
    if os.path.exists(path) and "dense_against_sparse" in json.load(open(path)):
        rec["dense_against_sparse"] = json.load(open(path))["dense_against_sparse"]      # measured on the device, like kernel_worst
    json.dump(rec, open(path, "w"), indent=1)
    print(path, {q: f"{v:.2e}" for q, v in floors.items()})


if __name__ == "__main__":
    if sys.argv[1:] == ["--tolerance"]:                       # the record as it is: only the tolerance file is made again
        write_tolerance(np.load(os.path.join(HERE, "g25_image_fusion.npz")))
    else:
        main()
