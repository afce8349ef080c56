#!/usr/bin/env python3
"""Generates tests/golden/g21_local_grouper.npz: what the reference's OWN two LocalGrouper classes (openpoints/models/backbone/pointmlp.py
and openpoints/models/PCM/PointMLP_layers.py, loaded by path under stub packages, as they are) compute on the CPU, in fp64, with autograd's
gradients, for unipre3d_amd/local_grouper.py and tests/local_grouper_ref.py.  `furthest_point_sample` is a stub (plain furthest point
sampling in fp64 from point 0); its result and the idx the reference's own knn_point returned inside the forward are recorded.  The
recipe asserts that no cloud has a distance tie among an anchor's first K + 1 neighbours, so the choice of the search cannot matter.
Only inputs and recorded results are stored.

  names                                the case names, in order
  {case}_module, _mode, _use_xyz, _k_stride, _sample_ratio     'pointmlp' / 'pcm', 'none' / 'center' / 'anchor', and the constructor's arguments
  {case}_xyz (B, N, 3), _points (B, N, D) fp32 (points on a 2^-5 grid), _alpha, _beta (D + A,) fp32 (absent with mode none)
  {case}_fps (B, S) int32             what the module used (PCM: sorted; absent where S == N), _idx (B, S, K) int32: what knn_point returned
  {case}_dout (B, S, K', 2D + A) fp32, K' = K / k_stride (stage1: a table of 61 values);  _points_res (B, N, 4) and _res64 (B, S, 4) for PCM
  {case}_out64, _new_xyz64, _dpoints64, _dalpha64, _dbeta64     fp64: the module's result and autograd's gradients of sum(out * dout)
  {case}_yard_{out,dpoints,dalpha,dbeta}     the yardsticks: max|fp32 - fp64| / max|fp64| of the reference's own fp32 run on the same idx
  stage1_rows, _cols, _dcols           stage1 keeps out64 at anchors rows and channels cols and dpoints64 at channels dcols, and its
                                       yardsticks are measured there, so that the file stays small

Cases (B, N, S, D, K): the six {none, center, anchor} x {xyz, noxyz} at (2, 16, 8, 8, 4), PointMLP's class; pcm_stride (1, 64, 32, 12, 24)
with k_stride 2, no xyz and points_res; pcm_full (1, 12, 12, 4, 3), S == N; scales (3, 32, 16, 8, 4), three clouds at scales 1, 10 and 100
(what separates a std per batch element from one over the whole tensor); stage1 (2, 256, 128, 64, 32), anchor with xyz.

With --tolerance it also measures the floors (the fp32 restatement in the kernels' order against the fp64 record) and writes
profiles/local_grouper/tolerance.json, keeping the kernels' recorded worst figures if the file already has them."""
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import local_grouper_ref as GR  # noqa: E402
import make_g12_ptv3_boundary as g12  # noqa: E402

# name: (module, B, N, S, D, K, mode, use_xyz, k_stride)
CASES = {f"{m}_{'xyz' if u else 'noxyz'}": ("pointmlp", 2, 16, 8, 8, 4, m, u, 1) for m in ("none", "center", "anchor") for u in (True, False)}
CASES.update({"pcm_stride": ("pcm", 1, 64, 32, 12, 24, "center", False, 2), "pcm_full": ("pcm", 1, 12, 12, 4, 3, "center", True, 1),
              "scales": ("pointmlp", 3, 32, 16, 8, 4, "center", True, 1), "stage1": ("pointmlp", 2, 256, 128, 64, 32, "anchor", True, 1)})
SEEN = {}


class _Registry:
    def register_module(self, *a, **k):
        return lambda c: c


def stub_fps(xyz, S):
    """Furthest point sampling from point 0, distances in fp64, ties to the lower index."""
    x = xyz.detach().double().numpy()
    B, N, _ = x.shape
    res = np.zeros((B, S), np.int64)
    for b in range(B):
        dmin = np.full(N, np.inf)
        cur = 0
        for i in range(S):
            res[b, i] = cur
            dmin = np.minimum(dmin, ((x[b] - x[b, cur]) ** 2).sum(-1))
            cur = int(np.argmax(dmin))
    SEEN["fps"] = res
    return torch.from_numpy(res).int()


def recording(fn):
    def knn_point(nsample, xyz, new_xyz, **kw):
        if "replay" in SEEN:
            return torch.from_numpy(SEEN["replay"]).long()
        idx = fn(nsample, xyz, new_xyz, **kw)
        x, q = xyz.detach().double().numpy(), new_xyz.detach().double().numpy()
        d2 = np.sort(((q[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1), axis=-1)[:, :, :nsample + 1]
        assert (np.diff(d2, axis=-1) > 0).all(), "a distance tie among the first K + 1 neighbours"
        SEEN["idx"] = idx.numpy().astype(np.int32)
        return idx
    return knn_point


def load_reference():
    g12._stub("g21")
    g12._stub("g21.backbone")
    names = ("random_sample", "LocalAggregation", "create_convblock2d", "three_interpolate", "three_nn", "gather_operation",
             "create_linearblock", "create_convblock1d", "create_grouper", "fps")
    g12._stub("g21.layers", furthest_point_sample=stub_fps, **{n: None for n in names})
    g12._stub("g21.layers.group", QueryAndGroup=None)
    g12._stub("g21.build", MODELS=_Registry())
    g12._stub("fusion", FeatureFusion=None)
    g12._stub("g21.PCM")
    g12._stub("g21.PCM.serialization", Point=object)
    mlp = g12._load("g21.backbone.pointmlp", "openpoints/models/backbone/pointmlp.py")
    g12._load("g21.PCM.PCM_utils", "openpoints/models/PCM/PCM_utils.py")
    pcm = g12._load("g21.PCM.PointMLP_layers", "openpoints/models/PCM/PointMLP_layers.py")
    for mod in (mlp, pcm):
        mod.knn_point = recording(mod.knn_point)
    return {"pointmlp": mlp.LocalGrouper, "pcm": pcm.LocalGrouper}


def grid(rng, shape, step, lo=-1.0, hi=1.0):
    return (np.round(rng.uniform(lo, hi, shape) / step) * step).astype(np.float32)


def inputs(name):
    module, B, N, S, D, K, mode, use_xyz, ks = CASES[name]
    rng = np.random.default_rng(2100 + list(CASES).index(name))
    Cn = D + (3 if use_xyz else 0)
    xyz = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    points = grid(rng, (B, N, D), 2.0 ** -5)
    if name == "scales":
        sc = np.array([1, 10, 100], np.float32).reshape(3, 1, 1)
        xyz, points = xyz * sc, points * sc
    alpha = grid(rng, (Cn,), 2.0 ** -6, 0.5, 1.5) * np.where(rng.uniform(size=Cn) < 0.25, -1, 1).astype(np.float32)
    beta = grid(rng, (Cn,), 2.0 ** -6, -0.5, 0.5)
    dout = rng.uniform(-1, 1, (B, S, K // ks, D + Cn)).astype(np.float32)
    if name == "stage1":     # a table of 61 values walked with strides prime to 61: every element differs from its neighbours, and it deflates
        b, s, k, c = np.ix_(*(np.arange(n) for n in dout.shape))
        dout = rng.uniform(-1, 1, 61).astype(np.float32)[(3 * b + 29 * s + 11 * k + 7 * c) % 61]
    res = grid(rng, (B, N, 4), 2.0 ** -5) if module == "pcm" else None
    return xyz, points, alpha, beta, dout, res


def record(classes, name, dtype, replay=None):
    module, B, N, S, D, K, mode, use_xyz, ks = CASES[name]
    xyz, points, alpha, beta, dout, res = inputs(name)
    kw = {"k_stride": ks} if module == "pcm" else {}
    m = classes[module](D, N // S, K, use_xyz=use_xyz, normalize=mode, **kw)
    if mode != "none":
        with torch.no_grad():
            m.affine_alpha.copy_(torch.from_numpy(alpha).view(1, 1, 1, -1))
            m.affine_beta.copy_(torch.from_numpy(beta).view(1, 1, 1, -1))
    m = m.to(dtype)
    SEEN.clear()
    if replay is not None:
        SEEN["replay"] = replay
    p = torch.from_numpy(points).to(dtype).requires_grad_(True)
    args = (torch.from_numpy(xyz).to(dtype), p) + ((torch.from_numpy(res).to(dtype),) if module == "pcm" else ())
    got = m(*args)
    (got[1] * torch.from_numpy(dout).to(dtype)).sum().backward()
    fps = SEEN.get("fps")
    if fps is not None and module == "pcm":
        fps = np.sort(fps, axis=-1)
    vals = {"out": got[1].detach().numpy(), "dpoints": p.grad.numpy()}
    if mode != "none":
        vals["dalpha"], vals["dbeta"] = m.affine_alpha.grad.numpy().reshape(-1), m.affine_beta.grad.numpy().reshape(-1)
    extra = {"new_xyz": got[0].detach().numpy(), "res": got[2].detach().numpy() if module == "pcm" else None}
    return vals, extra, fps, SEEN.get("idx")


def main():
    classes = load_reference()
    out, names = {}, []
    for name, (module, B, N, S, D, K, mode, use_xyz, ks) in CASES.items():
        names.append(name)
        xyz, points, alpha, beta, dout, res = inputs(name)
        v64, x64, fps, idx = record(classes, name, torch.float64)
        own32 = record(classes, name, torch.float32)[3]
        assert np.array_equal(np.sort(own32, -1), np.sort(idx, -1)), "the fp32 search selects other neighbours"
        v32 = record(classes, name, torch.float32, replay=idx)[0]
        assert (fps is None) == (S == N) and idx.shape == (B, S, K)
        assert all(np.isfinite(v).all() for v in list(v64.values()) + list(v32.values()))
        md = None if mode == "none" else mode
        case = {"fps": fps, "idx": idx, "k_stride": ks}
        uidx = GR.used_idx(case)
        # the fp64 restatement IS the reference's fp64 arithmetic, forward and gradient
        f64 = GR.forward_f64(xyz, points, fps, uidx, alpha, beta, md, use_xyz)
        r64 = dict(zip(GR.quantities(md), (f64[0],) + GR.backward_f64(xyz, points, fps, uidx, alpha, beta, dout, md, use_xyz)))
        for q in GR.quantities(md):
            assert GR.dist(r64[q], v64[q]) < 1e-12, (name, q, GR.dist(r64[q], v64[q]))
        assert np.array_equal(f64[1], x64["new_xyz"])
        cut = None
        if name == "stage1":
            dcols = (np.arange(0, D, 8) + np.arange(D // 8) % 8).astype(np.int32)
            cut = (np.arange(0, S, 8).astype(np.int32), np.concatenate([dcols, D + np.arange(3), D + 3 + dcols]).astype(np.int32), dcols)
            out.update(dict(zip(("stage1_rows", "stage1_cols", "stage1_dcols"), cut)))
        v64, v32 = GR.recorded(v64, cut), GR.recorded(v32, cut)
        out.update({f"{name}_module": np.asarray(module), f"{name}_mode": np.asarray(mode), f"{name}_use_xyz": np.asarray(use_xyz),
                    f"{name}_k_stride": np.asarray(ks), f"{name}_sample_ratio": np.asarray(N // S), f"{name}_xyz": xyz, f"{name}_points": points,
                    f"{name}_idx": idx, f"{name}_dout": dout, f"{name}_new_xyz64": x64["new_xyz"]})
        if fps is not None:
            out[f"{name}_fps"] = fps.astype(np.int32)
        if md is not None:
            out[f"{name}_alpha"], out[f"{name}_beta"] = alpha, beta
        if module == "pcm":
            out[f"{name}_points_res"], out[f"{name}_res64"] = res, x64["res"]
        for q in GR.quantities(md):
            out[f"{name}_{q}64"] = v64[q]
            out[f"{name}_yard_{q}"] = np.float64(GR.dist(v32[q], v64[q]))
        print(f"{name}: yardsticks " + " ".join(f"{q} {out[f'{name}_yard_{q}']:.3g}" for q in GR.quantities(md)))
    out["names"] = np.asarray(names)
    np.savez_compressed(GR.GOLDEN, **out)
    print("wrote", GR.GOLDEN, os.path.getsize(GR.GOLDEN), "bytes;", len(out), "keys")
    if "--tolerance" in sys.argv:
        write_tolerance(np.load(GR.GOLDEN, allow_pickle=False))


def write_tolerance(z):
    old = {}
    if os.path.exists(GR.TOLERANCE):
        with open(GR.TOLERANCE) as f:
            old = {c["case"]: c for c in json.load(f).get("cases", [])}
    rows, floors = [], {q: 0.0 for q in GR.QUANTITIES}
    for name in (str(n) for n in z["names"]):
        c = GR.golden_case(z, name)
        a = (c["xyz"], c["points"], c["fps"], GR.used_idx(c), c["alpha"], c["beta"])
        qs = GR.quantities(c["mode"])
        got = GR.recorded(dict(zip(qs, (GR.forward_kernel_f32(*a, c["mode"], c["use_xyz"])[0],)
                                   + GR.backward_kernel_f32(*a, c["dout"], c["mode"], c["use_xyz"]))), c["cut"])
        B, N, D = c["points"].shape
        row = {"case": name, "shape_BNSDK": [B, N, int(c["idx"].shape[1]), D, int(c["idx"].shape[2]) // c["k_stride"]]}
        for q in GR.QUANTITIES:
            if q not in qs:
                row[f"{q}_yardstick"] = row[f"{q}_restatement_f32"] = row[f"{q}_kernel_worst"] = None
                continue
            d = GR.dist(got[q], z[f"{name}_{q}64"])
            floors[q] = max(floors[q], d)
            row[f"{q}_yardstick"], row[f"{q}_restatement_f32"] = float(z[f"{name}_yard_{q}"]), d
            row[f"{q}_kernel_worst"] = old.get(name, {}).get(f"{q}_kernel_worst")
        rows.append(row)
    for r in rows:
        for q in GR.QUANTITIES:
            r[f"{q}_bar"] = None if r[f"{q}_yardstick"] is None else 2.0 * r[f"{q}_yardstick"] + floors[q]
    doc = {"unit": "max|x - reference fp64| / max|reference fp64|, per case, for out, d(points), d(alpha) and d(beta)",
           "rule": "bar = 2 x yardstick + floor.  yardstick: the reference's own fp32 run of its LocalGrouper against its fp64 run on the same "
                   "neighbours, per case.  floor: the largest distance of the fp32 restatement in the kernels' order "
                   "(tests/local_grouper_ref.py) from the fp64 record over the golden cases, per quantity, measured on the CPU.  A shape "
                   "without a recorded case takes its yardstick on the spot: the reference's lines in torch in fp32 against the fp64 "
                   "restatement.",
           "floors": floors, "cases": rows,
           "kernel_worst_source": "tests/test_gpu_local_grouper.py::test_golden_cases on one MI355X (the largest figure it prints over the "
                                  "input and output layouts), same unit"}
    os.makedirs(os.path.dirname(GR.TOLERANCE), exist_ok=True)
    with open(GR.TOLERANCE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", GR.TOLERANCE)
    print(floors)


if __name__ == "__main__":
    main()
