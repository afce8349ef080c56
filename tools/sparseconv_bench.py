#!/usr/bin/env python3
"""Sparse 3D convolution (unipre3d_amd.sparseconv): forward, input gradient and weight gradient of each conv of a SpUNet-shaped
encoder / decoder at its level shapes on unipre3d_amd.synthetic.sparse_voxel_scene (2 items, about 230 k voxels at level 0), plus the
whole stack of tests/test_gpu_sparseconv.py::test_spunet_stack_at_c5_scale (forward + backward).  Next to each, the torch restatement
in fp32 on the same device in the same run: per tap gather + matmul + index_add over precomputed pair lists (no host sync), its
gradients by autograd.

Effective TFLOP/s counts 2 * pairs * Cin * Cout (pairs = non-empty (output, tap) entries) against the 157 TF fp32 peak; gather bytes
are the gathered input rows (pairs * Cin), the rows written (rows * Cout) and the weight, 4 B each, against 8 TB/s.  Maps are built
once before timing (their cost is a row of its own).  One JSON line per row to --out (default profiles/sparseconv/sparseconv_bench.jsonl)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK, HBM = 157.3e12, 8.0e12


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e6


def _torch_conv(X, W, lists, rows_out):
    """Y = sum over taps of index_add(out_rows, X[src_rows] @ W_t): the restatement's gather + matmul + index_add."""
    Cout, Cin = W.shape[0], W.shape[-1]
    W3 = W.reshape(Cout, -1, Cin)
    Y = X.new_zeros(rows_out, Cout)
    for t, (o, s) in enumerate(lists):
        if o.numel():
            Y = Y.index_add(0, o, X[s] @ W3[:, t, :].t())
    return Y


def conv_lists(kind, m):
    if kind == "subm":
        T = m.table.long()
        out = []
        for t in range(T.shape[1]):
            o = torch.nonzero(T[:, t] >= 0).flatten()
            out.append((o, T[o, t]))
        return out, T.shape[0]
    K = m.k ** 3
    src = m.list_src.long()
    row = m.list_row.long()
    out = []
    for t in range(K):
        sel = torch.nonzero((src >= 0) & (src % K == t)).flatten()
        o, i = src[sel] // K, row[sel]
        out.append((o, i) if kind == "down" else (i, o))
    return out, (m.table.shape[0] if kind == "down" else row.shape[0])


def bench_conv(name, kind, conv, x, iters, warmup):
    y = conv(x)                                   # builds (or reuses) the map
    m = x.indice_dict[conv.indice_key]
    lists, rows_out = conv_lists(kind, m)
    pairs = sum(int(o.numel()) for o, _ in lists)
    Cin, Cout = conv.in_channels, conv.out_channels
    X = x.features.detach().requires_grad_(True)
    xx = x.replace_feature(X)
    gY = torch.randn_like(y.features)
    res = {"row": name, "kind": kind, "k": conv.kernel_size, "Cin": Cin, "Cout": Cout, "rows_in": int(x.features.shape[0]),
           "rows_out": int(y.features.shape[0]), "pairs": pairs, "taps": len(lists)}
    flops = 2.0 * pairs * Cin * Cout
    W = conv.weight
    with torch.no_grad():
        t_fwd = _time(lambda: conv(x), iters, warmup)
        r_fwd = _time(lambda: _torch_conv(x.features, W, lists, rows_out), iters, warmup)

    def dx():
        conv.weight.requires_grad_(False)
        torch.autograd.grad(conv(xx).features, X, gY)
        conv.weight.requires_grad_(True)

    def dw():
        torch.autograd.grad(conv(x).features, conv.weight, gY)

    Xr = x.features.detach().requires_grad_(True)
    Wr = W.detach().requires_grad_(True)
    t_dx = _time(dx, iters, warmup) - t_fwd
    t_dw = _time(dw, iters, warmup) - t_fwd
    r_dx = _time(lambda: torch.autograd.grad(_torch_conv(Xr, W.detach(), lists, rows_out), Xr, gY), iters, warmup) - r_fwd
    r_dw = _time(lambda: torch.autograd.grad(_torch_conv(x.features, Wr, lists, rows_out), Wr, gY), iters, warmup) - r_fwd
    gather = 4.0 * (pairs * Cin + res["rows_out"] * Cout + W.numel())
    for part, t, r in (("fwd", t_fwd, r_fwd), ("dx", t_dx, r_dx), ("dw", t_dw, r_dw)):
        res[f"{part}_us"] = round(t, 2)
        res[f"{part}_tflops"] = round(flops / (t * 1e-6) / 1e12, 2)
        res[f"{part}_frac_peak"] = round(flops / (t * 1e-6) / PEAK, 3)
        res[f"{part}_frac_hbm"] = round(gather / (t * 1e-6) / HBM, 3)
        res[f"{part}_torch_us"] = round(r, 2)
        res[f"{part}_speedup"] = round(r / t, 2)
    return y, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparseconv", "sparseconv_bench.jsonl"))
    a = ap.parse_args()
    from unipre3d_amd import sparseconv as sp
    from unipre3d_amd import synthetic
    dev = torch.device("cuda:0")
    sc = synthetic.sparse_voxel_scene(batch=2, seed=0)
    torch.manual_seed(0)
    x = sp.SparseConvTensor(sc["features"].to(dev), sc["indices"].to(dev), sc["spatial_shape"], sc["batch_size"])
    rows = []
    # map construction
    idx = x.indices
    t_subm = _time(lambda: sp.subm_map(idx, x.spatial_shape, 2, 3), a.iters, a.warmup)
    t_down = _time(lambda: sp.down_map(idx, x.spatial_shape, 2, 2), a.iters, a.warmup)
    rows.append({"row": "maps_level0", "rows_in": int(idx.shape[0]), "subm_k3_map_us": round(t_subm, 2), "down_s2_map_us": round(t_down, 2)})
    chans = [32, 64, 128, 256]
    convs = {}

    def mk(name, cls, *args, **kw):
        convs[name] = cls(*args, **kw).to(dev)
        return convs[name]

    skips = []
    y, r = bench_conv("stem_k5_6_32", "subm", mk("stem", sp.SubMConv3d, 6, 32, 5, padding=1, bias=False, indice_key="stem"), x, a.iters, a.warmup)
    rows.append(r)
    cur = y
    for lv, c in enumerate(chans):
        cin = cur.features.shape[1]
        if lv > 0:
            cur, r = bench_conv(f"down_l{lv - 1}_{cin}_{c}", "down", mk(f"down{lv}", sp.SparseConv3d, cin, c, 2, stride=2, bias=False,
                                                                         indice_key=f"spconv{lv}"), cur, a.iters, a.warmup)
            rows.append(r)
        cur, r = bench_conv(f"subm_l{lv}_{c}_{c}", "subm", mk(f"enc{lv}", sp.SubMConv3d, c, c, 3, padding=1, bias=False,
                                                             indice_key=f"subm{lv}"), cur.replace_feature(cur.features.detach()),
                            a.iters, a.warmup)
        rows.append(r)
        skips.append(cur)
    for lv in range(len(chans) - 1, 0, -1):
        cin, cout = cur.features.shape[1], chans[lv - 1]
        cur, r = bench_conv(f"inverse_l{lv}_{cin}_{cout}", "inv", mk(f"up{lv}", sp.SparseInverseConv3d, cin, cout, 2, bias=False,
                                                                       indice_key=f"spconv{lv}"), cur, a.iters, a.warmup)
        rows.append(r)
        cur = cur.replace_feature(torch.cat([cur.features, skips[lv - 1].features], 1).detach())
    cur, r = bench_conv("final_k1_64_13", "subm", mk("final", sp.SubMConv3d, cur.features.shape[1], 13, 1, bias=True,
                                                     indice_key="final"), cur, a.iters, a.warmup)
    rows.append(r)

    # the whole SpUNet-shaped stack of the GPU test (maps cached after the first call), forward + backward
    stem, down, enc = convs["stem"], convs["down1"], convs["enc1"]
    up = sp.SparseInverseConv3d(64, 32, 2, indice_key="spconv1", bias=False).to(dev)
    dec = sp.SubMConv3d(64, 32, 3, padding=1, bias=False, indice_key="subm0").to(dev)
    final = sp.SubMConv3d(32, 13, 1, bias=True, indice_key="final1").to(dev)
    X = x.features.detach().requires_grad_(True)

    def stack():
        x0 = stem(x.replace_feature(X))
        u = up(enc(down(x0)))
        y = final(dec(u.replace_feature(torch.cat([u.features, x0.features], 1))))
        y.features.sum().backward()

    t_stack = _time(stack, a.iters, a.warmup)
    rows.append({"row": "spunet_stack_fwd_bwd", "rows_in": int(x.features.shape[0]), "us": round(t_stack, 2)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
