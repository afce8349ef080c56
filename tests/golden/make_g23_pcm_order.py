#!/usr/bin/env python3
"""Generates tests/golden/g23_pcm_order.npz: the reference's OWN `serialization` (openpoints/models/PCM/PCM_utils.py:21-47) and `encode`
(openpoints/models/PCM/serialization.py) run on the CPU, for unipre3d_amd/pcm_order.py and tests/pcm_order_ref.py.

Stub: addict.Dict (an attribute dict).  Per case the inputs (pos, feat, x_res, grid_size), the orders run, and stacked over those
orders the reference's code (K, B N) and its reordered pos | feat | x_res side by side as rows (K, B N, 6).  Only recorded data is stored.

  orders     the nine shipped orders on a random cloud, B = 3, N = 64 (many equal codes: the reference's own order among them is its
             argsort's accident, so only the code and its monotony are comparable)
  tiefree    every axis of every item is a permutation of N distinct cells: no two codes are equal (asserted per order), the
             reference's reordered tensors are comparable bit for bit
  boundary   pos = k * float32(grid_size) for integer k: where x / g and x * (1 / g) floor differently (xyz, hilbert, z)
  planar     y constant and an odd largest z cell: under xyz the codes are negative and, the batch stride being 0, the items interleave
             (xyz, xzy, hilbert)
  onecell    the whole batch in one cell, depth 0 (xyz, z, and hilbert, on which the reference raises: its encode cannot take zero bits)
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

REF = "/root/reference/openpoints/models/PCM"
OUT = os.path.dirname(os.path.abspath(__file__))
SHIPPED = ("xyz", "xzy", "yxz", "yzx", "zxy", "zyx", "hilbert", "z", "z-trans")
GRID = 0.02
CASE_ORDERS = {"orders": SHIPPED, "tiefree": SHIPPED, "boundary": ("xyz", "hilbert", "z"), "planar": ("xyz", "xzy", "hilbert"),
               "onecell": ("xyz", "hilbert", "z")}


class Dict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def reference():
    sys.modules["addict"] = types.ModuleType("addict")
    sys.modules["addict"].Dict = Dict
    pk = types.ModuleType("pcm_ref")
    pk.__path__ = [REF]
    sys.modules["pcm_ref"] = pk
    mods = {}
    for name in ("z_order", "hilbert", "serialization", "PCM_utils"):
        spec = importlib.util.spec_from_file_location("pcm_ref." + name, os.path.join(REF, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["pcm_ref." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["serialization"], mods["PCM_utils"]


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.require(arrays[name], requirements="C"), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            zf.writestr(info, buf.getvalue())


def clouds():
    g = torch.Generator().manual_seed(23)
    gs = np.float32(GRID)
    out = {"orders": torch.rand(3, 64, 3, generator=g)}
    perm = torch.stack([torch.stack([torch.randperm(32, generator=g) for _ in range(3)], 1) for _ in range(2)])     # (2, 32, 3)
    out["tiefree"] = (perm.float() + 0.5) * float(gs) - 0.3
    k = torch.randint(0, 41, (2, 64, 3), generator=g)
    out["boundary"] = torch.from_numpy(k.numpy().astype(np.float32) * gs)
    planar = torch.rand(2, 48, 3, generator=g) * 0.3
    planar[:, :, 1] = 0.123
    planar[:, 0, 2], planar[:, 1, 2] = 0.001, 0.001 + 7 * GRID                         # largest z cell 7 in both items
    planar[:, 2:, 2] = planar[:, 2:, 2].clamp(0.005, 0.13)
    out["planar"] = planar
    out["onecell"] = 0.001 + 0.017 * torch.rand(2, 16, 3, generator=g)
    return out


def main():
    ser, utils = reference()
    g = torch.Generator().manual_seed(2300)
    arrays, report = {"grid_size": np.float64(GRID)}, []
    for case, pos in clouds().items():
        B, N, _ = pos.shape
        feat, x_res = torch.randn(B, N, 2, generator=g), torch.randn(B, N, 1, generator=g)
        arrays.update({f"{case}/pos": pos.numpy(), f"{case}/feat": feat.numpy(), f"{case}/x_res": x_res.numpy()})
        cell = torch.floor(pos / GRID).to(torch.int64)
        cell = (cell - cell.min(dim=1, keepdim=True)[0]).flatten(0, 1)
        batch = torch.arange(B).repeat_interleave(N)
        depth = int(cell.max()).bit_length()
        done, codes, rows = [], [], []
        for order in CASE_ORDERS[case]:
            try:
                code = ser.encode(cell, batch, depth, order=order)
                extra = [feat.clone()]
                p, f, x = utils.serialization(pos.clone(), feat.clone(), x_res.clone(), order=order, layers_outputs=extra, grid_size=GRID)
            except Exception as e:                       # the reference itself cannot run this order on this cloud
                assert case == "onecell", (case, order, e)
                report.append(f"{case}/{order}: reference raises {type(e).__name__}")
                continue
            assert torch.equal(extra[0], f) and code.dtype == torch.int64 and code.shape == (B * N,)
            if case == "tiefree":
                assert code.unique().numel() == code.numel(), (case, order)
            codes.append(code.numpy())
            rows.append(torch.cat([p, f, x], 2).flatten(0, 1).numpy())
            done.append(order)
            report.append(f"{case}/{order}: depth {depth}, {code.unique().numel()} distinct of {code.numel()}, min {int(code.min())}")
        arrays.update({f"{case}/orders": np.asarray(done), f"{case}/code": np.stack(codes), f"{case}/rows": np.stack(rows)})
        arrays[f"{case}/depth"] = np.int64(depth)
    planar = arrays["planar/code"][0]
    assert planar.min() < 0 and arrays["onecell/depth"] == 0 and arrays["onecell/orders"].tolist() == ["xyz", "z"]
    first = planar[:48]
    assert first.max() >= planar[48:].min()              # the two items' code ranges overlap: they interleave once sorted
    path = os.path.join(OUT, "g23_pcm_order.npz")
    save(path, arrays)
    print("\n".join(report))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
