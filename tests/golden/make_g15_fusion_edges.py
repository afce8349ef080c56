#!/usr/bin/env python3
"""Generates tests/golden/g15_fusion_edges.npz: the reference's OWN object-level FeatureFusion (fusion/feat_fusion.py, loaded from the
reference checkout with importlib and run as is on the CPU) on the edge set of tests/fusion_ref.py::edge_points.

Per image size (H, W) of fusion_ref.SIZES, tag "HxW": B = 2 (item 1 holds item 0's points in reverse order), C = 5, Cx = 3, identity
row-vector c2w, fx = fy = 1, cx = cy = 0, an identity fusion MLP, and both widths of x: with the transformer's CLS token (N + 1 rows,
suffix _cls) and without (N rows, the same x and cotangents minus row 0, suffix _plain).  Stored: center, feat, x, intr, the outputs, a
Gaussian and an integer-valued (|values| <= 8, stored as int8) cotangent, and the gradient with respect to the feature map under each.

The archive is written member by member with a fixed timestamp, so that a second run gives the same bytes.
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

REF = os.environ.get("U3D_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import fusion_ref as R  # noqa: E402

C, CX = 5, 3


def reference_module():
    spec = importlib.util.spec_from_file_location("ref_feat_fusion", os.path.join(REF, "fusion/feat_fusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ff = reference_module().FeatureFusion(torch.nn.Identity())
    intr = np.zeros((3, 4)); intr[0, 0] = intr[1, 1] = intr[2, 2] = 1.0
    out = {"intr": intr}
    for H, W in R.SIZES:
        tag = f"{H}x{W}"
        g = torch.Generator().manual_seed(1500 + 31 * H + W)
        pts = torch.tensor(R.edge_points(H, W)[:, :3])
        center = torch.stack([pts, pts.flip(0)])
        B, N = center.shape[:2]
        c2w = torch.eye(4).repeat(B, 1, 1)
        feat = torch.randn(B, C, H, W, generator=g)
        x = torch.randn(B, N + 1, CX, generator=g)
        w = torch.randn(B, N + 1, CX + C, generator=g)
        wi = torch.randint(-8, 9, (B, N + 1, CX + C), generator=g).float()
        out.update({f"{tag}_center": center.numpy(), f"{tag}_feat": feat.numpy(), f"{tag}_x": x.numpy(), f"{tag}_w": w.numpy(),
                    f"{tag}_wi": wi.numpy().astype(np.int8)})
        for kind, lo in (("cls", 0), ("plain", 1)):
            f = feat.clone().requires_grad_(True)
            y = ff(x[:, lo:], center, f, c2w, intr)
            assert y.shape == (B, N + 1 - lo, CX + C)
            (gw,) = torch.autograd.grad((y * w[:, lo:]).sum(), f, retain_graph=True)
            (gi,) = torch.autograd.grad((y * wi[:, lo:]).sum(), f)
            out.update({f"{tag}_out_{kind}": y.detach().numpy(), f"{tag}_gfeat_{kind}": gw.numpy(), f"{tag}_gfeat_int_{kind}": gi.numpy()})
        print(f"g15 {tag}: N = {N}, {int((y[..., CX:] != 0).any(-1).sum())} winners")
    path = os.path.join(OUT, "g15_fusion_edges.npz")
    save(path, out)
    print("g15_fusion_edges.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
