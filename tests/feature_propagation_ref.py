"""CPU restatements of the feature propagation of unipre3d_amd/feature_propagation.py (numpy; xyz1 (B, N, 3), xyz2 (B, S, 3), points1
(B, D1, N) or None, points2 (B, D2, S), out and dout (B, D1 + D2, N)), the contract of include/unipre3d_feature_propagation.h:

  search(xyz1, xyz2, dt)            idx (B, N, 3) int32, weight (B, N, 3) in dt: direct squared distances (dx dx + dy dy) + dz dz, the three
                                    smallest (d2, index) pairs in lexicographic order, r = 1 / (d2 + 1e-8), w = r / ((r0 + r1) + r2), every
                                    operation rounded in dt (np.float32: the kernels' arithmetic; np.float64: the yardstick)
  forward(...)                      out = cat(points1, (w0 p[i0] + w1 p[i1]) + w2 p[i2]) in dt
  inverse_lists(idx, S)             ptr (B, S + 1), ent (B, 3N): entries 3 n + j ascending inside a list, the out-of-range ones last
  backward(...)                     dpoints2 over the lists in ascending order: exact products, an f64 sum, rounded to dt once
  reference_form(...)               the reference's lines (matmul-form distances, full sort, gather, sum, cat, permute) in torch
  RefPropagate                      the restatement as a torch autograd function on the CPU, for the whole-module floors

and the tolerance rule of profiles/feature_propagation/tolerance.json: bar = 2 x floor per quantity, in max|x - fp64| / max|fp64|, where
the floor is the largest distance of the fp32 restatement from the fp64 record over the golden cases; the whole-module cases keep
bar = 2 x yardstick + floor."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g22_feature_propagation.npz")
TOLERANCE = os.path.join(ROOT, "profiles", "feature_propagation", "tolerance.json")
QUANTITIES = ("out", "dpoints2")
MODULE_QUANTITIES = ("out", "dpoints1", "dpoints2", "dparams")
f32, f64 = np.float32, np.float64


def dist(x, ref64):
    """max|x - fp64| / max|fp64| (the unit of every figure of the tolerance file)."""
    ref64 = np.asarray(ref64, f64)
    return float(np.abs(np.asarray(x, f64) - ref64).max() / max(np.abs(ref64).max(), 1e-300))


def params_dist(got, ref64):
    """The largest dist over a module's parameter gradients.  A gradient that is zero but for fp64 rounding (below 1e-9 of the module's
    largest: a convolution's bias in front of a BatchNorm in training mode) is measured against that largest gradient, not its own noise."""
    top = max(float(np.abs(r).max()) for r in ref64)
    scale = lambda r: float(np.abs(r).max()) if np.abs(r).max() >= 1e-9 * top else top
    return max(float(np.abs(np.asarray(g, f64) - r).max()) / scale(r) for g, r in zip(got, ref64))


def search(xyz1, xyz2, dt=f32):
    q, s = np.asarray(xyz1, f32).astype(dt), np.asarray(xyz2, f32).astype(dt)
    B, N, S = q.shape[0], q.shape[1], s.shape[1]
    if S == 2:
        raise ValueError("S = 2: three neighbours need three support points")
    if S == 1:
        w = np.zeros((B, N, 3), dt)
        w[:, :, 0] = 1
        return np.zeros((B, N, 3), np.int32), w
    d = q[:, :, None, :] - s[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    idx = np.argsort(d2, axis=-1, kind="stable")[:, :, :3]               # stable: equal distances keep the lower index first
    d3 = np.take_along_axis(d2, idx, axis=-1)
    r = dt(1) / (d3 + dt(1e-8))
    w = r / ((r[..., 0] + r[..., 1]) + r[..., 2])[..., None]
    assert d2.dtype == dt and w.dtype == dt
    return idx.astype(np.int32), w


def _gather(points2, idx, S):
    """(p (B, D2, N, 3), valid (B, 1, N, 3)): the three rows per query; an index outside [0, S) is never used."""
    idx = np.asarray(idx).astype(np.int64)
    valid = (idx >= 0) & (idx < S)
    safe = np.where(valid, idx, 0)
    B, D2 = points2.shape[:2]
    return points2[np.arange(B)[:, None, None, None], np.arange(D2)[None, :, None, None], safe[:, None]], valid[:, None]


def forward(xyz1, xyz2, points1, points2, dt=f32, neighbours=None):
    """-> out (B, D1 + D2, N) in dt, idx, weight."""
    idx, w = search(xyz1, xyz2, dt) if neighbours is None else (np.asarray(neighbours[0]), np.asarray(neighbours[1], f32).astype(dt))
    p2 = np.asarray(points2, f32).astype(dt)
    p, valid = _gather(p2, idx, p2.shape[2])
    t = np.where(valid, w[:, None] * p, dt(0))
    inter = (t[..., 0] + t[..., 1]) + t[..., 2]
    assert inter.dtype == dt
    out = inter if points1 is None else np.concatenate([np.asarray(points1, f32).astype(dt), inter], axis=1)
    return out, idx, w


def inverse_lists(idx, S):
    idx = np.asarray(idx).astype(np.int64)
    B, N, _ = idx.shape
    target = np.where((idx >= 0) & (idx < S), idx, S).reshape(B, 3 * N)
    ent = np.argsort(target, axis=1, kind="stable").astype(np.int32)
    ptr = np.zeros((B, S + 1), np.int32)
    for b in range(B):
        ptr[b, 1:] = np.cumsum(np.bincount(target[b], minlength=S + 1)[:S])
    return ptr, ent


def brute_force_lists(idx, S):
    """The same lists, entry by entry."""
    idx = np.asarray(idx)
    B, N, _ = idx.shape
    ptr, ent = np.zeros((B, S + 1), np.int32), np.zeros((B, 3 * N), np.int32)
    for b in range(B):
        lists = [[] for _ in range(S + 1)]
        for e in range(3 * N):
            v = int(idx[b, e // 3, e % 3])
            lists[v if 0 <= v < S else S].append(e)
        ent[b] = np.asarray([e for li in lists for e in li], np.int32)
        ptr[b, 1:] = np.cumsum([len(li) for li in lists[:S]])
    return ptr, ent


def backward(idx, weight, dout, D1, S, dt=f32):
    """-> dpoints2 (B, D2, S) in dt: per support point the sum over its list in ascending entry order, in f64, rounded once."""
    idx, w = np.asarray(idx).astype(np.int64), np.asarray(weight).astype(f64)
    g = np.asarray(dout, f32).astype(f64)[:, D1:, :]
    B, D2, N = g.shape
    target = np.where((idx >= 0) & (idx < S), idx, S).reshape(B, 3 * N)
    acc = np.zeros((B, S + 1, D2), f64)
    for b in range(B):
        contrib = w[b].reshape(3 * N, 1) * np.repeat(g[b].T, 3, axis=0)       # (3N, D2), entry e = 3 n + j
        np.add.at(acc[b], target[b], contrib)                                 # unbuffered: in ascending e
    return np.ascontiguousarray(acc[:, :S, :].transpose(0, 2, 1)).astype(dt)


def restatement(xyz1, xyz2, points1, points2, dout, dt=f32, neighbours=None):
    """{out, dpoints2, idx, weight} in dt."""
    out, idx, w = forward(xyz1, xyz2, points1, points2, dt, neighbours)
    D1 = 0 if points1 is None else np.asarray(points1).shape[1]
    return {"out": out, "dpoints2": backward(idx, w, dout, D1, np.asarray(xyz2).shape[1], dt), "idx": idx, "weight": w}


def reference_form(xyz1, xyz2, points1, points2):
    """The reference's forward lines in torch (any device, any floating type), with autograd."""
    import torch
    p2 = points2.permute(0, 2, 1)
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    if S == 1:
        inter = p2.repeat(1, N, 1)
    else:
        d = -2 * torch.matmul(xyz1, xyz2.permute(0, 2, 1))
        d += torch.sum(xyz1 ** 2, -1).view(B, N, 1)
        d += torch.sum(xyz2 ** 2, -1).view(B, 1, S)
        d, idx = d.sort(dim=-1)
        d, idx = d[:, :, :3], idx[:, :, :3]
        r = 1.0 / (d + 1e-8)
        w = r / torch.sum(r, dim=2, keepdim=True)
        rows = p2[torch.arange(B, device=idx.device).view(B, 1, 1), idx, :]
        inter = torch.sum(rows * w.view(B, N, 3, 1), dim=2)
    new = inter if points1 is None else torch.cat([points1.permute(0, 2, 1), inter], dim=-1)
    return new.permute(0, 2, 1)


def ref_propagate(xyz1, xyz2, points1, points2):
    """The fp32 restatement as a differentiable torch function on the CPU (the whole-module floors run the modules on it)."""
    import torch

    class RefPropagate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, p1, p2):
            out, idx, w = forward(xyz1.numpy(), xyz2.numpy(), None if p1 is None else p1.detach().numpy(), p2.detach().numpy(), f32)
            ctx.meta = (idx, w, 0 if p1 is None else p1.shape[1], xyz2.shape[1])
            return torch.from_numpy(np.ascontiguousarray(out))

        @staticmethod
        def backward(ctx, dout):
            idx, w, D1, S = ctx.meta
            d2 = torch.from_numpy(backward(idx, w, dout.contiguous().numpy(), D1, S, f32))
            return (dout[:, :D1, :] if D1 else None), d2

    return RefPropagate.apply(points1, points2)


# ---- the record ------------------------------------------------------------------------------------------------------------------
def golden_case(z, name):
    c = {k: z[f"{name}_{k}"] for k in ("xyz1", "xyz2", "points2", "dout", "idx64")}
    c["points1"] = z[f"{name}_points1"] if f"{name}_points1" in z.files else None
    c["cut"] = tuple(z[f"{name}_{k}"] for k in ("rows", "cols", "dcols")) if f"{name}_rows" in z.files else None
    return c


def recorded(vals, cut, D1):
    """out and dpoints2 as the record holds them: whole, or (the stage case) out at queries `rows` and channels `cols`, dpoints2 at the
    interpolated channels `dcols`."""
    if cut is None:
        return {q: vals[q] for q in QUANTITIES}
    rows, cols, dcols = cut
    return {"out": vals["out"][:, cols][:, :, rows], "dpoints2": vals["dpoints2"][:, dcols]}


def module_run(z, name, propagate, device="cpu"):
    """The project's module of case `name` with the recorded state_dict, on `propagate`'s result -> {out, dpoints1, dpoints2, dparams}."""
    import torch
    from unipre3d_amd import feature_propagation as fp
    kind, blocks = str(z[f"{name}_kind"]), int(z[f"{name}_blocks"])
    m = fp.PointNetFeaturePropagation(24, 16, blocks=blocks) if kind == "pointmlp" else fp.PCMPointNetFeaturePropagation(24, 16, blocks=blocks)
    m.load_state_dict({str(k): torch.from_numpy(z[f"{name}_sd_{i}"]) for i, k in enumerate(z[f"{name}_sd_names"])}, strict=True)
    m = m.to(device).train()
    t = lambda k, g=False: torch.from_numpy(z[f"{name}_{k}"]).to(device).requires_grad_(g)
    p1, p2 = t("points1", True), t("points2", True)
    out = m.extraction(m.fuse(propagate(t("xyz1"), t("xyz2"), p1, p2)))
    (out * t("dout")).sum().backward()
    params = dict(m.named_parameters())
    return {"out": out.detach().cpu().numpy(), "dpoints1": p1.grad.cpu().numpy(), "dpoints2": p2.grad.cpu().numpy(),
            "dparams": [params[str(k)].grad.cpu().numpy() for k in z[f"{name}_param_names"]]}


def module_dists(z, name, got):
    d = {q: dist(got[q], z[f"{name}_{q}_64" if q != "out" else f"{name}_out64"]) for q in ("out", "dpoints1", "dpoints2")}
    d["dparams"] = params_dist(got["dparams"], [z[f"{name}_dparam_{i}"] for i in range(len(got["dparams"]))])
    return d


def tolerance():
    with open(TOLERANCE) as f:
        return json.load(f)


def bars(tol):
    """{quantity: 2 x floor}."""
    return {q: 2.0 * tol["floors"][q] for q in QUANTITIES}


def module_bars(case, tol):
    row = next(r for r in tol["module_cases"] if r["case"] == case)
    return {q: row[f"{q}_bar"] for q in MODULE_QUANTITIES}
