"""CPU restatements of the dense attention of unipre3d_amd/mha.py (numpy; qkv (B, N, 3, H, D), out (B, N, H, D), lse (B, H, N)):

  forward_f64 / backward_f64           fp64, the plain formulas
  forward_kernel_f32 / backward_kernel_f32   fp32 in the kernel's order: dot products as k-ordered fma chains, an online softmax over
                                       blocks of 64 keys, exp2 with the scale folded into the exponent, P recomputed from lse
  reference_form                       the reference's four torch lines in fp32 (or fp64) with autograd's backward

and the tolerance rule of profiles/mha/tolerance.json: bar = 2 x yardstick + floor, in max|x - fp64| / max|fp64|."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g19_dense_attention.npz")
TOLERANCE = os.path.join(ROOT, "profiles", "mha", "tolerance.json")
CASES = ("object", "one", "odd17", "sharp17", "huge9")
BLOCK = 64
LOG2E = np.float32(1.4426950408889634)
f32 = np.float32


def default_scale(D=64):
    return float(D) ** -0.5


def dist(x, ref64):
    """max|x - fp64| / max|fp64| (the unit of every figure of the tolerance file)."""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - ref64).max() / max(np.abs(ref64).max(), 1e-300))


# ---- (a) fp64 ----------------------------------------------------------------------------------------------------------------
def forward_f64(qkv, scale=None):
    x = np.asarray(qkv, np.float64)
    scale = default_scale(x.shape[-1]) if scale is None else scale
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))           # (B, H, N, D)
    s = scale * (q @ k.transpose(0, 1, 3, 2))
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    out = (e / l) @ v
    return out.transpose(0, 2, 1, 3), (m + np.log(l))[..., 0]


def backward_f64(qkv, dout, scale=None):
    x = np.asarray(qkv, np.float64)
    scale = default_scale(x.shape[-1]) if scale is None else scale
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    do = np.asarray(dout, np.float64).transpose(0, 2, 1, 3)
    s = scale * (q @ k.transpose(0, 1, 3, 2))
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = p @ v
    dv = p.transpose(0, 1, 3, 2) @ do
    dp = do @ v.transpose(0, 1, 3, 2)
    ds = p * (dp - (do * o).sum(-1, keepdims=True))
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(0, 1, 3, 2) @ q)
    return np.stack([g.transpose(0, 2, 1, 3) for g in (dq, dk, dv)], axis=2)


# ---- (b) fp32 in the kernel's order ------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding
    that differs from a true fma in rare last-bit ties only)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _chain(a, b, acc=None):
    """acc + sum_k a[..., i, k] b[..., j, k] as a k-ordered fp32 fma chain (what v_mfma_f32_16x16x4_f32 computes) -> (..., i, j)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    out = np.zeros(a.shape[:-1] + (b.shape[-2],), f32) if acc is None else acc.astype(f32)
    for kk in range(a.shape[-1]):
        out = _fma(a[..., :, None, kk], b[..., None, :, kk], out)
    return out


def _exp2(x):
    return np.exp2(x.astype(f32)).astype(f32)


def forward_kernel_f32(qkv, scale=None):
    x = np.asarray(qkv, f32)
    B, N, _, H, D = x.shape
    scale = f32(default_scale(D) if scale is None else scale)
    c = f32(scale * LOG2E)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    m = np.full((B, H, N), -np.inf, f32)
    l = np.zeros((B, H, N), f32)
    o = np.zeros((B, H, N, D), f32)
    for kb in range(0, N, BLOCK):
        ke = min(kb + BLOCK, N)
        s = _chain(q, k[:, :, kb:ke])
        mn = np.maximum(m, s.max(-1))
        alpha = _exp2((m - mn) * c)
        p = _exp2(_fma(s, c, -(mn * c)[..., None]))
        l = _fma(l, alpha, p.sum(-1, dtype=f32))
        o = _fma(o, alpha[..., None], _chain(p, v[:, :, kb:ke].transpose(0, 1, 3, 2)))    # the block's sum in a chain of its own
        m = mn
    out = o * (f32(1) / l)[..., None]
    lse = _fma(m, scale, np.log(l).astype(f32))
    return out.transpose(0, 2, 1, 3), lse


def backward_kernel_f32(qkv, dout, scale=None, out=None, lse=None):
    x = np.asarray(qkv, f32)
    D = x.shape[-1]
    scale = f32(default_scale(D) if scale is None else scale)
    c = f32(scale * LOG2E)
    if out is None:
        out, lse = forward_kernel_f32(x, scale)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    do = np.asarray(dout, f32).transpose(0, 2, 1, 3)
    o = np.asarray(out, f32).transpose(0, 2, 1, 3)
    delta = _chain(do[..., None, :], o[..., None, :])[..., 0, 0]                     # (B, H, N)
    s = _chain(q, k)
    p = _exp2(_fma(s, c, -(np.asarray(lse, f32) * LOG2E)[..., None]))
    dp = _chain(do, v)
    ds = p * (dp - delta[..., None])
    dv = _chain(p.transpose(0, 1, 3, 2), do.transpose(0, 1, 3, 2))
    dq = _chain(ds, k.transpose(0, 1, 3, 2)) * scale
    dk = _chain(ds.transpose(0, 1, 3, 2), q.transpose(0, 1, 3, 2)) * scale
    return np.stack([g.transpose(0, 2, 1, 3) for g in (dq, dk, dv)], axis=2)


# ---- (c) the reference's form ------------------------------------------------------------------------------------------------
def reference_form(qkv, dout=None, scale=None, dtype="float32"):
    """q, k, v by the reference's permute, (q @ k^T) * scale, softmax(dim=-1), (attn @ v).transpose(1, 2) -- in torch on the CPU.
    Returns out (B, N, H, D), and d(qkv) through autograd when dout is given."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(qkv)).to(getattr(torch, dtype)).requires_grad_(dout is not None)
    scale = default_scale(t.shape[-1]) if scale is None else scale
    p = t.permute(2, 0, 3, 1, 4)
    q, k, v = p[0], p[1], p[2]
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.softmax(dim=-1)
    out = (attn @ v).transpose(1, 2)
    if dout is None:
        return out.detach().numpy()
    out.backward(torch.from_numpy(np.ascontiguousarray(dout)).to(t.dtype))
    return out.detach().numpy(), t.grad.numpy()


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def tolerance():
    with open(TOLERANCE) as f:
        return json.load(f)


def bars(yard_out, yard_dqkv, tol=None):
    """(bar for out, bar for dqkv) = 2 x yardstick + floor."""
    fl = (tolerance() if tol is None else tol)["floors"]
    return 2.0 * yard_out + fl["out"], 2.0 * yard_dqkv + fl["dqkv"]


def case_bars(name, tol=None):
    tol = tolerance() if tol is None else tol
    row = {r["case"]: r for r in tol["cases"]}[name]
    return bars(row["out_yardstick"], row["dqkv_yardstick"], tol)


def spot_bars(qkv, dout, scale=None, tol=None):
    """For a shape without a record: the yardstick on the spot (reference_form fp32 against the fp64 restatement).
    Returns (out64, dqkv64, bar_out, bar_dqkv)."""
    o64, g64 = forward_f64(qkv, scale)[0], backward_f64(qkv, dout, scale)
    o32, g32 = reference_form(qkv, dout, scale)
    return (o64, g64) + bars(dist(o32, o64), dist(g32, g64), tol)
