"""CPU restatements of the local norm pooling of unipre3d_amd/lnp.py (numpy; x (B, G, C), idx (B, G, K), alpha and beta (2C,),
out and dout (B, G, 2C)):

  forward_f64 / backward_f64                 fp64, the formulas of include/unipre3d_lnp.h (the backward in closed form)
  forward_kernel_f32 / backward_kernel_f32   fp32 in the kernels' order: d in fp32, its two sums in f64, v as one fma of d r, the row maximum
                                             subtracted, sums over k in ascending order, p recomputed as exp(v - lse), t in f64, the parameter
                                             sums per wave, then per workgroup of eight rows in fp32, then in f64, dx over the inverse lists
  inverse_lists                              ptr (B, G+1), ent (B, G K)
  reference_form                             the reference's lines (GroupFeature's gather, K_Norm, K_Pool) in torch with autograd

and the tolerance rule of profiles/lnp/tolerance.json: bar = 2 x yardstick + floor, in max|x - fp64| / max|fp64|."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g20_lnp.npz")
TOLERANCE = os.path.join(ROOT, "profiles", "lnp", "tolerance.json")
CASES = ("object", "kg", "tiny", "k8", "sharp", "huge")
QUANTITIES = ("out", "dx", "dalpha", "dbeta")
EPS = 1e-5
BWD_WAVES, BWD_MAX_WG = 8, 512          # csrc/u3d_lnp.hip
f32, f64 = np.float32, np.float64


def dist(x, ref64):
    """max|x - fp64| / max|fp64| (the unit of every figure of the tolerance file)."""
    ref64 = np.asarray(ref64, f64)
    return float(np.abs(np.asarray(x, f64) - ref64).max() / max(np.abs(ref64).max(), 1e-300))


def sanitize(idx):
    """An index outside [0, G) counts as the row itself."""
    idx = np.asarray(idx).astype(np.int64)
    G = idx.shape[1]
    own = np.broadcast_to(np.arange(G)[None, :, None], idx.shape)
    return np.where((idx >= 0) & (idx < G), idx, own)


def _gather(x, idx):
    return x[np.arange(x.shape[0])[:, None, None], idx]          # (B, G, K, C)


# ---- (a) fp64 ----------------------------------------------------------------------------------------------------------------
def _parts_f64(x, idx, alpha, beta, eps):
    x, alpha, beta = np.asarray(x, f64), np.asarray(alpha, f64).reshape(-1), np.asarray(beta, f64).reshape(-1)
    C = x.shape[2]
    d = _gather(x, sanitize(idx)) - x[:, :, None, :]
    n = d.size
    mu = d.mean()
    s = np.sqrt(((d - mu) ** 2).sum() / (n - 1))
    r = 1.0 / (s + eps)
    v = alpha[:C] * d * r + beta[:C]
    m = v.max(2, keepdims=True)
    e = np.exp(v - m)
    l = e.sum(2, keepdims=True)
    return x, alpha, beta, d, n, mu, s, r, v, e / l, (m + np.log(l))[:, :, 0]


def forward_f64(x, idx, alpha, beta, eps=EPS):
    """-> out (B, G, 2C), lse (B, G, C), mu, s."""
    x, alpha, beta, d, n, mu, s, r, v, p, lse = _parts_f64(x, idx, alpha, beta, eps)
    C = x.shape[2]
    return np.concatenate([(p * v).sum(2), alpha[C:] * x + beta[C:]], axis=2), lse, mu, s


def backward_f64(x, idx, alpha, beta, dout, eps=EPS):
    """-> dx (B, G, C), dalpha (2C,), dbeta (2C,), in closed form."""
    x, alpha, beta, d, n, mu, s, r, v, p, lse = _parts_f64(x, idx, alpha, beta, eps)
    B, G, C = x.shape
    dout = np.asarray(dout, f64)
    g1, g2 = dout[:, :, :C], dout[:, :, C:]
    o = (p * v).sum(2)
    gv = g1[:, :, None] * p * (1.0 + v - o[:, :, None])
    gu = gv * alpha[:C]
    t = (gu * d).sum()
    gd = gu * r - (t * r * r * (d - mu) / ((n - 1) * s) if s > 0 else 0.0)
    dx = alpha[C:] * g2 - gd.sum(2)
    np.add.at(dx, (np.arange(B)[:, None, None], sanitize(idx)), gd)
    dalpha = np.concatenate([(gv * d * r).sum((0, 1, 2)), (g2 * x).sum((0, 1))])
    dbeta = np.concatenate([gv.sum((0, 1, 2)), g2.sum((0, 1))])
    return dx, dalpha, dbeta


# ---- (b) fp32 in the kernels' order ------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma: the product is exact in fp64; the sum is rounded to fp64 and then to fp32."""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _stats_f32(d, eps):
    n = float(d.size)
    d64 = d.astype(f64)
    S1, S2 = d64.sum(), (d64 * d64).sum()
    var = max((S2 - S1 * S1 / n) / (n - 1.0), 0.0) if n > 1 else 0.0
    mu, sd = f32(S1 / n), f32(np.sqrt(var))
    r = f32(1) / f32(sd + f32(eps))
    c0 = f32(f64(r) * f64(r) / ((n - 1.0) * f64(sd))) if sd > 0 else f32(0)
    return mu, sd, r, c0


def forward_kernel_f32(x, idx, alpha, beta, eps=EPS):
    """-> out, lse, stats = (mu, s, r, r^2 / ((n - 1) s)), all fp32."""
    x, alpha, beta = np.asarray(x, f32), np.asarray(alpha, f32).reshape(-1), np.asarray(beta, f32).reshape(-1)
    C, K = x.shape[2], np.asarray(idx).shape[2]
    d = _gather(x, sanitize(idx)) - x[:, :, None, :]
    stats = _stats_f32(d, eps)
    v = _fma(alpha[:C], d * stats[2], beta[:C])
    m = v.max(2)
    l, acc = np.zeros_like(m), np.zeros_like(m)
    for k in range(K):
        e = np.exp(v[:, :, k] - m)
        l = l + e
        acc = _fma(e, v[:, :, k], acc)
    out = np.concatenate([acc / l, _fma(alpha[C:], x, beta[C:])], axis=2)
    return out, m + np.log(l), stats


def backward_kernel_f32(x, idx, alpha, beta, dout, eps=EPS, saved=None):
    """-> dx, dalpha, dbeta (fp32), from the forward's saved out, lse and stats."""
    x, alpha, beta = np.asarray(x, f32), np.asarray(alpha, f32).reshape(-1), np.asarray(beta, f32).reshape(-1)
    dout = np.asarray(dout, f32)
    B, G, C = x.shape
    K = np.asarray(idx).shape[2]
    out, lse, (mu, sd, r, c0) = forward_kernel_f32(x, idx, alpha, beta, eps) if saved is None else saved
    sidx = sanitize(idx)
    d = _gather(x, sidx) - x[:, :, None, :]
    u = d * r
    v = _fma(alpha[:C], u, beta[:C])
    g1, g2 = dout[:, :, None, :C], dout[:, :, C:]
    gv = (g1 * np.exp(v - lse[:, :, None, :])) * ((v - out[:, :, None, :C]) + f32(1))
    gu = gv * alpha[:C]
    t = (gu * d).astype(f64).sum()
    coef = f32(t * f64(c0))
    gd = _fma(gu, r, -(coef * (d - mu)))
    # parameter sums: row = slot + i * slots with slot = 8 workgroup + wave; a wave's rows and their k in one fp32 chain, the eight waves
    # of a workgroup in order in fp32, the workgroups in f64
    rows = B * G
    nwg = min(-(-rows // BWD_WAVES), BWD_MAX_WG)
    slots = nwg * BWD_WAVES
    acc = np.zeros((4, slots, C), f32)
    gvr, ur, xr, g2r = gv.reshape(rows, K, C), u.reshape(rows, K, C), x.reshape(rows, C), g2.reshape(rows, C)
    for i in range(-(-rows // slots)):
        sel = np.arange(i * slots, min((i + 1) * slots, rows))
        a = acc[:, :len(sel)].copy()
        a[2] = _fma(g2r[sel], xr[sel], a[2])
        a[3] = a[3] + g2r[sel]
        for k in range(K):
            a[0] = _fma(gvr[sel, k], ur[sel, k], a[0])
            a[1] = a[1] + gvr[sel, k]
        acc[:, :len(sel)] = a
    acc = acc.reshape(4, nwg, BWD_WAVES, C)
    wg = acc[:, :, 0]
    for w in range(1, BWD_WAVES):
        wg = wg + acc[:, :, w]
    par = wg.astype(f64).sum(1).astype(f32)          # (4, C): dalpha lower, dbeta lower, dalpha upper, dbeta upper
    dalpha, dbeta = np.concatenate([par[0], par[2]]), np.concatenate([par[1], par[3]])
    # dx: the inverse list in ascending (g, k), then the row's own K terms, then the upper half's fma
    ptr, ent = inverse_lists(idx)
    dx = np.zeros((B, G, C), f32)
    for b in range(B):
        for j in range(G):
            a = np.zeros(C, f32)
            for e in ent[b, ptr[b, j]:ptr[b, j + 1]]:
                a = a + gd[b, e // K, e % K]
            for k in range(K):
                a = a - gd[b, j, k]
            dx[b, j] = _fma(alpha[C:], g2[b, j], a)
    return dx, dalpha, dbeta


# ---- (c) the inverse lists ---------------------------------------------------------------------------------------------------
def inverse_lists(idx):
    """ptr (B, G+1) int32, ent (B, G K) int32: row j's entries e = g K + k with idx[b, g, k] == j, ascending."""
    sidx = sanitize(idx)
    B, G, K = sidx.shape
    ptr, ent = np.zeros((B, G + 1), np.int32), np.zeros((B, G * K), np.int32)
    for b in range(B):
        flat = sidx[b].reshape(-1)
        order = np.argsort(flat, kind="stable")
        ent[b] = order
        ptr[b, 1:] = np.cumsum(np.bincount(flat, minlength=G))
    return ptr, ent


# ---- (d) the reference's form ------------------------------------------------------------------------------------------------
def reference_form(x, idx, alpha, beta, dout=None, dtype="float32", stable=False, eps=EPS):
    """GroupFeature's gather, K_Norm and K_Pool, line by line, in torch on the CPU.  stable=True subtracts the row maximum before exp
    (the same function wherever the plain form is finite).  Returns out (B, G, 2C), and (dx, dalpha, dbeta) through autograd with dout."""
    import torch
    dt = getattr(torch, dtype)
    grad = dout is not None
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dt).requires_grad_(grad)
    a = torch.from_numpy(np.asarray(alpha).reshape(1, 1, 1, -1).copy()).to(dt).requires_grad_(grad)
    bt = torch.from_numpy(np.asarray(beta).reshape(1, 1, 1, -1).copy()).to(dt).requires_grad_(grad)
    B, G, C = t.shape
    K = np.asarray(idx).shape[2]
    flat = (torch.from_numpy(sanitize(idx)) + torch.arange(B).view(-1, 1, 1) * G).view(-1)
    knn_x = t.contiguous().view(-1, C)[flat, :].view(B, G, K, C)
    mean_x = t.unsqueeze(dim=-2)
    std_x = torch.std(knn_x - mean_x)
    knn_x = (knn_x - mean_x) / (std_x + eps)
    knn_x = torch.cat([knn_x, t.reshape(B, G, 1, -1).repeat(1, 1, K, 1)], dim=-1)
    w = (a * knn_x + bt).permute(0, 3, 1, 2)
    e_x = torch.exp(w - w.max(-1, keepdim=True)[0].detach()) if stable else torch.exp(w)
    out = torch.div((w * e_x).mean(-1), e_x.mean(-1)).permute(0, 2, 1)
    if not grad:
        return out.detach().numpy()
    out.backward(torch.from_numpy(np.ascontiguousarray(dout)).to(dt))
    return out.detach().numpy(), (t.grad.numpy(), a.grad.numpy().reshape(-1), bt.grad.numpy().reshape(-1))


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def tolerance():
    with open(TOLERANCE) as f:
        return json.load(f)


def bars(yards, tol=None):
    """{quantity: 2 x yardstick + floor}."""
    fl = (tolerance() if tol is None else tol)["floors"]
    return {q: 2.0 * float(yards[q]) + fl[q] for q in QUANTITIES}


def case_bars(name, tol=None):
    tol = tolerance() if tol is None else tol
    row = {r["case"]: r for r in tol["cases"]}[name]
    return bars({q: row[f"{q}_yardstick"] for q in QUANTITIES}, tol)


def spot_bars(x, idx, alpha, beta, dout, tol=None):
    """For a shape without a record: the yardsticks on the spot (reference_form in fp32 against the fp64 restatement).
    Returns ({quantity: fp64 value}, {quantity: bar})."""
    o64 = forward_f64(x, idx, alpha, beta)[0]
    ref = dict(zip(QUANTITIES, (o64,) + backward_f64(x, idx, alpha, beta, dout)))
    o32, g32 = reference_form(x, idx, alpha, beta, dout)
    got = dict(zip(QUANTITIES, (o32,) + g32))
    return ref, bars({q: dist(got[q], ref[q]) for q in QUANTITIES}, tol)


def golden_case(z, name):
    """(x, idx, alpha, beta, dout, cols) of a golden case; cols: the recorded channels of out and dx (None: all).  The record of `object`
    keeps every 8th channel, so that the file stays small: out at cols and C + cols, dx at cols."""
    cols = z[f"{name}_cols"] if f"{name}_cols" in z.files else None
    return z[f"{name}_x"], z[f"{name}_idx"], z[f"{name}_alpha"], z[f"{name}_beta"], z[f"{name}_dout"], cols


def recorded(values, cols):
    """{quantity: array} cut to the recorded channels."""
    if cols is None:
        return dict(values)
    C = values["dx"].shape[2]
    both = np.concatenate([cols, C + cols])
    return {"out": values["out"][:, :, both], "dx": values["dx"][:, :, cols], "dalpha": values["dalpha"], "dbeta": values["dbeta"]}
