"""Plain-torch restatements for tests of unipre3d_amd.attention / unipre3d_amd.scatter (any device; the CPU tests run them on the CPU).

attention_fp64     per-sequence softmax attention and its gradient (autograd) in fp64 on the fp16-valued inputs: the yardstick.
attention_rounded  the same in fp32 with fp16 roundings where a flash kernel has them (unnormalised P before P.V; P and dS before the
                   backward products, dO as given; outputs once).  Used only to size the backward tolerance.
segment_csr_ref    torch_scatter.segment_csr by explicit loops (numpy, fp32 sequential sums), with the argument rows of max / min.

Backward tolerance.  |dqkv - dqkv_fp64| is normalised per (sequence, head, one of q / k / v) by `block_den`: the largest |dqkv_fp64| of
that block, and for q and k not less than 2^-8 * |scale| * max|dO| * max|v| * max(|q|, |k|) over the block's rows.  (dS = P * (dP - delta)
subtracts two fp32 sums of 16 products of size up to max|dO| max|v|; evaluated in fp32 in any order that difference carries an absolute
error of up to 16 * 2^-23 of that size whatever its true value -- exactly 0 for a one-row sequence -- and reaches dq / dk multiplied by
|scale| max|k| / max|q|.  Below 2^12 times that, a bar of one fp16 ulp relative to the block's maximum cannot be met by fp32 arithmetic.)
The bar for a kernel is bwd_bar(attention_rounded's normalised error on the same inputs); BWD_YARDSTICK_ULPS records that error for
every case of CASES (re-derived and asserted on the CPU by test_attention_ref.py).
"""
import numpy as np
import torch

FWD_UNITS = 3.0                      # |out - out_fp64| <= FWD_UNITS * 2^-11 * max|v| over the keys of the (sequence, head)
ULP16 = 2.0 ** -11
SCALE = 0.25                         # softmax_scale of the cases (16 ** -0.5)
SEED = 1
# attention_rounded's normalised backward error against attention_fp64 on make_inputs(case, SEED), in units of 2^-11, computed on the
# CPU and recorded 10 % up (test_attention_ref.py re-derives every figure and asserts measured <= recorded <= 1.3 * measured).  The
# x8 cases have near one-hot softmax rows, so some blocks have tiny true gradients and every fp16 rounding weighs more there.
BWD_YARDSTICK_ULPS = {"short_h1": 1.52, "short_h2_p48": 1.77, "short_h32": 1.88, "short_h5_x8": 51.76, "mixed_h1": 1.58, "mixed_h2": 1.28,
                      "mixed_h32": 2.09, "mid_h3_p200": 1.54, "mid_h2_p500_x8": 2.23, "long_h2_x8": 3.48}


def bwd_bar(yardstick):
    """twice the restatement's own normalised error (a kernel may place its fp16 roundings one product earlier or later) plus one fp16 ulp"""
    return 2.0 * yardstick + ULP16

# name -> (sequence lengths, tail rows beyond cu_seqlens[-1], heads, max_seqlen, input scale)
MIXED = (0, 1, 15, 16, 17, 47, 48, 49, 300, 1024, 0, 33)
CASES = {
    "short_h1": ((48, 17, 0, 48, 1, 47, 49, 15, 16, 64, 33), 0, 1, 64, 1.0),
    "short_h2_p48": ((17, 48, 48, 48, 48, 34, 48, 48, 1, 0, 48), 5, 2, 48, 1.0),
    "short_h32": ((48, 47, 16, 1, 0, 15, 17, 48), 3, 32, 48, 1.0),
    "short_h5_x8": ((48, 17, 31, 48, 2), 0, 5, 48, 8.0),
    "mixed_h1": (MIXED, 0, 1, 1024, 1.0),
    "mixed_h2": (MIXED, 7, 2, 1024, 1.0),
    "mixed_h32": ((0, 1, 15, 16, 17, 47, 48, 49, 300, 0), 2, 32, 300, 1.0),
    "mid_h3_p200": ((200, 130, 65, 199, 0, 64), 1, 3, 200, 1.0),
    "mid_h2_p500_x8": ((500, 257, 1, 480), 0, 2, 500, 8.0),
    "long_h2_x8": ((1024, 700, 17), 4, 2, 1024, 8.0),
}


def cu_from_lengths(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int32)


def make_inputs(lengths, tail, H, scale_in, seed, D=16):
    """qkv (T,3,H,D) and dout (T,H,D), fp16 on the CPU, reproducible."""
    g = torch.Generator().manual_seed(seed)
    T = int(sum(lengths)) + tail
    qkv = (torch.randn(T, 3, H, D, generator=g) * scale_in).half()
    dout = torch.randn(T, H, D, generator=g).half()
    return qkv, dout, cu_from_lengths(lengths)


def _groups(cu):
    """rows of all sequences of one length as an (n, L) index array, per distinct length L > 0"""
    cu = np.asarray(cu, dtype=np.int64)
    lens = np.diff(cu)
    for L in np.unique(lens):
        if L > 0:
            starts = cu[:-1][lens == L]
            yield int(L), starts[:, None] + np.arange(L)[None, :]


def attention_fp64(qkv, cu, scale, dout=None, chunk=1 << 22):
    """out (T,H,D) fp64 (rows outside the sequences 0) and, with dout, d(sum(out * dout)) / d qkv (T,3,H,D) fp64 by autograd."""
    x = qkv.detach().double()
    out = torch.zeros(x.shape[0], x.shape[2], x.shape[3], dtype=torch.float64, device=x.device)
    dx = torch.zeros_like(x) if dout is not None else None
    for L, rows in _groups(cu):
        step = max(1, chunk // (L * L * x.shape[2]))
        for a in range(0, len(rows), step):
            idx = torch.as_tensor(rows[a:a + step], device=x.device)
            blk = x[idx].clone().requires_grad_(dout is not None)        # (n, L, 3, H, D)
            q, k, v = blk[:, :, 0], blk[:, :, 1], blk[:, :, 2]
            p = torch.softmax(torch.einsum("nqhd,nkhd->nhqk", q, k) * scale, dim=-1)
            o = torch.einsum("nhqk,nkhd->nqhd", p, v)
            out[idx] = o.detach()
            if dout is not None:
                (g,) = torch.autograd.grad(o, blk, dout.double()[idx])
                dx[idx] = g
    return out if dout is None else (out, dx)


def attention_rounded(qkv, cu, scale, dout=None, chunk=1 << 22):
    """fp32 with a flash kernel's fp16 roundings; returns fp16 out and, with dout (fp16), fp16 dqkv (explicit backward)."""
    x = qkv.detach().float()
    out = torch.zeros(x.shape[0], x.shape[2], x.shape[3], dtype=torch.float16, device=x.device)
    dx = torch.zeros(x.shape, dtype=torch.float16, device=x.device) if dout is not None else None
    r16 = lambda t: t.half().float()
    for L, rows in _groups(cu):
        step = max(1, chunk // (L * L * x.shape[2]))
        for a in range(0, len(rows), step):
            idx = torch.as_tensor(rows[a:a + step], device=x.device)
            blk = x[idx]
            q, k, v = blk[:, :, 0], blk[:, :, 1], blk[:, :, 2]
            s = torch.einsum("nqhd,nkhd->nhqk", q, k) * scale
            m = s.amax(-1, keepdim=True)
            e = torch.exp(s - m)
            l = e.sum(-1, keepdim=True)
            o = r16(torch.einsum("nhqk,nkhd->nqhd", r16(e), v) / l.permute(0, 2, 1, 3))
            out[idx] = o.half()
            if dout is not None:
                do = dout.float()[idx]
                p = torch.exp(s - (m + torch.log(l)))
                dv = torch.einsum("nhqk,nqhd->nkhd", r16(p), do)
                dp = torch.einsum("nqhd,nkhd->nhqk", do, v)
                delta = (do * o).sum(-1).permute(0, 2, 1)[..., None]
                ds = r16(p * (dp - delta))
                dq = torch.einsum("nhqk,nkhd->nqhd", ds, k) * scale
                dk = torch.einsum("nhqk,nqhd->nkhd", ds, q) * scale
                dx[idx] = torch.stack([dq, dk, dv], dim=2).half()
    return out if dout is None else (out, dx)


def fwd_bound(qkv, cu):
    """(T,H,1) fp64: FWD_UNITS * 2^-11 * max|v| over the keys of the row's (sequence, head); 0 outside the sequences"""
    v = qkv[:, 2].detach().double().abs().amax(-1)                      # (T,H)
    b = torch.zeros_like(v)
    for L, rows in _groups(cu):
        idx = torch.as_tensor(rows, device=v.device)
        b[idx] = v[idx].amax(1, keepdim=True).expand(-1, L, -1)
    return (FWD_UNITS * ULP16 * b)[..., None]


def block_den(qkv, dout, dref, cu, scale):
    """(T,3,H,1) fp64 denominators of the normalised backward error (module docstring); 1 outside the sequences (the error there must be 0)"""
    a = qkv.detach().double().abs().amax(-1)                            # (T,3,H)
    g = dout.detach().double().abs().amax(-1)                           # (T,H)
    d = dref.abs().amax(-1)                                             # (T,3,H)
    den = torch.ones_like(d)
    for L, rows in _groups(cu):
        idx = torch.as_tensor(rows, device=d.device)
        top = d[idx].amax(1, keepdim=True)                              # (n,1,3,H)
        am = a[idx].amax(1, keepdim=True)
        floor = 2.0 ** -8 * abs(scale) * g[idx].amax(1, keepdim=True) * am[:, :, 2] * torch.maximum(am[:, :, 0], am[:, :, 1])   # (n,1,H)
        top = torch.stack([torch.maximum(top[:, :, 0], floor), torch.maximum(top[:, :, 1], floor), top[:, :, 2]], dim=2)
        den[idx] = top.clamp_min(1e-300).expand(-1, L, -1, -1)
    return den[..., None]


def bwd_norm_err(d, dref, den):
    """worst normalised error over every element"""
    return float(((d.double() - dref).abs() / den).max()) if d.numel() else 0.0


def segment_csr_ref(src, indptr, reduce):
    """(out (M,C) fp32, arg (M,C) int64 or None): loops in ascending row order, fp32 sequential sums; empty segment 0 (arg -1);
    max / min: lowest row attaining the extremum, a NaN wins and the lowest NaN row is the argument."""
    src = np.asarray(src, dtype=np.float32)
    indptr = np.asarray(indptr, dtype=np.int64)
    M, C = len(indptr) - 1, src.shape[1]
    out = np.zeros((M, C), np.float32)
    arg = np.full((M, C), -1, np.int64) if reduce in ("max", "min") else None
    for m in range(M):
        a, b = int(indptr[m]), int(indptr[m + 1])
        if b <= a:
            continue
        if reduce in ("sum", "mean"):
            acc = np.zeros(C, np.float32)
            for n in range(a, b):
                acc = (acc + src[n]).astype(np.float32)
            out[m] = acc / np.float32(b - a) if reduce == "mean" else acc
        else:
            best, at = src[a].copy(), np.full(C, a, np.int64)
            for n in range(a + 1, b):
                v = src[n]
                with np.errstate(invalid="ignore"):
                    take = ~np.isnan(best) & (np.isnan(v) | ((v > best) if reduce == "max" else (v < best)))
                best = np.where(take, v, best)
                at = np.where(take, n, at)
            out[m], arg[m] = best, at
    return out, arg


def segment_csr_grad_ref(dout, indptr, arg, N, reduce):
    dout = np.asarray(dout, dtype=np.float32)
    indptr = np.asarray(indptr, dtype=np.int64)
    d = np.zeros((N, dout.shape[1]), np.float32)
    for m in range(len(indptr) - 1):
        a, b = int(indptr[m]), int(indptr[m + 1])
        for n in range(a, b):
            if reduce == "sum":
                d[n] = dout[m]
            elif reduce == "mean":
                d[n] = dout[m] / np.float32(b - a)
            else:
                d[n] = np.where(arg[m] == n, dout[m], np.float32(0))
    return d


def ptv3_padding(sizes, patch_size):
    """cu_seqlens (int32) that PTv3's serialized attention hands to flash-attn for a batch with these item sizes, restated: an item of
    at most patch_size points is ONE sequence of its own length; a larger item is padded (by repeating points) up to the next multiple
    of patch_size and cut into whole patches.  Returns (cu_seqlens, padded item sizes)."""
    starts, base, padded = [], 0, []
    for n in (int(v) for v in sizes):
        m = n if n <= patch_size else -(-n // patch_size) * patch_size
        starts.extend(range(base, base + m, patch_size))
        base += m
        padded.append(m)
    return np.asarray(starts + [base], dtype=np.int32), np.asarray(padded, dtype=np.int64)
