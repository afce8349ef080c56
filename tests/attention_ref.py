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


# ---- structured cases: the structure is a property of the inputs (make_structured); test_attention_ref.py asserts it on fp64 scores -----
# name -> (sequence lengths, tail rows, heads, max_seqlen, softmax_scale).  Every case starts from make_inputs(lengths, tail, H, 1.0,
# STRUCT_SEED) and applies the transformation in make_structured.  U16 is the fixed direction (+-1/4 per component, |U16| = 1).
STRUCT_SEED = 2
NEG_LENS = (1, 15, 17, 47, 49, 65, 130, 1009)
PEAK_LENS = (17, 48, 64, 65, 129, 1009, 1024)
HOT_LENS = (32, 16, 5, 9, 31, 1, 12, 17, 0, 2)
STRUCTURED = {
    "all_negative": (NEG_LENS, 3, 3, 1009, SCALE),
    "all_positive": (NEG_LENS, 3, 3, 1009, SCALE),
    "peak_last_key": (PEAK_LENS, 0, 2, 1024, SCALE),
    "rising_max": ((300, 1024), 2, 2, 1024, SCALE),
    "uniform_q0": ((48, 17, 1, 64, 65, 300), 1, 5, 300, SCALE),
    "uniform_k_equal": ((48, 17, 1, 64, 65, 300), 1, 5, 300, SCALE),
    "one_hot": (HOT_LENS, 0, 5, 32, SCALE),
    "one_hot_p200": (HOT_LENS, 0, 5, 200, SCALE),          # the same rows through the workgroup-per-head path
    "scale_neg": (MIXED, 7, 2, 1024, -0.25),
    "scale_zero": (MIXED, 7, 2, 1024, 0.0),
    "scale_2": (MIXED, 7, 2, 1024, 2.0),
    "v_large": ((48, 17, 1, 64, 130, 513), 2, 3, 513, SCALE),
    "subnormal": ((48, 17, 1, 64, 130), 2, 2, 130, SCALE),
    "dout_zero": (MIXED, 7, 2, 1024, SCALE),
}
# Magnitudes (the largest power of two, found on the CPU, at which attention_rounded against attention_fp64 keeps the forward inside
# ONE of the three forward units and the backward yardstick finite and not above the largest one of CASES, 51.76 ulp; a case that
# needs more says why).  The reached property values are those printed by test_attention_ref.py::test_structured_case.
NEG_A = 16.0        # all_negative / all_positive: q = eps/2 + A u, k = eps/2 -+ A u: every real q.k <= -NEG, reached NEG = 205.1 (>= 32 =
                    # 8 / |scale|; all_positive: every q.k >= 206.6).  A = 32 and 64 also keep the forward inside one unit (0.60, 0.56)
                    # but need 108.7 and 236.4 ulp: sum_j dS_ij = 0 cancels the common component A u of the keys in dq (and of the
                    # queries in dk), so every dq / dk block has a true gradient far below |dS| |k|.  A = 16 is the largest that
                    # stays under the largest yardstick of CASES.
PEAK_C = 8.0        # peak_last_key: q += C u, then the last key = B * mean of the sequence's q: reached margin over the second key 23.68
PEAK_B = 4.0        # (scaled score units).  From B = 4 on every row is one-hot to fp16 precision (the restatement's forward error is 0),
                    # so a larger B changes nothing; B = 2 (margin 9.69) needs 57.0 ulp, above the largest yardstick of CASES.
RISE_C = 8.0        # rising_max: q += C u, keys sorted by k.u ascending, key j += R * (j // 64) * u: the 64-key step maximum of every row
RISE_R = 12.0       # rises by at least 15.26 log2 units per step (required: 4).  R = 24 (rise 30.1) needs 63.5 ulp: not taken.
HOT_C = 8.0         # one_hot: k_j = eps/4 +- B e_(j mod 16) (sign - from key 16 on), q_i += +-C e at its hot key (L - 1 - i): reached margin
HOT_B = 64.0        # 44.97 (scaled score units): softmax rows are one-hot, the true dq / dk vanish and block_den's floor carries the bar
V_LARGE_MUL = 2.0 ** 13     # v_large: v *= 2^13: reached max|v| = 32864, inside [3e4, 6e4] (2^14 would overflow fp16)
V_LARGE_DOUT = 2.0 ** -1    # dO *= 2^-1: reached max|dS| = 12266, a factor 5 below the fp16 maximum (24531 with dO as given, which leaves a
                            # kernel that places its roundings differently less than a factor 3)
SUBNORMAL_MUL = 2.0 ** -15  # subnormal: qkv *= 2^-15: 95.6 % of the values are fp16 subnormals.  2^-16 (and so 2^-20) cannot keep an fp16 output
SUBNORMAL_DOUT = 2.0 ** 13  # inside one forward unit: out is subnormal, its rounding alone is 2^-25 against a unit of 2^-11 max|v| = 2^-25.
                            # dO *= 2^13 (the largest power of two that keeps dO finite) so that dq, dk ~ |dS| |k| are not flushed.
# attention_rounded's normalised backward error on make_structured(case), in units of 2^-11, measured on the CPU and recorded 10 % up like
# BWD_YARDSTICK_ULPS (re-derived by test_attention_ref.py).  uniform_k_equal: sum_j dS_ij k = 0, the true dq is exactly 0 and its
# blocks stand on block_den's floor.  dout_zero: every gradient is exactly 0.
STRUCTURED_YARDSTICK_ULPS = {"all_negative": 6.64, "all_positive": 6.67, "peak_last_key": 0.97, "rising_max": 27.56,
                             "uniform_q0": 1.24, "uniform_k_equal": 33.59, "one_hot": 0.12, "one_hot_p200": 0.12, "scale_neg": 1.83,
                             "scale_zero": 1.16, "scale_2": 4.5, "v_large": 1.42, "subnormal": 26.1, "dout_zero": 0.0}


def _u16():
    return torch.tensor([1, -1, 1, 1, -1, 1, -1, -1, 1, 1, -1, 1, -1, -1, 1, -1], dtype=torch.float32) / 4.0


def _hot_index(i, L):
    """the key that query i of a length-L sequence points at"""
    return (L - 1 - i) % L


def make_structured(name, seed=STRUCT_SEED):
    """(qkv, dout, cu_seqlens, max_seqlen, softmax_scale) of a STRUCTURED case: fp16 CPU tensors, reproducible.  Rows beyond
    cu_seqlens[-1] (the tail) keep their Gaussian values."""
    lens, tail, H, max_seqlen, scale = STRUCTURED[name]
    qkv, dout, cu = make_inputs(lens, tail, H, 1.0, seed)
    x, g, u = qkv.float(), dout.float(), _u16()
    for a, b in zip(cu[:-1].tolist(), cu[1:].tolist()):
        L = b - a
        if L == 0:
            continue
        q, k, v = x[a:b, 0], x[a:b, 1], x[a:b, 2]                     # views (L, H, 16)
        if name in ("all_negative", "all_positive"):
            q.mul_(0.5).add_(NEG_A * u)
            k.mul_(0.5).add_((-NEG_A if name == "all_negative" else NEG_A) * u)
        elif name == "peak_last_key":
            q.add_(PEAK_C * u)
            k[L - 1] = PEAK_B * q.half().float().mean(0)
        elif name == "rising_max":
            q.add_(RISE_C * u)
            order = torch.argsort(k @ u, dim=0)                         # (L, H): ascending score with the probe u
            k.copy_(torch.gather(k, 0, order[..., None].expand(-1, -1, 16)))
            k.add_((RISE_R * (torch.arange(L) // 64).float())[:, None, None] * u)
        elif name == "uniform_q0":
            q.zero_()
        elif name == "uniform_k_equal":
            k.copy_(k[:1].expand(L, -1, -1).clone())
        elif name in ("one_hot", "one_hot_p200"):
            j = torch.arange(L)
            sign = torch.where(j < 16, 1.0, -1.0)
            k.mul_(0.25)
            k[j, :, j % 16] += (HOT_B * sign)[:, None]
            hot = torch.tensor([_hot_index(i, L) for i in range(L)])
            q[j, :, hot % 16] += (HOT_C * sign[hot])[:, None]
    if name == "v_large":
        x[:, 2] *= V_LARGE_MUL
        g *= V_LARGE_DOUT
    elif name == "subnormal":
        x *= SUBNORMAL_MUL
        g *= SUBNORMAL_DOUT
    elif name == "dout_zero":
        g.zero_()
    return x.half(), g.half(), cu, max_seqlen, scale


def structured_property(name, qkv, cu, scale):
    """the value that states the case's structure, from the fp64 scores q.k of the fp16-valued inputs (None: the case has none);
    the requirement on it is asserted by test_attention_ref.py"""
    x = qkv.double()
    worst = None
    for a, b in zip(cu[:-1].tolist(), cu[1:].tolist()):
        L = b - a
        if L == 0:
            continue
        s = torch.einsum("qhd,khd->hqk", x[a:b, 0], x[a:b, 1])        # raw scores (H, L, L)
        if name == "all_negative":                                      # NEG: minus the largest real score
            val = float(-s.max())
        elif name == "all_positive":
            val = float(s.min())
        elif name == "peak_last_key":                                   # margin of the last key over the best other key, scaled units
            if L == 1:
                continue
            val = float((s[..., -1] - s[..., :-1].amax(-1)).min() * scale)
        elif name == "rising_max":                                      # smallest rise of the 64-key step maximum, log2 units
            steps = torch.stack([s[..., c:c + 64].amax(-1) for c in range(0, L, 64)], -1) * (scale * 1.4426950408889634)
            val = float((steps[..., 1:] - steps[..., :-1]).min())
        elif name in ("one_hot", "one_hot_p200"):                       # margin of the hot key over the best other key, scaled units
            if L == 1:
                continue
            hot = torch.tensor([_hot_index(i, L) for i in range(L)])
            top = torch.gather(s, 2, hot[None, :, None].expand(s.shape[0], -1, 1))[..., 0]
            rest = s.scatter(2, hot[None, :, None].expand(s.shape[0], -1, 1), float("-inf")).amax(-1)
            val = float((top - rest).min() * scale)
        elif name in ("uniform_q0", "uniform_k_equal"):                 # spread of a row's scores: exactly 0
            val = float((s.amax(-1) - s.amin(-1)).max())
            val = -val
        else:
            break
        worst = val if worst is None else min(worst, val)
    if name == "v_large":
        return float(qkv[:int(cu[-1]), 2].double().abs().max())
    if name == "subnormal":                                             # fraction of fp16 subnormals among the nonzero values
        r = qkv[:int(cu[-1])].double().abs()
        return float(((r < 2.0 ** -14) & (r > 0)).double().mean())
    return worst


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
