"""Numpy restatement of offset-batched furthest point sampling (TEST INFRASTRUCTURE ONLY): what
`unipre3d_amd.offset_ops.furthestsampling` / `u3d_offset_furthest_sampling` must return, index for index.

Semantics (include/unipre3d_pointops.h): segment s = rows [offset[s-1], offset[s]) of xyz, clamped to [0, n], writes
idx[new_offset[s-1] .. new_offset[s]) with absolute rows.  The first selection is the segment's first row; running minimum squared
distances start at 1e10; a selection takes the row of largest minimum distance, equal distances resolved the way a block of
bs = opt_n_threads(n_max) threads does it: thread t scans rows start + t, start + t + bs, ... and keeps its FIRST maximum (strict >),
a halving tree over the bs slots then keeps the LOWER slot on equal values (v2 > v1 takes the upper one).  n_max is the LARGEST
segment, so a small segment's ties follow the large one's block size.  A segment asked for more rows than it has goes on by the same
rule (all minima 0).  Departures from the reference: a segment asked for nothing writes nothing, an EMPTY segment asked for rows gets -1.

Two forms that must agree: `furthestsampling_ref` simulates the block (per-thread scan, then the tree), `furthestsampling_lex` takes
the lexicographic maximum of (distance bits, inverted tie key) -- the form the HIP kernel uses.  fp32 arithmetic in the three
contraction orders of oracle/pointops_oracle.c ('fma_llvm', 'fma_chain', 'none')."""
import numpy as np

F32 = np.float32


def floor_log2(n):
    """Integer floor(log2 n) for n >= 1."""
    return int(n).bit_length() - 1


def opt_n_threads(n):
    """2^floor(log2 n) capped at 1024 and at least 1 (n = 0: 1), by integer arithmetic."""
    return 1 if n < 1 else min(1 << floor_log2(n), 1024)


def _fma(a, b, c):
    """fp32 fused multiply-add, exactly rounded: the product of two fp32 values is exact in fp64; the fp64 sum is made
    round-to-odd (TwoSum's error term says whether it was inexact and on which side) so that the final rounding to fp32 is the
    rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def dist2(centre, pts, contraction):
    """(x2-x1)^2 + (y2-y1)^2 + (z2-z1)^2 with (x1,y1,z1) the centre, fp32, in the given contraction order."""
    d = pts.astype(F32) - centre.astype(F32)[None, :]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    if contraction == "fma_llvm":
        return _fma(dz, dz, _fma(dx, dx, dy * dy))
    if contraction == "fma_chain":
        return _fma(dz, dz, _fma(dy, dy, dx * dx))
    if contraction == "none":
        return (dx * dx + dy * dy) + dz * dz
    raise ValueError(contraction)


def segments(n, m, offset, new_offset):
    """[(start, length, out_start, requested)] with the offsets clamped to [0, n] / [0, m]; end < start counts as empty."""
    out, prev, nprev = [], 0, 0
    for e, me in zip(np.asarray(offset).tolist(), np.asarray(new_offset).tolist()):
        e, me = min(max(int(e), 0), n), min(max(int(me), 0), m)
        out.append((prev, max(e - prev, 0), nprev, max(me - nprev, 0)))
        prev, nprev = e, me
    return out


def _block_argmax(t, bs):
    """Row (relative to the segment) a block of bs threads selects from the minimum distances t."""
    ln = len(t)
    rows = -(-ln // bs)
    pad = np.full(rows * bs, -1.0, F32)                  # threads without a row keep best = -1, besti = first row
    pad[:ln] = t
    grid = pad.reshape(rows, bs)
    q = np.argmax(grid, axis=0)                          # first maximum of every thread's strided scan (strict >)
    dists = grid[q, np.arange(bs)].copy()
    dists_i = q * bs + np.arange(bs)
    dists_i[dists < 0] = 0
    s = bs // 2
    while s >= 1:
        v1, v2 = dists[:s], dists[s:2 * s]
        take = v2 > v1
        dists_i[:s] = np.where(take, dists_i[s:2 * s], dists_i[:s])
        dists[:s] = np.maximum(v1, v2)
        s //= 2
    return int(dists_i[0])


def tie_key(k, lg):
    """(bit-reversed (k mod 2^lg), k div 2^lg) packed as r << 22 | q: the smaller key wins among equal distances."""
    k = np.asarray(k, dtype=np.uint64)
    r = np.zeros_like(k)
    low = k & np.uint64((1 << lg) - 1)
    for bit in range(lg):
        r |= ((low >> np.uint64(bit)) & np.uint64(1)) << np.uint64(lg - 1 - bit)
    return (r << np.uint64(22)) | (k >> np.uint64(lg))


def _lex_argmax(t, inv_keys):
    key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | inv_keys
    return int(np.argmax(key))


def _run(xyz, offset, new_offset, contraction, m, lex):
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    n = xyz.shape[0]
    if m is None:
        m = int(np.asarray(new_offset)[-1]) if len(new_offset) else 0
    idx = np.full(m, -1, np.int32)
    segs = segments(n, m, offset, new_offset)
    n_max = max([ln for _, ln, _, _ in segs], default=0)
    bs = opt_n_threads(n_max)
    lg = floor_log2(bs)
    for start, ln, ostart, req in segs:
        if req == 0:
            continue
        if ln == 0:
            idx[ostart:ostart + req] = -1
            continue
        pts = xyz[start:start + ln]
        t = np.full(ln, 1e10, F32)
        inv = (np.uint64(0xFFFFFFFF) - tie_key(np.arange(ln), lg)) if lex else None
        old = 0
        idx[ostart] = start
        for j in range(1, req):
            t = np.minimum(t, dist2(pts[old], pts, contraction))
            old = _lex_argmax(t, inv) if lex else _block_argmax(t, bs)
            idx[ostart + j] = start + old
    return idx


def furthestsampling_ref(xyz, offset, new_offset, contraction="fma_llvm", m=None):
    """The block simulation."""
    return _run(xyz, offset, new_offset, contraction, m, lex=False)


def furthestsampling_lex(xyz, offset, new_offset, contraction="fma_llvm", m=None):
    """The lexicographic-maximum form."""
    return _run(xyz, offset, new_offset, contraction, m, lex=True)


def dense_as_ragged(xyz, m, contraction="fma_llvm", lex=True):
    """(B,N,3), m -> (B,m) cloud-relative indices through the ragged form (every cloud has N rows, so n_max = N)."""
    B, N, _ = xyz.shape
    off = (np.arange(B) + 1) * N
    noff = (np.arange(B) + 1) * m
    flat = _run(xyz.reshape(B * N, 3), off, noff, contraction, B * m, lex)
    return (flat.reshape(B, m) - (np.arange(B) * N)[:, None]).astype(np.int32)
