"""CPU restatement of include/unipre3d_offsetops.h (numpy).

Searches.  `dist2_rows` forms d2 in fp32 exactly as tests/knn_ref.py does: dx = q - s per coordinate, then (dx*dx + dy*dy) + dz*dz,
every operation rounded on its own.  `knn` is the CONTRACT: per query the k smallest (d2, index) pairs of its own segment in
lexicographic order (a stable sort on d2), then the fill -- dist2 1e10 with the segment's first row, or -1 where the segment is
empty.  `ballquery` is the first nsample rows with d2 < fp32(radius * radius) in index order, padded with the first hit, zeros
without one.

`knn_heap` restates the REFERENCE's algorithm (openpoints/cpp/pointops knnquery: a per-thread max-heap of nsample slots that start
as (1e10, segment start), a candidate replacing the root only where strictly closer, a sift-down after each replacement and a final
heap sort) so that the lexicographic contract is tied to it.  Two facts, from a trial of 300 seeded ragged batches (1 to 3 segments
of 1..199 points, k cycling through 1, 3, 16, 64): on uniform random coordinates, which have no equal distances, the heap's rows
equalled `knn`'s in all 300, order and fill slots included; on coordinates drawn from the integer lattice {0..3}^3, full of exact
ties, the distances agreed in all 300 but the indices differed in 222 -- which of several equally distant points survives at the
k-th place, and in which order equal ones come out, is an accident of the heap's layout.  So the contract is lexicographic and the
heap is compared on tie-free inputs only (tests/test_offsetops_ref.py; `min_gap` is the generator's guard).

Float operators.  Every sum has an fp64 form that also returns, per output element, S = sum |term| and D = the number of terms, for
the recursive-summation bound (D + 2) * 2^-23 * S (`bound`), valid for any order of addition.  An index outside its tensor follows
the header: group reads 0, subtract reads the missing row as 0, interpolate and aggregate drop the term and its gradients, the
scatter-adds add nothing."""
import numpy as np

FILL_D2 = np.float32(1e10)


def _np(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def ranges(m, n, offset, new_offset):
    """(m,2) int64 [start, end) of every query row: the header's segment rule, clamped, empty as start == end."""
    offset, new_offset = _np(offset, np.int64), _np(new_offset, np.int64)
    out = np.zeros((m, 2), np.int64)
    for j in range(m):
        s = 0
        while s < len(new_offset) and j >= new_offset[s]:
            s += 1
        if s < len(new_offset):
            a = 0 if s == 0 else offset[s - 1]
            a, e = min(max(a, 0), n), min(max(offset[s], 0), n)
            out[j] = (a, max(a, e))
    return out


def dist2_rows(q, pts, dtype=np.float32):
    """q (3,), pts (r,3) -> (r,) squared distances in `dtype`, each operation rounded in it."""
    q, pts = np.asarray(q, np.float32).astype(dtype), np.asarray(pts, np.float32).astype(dtype)
    dx, dy, dz = q[0] - pts[:, 0], q[1] - pts[:, 1], q[2] - pts[:, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == dtype
    return d


def knn(k, xyz, new_xyz, offset, new_offset):
    """-> (dist2 (m,k) fp32, idx (m,k) int32): what u3d_offset_knn writes, bit for bit."""
    xyz, new_xyz = _np(xyz, np.float32).reshape(-1, 3), _np(new_xyz, np.float32).reshape(-1, 3)
    n, m = len(xyz), len(new_xyz)
    d2, idx = np.full((m, k), FILL_D2, np.float32), np.full((m, k), -1, np.int32)
    for j, (a, e) in enumerate(ranges(m, n, offset, new_offset)):
        if a == e:
            continue
        d = dist2_rows(new_xyz[j], xyz[a:e])
        order = np.argsort(d, kind="stable")[:k]                       # stable: equal distances stay in index order
        d2[j, :len(order)], idx[j, :len(order)] = d[order], a + order
        idx[j, len(order):] = a
    return d2, idx


def knn_heap(k, xyz, new_xyz, offset, new_offset):
    """The reference's per-thread max-heap, step for step, on the same fp32 d2 (rows beyond new_offset[-1], which the reference never
    launches correctly, and empty segments are left as the contract's fill)."""
    xyz, new_xyz = _np(xyz, np.float32).reshape(-1, 3), _np(new_xyz, np.float32).reshape(-1, 3)
    n, m = len(xyz), len(new_xyz)
    d2, idx = np.full((m, k), FILL_D2, np.float32), np.full((m, k), -1, np.int32)

    def sift_down(hd, hi, size):
        root, child = 0, 1
        while child < size:
            if child + 1 < size and hd[child + 1] > hd[child]:
                child += 1
            if hd[root] > hd[child]:
                return
            hd[root], hd[child] = hd[child], hd[root]
            hi[root], hi[child] = hi[child], hi[root]
            root, child = child, 2 * child + 1

    for j, (a, e) in enumerate(ranges(m, n, offset, new_offset)):
        if a == e:
            continue
        hd, hi = [FILL_D2] * k, [int(a)] * k
        for i, d in zip(range(a, e), dist2_rows(new_xyz[j], xyz[a:e])):
            if d < hd[0]:                                              # strictly closer than the farthest kept
                hd[0], hi[0] = d, i
                sift_down(hd, hi, k)
        for last in range(k - 1, 0, -1):                               # heap sort: the largest to the back, one by one
            hd[0], hd[last] = hd[last], hd[0]
            hi[0], hi[last] = hi[last], hi[0]
            sift_down(hd, hi, last)
        d2[j], idx[j] = hd, hi
    return d2, idx


def min_gap(k, xyz, new_xyz, offset, new_offset):
    """Smallest fp64 gap between consecutive distances among any query's first k + 1 of its segment (inf where no query has two)."""
    xyz, new_xyz = _np(xyz, np.float32).reshape(-1, 3), _np(new_xyz, np.float32).reshape(-1, 3)
    gap = np.inf
    for j, (a, e) in enumerate(ranges(len(new_xyz), len(xyz), offset, new_offset)):
        d = np.sort(dist2_rows(new_xyz[j], xyz[a:e], np.float64))[:k + 1]
        if len(d) > 1:
            gap = min(gap, float(np.diff(d).min()))
    return gap


def ballquery(radius, nsample, xyz, new_xyz, offset, new_offset):
    """-> idx (m,nsample) int32: what u3d_offset_ballquery writes."""
    xyz, new_xyz = _np(xyz, np.float32).reshape(-1, 3), _np(new_xyz, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    idx = np.zeros((len(new_xyz), nsample), np.int32)
    for j, (a, e) in enumerate(ranges(len(new_xyz), len(xyz), offset, new_offset)):
        hits = a + np.flatnonzero(dist2_rows(new_xyz[j], xyz[a:e]) < r2)[:nsample]
        if len(hits):
            idx[j, :len(hits)], idx[j, len(hits):] = hits, hits[0]
    return idx


def ball_margin(radius, xyz, new_xyz, offset, new_offset):
    """Smallest |d2 - r^2| / r^2 in fp64 over every (query, point of its segment): above 1e-5 no fp32 rounding flips a decision."""
    xyz, new_xyz = _np(xyz, np.float32).reshape(-1, 3), _np(new_xyz, np.float32).reshape(-1, 3)
    r2, worst = float(radius) ** 2, np.inf
    for j, (a, e) in enumerate(ranges(len(new_xyz), len(xyz), offset, new_offset)):
        if e > a:
            worst = min(worst, float(np.abs(dist2_rows(new_xyz[j], xyz[a:e], np.float64) - r2).min()) / r2)
    return worst


def bound(D, S):
    """(D + 2) * 2^-23 * S: recursive summation of D terms in fp32 in ANY order costs at most (D - 1) u S to first order (u = 2^-24);
    the unit is doubled and 2 added to D for the roundings inside a term (its product, its input + position sum) and second order."""
    return (np.asarray(D, np.float64) + 2) * 2.0 ** -23 * np.asarray(S, np.float64)


def _ok(idx, rows):
    idx = _np(idx, np.int64)
    return idx, (idx >= 0) & (idx < rows)


def _scatter(n, c, rows, terms):
    """Sum `terms` (r,c) into rows `rows` (r,) of an (n,c) array: -> (sum, sum |term|, count), all fp64 / int."""
    out, s, d = np.zeros((n, c)), np.zeros((n, c)), np.zeros((n, 1), np.int64)
    np.add.at(out, rows, terms)
    np.add.at(s, rows, np.abs(terms))
    np.add.at(d, rows, 1)
    return out, s, d


def group_forward(x, idx):
    """fp32, exact: x[idx], 0 where idx is outside."""
    x = _np(x, np.float32)
    idx, ok = _ok(idx, len(x))
    out = np.zeros(idx.shape + (x.shape[1],), np.float32)
    out[ok] = x[idx[ok]]
    return out


def group_backward(g, idx, n):
    g = _np(g, np.float64)
    idx, ok = _ok(idx, n)
    return _scatter(n, g.shape[-1], idx[ok], g[ok])


def interpolate_forward(x, idx, w):
    x, w = _np(x, np.float64), _np(w, np.float64)
    idx, ok = _ok(idx, len(x))
    terms = np.where(ok[..., None], x[np.where(ok, idx, 0)], 0.0) * w[..., None] if len(x) else np.zeros(idx.shape + (x.shape[1],))
    return terms.sum(1), np.abs(terms).sum(1), ok.sum(1, keepdims=True)


def interpolate_backward(g, idx, w, m_in):
    g, w = _np(g, np.float64), _np(w, np.float64)
    idx, ok = _ok(idx, m_in)
    terms = g[:, None, :] * w[..., None]
    return _scatter(m_in, g.shape[1], idx[ok], terms[ok])


def subtract_forward(a, b, idx):
    """fp32, exact: a[i] - b[idx[i,s]], the missing row read as 0."""
    a = _np(a, np.float32)
    return a[:, None, :] - group_forward(b, idx)


def subtract_backward(g, idx):
    """-> (grad_in1, S, D), (grad_in2, S, D)"""
    g = _np(g, np.float64)
    n, ns, c = g.shape
    idx, ok = _ok(idx, n)
    return (g.sum(1), np.abs(g).sum(1), np.full((n, 1), ns)), _scatter(n, c, idx[ok], -g[ok])


def _aggregate_parts(x, p, w, idx):
    x, p, w = _np(x, np.float64), _np(p, np.float64), _np(w, np.float64)
    n, ns, c = p.shape
    idx, ok = _ok(idx, n)
    gathered = x[np.where(ok, idx, 0)] + p                              # (n,ns,c)
    wide = np.tile(w, (1, 1, c // w.shape[2]))                          # weight[..., ch % w_c]
    return gathered, wide, idx, ok


def aggregate_forward(x, p, w, idx):
    gathered, wide, idx, ok = _aggregate_parts(x, p, w, idx)
    terms = np.where(ok[..., None], gathered * wide, 0.0)
    return terms.sum(1), np.abs(terms).sum(1), ok.sum(1, keepdims=True)


def aggregate_backward(x, p, w, idx, g):
    """-> (grad_input, S, D), (grad_position, S, D), (grad_weight, S, D)"""
    gathered, wide, idx, ok = _aggregate_parts(x, p, w, idx)
    g = _np(g, np.float64)
    n, ns, c = gathered.shape
    w_c = np.shape(w)[2]
    gw = np.where(ok[..., None], g[:, None, :] * wide, 0.0)            # grad_position, and the terms of grad_input
    tw = np.where(ok[..., None], g[:, None, :] * gathered, 0.0).reshape(n, ns, c // w_c, w_c)
    return (_scatter(n, c, idx[ok], gw[ok]), (gw, np.abs(gw), 1), (tw.sum(2), np.abs(tw).sum(2), c // w_c))


def ragged(sizes, seed, scale=1.0):
    """A concatenated cloud of the given segment sizes: (xyz (sum,3) fp32 uniform in [-scale, scale], cumulative ends int32)."""
    sizes = np.asarray(sizes, np.int64)
    xyz = np.random.default_rng(seed).uniform(-scale, scale, (int(sizes.sum()), 3)).astype(np.float32)
    return xyz, np.cumsum(sizes).astype(np.int32)
