"""Torch restatement of unipre3d_amd.sparseconv in gather form (DESIGN.md §7 "Sparse 3D convolution"): maps built by numpy
dictionaries, convolutions as per-tap gather + matmul + index_add.  Runs in any dtype on CPU or on the device; the tests use fp64.

Weights are (Cout, k, k, k, Cin); tap t = (k0 * k + k1) * k + k2.  Repeated sites: SubM reads a site's lowest row at every tap, the
strided conv sums every row at a site, the inverse writes every row."""
import numpy as np
import torch


def _sites(indices):
    return [tuple(int(v) for v in r) for r in np.asarray(indices).reshape(-1, 4)]


def subm_table(indices, spatial_shape, k):
    """(N, k^3) int64: the lowest row at site + (k0, k1, k2) - k // 2, or -1."""
    sites = _sites(indices)
    lowest = {}
    for i, s in enumerate(sites):
        lowest.setdefault(s, i)
    h, D = k // 2, [int(d) for d in spatial_shape]
    offs = [(a - h, b - h, c - h) for a in range(k) for b in range(k) for c in range(k)]
    T = np.full((len(sites), k ** 3), -1, dtype=np.int64)
    for i, (b, x, y, z) in enumerate(sites):
        for t, (dx, dy, dz) in enumerate(offs):
            q = (b, x + dx, y + dy, z + dz)
            if 0 <= q[1] < D[0] and 0 <= q[2] < D[1] and 0 <= q[3] < D[2]:
                T[i, t] = lowest.get(q, -1)
    return T


def down_map(indices, spatial_shape, s):
    """SparseConv3d with kernel == stride = s: out_indices (M,4) ascending, out_shape, row_out (N) (-1: dropped), row_tap (N),
    table (M, s^3) lowest row per (output, tap)."""
    sites = _sites(indices)
    O = [(int(d) - s) // s + 1 for d in spatial_shape]
    outs, row_out, row_tap = set(), [], []
    for (b, x, y, z) in sites:
        o = (b, x // s, y // s, z // s)
        if o[1] < O[0] and o[2] < O[1] and o[3] < O[2]:
            outs.add(o)
    out_list = sorted(outs)
    rank = {o: i for i, o in enumerate(out_list)}
    K = s ** 3
    table = np.full((len(out_list), K), -1, dtype=np.int64)
    for i, (b, x, y, z) in enumerate(sites):
        o = (b, x // s, y // s, z // s)
        t = ((x % s) * s + y % s) * s + z % s
        if o in rank:
            row_out.append(rank[o])
            row_tap.append(t)
            if table[rank[o], t] < 0:
                table[rank[o], t] = i
        else:
            row_out.append(-1)
            row_tap.append(-1)
    out_indices = np.array(out_list, dtype=np.int64).reshape(-1, 4)
    return dict(out_indices=out_indices, out_shape=O, row_out=np.array(row_out, dtype=np.int64), row_tap=np.array(row_tap, dtype=np.int64),
                table=table)


def _w(W, t):   # tap t of a (Cout, k, k, k, Cin) weight as (Cin, Cout)
    Cout, Cin = W.shape[0], W.shape[-1]
    return W.reshape(Cout, -1, Cin)[:, t, :].t()


def subm(X, W, b, T):
    """Y[o] = b + sum_k X[T[o,k]] W_k."""
    T = torch.as_tensor(T, device=X.device)
    Y = X.new_zeros(X.shape[0], W.shape[0])
    for t in range(T.shape[1]):
        rows = torch.nonzero(T[:, t] >= 0).flatten()
        if rows.numel():
            Y = Y.index_add(0, rows, X[T[rows, t]] @ _w(W, t))
    return Y if b is None else Y + b


def down(X, W, b, m):
    """Y[o] = b + sum over rows i with output o of X[i] W_tap(i)."""
    row_out, row_tap = (torch.as_tensor(m[k], device=X.device) for k in ("row_out", "row_tap"))
    Y = X.new_zeros(len(m["out_indices"]), W.shape[0])
    for t in range(W.reshape(W.shape[0], -1, W.shape[-1]).shape[1]):
        rows = torch.nonzero(row_tap == t).flatten()
        if rows.numel():
            Y = Y.index_add(0, row_out[rows], X[rows] @ _w(W, t))
    return Y if b is None else Y + b


def inverse(X, W, b, m):
    """Y[i] = b + X[out(i)] W_tap(i) at every input row of the paired conv (dropped rows: b)."""
    row_out, row_tap = (torch.as_tensor(m[k], device=X.device) for k in ("row_out", "row_tap"))
    Y = X.new_zeros(len(m["row_out"]), W.shape[0])
    for t in range(W.reshape(W.shape[0], -1, W.shape[-1]).shape[1]):
        rows = torch.nonzero(row_tap == t).flatten()
        if rows.numel():
            Y = Y.index_add(0, rows, X[row_out[rows]] @ _w(W, t))
    return Y if b is None else Y + b


def dense_grid(X, indices, spatial_shape, batch_size):
    """(B, C, D0, D1, D2) with the rows scattered at their sites (sites assumed distinct)."""
    idx = torch.as_tensor(np.asarray(indices), device=X.device).long()
    G = X.new_zeros(batch_size, *[int(d) for d in spatial_shape], X.shape[1])
    G = G.index_put((idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]), X)
    return G.permute(0, 4, 1, 2, 3)


def sample(G, indices):
    idx = torch.as_tensor(np.asarray(indices), device=G.device).long()
    return G.permute(0, 2, 3, 4, 1)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]


def _lin(idx, D):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 4)
    return ((idx[:, 0] * D[0] + idx[:, 1]) * D[1] + idx[:, 2]) * D[2] + idx[:, 3]


def subm_table_np(indices, spatial_shape, k):
    """subm_table vectorized (sorted keys + searchsorted) for the large scenes; tests pin it to the dictionary version."""
    D = [int(d) for d in spatial_shape]
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    keys = _lin(idx, D)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    h = k // 2
    T = np.full((len(idx), k ** 3), -1, dtype=np.int64)
    t = 0
    for a in range(k):
        for b in range(k):
            for c in range(k):
                q = idx + np.array([0, a - h, b - h, c - h])
                ok = (q[:, 1:] >= 0).all(1) & (q[:, 1] < D[0]) & (q[:, 2] < D[1]) & (q[:, 3] < D[2])
                qk = _lin(np.where(ok[:, None], q, 0), D)
                p = np.minimum(np.searchsorted(sk, qk), max(len(sk) - 1, 0))
                hit = ok & (len(sk) > 0) & (sk[p] == qk if len(sk) else False)
                T[hit, t] = order[p[hit]]
                t += 1
    return T


def chains_np(indices, spatial_shape):
    """(first, next) int64 over the rows of each site: first[r] the lowest row at r's site, next[r] the next higher row there or -1."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    keys = _lin(idx, [int(d) for d in spatial_shape])
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    first, nxt = np.empty(len(idx), np.int64), np.full(len(idx), -1, np.int64)
    head = np.concatenate([[True], sk[1:] != sk[:-1]]) if len(idx) else np.zeros(0, bool)
    first[order] = order[np.maximum.accumulate(np.where(head, np.arange(len(idx)), 0))] if len(idx) else 0
    same = ~head[1:] if len(idx) else head
    nxt[order[:-1][same]] = order[1:][same]
    return first, nxt
