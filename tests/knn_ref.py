"""CPU restatement of include/unipre3d_knn.h: the k smallest (d2, index) pairs in lexicographic order, ascending.

`knn` computes d2 in fp32 exactly as the header states it -- dx = q - s per coordinate, then (dx*dx + dy*dy) + dz*dz with every
operation rounded on its own (numpy's elementwise fp32 arithmetic never fuses) -- and takes a STABLE sort on d2, which orders equal
distances by index.  `knn_f64` is the same selection on distances computed in fp64 from the same fp32 coordinates.  `gaps` gives,
per query, the smallest fp64 gap between consecutive distances among its first k + 1: where that exceeds the rounding error of an
fp32 form, the form cannot select anything else."""
import numpy as np


def _np(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def dist2(support, query, dtype=np.float32):
    """(B,N,3), (B,M,3) -> (B,M,N) squared distances in `dtype`, each operation rounded in it."""
    s, q = _np(support, np.float32).astype(dtype), _np(query, np.float32).astype(dtype)
    dx = q[:, :, None, 0] - s[:, None, :, 0]
    dy = q[:, :, None, 1] - s[:, None, :, 1]
    dz = q[:, :, None, 2] - s[:, None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == dtype
    return d


def _select(d, k):
    n = d.shape[-1]
    if not 1 <= k <= n:
        raise ValueError(f"k = {k} is outside 1..{n}")
    order = np.argsort(d, axis=-1, kind="stable")[..., :k]            # stable: equal distances stay in index order
    return np.take_along_axis(d, order, -1), order.astype(np.int32)


def knn(k, support, query):
    """-> (dist2 (B,M,k) fp32, idx (B,M,k) int32): what u3d_knn writes, bit for bit."""
    return _select(dist2(support, query, np.float32), k)


def knn_f64(k, support, query):
    return _select(dist2(support, query, np.float64), k)


def gaps(k, support, query):
    """(B,M) smallest fp64 gap between consecutive distances among each query's first min(k + 1, N)."""
    d = np.sort(dist2(support, query, np.float64), axis=-1)[..., :k + 1]
    return np.diff(d, axis=-1).min(-1) if d.shape[-1] > 1 else np.full(d.shape[:2], np.inf)


def keys(d2, idx):
    """The uint64 selection keys (bits(d2) << 32) | index of a result."""
    return (np.ascontiguousarray(d2, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def lattice():
    """The 4 x 4 x 4 integer lattice, (1, 64, 3): many exactly equal distances."""
    g = np.arange(4, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, 64, 3)


def duplicated(n=48, seed=3):
    """(1, 2n, 3): a seeded cloud followed by a copy of itself, so every point has a twin at distance 0 with a higher index."""
    p = np.random.default_rng(seed).uniform(-1, 1, (1, n, 3)).astype(np.float32)
    return np.concatenate([p, p], 1)
