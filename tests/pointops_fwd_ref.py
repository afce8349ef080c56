"""Plain fp64 references, input builders and tie constructions for the FORWARD kernels of the point operators (u3d_group_points /
u3d_gather_points, u3d_three_interpolate, u3d_three_nn).  No GPU, no oracle library: numpy only.

References: group / gather are `take_along_axis` (a copy: the bits of the source element); three_interpolate is the fp64 sum of three products
with the magnitude sum |w_k p_k| a rounding bound scales with; three_nn is DEFINED here as the three smallest (squared distance, index) pairs
in lexicographic order, from fp64 squared distances -- not as a scan.

Exact inputs: features are integers in [-8, 8], weights multiples of 1/8 in [0, 1], coordinates multiples of 1/4 in [-2, 2].  Every product, every
partial sum and every squared distance is then a small dyadic number that fp32 holds exactly whichever product a fused multiply-add leaves
unrounded, so every correct implementation gives the fp64 result bit for bit in all three contraction modes.

Constructions return the inputs together with the answer they claim, so that a test asserts the claim on the reference before it uses them."""
import numpy as np

NN_TILE, NN_SPLIT = 2048, 4          # three_nn walks the known cloud in LDS tiles of 2048 and deals a tile's points to 4 lanes (j % 4)
RESERVED_X = 2.0                     # background clouds of the constructions keep x <= 1: what is placed at x = 2 is at least 1 away from them


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def group(points, idx):
    """points (B, C, N), idx (B, npoint, nsample) -> (B, C, npoint, nsample): out[b, c, p, s] = points[b, c, idx[b, p, s]], copied."""
    points, idx = np.asarray(points), np.asarray(idx)
    B, C, _ = points.shape
    flat = idx.reshape(B, 1, -1).astype(np.int64)
    assert flat.size == 0 or (flat.min() >= 0 and flat.max() < points.shape[2])
    out = np.take_along_axis(points, np.broadcast_to(flat, (B, C, flat.shape[2])), axis=2)
    return out.reshape((B, C) + idx.shape[1:])


def gather(points, idx):
    """points (B, C, N), idx (B, npoint) -> (B, C, npoint)"""
    return group(points, np.asarray(idx)[:, :, None])[..., 0]


def three_interpolate_fp64(points, idx, w):
    """points (B, C, M), idx / w (B, n, 3) -> (out (B, C, n) fp64 = sum_k w_k p[idx_k], mag (B, C, n) = sum_k |w_k p[idx_k]|)"""
    p = np.asarray(points).astype(np.float64)
    ix, wt = np.asarray(idx).astype(np.int64), np.asarray(w).astype(np.float64)
    B, C, M = p.shape
    n = ix.shape[1]
    assert ix.shape == (B, n, 3) and wt.shape == (B, n, 3) and (ix.size == 0 or (ix.min() >= 0 and ix.max() < M))
    out, mag = np.zeros((B, C, n)), np.zeros((B, C, n))
    for k in range(3):
        term = np.take_along_axis(p, np.broadcast_to(ix[:, None, :, k], (B, C, n)), axis=2) * wt[:, None, :, k]
        out += term
        mag += np.abs(term)
    return out, mag


def three_nn_lex(unknown, known):
    """unknown (B, n, 3), known (B, m, 3) -> (d2 (B, n, 3) fp64 squared distances, idx (B, n, 3) int32): the three smallest (distance, index)
    pairs in lexicographic order.  A known point whose squared distance is not finite IN FP32 is no candidate (the operator's initial
    best is 1e40 and `inf < 1e40` is false); a slot without a candidate (m < 3, m = 0) is (+inf, 0)."""
    u, k = np.asarray(unknown).astype(np.float64), np.asarray(known).astype(np.float64)
    B, n, _ = u.shape
    m = k.shape[1]
    d2, idx = np.full((B, n, 3), np.inf), np.zeros((B, n, 3), np.int32)
    if m == 0 or n == 0:
        return d2, idx
    diff = u[:, :, None, :] - k[:, None, :, :]
    d = (diff * diff).sum(-1)                                            # (B, n, m)
    with np.errstate(over="ignore"):
        d[~np.isfinite(d.astype(np.float32))] = np.inf
    order = np.argsort(d, axis=-1, kind="stable")[:, :, :3]             # stable: equal distances stay in index order
    best = np.take_along_axis(d, order, -1)
    t = min(m, 3)
    d2[:, :, :t] = best
    idx[:, :, :t] = np.where(np.isfinite(best), order, 0)
    return d2, idx


# ---- exact inputs ---------------------------------------------------------------------------------------------------------------------------
def exact_features(b, c, m):
    """integers in [-8, 8] that tell clouds, channels and points apart: the value changes with every one of the three indices"""
    bi, ci, p = np.arange(b)[:, None, None], np.arange(c)[None, :, None], np.arange(m)[None, None, :]
    return (((7 * p + 3 * ci + 5 * bi + (p * p) // 3 + ci * (p % 3)) % 17) - 8).astype(np.float32)


def exact_weights(b, n, seed):
    return (np.random.RandomState(seed).randint(0, 9, (b, n, 3)) / 8.0).astype(np.float32)


def exact_coords(b, n, seed, xmax=2.0):
    """multiples of 1/4 in [-2, 2]^3 (x <= xmax), another cloud per batch entry; 17^3 sites, so larger clouds repeat sites: exact ties"""
    rng = np.random.RandomState(seed)
    xyz = rng.randint(-8, 9, (b, n, 3)).astype(np.float32) / np.float32(4)
    xyz[..., 0] = rng.randint(-8, int(xmax * 4) + 1, (b, n)).astype(np.float32) / np.float32(4)
    return xyz


def interp_index_sets(b, m, n, seed):
    """{name: (idx (b, n, 3) int32, w (b, n, 3) fp32 in eighths)}: random triples, i0 == i1 == i2, every index m - 1, every index 0, and a
    set whose middle weight is exactly 0 (on a finite feature: the term must vanish, not poison)."""
    rng = np.random.RandomState(seed)
    w = exact_weights(b, n, seed + 1)
    rnd = rng.randint(0, m, (b, n, 3)).astype(np.int32)
    same = np.repeat(rng.randint(0, m, (b, n, 1)), 3, axis=2).astype(np.int32)
    w0 = np.maximum(w, np.float32(0.125)); w0[:, :, 1] = 0
    return {"random": (rnd, w), "same": (same, w), "last": (np.full((b, n, 3), m - 1, np.int32), w),
            "first": (np.zeros((b, n, 3), np.int32), w), "zero_weight": (rnd, w0)}


def gauss_interp_inputs(b, c, m, n, seed):
    """Gaussian features, uniform weights, random triples: the inputs on which the contraction modes differ in the last bit"""
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((b, c, m)).astype(np.float32), rng.randint(0, m, (b, n, 3)).astype(np.int32),
            rng.rand(b, n, 3).astype(np.float32))


# ---- group / gather inputs ------------------------------------------------------------------------------------------------------------------
# -0.0, the smallest denormal, a larger denormal, +Inf, -Inf, two quiet NaNs of different payload and sign
SPECIALS = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345], np.uint32)


def special_features(b, c, n, seed):
    """(b, c, n) fp32 normals with the SPECIALS planted at both ends of every row and at every fifth element between, another one per
    (cloud, channel, point); rows of any length start and end with one."""
    bits = np.random.RandomState(seed).standard_normal((b, c, n)).astype(np.float32).view(np.uint32).copy()
    bi, ci, p = np.arange(b)[:, None, None], np.arange(c)[None, :, None], np.arange(n)[None, None, :]
    which = np.broadcast_to((p + 2 * ci + 3 * bi) % len(SPECIALS), bits.shape)
    plant = np.broadcast_to((p < 7) | (p >= n - 7) | (p % 5 == 0), bits.shape)
    bits[plant] = SPECIALS[which[plant]]
    return bits.view(np.float32)


def group_index_sets(b, n, npoint, nsample, seed):
    """{name: idx (b, npoint, nsample) int32}: random, all 0, all n - 1, and ball-query padding (a group's first hit repeated from a
    random position on)"""
    rng = np.random.RandomState(seed)
    rnd = rng.randint(0, n, (b, npoint, nsample)).astype(np.int32)
    pad = rnd.copy()
    hits = rng.randint(1, nsample + 1, (b, npoint, 1))
    pad = np.where(np.arange(nsample)[None, None, :] < hits, pad, pad[:, :, :1]).astype(np.int32)
    return {"random": rnd, "first": np.zeros_like(rnd), "last": np.full_like(rnd, n - 1), "padded": pad}


# ---- three_nn constructions -----------------------------------------------------------------------------------------------------------------
def _background(b, n, m, seed):
    """queries anywhere on the quarter lattice, known points with x <= 1"""
    return exact_coords(b, n, seed), exact_coords(b, m, seed + 1, xmax=1.0)


def twins_over_tile_edge(b=2, n=8, seed=41):
    """m = 4100 (two full LDS tiles and four points).  Known 2047 and 2048 -- the last point of tile 0 and the first of tile 1 -- coincide
    with query 0; known 0 and 4099 with query 1; known 2046 .. 2049 are all at squared distance 1/4 from query 2.  Lower index first:
    query 0 -> (2047, 2048, 2046) [2046 and 2049 tie at 1/2], query 1 -> (0, 4099, .), query 2 -> (2046, 2047, 2048).
    -> (unknown, known, {query: expected leading indices})"""
    m = 4100
    unk, kn = _background(b, n, m, seed)
    P = np.array([2, 2, 2], np.float32)
    unk[:, 0] = P; kn[:, 2047] = P; kn[:, 2048] = P
    Q = np.array([2, -2, -2], np.float32)
    unk[:, 1] = Q; kn[:, 0] = Q; kn[:, 4099] = Q
    unk[:, 2] = [2, 2, 1.5]
    kn[:, 2046] = [2, 1.5, 1.5]; kn[:, 2049] = [1.5, 2, 1.5]
    return unk, kn, {0: (2047, 2048, 2046), 1: (0, 4099), 2: (2046, 2047, 2048)}


def all_known_identical(m, b=2, n=5, seed=43):
    """every known point at one site: all distances tie, the winners are the lowest indices -- for m = 7 indices 0, 1, 2, which three
    DIFFERENT lanes of the quad hold; for m = 2 (0, 1) and an unfilled third slot (+inf, index 0).
    -> (unknown, known, expected index triple of every query, number of filled slots)"""
    unk = exact_coords(b, n, seed)
    kn = np.empty((b, m, 3), np.float32)
    kn[:] = np.array([0.25, -0.5, 1.0], np.float32)
    want = [0, 1, 2][:min(m, 3)] + [0] * (3 - min(m, 3))
    return unk, kn, tuple(want), min(m, 3)


def last_three_nearest(b=2, n=6, seed=47):
    """m = 2051: the second tile holds exactly three points, and they are the three nearest of every query (the queries sit at x = 2 beside
    them, every other known point has x <= 1).  -> (unknown, known, expected (2048, 2049, 2050))"""
    m = 2051
    _, kn = _background(b, n, m, seed)
    unk = exact_coords(b, n, seed + 2)
    unk[..., 0] = 2.0; unk[..., 1] = np.float32(0.5) + np.float32(0.25) * (np.arange(n) % 3)[None, :]; unk[..., 2] = 0
    kn[:, 2048] = [2, 0.75, -0.25]; kn[:, 2049] = [2, 0.75, -0.5]; kn[:, 2050] = [2, 0.75, -0.75]   # in index order for every query, all within 0.625
    return unk, kn, (2048, 2049, 2050)


def nearest_in_every_sublane(b=2, m=70, seed=53):
    """query s (s = 0 .. 3) coincides with known point 4 (3 + 2 s) + s -- index 4 k + s, scanned by lane s of the quad -- and with no other.
    -> (unknown, known, expected nearest index per query)"""
    unk, kn = _background(b, 4, m, seed)
    want = tuple(4 * (3 + 2 * s) + s for s in range(NN_SPLIT))
    for s, k in enumerate(want):
        site = np.array([2, -2 + s, 2 - s], np.float32)
        unk[:, s] = site; kn[:, k] = site
    return unk, kn, want


def far_known_point(m, b=2, n=3, seed=59):
    """known point 1 sits at 2e19 on every axis: its squared distance overflows fp32 to +inf in every contraction, and +inf is never
    inserted.  m = 2: (0, -, -) with two unfilled slots; m = 4: (the three finite points in distance order).
    -> (unknown, known, index of the far point)"""
    unk, kn = _background(b, n, m, seed)
    kn[:, 1] = np.float32(2e19)
    return unk, kn, 1
