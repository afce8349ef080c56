"""Scalar-loop reference and case builders for the object-level z-buffer fusion (unipre3d_amd/csrc/u3d_fusion.hip).  No GPU, no oracle
library: numpy only.

`zbuffer_loop` is a second, independent statement of what oracle/fusion_oracle.py vectorises (tests/test_fusion_ref.py holds the two
bit for bit against each other and against golden G15, recorded from the reference's own module): one Python loop over the points, one
dict per item, every pixel operation a scalar np.float32 operation.  `grad_loop` is the fp64 scatter-add of the winners' rows;
for integer cotangents every sum is exact, so it is THE result in any order.

Builders: every scene is made of camera-space points (x, y, z, 1) for fx = fy = 1, cx = cy = 0, where the pixel is (rint(x / z),
rint(y / z)).  `points_at` places a point on pixel s = px * W + py at a depth that is a power of two, so x = px * z and the quotient
are exact.  Each scene returns what it claims to hold next to the points, and test_fusion_ref.py asserts the claims.
"""
import numpy as np

F32 = np.float32
EMPTY = 0xFFFFFFFFFFFFFFFF
SIZES = ((6, 9), (9, 6), (8, 12))                 # image sizes of the edge set: H < W, H > W, and H * W a multiple of 4
U24 = 2.0 ** -24                                   # fp32 unit roundoff


def depth_bits(z):
    """bits of an fp32 depth >= 0 as the winner word holds them (-0.0 counts as +0.0)"""
    z = F32(z)
    return int(np.array(F32(0.0) if z == 0 else z, F32).view(np.uint32))


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def zbuffer_loop(cam, feat, fx, fy, cx, cy):
    """cam (B,N,4), feat (B,C,H,W) -> (mapped (B,N,C) fp32, sel (B,N) int32, table): table[b] maps a pixel s = px*W + py that holds a
    point to (bits of its minimum depth, smallest index among the points at that depth); pixels without a point are absent."""
    cam, feat = np.asarray(cam, F32), np.asarray(feat, F32)
    B, N = cam.shape[:2]
    _, C, H, W = feat.shape
    fx, fy, cx, cy = F32(fx), F32(fy), F32(cx), F32(cy)
    mapped, sel, table = np.zeros((B, N, C), F32), np.full((B, N), -1, np.int32), []
    for b in range(B):
        where, best = [None] * N, {}
        for n in range(N):
            x, y, z = cam[b, n, 0], cam[b, n, 1], cam[b, n, 2]
            with np.errstate(all="ignore"):
                u = np.rint(F32(F32(x * fx) / z) + cx)
                v = np.rint(F32(F32(y * fy) / z) + cy)
            if not (abs(u) < F32(1e9)) or not (abs(v) < F32(1e9)):      # NaN, infinite or beyond any image: outside
                continue
            px, py = int(u), int(v)                                      # -0.0 is pixel 0
            if px < 0 or py < 0 or px >= H or py >= W or not (z >= 0):   # the reference compares px with H and py with W
                continue
            s = px * W + py
            where[n] = s
            if s not in best or z < best[s][0]:
                best[s] = (z, n)
        for n in range(N):
            s = where[n]
            if s is not None and cam[b, n, 2] == best[s][0]:
                sel[b, n] = s
                for c in range(C):
                    mapped[b, n, c] = feat[b, c, s // W, s % W]
        table.append({s: (depth_bits(z), n) for s, (z, n) in best.items()})
    return mapped, sel, table


def winner_words(table, H, W):
    """the table of zbuffer_loop as the (B, H*W) uint64 words of include/unipre3d_fusion.h: depth bits << 32 | first winner, all-ones if empty"""
    out = np.full((len(table), H * W), EMPTY, np.uint64)
    for b, t in enumerate(table):
        for s, (bits, n) in t.items():
            out[b, s] = (bits << 32) | n
    return out


def grad_loop(grad_mapped, sel, B, C, H, W):
    """fp64 scatter-add of the winners' rows: grad[b, :, px, py] += grad_mapped[b, n, :] for sel[b, n] = px*W + py >= 0"""
    g = np.zeros((B, C, H * W), np.float64)
    for b in range(B):
        for n in range(sel.shape[1]):
            s = int(sel[b, n])
            if s >= 0:
                for c in range(C):
                    g[b, c, s] += float(grad_mapped[b, n, c])
    return g.reshape(B, C, H, W)


def grad_terms(grad_mapped, sel, B, C, H, W):
    """-> (count (B,1,H,W) rows added into a pixel, mag (B,C,H,W) fp64 sum of their absolute values)"""
    cnt, mag = np.zeros((B, 1, H * W)), np.zeros((B, C, H * W))
    for b in range(B):
        for n in range(sel.shape[1]):
            s = int(sel[b, n])
            if s >= 0:
                cnt[b, 0, s] += 1
                mag[b, :, s] += np.abs(np.asarray(grad_mapped[b, n], np.float64))
    return cnt.reshape(B, 1, H, W), mag.reshape(B, C, H, W)


def assert_grad_any_order(got, grad_mapped, sel, B, C, H, W):
    """An element fed by at most one row is a copy (or a zero): bit for bit.  One fed by k rows is k - 1 fp32 additions in some order:
    within k * 2^-24 * sum |g_i| of the fp64 sum (the standard bound; the k-th unit covers the rounding of the comparison's own operands)."""
    ref = grad_loop(grad_mapped, sel, B, C, H, W)
    cnt, mag = grad_terms(grad_mapped, sel, B, C, H, W)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape
    single = np.broadcast_to(cnt <= 1, ref.shape)
    assert np.array_equal(got[single], ref.astype(F32)[single])
    assert np.all(np.abs(got.astype(np.float64) - ref)[~single] <= (np.broadcast_to(cnt, ref.shape) * U24 * mag)[~single])


# ---- placing points ---------------------------------------------------------------------------------------------------------------------------
def points_at(s, depth, W):
    """points on the pixels s = px*W + py at the depths given (powers of two keep x = px * z and x / z exact) -> (len(s), 4) fp32"""
    s, z = np.asarray(s, np.int64).reshape(-1), np.broadcast_to(np.asarray(depth, F32), np.asarray(s).reshape(-1).shape)
    return np.stack([(s // W).astype(F32) * z, (s % W).astype(F32) * z, z, np.ones_like(z)], axis=1).astype(F32)


BEHIND = np.array([1.0, 1.0, -1.0, 1.0], F32)     # pixel (-1, -1) and a negative depth: never inside


def behind(n):
    return np.tile(BEHIND, (n, 1))


def _edge_rows(H, W):
    """(name, [(x, y, z), ...], pixel every row of the group lands on or None if they differ, whether every row wins its pixel or None)"""
    below = np.nextafter(F32(-0.5), F32(-1))                     # the float just below -0.5: rounds to -1
    ulp = np.nextafter(F32(1), F32(2))
    half = []
    for k in range(6):                                            # half-integer pixels on both axes: k + 0.5 goes to the EVEN neighbour
        half += [(k + 0.5, k, 1), (k, k + 0.5, 1)]
    border = []
    for a in (H - 0.5, H - 1, H, W - 0.5, W - 1, W):              # the borders: px is compared with H, py with W
        border += [(a, 0, 1), (0, a, 1)]
    return [
        ("half", half, None, None),
        ("minus_half", [(-0.5, 3, 1), (3, -0.5, 1), (-0.5, -0.5, 1)], None, True),      # -0.5 rounds to -0.0, which is pixel 0
        ("below_minus_half", [(below, 3, 1), (3, below, 1)], None, False),
        ("border", border, None, None),
        ("corner", [(H - 1, W - 1, 1), (W - 1, H - 1, 1)], None, None),                  # the last pixel, and its transpose
        ("behind", [(-2, -3, -1), (-1, -1, -0.5)], None, False),                         # z < 0 with an inside pixel: (2, 3) and (2, 2)
        ("zero_depth", [(0, 0, 0), (1, 2, 0), (1, 2, -0.0), (-1, 2, 0)], None, False),   # 0/0 = NaN, x/0 = inf, x/-0.0 = -inf
        ("subnormal", [(1, 1, 1e-45), (1, 1, 1e-40)], None, False),                      # the quotient overflows
        ("huge", [(3e30, 2e30, 1e30)], (3, 2), True),
        ("ulp_far", [(4 * ulp, ulp, ulp)], (4, 1), False),                               # two depths one ulp apart: the later, nearer one wins
        ("ulp_near", [(4, 1, 1)], (4, 1), True),
        ("far3", [(2 * 4, 5 * 4, 4)], (2, 5), False),
        ("tie3", [(2 * 2, 5 * 2, 2)] * 3, (2, 5), True),
        ("far70", [(5, 2, 1)], (5, 2), False),
        ("tie70", [(5 * 0.5, 2 * 0.5, 0.5)] * 70, (5, 2), True),
    ]


def edge_points(H, W):
    """The edge set: (117, 4) camera-space points for fx = fy = 1, cx = cy = 0 (pixel = rint(x / z), rint(y / z)).  The pixels it names
    outright have both coordinates <= 5, so the set fits the three SIZES; the border rows depend on (H, W)."""
    rows = [r for _, g, _, _ in _edge_rows(H, W) for r in g]
    out = np.ones((len(rows), 4), F32)
    out[:, :3] = np.array(rows, F32)
    return out


def edge_claims(H, W):
    """what edge_points promises: [(name, first index, count, pixel (px, py) or None, wins or None)]"""
    out, at = [], 0
    for name, g, pixel, wins in _edge_rows(H, W):
        out.append((name, at, len(g), pixel, wins))
        at += len(g)
    return out


def with_nonfinite(cam, H, W):
    """B = 2 from one (N, 4) set, for direct kernel calls (the world-to-camera matmul cannot carry an infinity).  Both items end with
    NaN in x, in y and in z and a +inf-depth point (pixel (0, 0): finite / inf = 0).  Item 0 keeps the set, so the +inf depth shares pixel
    (0, 0) with finite points and loses; in item 1 every point of the set that lands on pixel (0, 0) is moved behind the camera, so the
    +inf depth is alone there and wins.  -> (cam (2, N + 4, 4), index of the +inf point)"""
    nan, inf = F32(np.nan), F32(np.inf)
    tail = np.array([[nan, 1, 1, 1], [1, nan, 1, 1], [1, 1, nan, 1], [3, 2, inf, 1]], F32)
    a = np.concatenate([cam, tail])
    b = a.copy()
    with np.errstate(all="ignore"):
        on0 = (np.rint(cam[:, 0] / cam[:, 2]) == 0) & (np.rint(cam[:, 1] / cam[:, 2]) == 0)
    b[:len(cam)][on0] = BEHIND
    return np.stack([a, b]), len(a) - 1


# ---- structured scenes ------------------------------------------------------------------------------------------------------------------------
def image_for(n_pixels):
    """the smallest of the images (h, h) and (h, h + 1) that holds n_pixels pixels"""
    h = 1
    while h * (h + 1) < n_pixels:
        h += 1
    return (h, h) if h * h >= n_pixels else (h, h + 1)


def launch_scene(B, N, H, W, seed=0):
    """Two thirds of an item's points on distinct pixels at depth 1, the rest duplicated onto them: the even ones at depth 1 (they tie),
    the odd ones at depth 2 (they lose); the order is shuffled per item.  -> (cam (B,N,4), claims: per item (winners, losers, tied pixels))"""
    rng = np.random.RandomState(seed)
    nd = max(1, (2 * N + 2) // 3)
    assert nd <= H * W
    cam, claims = np.zeros((B, N, 4), F32), []
    for b in range(B):
        pix = rng.permutation(H * W)[:nd]
        s = np.concatenate([pix, pix[np.arange(N - nd) % nd]])
        z = np.concatenate([np.ones(nd, F32), np.where(np.arange(N - nd) % 2 == 0, F32(1), F32(2))])
        order = rng.permutation(N)
        cam[b] = points_at(s, z, W)[order]
        losers = int(np.sum(z == 2))
        claims.append((N - losers, losers, int(np.sum(np.arange(N - nd) % 2 == 0))))
    return cam, claims


def tie_scene(k, variant, B, N, H, W):
    """k points at depth 2 on pixel T = H*W // 2 of every item, at indices spread evenly from 3 to N - 2 (first and last more than 256 apart
    for N >= 300; in item b they are the launch's points b*N + 3 .. b*N + N - 2).  variant "plain": nothing else on T.  "nearer_late": index
    N - 1 holds a point on T at depth 1, so all k lose.  "farther_early": index 0 holds a point on T at depth 4, which loses.
    Every other index is behind the camera except index 1, a single winner on pixel 0.  -> (cam (B,N,4), tied indices, T)"""
    assert N >= k + 5 and H * W >= 2
    T = (H * W) // 2
    idx = np.unique(np.round(np.linspace(3, N - 2, k)).astype(np.int64)) if k > 1 else np.array([3])
    assert len(idx) == k
    one = behind(N)
    one[idx] = points_at([T] * k, 2, W)
    one[1] = points_at([0], 1, W)[0]
    if variant == "nearer_late":
        one[N - 1] = points_at([T], 1, W)[0]
    elif variant == "farther_early":
        one[0] = points_at([T], 4, W)[0]
    else:
        assert variant == "plain"
    return np.tile(one[None], (B, 1, 1)), idx, T


def permutation_scene(B, H, W, seed=0):
    """N = H*W points, one per pixel, in a different random order in every item -> (cam, perm (B, N): pixel of point n)"""
    rng = np.random.RandomState(seed)
    perm = np.stack([rng.permutation(H * W) for _ in range(B)])
    return np.stack([points_at(p, 1, W) for p in perm]), perm


def single_scene(B, N, H, W, s, at=None):
    """N points per item of which exactly one, index `at` (default N // 2), is inside: on pixel s.  s = None: no point is inside."""
    cam = np.tile(behind(N)[None], (B, 1, 1))
    if s is not None:
        cam[:, N // 2 if at is None else at] = points_at([s], 1, W)[0]
    return cam


def backward_scenes(B, H, W):
    """name -> cam for the scenes of the backward sweep: one winner on every pixel, none, pixel 0, pixel HW-1 and, where H*W is a multiple of 4,
    position j of the first and of the last quad"""
    HW = H * W
    out = {"permutation": permutation_scene(B, H, W, seed=HW)[0], "none": single_scene(B, 5, H, W, None), "first": single_scene(B, 5, H, W, 0),
           "last": single_scene(B, 5, H, W, HW - 1)}
    if HW % 4 == 0:
        for q in sorted({0, HW // 4 - 1}):
            for j in range(4):
                out[f"quad{q}_pos{j}"] = single_scene(B, 5, H, W, 4 * q + j)
    return out


def items_differ_scene(N, H, W, seed=0):
    """B = 3: items 0 and 2 hold the same points (launch_scene), item 1 has every point behind the camera"""
    cam, claims = launch_scene(1, N, H, W, seed)
    return np.stack([cam[0], behind(N), cam[0]]), claims[0]


def integer_cotangent(shape, seed=0):
    """integers in [-8, 8] as fp32: every partial sum of up to 2^20 of them is an exactly representable integer"""
    return np.random.RandomState(seed).randint(-8, 9, shape).astype(F32)
