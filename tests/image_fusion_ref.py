"""Restatement of the pixel-sparse image branch (unipre3d_amd/image_fusion.py, csrc/u3d_image_fusion.hip) in numpy: GroupNorm's statistics,
the normalised rows of the points that win their pixel, the 1x1 convolution on them, and the closed-form backward through
S[o][c] = sum_r dout[r][o] xhat[r][c] and s[o] = sum_r dout[r][o].  No GPU, no library.

`forward(..., np.float64)` / `backward(..., np.float64)` are the mathematics.  `forward32` / `backward32` follow the kernels' order in
fp32: f64 statistics rounded to fp32, xhat = (x - mean) * rstd, y = fma(xhat, gamma, beta), the products as one fused multiply-add per
reduction step (rows in ascending order inside a row split, the splits added in order), dW = fma(gamma, S, beta * s), the affine
gradients as f64 column sums.  (An fma is restated as the f64 product-and-sum rounded to fp32: the product of two fp32 numbers is exact
in f64.)  `variant=` names the wrong semantics the tests hold at a distance.

`case_inputs(tag)` builds the large inputs of golden G25's cases (map, parameters, cotangent) from numpy's frozen RandomState, so that the
record holds results, the small scene arrays and a checksum only.  tests/golden/make_g25_image_fusion.py and the tests share it."""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = 1e-6
BK = 32

# tag -> B, N, Cin, G, Cout, H, W (+ cls: the transformer's CLS token is in x)
CASES = {
    "sq": dict(B=2, N=64, Cin=8, G=2, Cout=6, H=16, W=16, cls=True),
    "rect": dict(B=3, N=40, Cin=12, G=3, Cout=5, H=12, W=20),
    "dims": dict(B=2, N=32, Cin=128, G=32, Cout=384, H=16, W=16),
    "const": dict(B=2, N=24, Cin=8, G=4, Cout=6, H=4, W=5),      # 40 elements per group: the unbiased variance is 2.5 % off
    "offset": dict(B=2, N=24, Cin=8, G=4, Cout=6, H=4, W=5),
    "nowin": dict(B=2, N=24, Cin=8, G=4, Cout=6, H=4, W=5),
}
QUANTITIES = ("out", "dW", "dbias", "dgamma", "dbeta")


def case_inputs(tag):
    """map (B,Cin,H,W), gamma, beta (Cin), weight (Cout,Cin), bias (Cout), cot (B,N,Cout): fp32, the same on every machine"""
    c = CASES[tag]
    B, N, Cin, G, Cout, H, W = (c[k] for k in ("B", "N", "Cin", "G", "Cout", "H", "W"))
    rs = np.random.RandomState(2500 + sorted(CASES).index(tag))
    x = rs.randn(B, Cin, H, W)
    cpg = Cin // G
    if tag == "const":
        x[0, :cpg] = 1.5                                   # exactly constant: var = 0, rstd = 1 / sqrt(eps)
        x[0, cpg:2 * cpg] *= 1e-3                          # var about eps: where eps sits decides rstd
    if tag == "offset":
        x = 0.1 * x + (10.0 + np.arange(Cin) // cpg)[None, :, None, None]
    out = {"map": x, "gamma": 1.0 + 0.3 * rs.randn(Cin), "beta": 0.3 * rs.randn(Cin),
           "weight": rs.randn(Cout, Cin) / np.sqrt(Cin), "bias": 0.3 * rs.randn(Cout), "cot": rs.randn(B, N, Cout)}
    return {k: np.ascontiguousarray(v, dtype=F32) for k, v in out.items()}


# shapes without a recorded case: one per dispatch class of the kernels (tests/test_gpu_image_fusion.py lists what each one covers)
# name -> (B, N, Cin, G, Cout, H, W, scene of tests/fusion_ref.py)
EDGE_SHAPES = {
    "odd_group": (2, 23, 12, 4, 6, 5, 7, "launch"),          # 105 floats a group: heads and tails, a group shorter than one pass
    "split_group": (1, 7, 6, 2, 6, 53, 53, "launch"),        # 8427 floats a group: two chunks, a ragged and misaligned last one; B = 1
    "one_point": (3, 1, 12, 4, 6, 5, 7, "first"),            # N = 1
    "all_win": (2, 35, 12, 4, 6, 5, 7, "permutation"),       # every row a winner
    "none_win": (2, 9, 12, 4, 6, 5, 7, "none"),              # no winner at all
    "two_splits": (2, 150, 12, 4, 6, 13, 13, "launch"),      # 300 rows: two row splits of 160, the last with 140; five row tiles
    "ragged_tiles": (2, 40, 40, 5, 70, 6, 9, "launch"),      # two column tiles and two reduction stages, both ragged
}


def edge_inputs(name):
    """(inputs like case_inputs, cam (B,N,4) for fx = fy = 1 and cx = cy = 0, sel (B,N))"""
    import fusion_ref
    B, N, Cin, G, Cout, H, W, kind = EDGE_SHAPES[name]
    rs = np.random.RandomState(2600 + sorted(EDGE_SHAPES).index(name))
    inp = {"map": rs.randn(B, Cin, H, W), "gamma": 1.0 + 0.3 * rs.randn(Cin), "beta": 0.3 * rs.randn(Cin),
           "weight": rs.randn(Cout, Cin) / np.sqrt(Cin), "bias": 0.3 * rs.randn(Cout), "cot": rs.randn(B, N, Cout)}
    inp = {k: np.ascontiguousarray(v, dtype=F32) for k, v in inp.items()}
    if kind == "launch":
        cam = fusion_ref.launch_scene(B, N, H, W, seed=N)[0]
    elif kind == "permutation":
        cam = fusion_ref.permutation_scene(B, H, W, seed=N)[0]
    else:
        cam = fusion_ref.single_scene(B, N, H, W, None if kind == "none" else 3, at=0)
    _, sel, _ = fusion_ref.zbuffer_loop(cam, inp["map"], 1.0, 1.0, 0.0, 0.0)
    return inp, np.ascontiguousarray(cam, dtype=F32), sel


def tolerance():
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "image_fusion", "tolerance.json")))


def checksum(inp):
    return np.array([np.sum(inp[k].astype(F64) * np.cos(np.arange(inp[k].size)).reshape(inp[k].shape)) for k in sorted(inp)], F64)


# ---- the kernels' work decomposition (host arithmetic of csrc/u3d_image_fusion.hip) -----------------------------------------------
CHUNK = 8192


def stats_chunks(Cin, G, H, W):
    return -(-(Cin // G) * H * W // CHUNK)


def rows_per_split(rows):
    s = max(1, min(64, (rows + 255) // 256))
    return (-(-rows // s) + BK - 1) // BK * BK


def row_splits(rows):
    return -(-rows // rows_per_split(rows))


# ---- pieces -----------------------------------------------------------------------------------------------------------------------------
def group_of(Cin, G, variant=None):
    c = np.arange(Cin)
    return c % G if variant == "group_mod" else c // (Cin // G)


def group_stats(x, G, eps=EPS, variant=None):
    """(mean, rstd) (B, G) in f64 from the map as stored; biased variance, eps under the root"""
    B, Cin = x.shape[:2]
    seg = np.asarray(x, F64).reshape(B, G, -1)
    L = seg.shape[2]
    mean = seg.sum(axis=2) / L
    var = np.maximum((seg * seg).sum(axis=2) / L - mean * mean, 0.0)
    if variant == "unbiased":
        var = var * L / (L - 1)
    rstd = 1.0 / (np.sqrt(var) + eps) if variant == "eps_outside" else 1.0 / np.sqrt(var + eps)
    return mean, rstd


def gather(x, sel):
    """rows (B,N,Cin): the pixel column sel = px * W + py of the map, zeros where sel < 0"""
    B, Cin, H, W = x.shape
    flat = x.reshape(B, Cin, H * W)
    rows = np.zeros((B, sel.shape[1], Cin), x.dtype)
    for b in range(B):
        win = sel[b] >= 0
        rows[b, win] = flat[b][:, sel[b][win]].T
    return rows


def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _xhat(rows, sel, mean, rstd, G, dtype, variant=None):
    B, N, Cin = rows.shape
    g = group_of(Cin, G, variant)
    m, r = mean.astype(dtype)[:, g][:, None, :], rstd.astype(dtype)[:, g][:, None, :]
    xh = ((rows.astype(dtype) - m) * r).astype(dtype)
    return np.where((sel >= 0)[:, :, None], xh, dtype(0))


# ---- mathematics (any dtype, numpy's own order) -----------------------------------------------------------------------------------
def forward(x, sel, p, G, dtype=F64, eps=EPS, variant=None):
    mean, rstd = group_stats(x, G, eps, variant)
    xh = _xhat(gather(x, sel), sel, mean, rstd, G, dtype, variant)
    y = xh * p["gamma"].astype(dtype) + p["beta"].astype(dtype)
    out = y @ p["weight"].astype(dtype).T + p["bias"].astype(dtype)
    return np.where((sel >= 0)[:, :, None], out, dtype(0)).astype(dtype)


def backward(x, sel, p, G, cot, dtype=F64, eps=EPS, variant=None):
    """{dW, dbias, dgamma, dbeta} by the S / s identity"""
    mean, rstd = group_stats(x, G, eps, variant)
    xh = _xhat(gather(x, sel), sel, mean, rstd, G, dtype, variant).reshape(-1, x.shape[1])
    d = np.where((sel >= 0)[:, :, None], cot.astype(dtype), dtype(0)).reshape(-1, cot.shape[2])
    S, s = d.T @ xh, d.sum(axis=0)
    W = p["weight"].astype(dtype)
    return {"dW": p["gamma"].astype(dtype)[None] * S + p["beta"].astype(dtype)[None] * s[:, None], "dbias": s,
            "dgamma": (W * S).sum(axis=0), "dbeta": (W * s[:, None]).sum(axis=0)}


# ---- fp32 in the kernels' order ---------------------------------------------------------------------------------------------------------
def forward32(x, sel, p, G, eps=EPS):
    mean, rstd = group_stats(x, G, eps)
    xh = _xhat(gather(x, sel), sel, mean, rstd, G, F32)
    B, N, Cin = xh.shape
    y = _fma(xh, p["gamma"], p["beta"]).reshape(B * N, Cin)
    W = p["weight"]
    acc = np.zeros((B * N, W.shape[0]), F32)
    for k in range(Cin):
        acc = _fma(y[:, k:k + 1], W[None, :, k], acc)
    out = (acc + p["bias"][None]).astype(F32).reshape(B, N, -1)
    return np.where((sel >= 0)[:, :, None], out, F32(0))


def backward32(x, sel, p, G, cot, eps=EPS):
    mean, rstd = group_stats(x, G, eps)
    Cin = x.shape[1]
    xh = _xhat(gather(x, sel), sel, mean, rstd, G, F32).reshape(-1, Cin)
    d = np.where((sel >= 0)[:, :, None], cot, F32(0)).reshape(-1, cot.shape[2]).astype(F32)
    R, Cout = d.shape
    rps = rows_per_split(R)
    S, s = np.zeros((Cout, Cin), F32), np.zeros(Cout, F32)
    for r0 in range(0, R, rps):
        Sp, sp = np.zeros((Cout, Cin), F32), np.zeros(Cout, F32)
        for r in range(r0, min(R, r0 + rps)):
            Sp = _fma(d[r][:, None], xh[r][None, :], Sp)
            sp = (sp + d[r]).astype(F32)
        S, s = (S + Sp).astype(F32), (s + sp).astype(F32)
    W = p["weight"].astype(F64)
    dW = _fma(p["gamma"][None], S, (p["beta"][None] * s[:, None]).astype(F32))
    return {"dW": dW, "dbias": s, "dgamma": (W * S.astype(F64)).sum(axis=0).astype(F32),
            "dbeta": (W * s.astype(F64)[:, None]).sum(axis=0).astype(F32)}


def distance(got, want):
    """the unit of profiles/image_fusion/tolerance.json: max|x - record| / max|record|"""
    want = np.asarray(want, F64)
    return float(np.max(np.abs(np.asarray(got, F64) - want)) / max(float(np.max(np.abs(want))), 1e-300))
