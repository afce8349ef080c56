"""Plain fp64 references and index-set builders for the scatter-add gradients of the point operators (u3d_group_points_grad,
u3d_three_interpolate_grad).  No GPU, no oracle library: numpy only.

References: a cloud's gradient is `grad_out (C x total) @ S (total x n)` with S one-hot (grouping) or weight-valued (interpolation), in fp64.
Columns of S that no index names are all zero and are skipped (the result is scattered into zeros), so a cloud of 16385 destinations of which
48 are used costs 48 columns.  For integer cotangents and weights that are multiples of 1/8 every product and partial sum is exactly representable:
the fp64 result is THE result, in any summation order.

Index sets: the grouping kernel walks a cloud's `total` entries in steps of 256, four waves of 64 lanes per step, and merges runs of equal
consecutive destinations inside a wave (16-lane DPP rows, then two row broadcasts).  `layout` places runs, `wave_view` reports what every wave
of every step sees, so a test can assert WHERE the runs of a set fall before it trusts the set."""
import numpy as np

STEP, WAVE, ROW = 256, 64, 16


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def group_grad_fp64(go, idx, n, with_mag=True):
    """go (B, C, ...) cotangents, idx (B, ...) destinations (the trailing shapes flatten to `total`) ->
    (grad (B, C, n) fp64, count (B, 1, n) terms per element, mag (B, C, n) sum of |terms|; None if not with_mag)."""
    go = np.asarray(go); B, C = go.shape[:2]
    g = go.reshape(B, C, -1).astype(np.float64)
    ix = np.asarray(idx).reshape(B, -1).astype(np.int64)
    assert ix.shape[1] == g.shape[2] and (ix.size == 0 or (ix.min() >= 0 and ix.max() < n))
    grad, mag, cnt = np.zeros((B, C, n)), np.zeros((B, C, n)) if with_mag else None, np.zeros((B, 1, n))
    for b in range(B):
        cols, inv = np.unique(ix[b], return_inverse=True)
        S = np.zeros((ix.shape[1], len(cols)))
        S[np.arange(ix.shape[1]), inv.reshape(-1)] = 1.0
        grad[b][:, cols] = g[b] @ S
        if with_mag:
            mag[b][:, cols] = np.abs(g[b]) @ S
        cnt[b, 0, cols] = S.sum(0)
    return grad, cnt, mag


def interp_grad_fp64(go, idx, w, m, with_mag=True):
    """go (B, C, n) cotangents, idx / w (B, n, 3) -> (grad (B, C, m) fp64, count (B, 1, m), mag (B, C, m) sum of |g| |w|).
    A point that names one destination twice contributes two terms to it."""
    go = np.asarray(go); B, C, n = go.shape
    g = go.astype(np.float64)
    ix = np.asarray(idx).astype(np.int64); wt = np.asarray(w).astype(np.float64)
    assert ix.shape == (B, n, 3) and wt.shape == (B, n, 3) and (ix.size == 0 or (ix.min() >= 0 and ix.max() < m))
    grad, mag, cnt = np.zeros((B, C, m)), np.zeros((B, C, m)) if with_mag else None, np.zeros((B, 1, m))
    rows = np.repeat(np.arange(n), 3)
    for b in range(B):
        cols, inv = np.unique(ix[b], return_inverse=True)
        inv = inv.reshape(-1)
        S, A, N1 = (np.zeros((n, len(cols))) for _ in range(3))
        np.add.at(S, (rows, inv), wt[b].reshape(-1))
        np.add.at(A, (rows, inv), np.abs(wt[b]).reshape(-1))
        np.add.at(N1, (rows, inv), 1.0)
        grad[b][:, cols] = g[b] @ S
        if with_mag:
            mag[b][:, cols] = np.abs(g[b]) @ A
        cnt[b, 0, cols] = N1.sum(0)
    return grad, cnt, mag


# ---- run-structured index sets (grouping) ---------------------------------------------------------------------------------------------------
def layout(runs):
    """[(destination, run length), ...] laid out consecutively -> int32 (total,)."""
    return np.concatenate([np.full(l, d, np.int32) for d, l in runs]) if runs else np.zeros(0, np.int32)


def runs_of(idx):
    """maximal runs of equal consecutive destinations of a 1-D index set: [(first position, length, destination), ...]"""
    idx = np.asarray(idx).reshape(-1)
    if idx.size == 0:
        return []
    starts = np.concatenate([[0], np.nonzero(idx[1:] != idx[:-1])[0] + 1, [idx.size]])
    return [(int(s), int(e - s), int(idx[s])) for s, e in zip(starts[:-1], starts[1:])]


def wave_view(idx):
    """What each of the four waves sees in every 256-entry step: a list of dicts
    {step, wave, active (lanes with an entry), segs [(first lane, last lane, destination), ...] (the wave's runs among its active lanes),
     scan (False: no adjacent duplicates -- the wave skips the segmented scan)}."""
    idx = np.asarray(idx).reshape(-1)
    total, out = idx.size, []
    for e0 in range(0, total, STEP):
        for w in range(STEP // WAVE):
            lo = e0 + w * WAVE
            active = max(0, min(WAVE, total - lo))
            segs = [(s, s + l - 1, d) for s, l, d in runs_of(idx[lo:lo + active])]
            out.append(dict(step=e0 // STEP, wave=w, active=active, segs=segs, scan=any(b > a for a, b, _ in segs)))
    return out


class _Filler:
    """runs of length 1 on the destinations 40 .. 47 in turn, continuing where the previous call stopped (neighbours always differ)"""

    def __init__(self):
        self.k = 0

    def __call__(self, count, base=40):
        out = [(base + (self.k + i) % 8, 1) for i in range(count)]
        self.k += count
        return out


N_DEST = 48          # every named set uses destinations 0 .. 47: runs take 0 .. 39 in order of appearance, fillers 40 .. 47


def main_set():
    """The 604-entry structured set.  Positions (step = p // 256, wave = p % 256 // 64, lane = p % 64):
      step 0 wave 0: singles, run of 3 on lanes 14-16 (crosses 15/16), run of 2 on 31-32, run of 15 on 40-54 (crosses 47/48)
             wave 1: singles, run of 16 on lanes 16-31 (exactly one row) meeting a run of 17 on 32-48 at the row boundary
             wave 2: a single, run of 63 on lanes 1-63 (begins before 16, ends after 48, crosses all three row pairs)
             wave 3: singles, then a run of 65 from lane 31 over the STEP boundary to lane 31 of
      step 1 wave 0, followed by a run of 33 from lane 32 over the WAVE boundary to lane 0 of
             wave 1: run of 31 on lanes 1-31, run of 32 on 32-63
             wave 2: run of 64: exactly one wave
             wave 3: 64 singles: no adjacent duplicates, the scan is skipped
      step 2 wave 0: a, b, a, b, ... on lanes 0-31, then a run of 60 that the end of the set cuts short in
             wave 1 at lane 27: the last step is partial and ends inside a run."""
    d, _singles = iter(range(40)), _Filler()
    r = _singles(14, 40) + [(next(d), 3)] + _singles(14, 40) + [(next(d), 2)] + _singles(7, 40) + [(next(d), 15)] + _singles(9, 40)
    r += _singles(16, 40) + [(next(d), 16), (next(d), 17)] + _singles(15, 40)
    r += _singles(1, 40) + [(next(d), 63)]
    r += _singles(31, 40) + [(next(d), 65)]
    r += [(next(d), 33), (next(d), 31), (next(d), 32), (next(d), 64)]
    r += _singles(64, 40)
    a, b = next(d), next(d)
    r += [(a, 1), (b, 1)] * 16 + [(next(d), 60)]
    return layout(r)


def long_set():
    """5 singles, a run of 300 (positions 5 .. 304: three whole waves of step 0, the step boundary, lanes 0-48 of step 1), a run of 2: 307 entries"""
    return layout(_Filler()(5) + [(0, 300), (1, 2)])


def alternating_set(total=130):
    """a, b, a, b, ...: no runs at all, and every lane of a wave collides with 31 others on the compare-and-swap"""
    return layout([(3, 1), (9, 1)] * (total // 2) + [(3, 1)] * (total % 2))


def one_destination_set(total):
    return layout([(5, total)])


TOTALS = (1, 63, 64, 65, 255, 256, 257, 600)


def ball_query_set(n=N_DEST, seed=0):
    """33 groups of K = 32 shaped like ball-query output: group h holds h distinct hits in ascending order, then 32 - h copies of its FIRST hit
    (h = 0: no hit at all, the group is all zeros).  (33, 32) int32."""
    rng = np.random.RandomState(seed)
    out = np.zeros((33, 32), np.int32)
    for h in range(1, 33):
        hits = np.sort(rng.choice(n, h, replace=False))
        out[h, :h] = hits
        out[h, h:] = hits[0]
    return out


def named_sets():
    """name -> 1-D int32 index set over N_DEST destinations"""
    s = {"main": main_set(), "long300": long_set(), "alternating": alternating_set(), "ball_query": ball_query_set().reshape(-1)}
    for t in TOTALS:
        s[f"one_destination_{t}"] = one_destination_set(t)
    for t in (63, 65, 255, 257):
        s[f"main_first_{t}"] = main_set()[:t]
    return s


def overflow_set():
    """Three places where a run of TWO entries is immediately followed by a run of FOUR: inside a row (lanes 5-6 | 7-10), ending on a row
    boundary (lanes 30-31 | 32-35) and straddling one (lanes 47-48 | 49-52).  Four, because the last lane of the following run -- the one
    whose sum reaches memory -- then reads the pair's second lane in the scan's `row_shr:4` step (lane 10 - 4 = 6); across the boundary
    every lane of the next row reads lane 31 in the row broadcast.  Returns (idx (64,), [(first lane of the pair, its destination, the
    following run's destination), ...])."""
    _singles = _Filler()
    r = _singles(5) + [(0, 2), (1, 4)] + _singles(19) + [(2, 2), (3, 4)] + _singles(11) + [(4, 2), (5, 4)] + _singles(11)
    return layout(r), [(5, 0, 1), (30, 2, 3), (47, 4, 5)]


# ---- index sets (interpolation) --------------------------------------------------------------------------------------------------------------
def interp_sets(B, n, m, seed=0):
    """name -> idx (B, n, 3) int32 over m destinations"""
    rng = np.random.RandomState(seed)
    s = {"random": rng.randint(0, m, (B, n, 3)).astype(np.int32)}
    same = rng.randint(0, m, (B, n, 1)).astype(np.int32)
    s["same_triple"] = np.ascontiguousarray(np.repeat(same, 3, axis=2))                 # i0 == i1 == i2
    s["one_destination"] = np.full((B, n, 3), m // 3, np.int32)
    crowd = rng.randint(0, m, (B, n, 3)).astype(np.int32)                               # the (40, 2048, 512) pattern of test_gpu_pointops.py
    crowd[:, ::2, 0] = 7 % m; crowd[:, 1::3, 2] = 7 % m
    s["crowded"] = crowd
    return s
