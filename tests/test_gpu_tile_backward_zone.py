"""The tile backward's position limits and transmittance recurrence (unipre3d_amd/csrc/u3d_render.hip, tile_backward) on scenes built around
WHERE in a tile's walk its pixels stop:

  * a pixel that stopped early, or lies outside the image, contributes exactly nothing from its stop position on, and the recurrence
    returns from T_final ~ 1e-4 to 1 through alpha = 0.95 .. 0.99;
  * the per-pixel limit test `pos < lim` is a no-op in front of the tile's EARLIEST stop position and decides behind it: the scenes put
    that position in the middle of a walk, in the second of three staging batches, at 0 (partial tiles) and nowhere (no pixel stops).

The walk that ships is one loop that carries T and tests the limit at every entry.  The scenes are also the boundaries that the two forms
measured in round 7 and not kept would meet (EXPERIMENTS.md: T carried as its reciprocal, where only the limit keeps an outside pixel out
of the sums; the entries in front of the earliest stop position as a loop of their own).

Every case is one item and one view through the single- and the two-pass fused step (test_gpu_tile_backward_forms.check_fused).  Bar:
d(head_out) within TOL = 1e-4 (relative L2) of the fp64 arbiter -- the FIRST line of tests/arbiter.py's rule, asserted directly -- with the
precondition that the fp32 restatement of the oracle itself sits within 0.3 x TOL of it; loss and image as in check_fused.  Each case
also asserts, from an fp32 re-walk of the oracle's own tile lists (checked against the oracle's n_contrib), that the scene is what it
claims."""
import numpy as np
import pytest
import torch

import test_gpu_tile_backward_forms as forms
from arbiter import oracle_view
from gradient_rows import fused_step, place

pytestmark = pytest.mark.gpu

NO_STOP = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------------
# what the oracle says about one tile's walk

def tile_walk(oracle_mod, b, tx, ty, bi=0, v=0, r=None):
    """Tile (tx, ty) of view (bi, v) of batch `b` (or of its fp32 oracle render `r`, which then stays open), from the oracle's state: per
    pixel of the tile that lies inside the image the sorted position (1-based, in the VIEW's depth order, which is what the kernels stage
    in batches of 64) at which it stopped -- NO_STOP if it never did -- the view positions of the entries the tile walks (up to the last one that contributed to any pixel), and final_T."""
    from unipre3d_amd import synthetic
    H, W = b.gt.shape[-2:]
    own = r is None
    if own:
        with torch.no_grad():
            g = synthetic.gaussians_from_batch(b)
        r = oracle_view(oracle_mod, g, b, bi, v, H, W, np.float32)
    f = np.float32
    depths, radii, m2, co = r.depths, r.radii, r.means2D.astype(f), r.conic_opacity.astype(f)
    vis = np.flatnonzero(radii > 0)
    order = vis[np.lexsort((vis, depths[vis]))]            # depth key, index ties
    viewpos = np.zeros(radii.shape[0], dtype=np.int64)
    viewpos[order] = np.arange(1, order.size + 1)
    gx = (W + 15) // 16
    r0, r1 = (int(x) for x in r.ranges[ty * gx + tx])
    pl = r.point_list[r0:r1].astype(np.int64)
    ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
    T = np.ones(ys.shape, dtype=f)
    stop = np.full(ys.shape, NO_STOP, dtype=np.int64)
    last = np.zeros(ys.shape, dtype=np.int64)
    alive = np.ones(ys.shape, dtype=bool)
    for k, gi in enumerate(pl):
        dx, dy = m2[gi, 0] - xs.astype(f), m2[gi, 1] - ys.astype(f)
        power = f(-0.5) * (co[gi, 0] * dx * dx + co[gi, 2] * dy * dy) - co[gi, 1] * dx * dy
        alpha = np.minimum(f(0.99), co[gi, 3] * np.exp(power, dtype=f))
        take = alive & (power <= 0) & (alpha >= f(1.0) / f(255.0))
        test = T * (f(1) - alpha)
        stops = take & (test < f(0.0001))
        stop[stops] = viewpos[gi]
        alive &= ~stops
        take &= ~stops
        T[take] = test[take]
        last[take] = k + 1
    n_contrib = r.n_contrib[ys, xs].astype(np.int64)
    final_T = r.final_T.copy()
    if own:
        r.close()
    assert np.array_equal(last, n_contrib), "the re-walk does not reproduce the oracle's n_contrib: it says nothing about this scene"
    assert np.all(viewpos[pl] > 0) and np.all(np.diff(viewpos[pl]) > 0), "a tile's list is a subsequence of the view's order"
    return dict(stop=stop, walked=viewpos[pl[:int(last.max())]], final_T=final_T, n_visible=int(order.size))


def zone(w):
    """(entries of the walk in front of the tile's earliest stop position, entries of the walk, that position)."""
    lmin = int(w["stop"].min())
    return int((w["walked"] < lmin).sum()), int(w["walked"].size), lmin


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes

def _stack(b, first, n, cx, cy, z0, logit, seed, raw_scale=-0.5, spread=5.0):
    """n Gaussians one behind the other around pixel (cx, cy), depths z0 + 0.05 i, peak alpha sigmoid(logit)."""
    g = torch.Generator().manual_seed(seed)
    off = (torch.rand(n, 2, generator=g) - 0.5) * spread
    for i in range(n):
        place(b, first + i, cx + float(off[i, 0]), cy + float(off[i, 1]), z0 + 0.05 * i)
    b.raw[0, 4:7, first:first + n] = raw_scale + 0.1 * b.raw[0, 4:7, first:first + n]
    b.raw[0, 3, first:first + n] = logit


def _faint(b, idx, z_lo, z_hi, seed, box):
    """Gaussians `idx` at opacity sigmoid(-3) = 0.047, centres drawn over the pixel box (x0, x1, y0, y1), depths spread over [z_lo, z_hi]."""
    g = torch.Generator().manual_seed(seed)
    idx = list(idx)
    u = torch.rand(len(idx), 2, generator=g)
    for n, i in enumerate(idx):
        place(b, i, box[0] + float(u[n, 0]) * (box[1] - box[0]), box[2] + float(u[n, 1]) * (box[3] - box[2]),
              z_lo + (z_hi - z_lo) * (n + 0.5) / len(idx))
    b.raw[0, 3, idx] = -3.0


def staggered_scene(seed=5):
    """(a) 32 x 32, tile (0, 0): an opaque stack (8 Gaussians of the smallest scale the head produces, peak alpha 0.95) over the tile's left
    half between 3 faint splats in front of it and 3 behind it over the right half: the left pixels stop inside the stack, the right ones
    walk all 14 entries."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 14, 1, 32, 32, level="object", seed=seed)
    _faint(b, range(0, 3), 1.40, 1.48, seed + 1, (10.0, 14.0, 4.0, 12.0))
    _stack(b, 3, 8, 3.5, 7.5, 1.55, 3.0, seed + 2, raw_scale=-1.0, spread=3.0)
    _faint(b, range(11, 14), 2.05, 2.15, seed + 3, (10.0, 14.0, 4.0, 12.0))
    b.bg = torch.tensor((0.2, 0.5, 0.8), dtype=torch.float32)
    return b


N_FRONT, N_STACK, N_BEHIND = 70, 8, 56


def batches_scene(seed=5):
    """(b) 32 x 32: 70 faint Gaussians in front of an opaque stack over the image centre, 56 more behind it -- 134 sorted positions, three
    staging batches.  The pixels near the centre stop inside the stack, at positions 71 .. 78 (second batch); the others walk on to the
    third batch, whose rows (like the second's) leave through f64 atomics."""
    from unipre3d_amd import synthetic
    P = N_FRONT + N_STACK + N_BEHIND
    b = synthetic.make_batch(1, P, 1, 32, 32, level="object", seed=seed)
    _faint(b, range(0, N_FRONT), 1.20, 1.45, seed + 1, (0.0, 31.0, 0.0, 31.0))
    _stack(b, N_FRONT, N_STACK, 15.5, 15.5, 1.50, 3.0, seed + 2)
    _faint(b, range(N_FRONT + N_STACK, P), 2.00, 2.30, seed + 3, (0.0, 31.0, 0.0, 31.0))
    return b


def partial_scene(seed=5):
    """(c) 12 x 23 (partial tiles, W % 4 != 0): the opaque stack over the seam between the two tiles."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 8, 1, 12, 23, level="object", seed=seed)
    _stack(b, 0, 8, 14.0, 6.0, 1.50, 3.0, seed + 2)
    b.bg = torch.tensor((0.2, 0.5, 0.8), dtype=torch.float32)
    return b


def no_stop_scene():
    """(d) the 130 faint Gaussians of the forms tests on a single tile."""
    return forms.long_scene(H=16, W=16)


def deep_scene(logit):
    """(e) the forms tests' opaque stack, twelve deep: T_final down to ~1e-4 behind alpha = 0.95 (PLAIN loops) / 0.99 (general loops)."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 12, 1, 32, 32, level="object", seed=7)
    _stack(b, 0, 12, 15.5, 15.5, 1.50, logit, 8)
    b.bg = torch.tensor((0.2, 0.5, 0.8), dtype=torch.float32)
    return b


def many_scene(seed=5):
    """(f) P = 300 > 256 on 32 x 32: the instantiation with two partial-row blocks (the scene-level form of the tile kernels); 292 faint
    Gaussians around an opaque stack at positions 101 .. 108."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 300, 1, 32, 32, level="object", seed=seed)
    _faint(b, range(0, 100), 1.20, 1.45, seed + 1, (0.0, 31.0, 0.0, 31.0))
    _stack(b, 100, 8, 15.5, 15.5, 1.50, 3.0, seed + 2)
    _faint(b, range(108, 300), 2.00, 2.40, seed + 3, (0.0, 31.0, 0.0, 31.0))
    return b


SCENES = dict(staggered=staggered_scene, batches=batches_scene, partial=partial_scene, no_stop=no_stop_scene,
              deep_plain=lambda: deep_scene(3.0), deep_general=lambda: deep_scene(6.0), many=many_scene)


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenes are what they claim (shared with the CPU pre-check of the seeds)

def claim_staggered(oracle_mod, b):
    w = tile_walk(oracle_mod, b, 0, 0)
    front, total, lmin = zone(w)
    assert total == 14 and 2 <= lmin <= 11 and 0 < front < total, (front, total, lmin)
    assert (w["stop"] == NO_STOP).sum() >= 32 and (w["stop"] != NO_STOP).sum() >= 32, "both halves of the tile are populated"


def claim_batches(oracle_mod, b):
    for tx, ty in ((0, 0), (1, 0), (0, 1), (1, 1)):       # the stack sits on the corner the four tiles share
        w = tile_walk(oracle_mod, b, tx, ty)
        front, total, lmin = zone(w)
        assert w["n_visible"] == N_FRONT + N_STACK + N_BEHIND
        assert 64 < lmin <= N_FRONT + N_STACK, (tx, ty, lmin)
        assert front >= 64 and w["walked"].max() > 128, (tx, ty, front, total)
        assert (w["walked"] <= 64).sum() >= 60, "batch 0 is (almost) full and lies entirely in front of the earliest stop"


def claim_partial(oracle_mod, b):
    H, W = b.gt.shape[-2:]
    assert H % 16 and W % 16 and W % 4
    for tx in (0, 1):
        w = tile_walk(oracle_mod, b, tx, 0)
        assert (w["stop"] != NO_STOP).any() and (w["stop"] == NO_STOP).any(), tx
        assert w["final_T"].min() < 1e-3, tx


def claim_no_stop(oracle_mod, b):
    w = tile_walk(oracle_mod, b, 0, 0)
    assert (w["stop"] == NO_STOP).all() and w["walked"].size > 128, w["walked"].size


def claim_deep(oracle_mod, b):
    w = tile_walk(oracle_mod, b, 0, 0)
    front, total, lmin = zone(w)
    assert w["final_T"].min() < 1e-3 and (w["final_T"] < 1e-2).mean() > 0.05, w["final_T"].min()
    assert 2 <= lmin < total and total >= 10, (lmin, total)     # (the stack is alone in the view: position = index in the walk)


def claim_many(oracle_mod, b):
    assert b.raw.shape[2] > 256
    w = tile_walk(oracle_mod, b, 0, 0)
    front, total, lmin = zone(w)
    assert w["n_visible"] > 256 and 100 < lmin <= 108 and w["walked"].max() > 128, (w["n_visible"], lmin, total)


CLAIMS = dict(staggered=claim_staggered, batches=claim_batches, partial=claim_partial, no_stop=claim_no_stop, deep_plain=claim_deep,
              deep_general=claim_deep, many=claim_many)


@pytest.mark.parametrize("case", sorted(SCENES))
def test_zone(oracle_mod, case):
    b = SCENES[case]()
    CLAIMS[case](oracle_mod, b)
    forms.check_fused(oracle_mod, b, f"zone {case}")


def test_zone_steps_are_deterministic():
    """the single-pass fused step of every scene twice: loss and gradient equal bit for bit.  (Three of the scenes have more than 128
    Gaussians, i.e. three or more 64-Gaussian blocks of the projection's backward: their across-point quaternion sums meet in f64 atomics,
    where a sum of fp32-valued terms is exact in any order; as fp32 atomics they differed from step to step by ~2e-6 in the rotation channels.)"""
    for case in sorted(SCENES):
        bd = SCENES[case]().to(torch.device("cuda:0"))
        one, two = fused_step(bd, True), fused_step(bd, True)
        assert torch.equal(one[0], two[0]) and torch.equal(one[2], two[2]), case
        assert one[2].abs().max().item() > 0 and bool(torch.isfinite(one[2]).all()), case
