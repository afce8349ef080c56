"""Row and channel-group comparison of head-level (and operator-level) gradients, with the seeded scenes its tests share (TEST
INFRASTRUCTURE, beside tests/arbiter.py).

`arbiter.assert_parity` measures ONE relative L2 norm over a whole gradient tensor.  At head level that tensor holds all 23 head channels
of all Gaussians, 3/4 of its norm is features_rest and 3e-3 of it is the rotation group: an error confined to one channel group or to one
Gaussian stays far below the 1e-4 bar (tests/test_gradient_rows.py plants four and shows it).  `assert_group_rows` applies the SAME rule
with the SAME constants per channel group, and per Gaussian inside every group:

  group:  arbiter._rule (TOL, GAP_K, GAP_CEIL, RESTATEMENT_CEIL) on the group's relative L2;
  rows:   e_i = ||x_i - o64_i|| / max_j ||o64_j|| over the group's channels (the group's own largest row is the scale), y_i the same
          figure of the fp32 restatement;  pass <=> max e_i <= TOL, or max e_i <= GAP_K * max y_i and <= GAP_CEIL * TOL (such a pass is
          appended to arbiter.GAP_PASSES and shows in the session summary);
  zeros:  a row that is exactly zero in both restatements is exactly zero in the result.

Every oracle-backed case first asserts `assert_yardstick`: the fp32 restatement's own group figure and worst row figure are <= 0.3 x TOL
for every group, so that the first line of either rule is a statement about the kernel and not about what fp32 resolves on the draw.  The
seeds below were chosen on the CPU for that (tests/test_gradient_rows.py re-checks every case without a GPU).

U3D_GRADIENT_ROWS_OUT=<file>: the GPU tests write every measured figure there (profiles/gradient_rows/figures.json)."""
import dataclasses
import math

import numpy as np
import torch

import arbiter
from arbiter import GAP_CEIL, GAP_K, TOL, head_grad_arbiter, one_tile_per_thread, oracle_view, parity_errors

HEAD_GROUPS = (("xyz", slice(0, 3)), ("opacity", slice(3, 4)), ("scaling", slice(4, 7)), ("rotation", slice(7, 11)),
               ("dc", slice(11, 14)), ("rest", slice(14, None)))
YARDSTICK_MAX = 0.3 * TOL
FIGURES = []         # one record per assert_group_rows call of the GPU tests (written out by their module fixture)


def _named(groups):
    if groups is None:
        return list(HEAD_GROUPS)
    return [(g if isinstance(g, tuple) else (f"{g.start}:{g.stop}", g)) for g in groups]


def _row_norms(a):
    return np.sqrt((a * a).sum(axis=0))


def group_row_figures(x, o32, o64, groups=None):
    """Per group: relative L2 of x from o64 / from o32, of o32 from o64, the worst row figure of x and of o32 (against the group's largest
    o64 row), where they sit, and the rows that are non-zero in x although both restatements are exactly zero there."""
    x, o32, o64 = (np.asarray(a, dtype=np.float64) for a in (x, o32, o64))
    assert x.shape == o32.shape == o64.shape and x.ndim == 2, (x.shape, o32.shape, o64.shape)
    out = {}
    for name, sl in _named(groups):
        gx, g32, g64 = x[sl], o32[sl], o64[sl]
        zero_rows = ~(np.any(g32 != 0, axis=0) | np.any(g64 != 0, axis=0))
        stray = np.flatnonzero(zero_rows & np.any(gx != 0, axis=0))
        fig = {"zero_rows": int(zero_rows.sum()), "stray_rows": [int(i) for i in stray[:8]]}
        if zero_rows.all():
            fig.update(all_zero=True, e64=0.0, e32=0.0, gap=0.0, row_e=0.0, row_y=0.0, row_at=-1, row_y_at=-1)
        else:
            e64, e32, gap = parity_errors(gx, g32, g64)
            scale = max(float(_row_norms(g64).max()), 1e-30)
            e, y = _row_norms(gx - g64) / scale, _row_norms(g32 - g64) / scale
            fig.update(all_zero=False, e64=e64, e32=e32, gap=gap, row_e=float(e.max()), row_y=float(y.max()), row_at=int(e.argmax()),
                       row_y_at=int(y.argmax()))
        out[name] = fig
    return out


def assert_group_rows(x, o32, o64, groups=None, what=""):
    """x: the HIP result, o32 / o64: the CPU restatement in fp32 / fp64, all (C, P); groups: channel slices or (name, slice) pairs, the
    six head groups by default.  Prints every figure, then asserts the group rule, the row rule and the exact zeros; returns the figures."""
    figs = group_row_figures(x, o32, o64, groups)
    bad, leaning = [], []     # (passes through a gap branch are logged only when the whole comparison passes)
    for name, f in figs.items():
        tag = f"{what} [{name}]"
        print(f"[rows] {tag}: group |x-f64| {f['e64']:.2e} |x-f32| {f['e32']:.2e} |f32-f64| {f['gap']:.2e}; worst row {f['row_e']:.2e} "
              f"(Gaussian {f['row_at']}), restatement's worst row {f['row_y']:.2e} (Gaussian {f['row_y_at']}); {f['zero_rows']} zero rows")
        if f["stray_rows"]:
            bad.append(f"{tag}: rows {f['stray_rows']} are exactly zero in both restatements and not in the result")
        if f["all_zero"]:
            continue
        if not arbiter._rule(f["e64"], f["e32"], f["gap"], TOL, GAP_K):
            bad.append(f"{tag}: group |x-f64| {f['e64']:.2e}, |x-f32| {f['e32']:.2e}, restatement's own {f['gap']:.2e} (bar {TOL:.0e})")
        elif f["e64"] > TOL:
            leaning.append((tag + (" [= fp32 restatement]" if f["e32"] <= TOL else " [capped gap]"), f["e64"], f["gap"]))
        if f["row_e"] > TOL:
            if f["row_e"] <= GAP_K * f["row_y"] and f["row_e"] <= GAP_CEIL * TOL:
                leaning.append((tag + f" [row {f['row_at']}, capped gap]", f["row_e"], f["row_y"]))
            else:
                bad.append(f"{tag}: row {f['row_at']} is {f['row_e']:.2e} of the group's largest row from the fp64 arbiter, the fp32 "
                           f"restatement's worst row {f['row_y']:.2e} (bar {TOL:.0e}, or {GAP_K:g} x that under {GAP_CEIL * TOL:.0e})")
    assert not bad, "\n".join(bad)
    arbiter.GAP_PASSES.extend(leaning)
    return figs


def assert_yardstick(o32, o64, groups=None, what=""):
    """The precondition of every oracle-backed case: the fp32 restatement itself sits within 0.3 x TOL of the fp64 arbiter in every
    group and in every row, and the arbiter is not all-zero."""
    figs = group_row_figures(o32, o32, o64, groups)
    assert np.any(np.asarray(o64) != 0), f"{what}: the arbiter is all-zero"
    bad = [f"{what} [{n}]: group {f['gap']:.2e}, worst row {f['row_y']:.2e} (Gaussian {f['row_y_at']})" for n, f in figs.items()
           if f["gap"] > YARDSTICK_MAX or f["row_y"] > YARDSTICK_MAX]
    assert not bad, "the scene is no yardstick (fp32 restatement's own distance, bar %.0e):\n" % YARDSTICK_MAX + "\n".join(bad)
    return figs


def record(case, figs, **extra):
    FIGURES.append(dict(case=case, groups={n: {k: v for k, v in f.items() if k != "stray_rows"} for n, f in figs.items()}, **extra))


def stack_operator(grads, P):
    """Operator-level gradients (dict over scenes.DIFF_KEYS, (P, ...) each) as one (C, P) array, with one group per key."""
    from scenes import DIFF_KEYS
    rows, groups, c = [], [], 0
    for k in DIFF_KEYS:
        a = np.asarray(grads[k], dtype=np.float64).reshape(P, -1).T
        rows.append(a)
        groups.append((k, slice(c, c + a.shape[0])))
        c += a.shape[0]
    return np.concatenate(rows), groups


def operator_pair(oracle_mod, sc, dcol, dinv):
    """Operator-level gradients of one tests/scenes.py scene for the cotangents (dcol, dinv) in fp32 and fp64 (the arbiter under the fp32
    run's discrete decisions), stacked by `stack_operator`: (o32, o64, groups)."""
    from scenes import to_numpy
    P = sc["means3D"].shape[0]
    r32 = oracle_mod.forward(dtype=np.float32, **to_numpy(sc))
    r64 = oracle_mod.forward(dtype=np.float64, discrete_from="fp32", **to_numpy(sc))
    H, W = sc["image_height"], sc["image_width"]
    with one_tile_per_thread(oracle_mod, H, W):
        g32 = oracle_mod.backward(r32, dcol.numpy(), dinv.numpy())
    g64 = oracle_mod.backward(r64, dcol.numpy().astype(np.float64), dinv.numpy().astype(np.float64))
    r32.close(); r64.close()
    o32, groups = stack_operator(g32, P)
    o64, _ = stack_operator(g64, P)
    return o32, o64, groups


# ---------------------------------------------------------------------------------------------------------------------------------
# one fused step, and a Gaussian put where a view sees it (shared with tests/test_gpu_tile_backward_forms.py)

def place(b, i, px, py, z, view=0):
    """Put Gaussian i of item 0 where view (0, `view`) projects it to pixel coordinates (px, py) (integers are pixel centres) at view depth z:
    the head's offset channels are zeroed (tanh(0) = 0), so the position is the centre."""
    H, W = b.gt.shape[-2:]
    t = math.tan(b.fov_deg * math.pi / 360)
    pv = torch.tensor([((2 * px + 1) / W - 1) * t * z, ((2 * py + 1) / H - 1) * t * z, z, 1.0], dtype=torch.float64)
    pw = pv @ torch.linalg.inv(b.world_view[0, view].double())
    b.raw[0, 0:3, i] = 0.0
    b.center[0, i] = pw[:3].float()


def fused_step(bd, single_pass=True, isotropic=False):
    from unipre3d_amd import fused
    H, W = bd.gt.shape[-2:]
    h = bd.raw.permute(0, 2, 1).contiguous().requires_grad_(True)
    loss, img, _ = fused.render_loss_fused(h, bd.center, bd.world_view, bd.full_proj, bd.camera_center, bd.gt, bd.bg, bd.fov_deg, H, W,
                                           level=bd.level, offset_scale=bd.offset_scale, loss_kind="l2", single_pass=single_pass,
                                           isotropic=isotropic)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), img.detach(), h.grad.detach()


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements of one item's views (computed once per case and shared)

_PAIRS = {}


def view_pairs(oracle_mod, b, key, isotropic=False):
    """[(d loss / d raw of view v alone in fp32, in fp64)] for every view of the one-item batch `b`, each (C, P), under the l2 loss
    normalised to all V views; cached under `key`.  The fp32 restatement runs with one oracle thread per tile, so that its summation
    order -- and with it the yardstick -- is the same on every host."""
    if key not in _PAIRS:
        H, W = b.gt.shape[-2:]
        V = b.world_view.shape[1]
        out = []
        for v in range(V):
            with one_tile_per_thread(oracle_mod, H, W):
                a32 = head_grad_arbiter(oracle_mod, b, 0, v, H, W, V, "l2", np.float32, isotropic=isotropic)[0]
            a64 = head_grad_arbiter(oracle_mod, b, 0, v, H, W, V, "l2", np.float64, isotropic=isotropic)[0]
            out.append((a32, a64))
        _PAIRS[key] = out
    return _PAIRS[key]


def summed_pair(pairs):
    return sum(p[0] for p in pairs), sum(p[1] for p in pairs)


def visible_views(oracle_mod, b, i):
    """[view v renders Gaussian i of item 0 (non-zero radius in the fp32 oracle)]."""
    from unipre3d_amd import synthetic
    H, W = b.gt.shape[-2:]
    with torch.no_grad():
        g = synthetic.gaussians_from_batch(b)
    out = []
    for v in range(b.world_view.shape[1]):
        r = oracle_view(oracle_mod, g, b, 0, v, H, W, np.float32)
        out.append(bool(r.radii[i] > 0))
        r.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes.  Every one has raw[:, 3] -= 3 (opacity about 0.05): no pixel saturates, so every visible row carries gradient.

def faint_batch(level, P, V, H, W, seed):
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, P, V, H, W, level=level, seed=seed)
    b.raw[:, 3] -= 3.0
    return b


# (a) the quaternion-norm routes: P <= 256 in-block norms of the forward projection, 257 the norm kernel with five backward blocks feeding
# qdot, 1100 the 1024-thread norm kernel's second trip
ROUTE_P = (64, 256, 257, 1100)
ROUTE_SEED = {}


def route_scene(level, P):
    return faint_batch(level, P, 1, 48, 48, ROUTE_SEED.get((level, P), 11))


# (b) view counts around the backward's four view slots per Gaussian (vslot = lane & 3, vk += 4); P = 70 is two backward blocks, the
# second with six Gaussians
VIEW_COUNTS = (1, 3, 4, 5, 8, 9)
# (scene level, seed 11: one xyz row of the fp32 restatement sits 2e-5 .. 4e-5 from the arbiter at V >= 3, and so does a scaling row of
# the object-level V = 9 scene when view 8 stands alone; these stay under 1e-5)
VIEW_SEED = {("object", 9): 12, ("scene", 3): 13, ("scene", 4): 13, ("scene", 5): 12, ("scene", 8): 12, ("scene", 9): 13}
ISOLATED_VIEWS = (0, 3, 4, 8)


def view_scene(level, V):
    return faint_batch(level, 70, V, 32, 32, VIEW_SEED.get((level, V), 11))


# (c) one Gaussian per branch
BRANCH = dict(scale_below=0, scale_at_clamp=1, scale_one_axis=2, dc_one=3, dc_two=4, dc_three=5, behind=6, far_mean=7, quat_eps=8,
              quat_small=9)
BRANCH_SEED = {"object": 11, "scene": 11}
_BRANCH_PIXELS = ((5, 5), (13, 5), (21, 5), (27, 6), (5, 13), (13, 13), (21, 13), (27, 14), (5, 22), (13, 22), (21, 22), (27, 24))


def branch_scene(level):
    """12 Gaussians placed over view (0, 0) of a 32 x 32 image, the first ten each on one branch of the activations' backward (indices in
    BRANCH; quat_eps / quat_small are ordinary at object level, where the quaternion norm runs across points)."""
    b = faint_batch(level, 12, 1, 32, 32, BRANCH_SEED[level])
    for i, (px, py) in enumerate(_BRANCH_PIXELS):
        place(b, i, px + 0.3, py - 0.2, 1.5 + 0.04 * i)
    r = b.raw[0]
    r[4:7, BRANCH["scale_below"]] = -1.5                                 # clamp(x, -1, 20) active on all axes: no scaling gradient
    r[4:7, BRANCH["scale_at_clamp"]] = -1.0                              # exactly on the bound: torch's clamp mask is inclusive
    r[4:7, BRANCH["scale_one_axis"]] = torch.tensor([0.2, -1.5, -0.3])   # only axis 1 clamped
    for k, n in ((BRANCH["dc_one"], 1), (BRANCH["dc_two"], 2), (BRANCH["dc_three"], 3)):
        r[14:23, k] *= 0.2                                               # (small view-dependent part: the dc term decides the clamp)
        r[11:14, k] = 1.0
        r[11:11 + n, k] = -20.0                                          # 0.5 + C0 dc + ... < 0: colour channels 0 .. n-1 are clamped to 0
    place(b, BRANCH["behind"], 16.0, 16.0, 0.1)                          # view depth <= 0.2: culled
    place(b, BRANCH["far_mean"], 15.5 + 450.0, 11.0, 1.6)                # mean far outside the frustum, splat of several hundred pixels
    r[4:7, BRANCH["far_mean"]] = torch.tensor([3.5, 3.0, 3.3])          # (anisotropic: its orientation matters)
    r[3, BRANCH["far_mean"]] = 2.0
    if level == "scene":
        for k, n in ((BRANCH["quat_eps"], 1e-8), (BRANCH["quat_small"], 1e-4)):   # below F.normalize's eps = 1e-6 (g / eps), and above
            q = r[7:11, k].double()
            r[7:11, k] = (q / q.norm() * n).float()
    return b


TWO_VIEW_GAUSSIAN = 3


def two_view_scene(level):
    """V = 5, 12 Gaussians, 32 x 32: Gaussian 3 lies 2.5 behind the point the cameras look at, seen from views 0 and 4 (which stand on the
    other side of that point), and behind the cameras of views 1, 2, 3 -- the backward's view slot 0 meets it on its first AND its second
    trip, the other slots never."""
    from unipre3d_amd import cameras
    b = faint_batch(level, 12, 5, 32, 32, 11)
    if level == "object":
        target, zn, zf = np.zeros(3), cameras.OBJECT_ZNEAR, cameras.OBJECT_ZFAR
    else:
        target, zn, zf = np.array([3.0, 2.5, 1.5]), cameras.SCENE_ZNEAR, cameras.SCENE_ZFAR
    fov = math.radians(b.fov_deg)
    proj = cameras.projection_matrix(zn, zf, fov, fov)
    az0 = 0.7
    dirv = lambda az, el: np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    rad = math.radians
    # (azimuth, elevation) of the eye as seen from the target: views 0 and 4 on the side of dirv(az0, 0), views 1..3 opposite
    eyes = [(az0 + rad(10), rad(4)), (az0 + math.pi - rad(25), rad(-6)), (az0 + math.pi, rad(8)), (az0 + math.pi + rad(20), rad(3)),
            (az0 - rad(12), rad(-5))]
    for v, (az, el) in enumerate(eyes):
        R, t = cameras.look_at_R_t(target + cameras.OBJECT_CAMERA_DISTANCE * dirv(az, el), target)
        b.world_view[0, v], b.full_proj[0, v], b.camera_center[0, v] = cameras.assemble_camera(R, t, proj)
    i = TWO_VIEW_GAUSSIAN
    b.raw[0, 0:3, i] = 0.0
    b.raw[0, 4:7, i] = 0.0
    b.center[0, i] = torch.tensor(target - 2.5 * dirv(az0, 0.0), dtype=torch.float32)
    return b


def isotropic_scene():
    return faint_batch("object", 70, 3, 32, 32, 11)


def isolate_view(b, images, v):
    """Copy of the one-item batch whose targets are the rendered `images` (V, 3, H, W) in every view but v: under the l2 loss the other
    views then hand back exact zeros and the step's gradient is view v's alone."""
    gt = images.detach().cpu().reshape(b.gt.shape).clone()
    gt[0, v] = b.gt[0, v]
    return dataclasses.replace(b, gt=gt)
