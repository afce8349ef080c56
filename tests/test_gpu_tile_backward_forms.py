"""The tile backward's arithmetic forms (unipre3d_amd/csrc/u3d_render.hip, tile_backward) on the scenes where each of them could go wrong:

  * the NORMALISED remainder rho_i = R_i / T_{i+1} (seeded with bg . dL/dC, no T_final factor): opaque stacks that take T_final to ~1e-4,
    in the PLAIN loop variant (opacity <= 0.98) and in the general one (opacity above it, alpha clamped to 0.99), background zero and not;
  * the lane-local moments about the centre of a lane's 4-pixel run: a single splat centred on a pixel centre and half-way between two
    pixels (the run straddles the centre, where the moments cancel most), on images with partial tiles and W % 4 != 0, and a splat whose
    centre lies hundreds of pixels outside the image (dx ~ 450, dx^2 ~ 2e5);
  * the cross-lane reduction with the bank-masked levels first: every case, plus the 10-value order of the inverse-depth instantiation
    through the operator path, and sorted positions beyond the first staging batch (the rows that leave through f64 atomics).

Bar: every gradient within TOL = 1e-4 (relative L2) of the fp64 arbiter -- the FIRST line of tests/arbiter.py's rule, asserted directly.  The
scenes are seeded so that the fp32 restatement of the oracle itself sits within 0.3 x TOL of the arbiter (asserted too: it is the
precondition that makes the first line a statement about the kernel and not about what fp32 can resolve on the draw)."""
import math

import numpy as np
import pytest
import torch

from arbiter import TOL, head_grad_arbiter, oracle_view
from conftest import rel_l2
from gradient_rows import fused_step, place
from scenes import cotangents

pytestmark = pytest.mark.gpu

GAP_MAX = 0.3 * TOL


def needle_scene(H, W, cx, cy, seed=11):
    """(a) one Gaussian of the minimum scale the head produces (exp(-1)) centred at pixel coordinates (cx, cy)."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 1, 1, H, W, level="object", seed=seed)
    b.raw[0, 4:7, 0] = -1.0
    b.raw[0, 3, 0] = 1.5
    place(b, 0, cx, cy, 1.75)
    return b


def stack_scene(logit, bgv, seed=5, H=32, W=32):
    """(b) 8 Gaussians one behind the other over the image centre, sigma ~ 12 px, peak alpha sigmoid(logit) (0.99 after the clamp for
    logit = 6): the pixels near the centre saturate after 2-4 entries, those around them end with T_final ~ 1e-4 .. 1e-2."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 8, 1, H, W, level="object", seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    off = (torch.rand(8, 2, generator=g) - 0.5) * 5.0
    for i in range(8):
        place(b, i, 15.5 + float(off[i, 0]), 15.5 + float(off[i, 1]), 1.5 + 0.06 * i)
    b.raw[0, 4:7] = -0.5 + 0.1 * b.raw[0, 4:7]
    b.raw[0, 3] = logit
    b.bg = torch.tensor(bgv, dtype=torch.float32)
    return b


def far_scene(seed=3, H=32, W=32):
    """(c) a splat centred 450 px to the right of the image with a standard deviation of several hundred pixels, over three ordinary ones."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 4, 1, H, W, level="object", seed=seed)
    place(b, 0, 15.5 + 450.0, 11.0, 1.6)
    b.raw[0, 4:7, 0] = 3.5
    b.raw[0, 3, 0] = 2.0
    return b


def long_scene(seed=7, H=32, W=32):
    """(d) 130 faint Gaussians (opacity 0.047): no pixel saturates, so every tile walks all 130 sorted positions -- three staging batches,
    the last two beyond the position-indexed partial rows."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 130, 1, H, W, level="object", seed=seed)
    b.raw[0, 3] = -3.0
    return b


def check_fused(oracle_mod, b, what):
    """single- and two-pass fused step of the one-item, one-view batch against head_grad_arbiter, first line of the rule."""
    H, W = b.gt.shape[-2:]
    a32, _, _ = head_grad_arbiter(oracle_mod, b, 0, 0, H, W, 1, "l2", np.float32)
    a64, l64, i64 = head_grad_arbiter(oracle_mod, b, 0, 0, H, W, 1, "l2", np.float64)
    gap = rel_l2(a32, a64)
    assert np.any(a64) and gap <= GAP_MAX, f"{what}: the scene is no yardstick, fp32 restatement's own gap {gap:.2e}"
    bd = b.to(torch.device("cuda:0"))
    out = {}
    for sp in (True, False):
        loss, img, grad = fused_step(bd, sp)
        e64, e32 = rel_l2(grad[0].cpu().numpy().T, a64), rel_l2(grad[0].cpu().numpy().T, a32)
        print(f"[{what}] {'single' if sp else 'two'}-pass: |hip-f64| {e64:.2e} |hip-f32| {e32:.2e} |f32-f64| {gap:.2e}")
        assert abs(loss.item() - l64) <= TOL * abs(l64), (what, loss.item(), l64)
        assert rel_l2(img.cpu().numpy().reshape(i64.shape), i64) <= TOL, what
        out[sp] = e64
    for sp, e64 in out.items():
        assert e64 <= TOL, f"{what} ({'single' if sp else 'two'}-pass): d(head_out) {e64:.2e} from the fp64 arbiter, bar {TOL:.0e}"
    return a64


@pytest.mark.parametrize("H,W", [(16, 16), (12, 23)])
@pytest.mark.parametrize("where", ["pixel_centre", "between_pixels"])
def test_needle(oracle_mod, H, W, where):
    cx = (W // 2) + (0.0 if where == "pixel_centre" else 0.5)
    check_fused(oracle_mod, needle_scene(H, W, cx, float(H // 2)), f"needle {H}x{W} {where}")


@pytest.mark.parametrize("bgv", [(0.0, 0.0, 0.0), (0.2, 0.5, 0.8)], ids=["bg_zero", "bg_colour"])
@pytest.mark.parametrize("logit", [3.0, 6.0], ids=["plain", "general"])
def test_opaque_stack(oracle_mod, logit, bgv):
    b = stack_scene(logit, bgv)
    H, W = b.gt.shape[-2:]
    check_fused(oracle_mod, b, f"stack logit {logit:g} bg {bgv}")
    # the scene is what it claims: T_final reaches ~1e-4 on part of the image (the oracle's own final_T)
    from unipre3d_amd import synthetic
    with torch.no_grad():
        g = synthetic.gaussians_from_batch(b)
    r = oracle_view(oracle_mod, g, b, 0, 0, H, W, np.float32)
    tf = r.final_T.copy()
    r.close()
    assert tf.min() < 1e-3 and (tf < 1e-2).mean() > 0.05, (tf.min(), (tf < 1e-2).mean())


def test_far_centre(oracle_mod):
    b = far_scene()
    H, W = b.gt.shape[-2:]
    a64 = check_fused(oracle_mod, b, "far centre")
    assert np.abs(a64[:, 0]).max() > 1e-3 * np.abs(a64).max(), "the far splat takes part in the gradient"
    from unipre3d_amd import synthetic
    with torch.no_grad():
        g = synthetic.gaussians_from_batch(b)
    r = oracle_view(oracle_mod, g, b, 0, 0, H, W, np.float32)
    m = r.means2D[0].copy()
    r.close()
    assert m[0] - (W - 1) >= 400.0, m


def test_two_staging_batches(oracle_mod):
    b = long_scene()
    a64 = check_fused(oracle_mod, b, "130 faint Gaussians")
    assert (np.abs(a64).sum(axis=0) > 0).sum() > 100, "positions beyond the first 64 carry gradient"


def test_inverse_depth_operator_path(oracle_mod):
    """(e) the operator's backward with a non-zero dL/dinvdepth: the 10-value order of the reduction (g_d packed beside g_b)."""
    from unipre3d_amd import head, synthetic
    from unipre3d_amd.rasterizer import rasterize_gaussians_batched
    P, H, W = 48, 40, 56
    b = synthetic.make_batch(1, P, 1, H, W, level="object", seed=3)
    bd = b.to(torch.device("cuda:0"))
    with torch.no_grad():
        g0 = synthetic.gaussians_from_batch(bd)
    g = {k: v.detach().clone().requires_grad_(True) for k, v in g0.items()}
    shs = head.concat_sh(g["features_dc"], g["features_rest"])
    shs.retain_grad()
    m2d = torch.zeros(1, P, 3, device=bd.raw.device, requires_grad=True)
    t = math.tan(b.fov_deg * math.pi / 360)
    color, _, invd = rasterize_gaussians_batched(g["xyz"], g["opacity"], bd.world_view, bd.full_proj, bd.camera_center, bd.bg, H, W, t, t,
                                                 shs=shs, scales=g["scaling"], rotations=g["rotation"], sh_degree=1, means2D=m2d)
    dcol, dinv = cotangents(H, W)
    ((color[0, 0] * dcol.to(color.device)).sum() + (invd[0, 0] * dinv.to(color.device)).sum()).backward()
    torch.cuda.synchronize()
    gc = {k: v.detach().cpu() for k, v in g0.items()}
    r32, r64 = oracle_view(oracle_mod, gc, b, 0, 0, H, W, np.float32), oracle_view(oracle_mod, gc, b, 0, 0, H, W, np.float64)
    g32 = oracle_mod.backward(r32, dcol.numpy(), dinv.numpy())
    g64 = oracle_mod.backward(r64, dcol.numpy().astype(np.float64), dinv.numpy().astype(np.float64))
    # the depth cotangent matters: without it the gradients are others
    g64_nod = oracle_mod.backward(r64, dcol.numpy().astype(np.float64))
    assert rel_l2(g64_nod["means3D"], g64["means3D"]) > 100 * TOL
    assert rel_l2(invd[0, 0].detach().cpu().numpy(), r64.invdepth) <= TOL
    got = {"means3D": g["xyz"].grad[0], "opacities": g["opacity"].grad[0], "scales": g["scaling"].grad[0], "rotations": g["rotation"].grad[0],
           "shs": shs.grad[0], "means2D": m2d.grad[0]}
    bad = []
    for k, x in got.items():
        x = x.cpu().numpy().reshape(g64[k].shape)
        e64, gap = rel_l2(x, g64[k]), rel_l2(g32[k], g64[k])
        print(f"[inverse depth] d{k}: |hip-f64| {e64:.2e} |f32-f64| {gap:.2e}")
        assert gap <= GAP_MAX, f"d{k}: the scene is no yardstick, fp32 restatement's own gap {gap:.2e}"
        if e64 > TOL:
            bad.append((k, e64))
    r32.close(); r64.close()
    assert not bad, bad


def test_fused_step_is_deterministic():
    """(f) the same fused step twice: gradients equal bit for bit (fixed summation order in the lanes, the rows and across the tiles)."""
    for b in (stack_scene(3.0, (0.2, 0.5, 0.8)), needle_scene(12, 23, 11.5, 6.0)):
        bd = b.to(torch.device("cuda:0"))
        for sp in (True, False):
            one, two = fused_step(bd, sp), fused_step(bd, sp)
            assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])
            assert one[2].abs().max().item() > 0
