"""The fused render-loss step's gradient per channel group and per Gaussian (tests/gradient_rows.py::assert_group_rows), on the routes the
whole-tensor rule of tests/arbiter.py cannot see into:

  (a) the across-point quaternion norms of the object level: in-block (P <= 256), quat_norms_kernel with several backward blocks feeding
      qdot (257), the norm kernel's second trip (1100) -- and the same sizes at scene level;
  (b) view counts around preprocess_bwd_kernel's four view slots per Gaussian (V = 1, 3, 4, 5, 8, 9), and every view slot pinned to its
      own camera (V = 9, all views but one silenced);
  (c) one Gaussian per branch of the activations' backward (scaling clamp, colour clamp, near cull, far mean, tiny quaternions,
      visible in views 0 and 4 only, the isotropic head);
  (d) the operator's gradients of scenes.SMALL_CASES, one group per input;
  (e) the forward projection's four-views-per-thread form with a partial last slice (total P >= 65536, V = 5, 6, 7), bit for bit against
      one-view calls;
  (f) determinism at V = 9.

Every oracle-backed case asserts its precondition first (gradient_rows.assert_yardstick; tests/test_gradient_rows.py checks the same on
the CPU) and prints every figure before it asserts; U3D_GRADIENT_ROWS_OUT=<file> collects them (profiles/gradient_rows/figures.json)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import gradient_rows as gr
from arbiter import GAP_CEIL, GAP_K, TOL
from gradient_rows import assert_group_rows, assert_yardstick, fused_step
from scenes import SMALL_CASES, cotangents, scene
from test_gradient_rows import check_branch_rows, row_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def figures_out():
    n0 = len(gr.FIGURES)
    yield
    path = os.environ.get("U3D_GRADIENT_ROWS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"unit": "per channel group: e64 / e32 = relative L2 of the HIP gradient from the fp64 arbiter / the fp32 restatement, gap = "
                               "the restatement's own; row_e / row_y = worst ||row - f64 row|| / largest f64 row of the group for HIP / for the "
                               "restatement (tests/gradient_rows.py); bar 1e-4, or 2 x the restatement's figure under 1e-3",
                       "cases": gr.FIGURES[n0:]}, f, indent=1)


def check_step(b, o32, o64, what, isotropic=False):
    """Single- and two-pass fused step of the one-item batch against the restatements, by group and by row.  {single_pass: (C, P) gradient}."""
    assert_yardstick(o32, o64, what=what)
    bd = b.to(torch.device("cuda:0"))
    out = {}
    for sp in (True, False):
        x = fused_step(bd, sp, isotropic)[2][0].cpu().numpy().T
        out[sp] = x
        tag = f"{what}, {'single' if sp else 'two'}-pass"
        gr.record(tag, assert_group_rows(x, o32, o64, what=tag))
    return out


@pytest.mark.parametrize("P", gr.ROUTE_P)
@pytest.mark.parametrize("level", ["object", "scene"])
def test_quaternion_norm_routes(oracle_mod, level, P):
    b = gr.route_scene(level, P)
    o32, o64 = gr.summed_pair(gr.view_pairs(oracle_mod, b, ("route", level, P)))
    check_step(b, o32, o64, f"{level} P={P} 48x48")


@pytest.mark.parametrize("V", gr.VIEW_COUNTS)
@pytest.mark.parametrize("level", ["object", "scene"])
def test_view_counts(oracle_mod, level, V):
    b = gr.view_scene(level, V)
    o32, o64 = gr.summed_pair(gr.view_pairs(oracle_mod, b, ("views", level, V)))
    check_step(b, o32, o64, f"{level} P=70 V={V}")


@pytest.mark.parametrize("v", gr.ISOLATED_VIEWS)
@pytest.mark.parametrize("level", ["object", "scene"])
def test_each_view_slot_reads_its_own_camera(oracle_mod, level, v):
    """V = 9: the targets of all views but v are the rendered images themselves, so under l2 those views hand back exact zeros and the
    gradient is view v's alone (head_grad_arbiter with n_views_total = 9).  v = 4 and 8 are the second and third trip of view slot 0,
    v = 3 the last slot: a slot that read another view's camera or accumulators fails here."""
    b = gr.view_scene(level, 9)
    o32, o64 = gr.view_pairs(oracle_mod, b, ("views", level, 9))[v]
    bd = b.to(torch.device("cuda:0"))
    _, img, _ = fused_step(bd, True)
    check_step(gr.isolate_view(b, img, v), o32, o64, f"{level} P=70 V=9, view {v} alone")


@pytest.mark.parametrize("level", ["object", "scene"])
def test_branch_rows(oracle_mod, level):
    b = gr.branch_scene(level)
    o32, o64 = gr.summed_pair(gr.view_pairs(oracle_mod, b, ("branch", level)))
    check_branch_rows(o64, level, "fp64 arbiter")
    for sp, x in check_step(b, o32, o64, f"{level} branches").items():
        check_branch_rows(x, level, f"HIP {'single' if sp else 'two'}-pass")


@pytest.mark.parametrize("level", ["object", "scene"])
def test_gaussian_seen_by_views_0_and_4_only(oracle_mod, level):
    """Its row is the sum of the two one-view arbiters: both trips of view slot 0 and nothing from the other slots (same rule and constants
    as the row rule, against the row's own norm)."""
    b = gr.two_view_scene(level)
    i = gr.TWO_VIEW_GAUSSIAN
    pairs = gr.view_pairs(oracle_mod, b, ("two_view", level))
    o32, o64 = gr.summed_pair(pairs)
    s32, s64 = pairs[0][0][:, i] + pairs[4][0][:, i], pairs[0][1][:, i] + pairs[4][1][:, i]
    keep = np.r_[0:7, 11:23] if level == "object" else np.r_[0:23]     # (object level: every view's column term reaches the rotation entries)
    assert np.array_equal(o64[keep, i], s64[keep]) and np.all(s64[0:7] != 0)
    y = row_error(s32[keep], s64[keep])
    for sp, x in check_step(b, o32, o64, f"{level} two-view Gaussian").items():
        e = row_error(x[keep, i], s64[keep])
        print(f"[rows] {level} two-view Gaussian row, {'single' if sp else 'two'}-pass: |x-f64| {e:.2e}, restatement's own {y:.2e}")
        gr.record(f"{level} two-view Gaussian row, {'single' if sp else 'two'}-pass", {}, row_e=e, row_y=y)
        assert e <= TOL or (e <= GAP_K * y and e <= GAP_CEIL * TOL), (sp, e, y)
        # one view alone is another gradient: the second trip contributes
        assert row_error(x[keep, i], pairs[0][1][keep, i]) > 100 * TOL and row_error(x[keep, i], pairs[4][1][keep, i]) > 100 * TOL


def test_isotropic_head_rows(oracle_mod):
    b = gr.isotropic_scene()
    o32, o64 = gr.summed_pair(gr.view_pairs(oracle_mod, b, ("isotropic",), isotropic=True))
    for sp, x in check_step(b, o32, o64, "isotropic head", isotropic=True).items():
        assert not np.any(x[5:7]) and np.any(x[4] != 0)
    # and the anisotropic arbiter is another answer
    a64 = gr.summed_pair(gr.view_pairs(oracle_mod, b, ("isotropic", "off")))[1]
    assert row_error(a64[4:7].ravel(), o64[4:7].ravel()) > 100 * TOL


@pytest.mark.parametrize("case", range(len(SMALL_CASES)))
def test_operator_level_rows(oracle_mod, case):
    from test_gpu_parity import _run_gpu
    P, H, W, level, compact, deg, seed = SMALL_CASES[case]
    sc = scene(P, H, W, seed, level, compact, deg)
    dcol, dinv = cotangents(H, W)
    o32, o64, groups = gr.operator_pair(oracle_mod, sc, dcol, dinv)
    what = f"operator P={P} {H}x{W} {level} deg {deg}"
    assert_yardstick(o32, o64, groups, what=what)
    g = _run_gpu(sc, dcol, dinv)[3]
    x, _ = gr.stack_operator(g, P)
    gr.record(what, assert_group_rows(x, o32, o64, groups, what))


@pytest.mark.parametrize("V", [5, 6, 7])
def test_forward_partial_view_slice(V):
    """total P >= 65536: preprocess_fwd_kernel walks four views per thread and the last slice holds V - 4 of them.  The V-view call equals
    V one-view calls (one view per thread) bit for bit: images, inverse depths, radii."""
    from unipre3d_amd import head, synthetic
    from unipre3d_amd.rasterizer import rasterize_gaussians_batched
    P, H, W = 65536, 32, 32
    b = synthetic.make_batch(1, P, V, H, W, level="scene", seed=11).to(torch.device("cuda:0"))
    with torch.no_grad():
        g = synthetic.gaussians_from_batch(b)
        shs = head.concat_sh(g["features_dc"], g["features_rest"])
        t = math.tan(b.fov_deg * math.pi / 360)
        run = lambda vs: rasterize_gaussians_batched(g["xyz"], g["opacity"], b.world_view[:, vs], b.full_proj[:, vs], b.camera_center[:, vs], b.bg,
                                                     H, W, t, t, shs=shs, scales=g["scaling"], rotations=g["rotation"], sh_degree=1)
        color, radii, invd = run(slice(0, V))
        torch.cuda.synchronize()
        for v in range(V):
            c1, r1, d1 = run(slice(v, v + 1))
            assert torch.equal(radii[0, v], r1[0, 0]), f"radii of view {v}"
            assert torch.equal(color[0, v], c1[0, 0]) and torch.equal(invd[0, v], d1[0, 0]), f"image of view {v}"
        bgim = b.bg[:, None, None].expand(3, H, W)
        assert any(bool((radii[0, v] > 0).any()) and not torch.equal(color[0, v], bgim) for v in range(4, V)), "the partial slice renders nothing"


def test_nine_view_step_is_deterministic():
    """Object level reduces in a fixed order (lanes, rows, tiles, view slots; the two backward blocks of P = 70 add their qdot shares
    to a cleared word, and a + b = b + a): the same step twice gives the same bits."""
    bd = gr.view_scene("object", 9).to(torch.device("cuda:0"))
    for sp in (True, False):
        one, two = fused_step(bd, sp), fused_step(bd, sp)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])
        assert one[2].abs().max().item() > 0
