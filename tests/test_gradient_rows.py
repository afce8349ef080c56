"""tests/gradient_rows.py on the CPU: what `assert_group_rows` sees and `arbiter.assert_parity` does not, and the precondition of every
case of tests/test_gpu_gradient_rows.py (the fp32 restatement of each scene resolves every group and every row to 0.3 x TOL, and the
branch scenes are what they claim), so that the seeds are checked without a GPU."""
import dataclasses

import numpy as np
import pytest

import arbiter
import gradient_rows as gr
from arbiter import TOL, assert_parity, head_grad_arbiter
from conftest import rel_l2
from gradient_rows import BRANCH, assert_group_rows, assert_yardstick


@pytest.fixture(scope="module")
def gap_scene(oracle_mod):
    """Object level, P = 128, 64 x 64, one view, l2, make_batch(seed=5): (batch, fp32 restatement, fp64 arbiter), each (23, 128)."""
    from unipre3d_amd import synthetic
    b = synthetic.make_batch(1, 128, 1, 64, 64, level="object", seed=5)
    o32 = head_grad_arbiter(oracle_mod, b, 0, 0, 64, 64, 1, "l2", np.float32)[0]
    o64 = head_grad_arbiter(oracle_mod, b, 0, 0, 64, 64, 1, "l2", np.float64)[0]
    return b, o32, o64


def test_clean_restatement_passes(gap_scene):
    _, o32, o64 = gap_scene
    n0 = len(arbiter.GAP_PASSES)
    figs = assert_group_rows(o32, o32, o64, what="clean fp32")
    assert len(arbiter.GAP_PASSES) == n0
    assert all(f["row_e"] <= TOL and f["e64"] <= TOL for f in figs.values())
    # the shares of the whole-tensor norm that make the whole-tensor rule blind to the small groups
    share = {n: float(np.linalg.norm(o64[sl]) / np.linalg.norm(o64)) for n, sl in gr.HEAD_GROUPS}
    print("shares of the whole-tensor norm:", {n: f"{s:.1e}" for n, s in share.items()})
    assert share["rotation"] < 1e-2 and share["rest"] > 0.5


def _plant(o32, o64, kind):
    rot = slice(7, 11)
    x = o32.copy()
    n = np.linalg.norm(o64[rot], axis=0)
    if kind == "largest_row_1pc":
        x[rot, int(n.argmax())] *= 1.01
    elif kind == "median_row_zero":
        x[rot, int(np.argsort(n)[len(n) // 2])] = 0.0
    elif kind == "group_3pc":
        x[rot] *= 1.03
    return x


@pytest.mark.parametrize("kind", ["largest_row_1pc", "median_row_zero", "group_3pc"])
def test_planted_rotation_errors_pass_the_tensor_rule_and_fail_the_row_rule(gap_scene, kind):
    """The gap this module closes: three errors confined to the rotation group (3e-3 of the tensor's norm) are accepted by assert_parity
    on the whole (23, P) gradient and rejected per group / per row."""
    _, o32, o64 = gap_scene
    x = _plant(o32, o64, kind)
    n0 = len(arbiter.GAP_PASSES)
    e64, _, _ = assert_parity(x, o32, o64, kind)
    print(f"{kind}: whole-tensor |x-f64| {e64:.2e}, rotation group {rel_l2(x[7:11], o64[7:11]):.2e}")
    assert e64 <= TOL
    with pytest.raises(AssertionError, match="rotation"):
        assert_group_rows(x, o32, o64, what=kind)
    del arbiter.GAP_PASSES[n0:]
    # ... and the other five groups are untouched
    assert_group_rows(x, o32, o64, groups=[g for g in gr.HEAD_GROUPS if g[0] != "rotation"], what=kind)


def test_wrong_levels_quaternion_chain_is_rejected(oracle_mod, gap_scene):
    """The fp64 gradient recomputed with the rotation normalised per quaternion (the scene branch's formula) on the object-level scene."""
    b, o32, o64 = gap_scene
    wrong = head_grad_arbiter(oracle_mod, dataclasses.replace(b, level="scene"), 0, 0, 64, 64, 1, "l2", np.float64)[0]
    with pytest.raises(AssertionError, match="rotation"):
        assert_group_rows(wrong, o32, o64, what="per-quaternion chain at object level")


def test_row_rule_branches():
    """The row rule on synthetic (1, P) groups: first line, capped gap (logged), beyond the gap, beyond the cap, stray non-zero row."""
    o64 = np.ones((1, 50))
    o64[0, 7] = 0.0
    mk = lambda e, at=3: o64 + e * (np.arange(50) == at)
    n0 = len(arbiter.GAP_PASSES)
    g = [("g", slice(0, 1))]
    assert_group_rows(mk(5e-5), mk(2e-5), o64, g, "first line")
    assert len(arbiter.GAP_PASSES) == n0
    assert_group_rows(mk(5e-4), mk(3e-4), o64, g, "capped gap")
    assert len(arbiter.GAP_PASSES) == n0 + 1 and "row 3" in arbiter.GAP_PASSES[n0][0]
    del arbiter.GAP_PASSES[n0:]
    for x, o32 in ((mk(5e-4), mk(2e-4)), (mk(3e-3), mk(2e-3)), (mk(2e-4), mk(1e-6))):
        with pytest.raises(AssertionError, match="row 3"):
            assert_group_rows(x, o32, o64, g, "must fail")
    z32 = mk(0.0)
    with pytest.raises(AssertionError, match="exactly zero"):
        assert_group_rows(mk(1e-9, at=7), z32, o64, g, "stray")
    assert len(arbiter.GAP_PASSES) == n0


# ---------------------------------------------------------------------------------------------------------------------------------
# the preconditions of the GPU cases

@pytest.mark.parametrize("P", gr.ROUTE_P)
@pytest.mark.parametrize("level", ["object", "scene"])
def test_yardstick_norm_routes(oracle_mod, level, P):
    o32, o64 = gr.summed_pair(gr.view_pairs(oracle_mod, gr.route_scene(level, P), ("route", level, P)))
    assert_yardstick(o32, o64, what=f"{level} P={P}")
    live = [float(np.any(o64[sl] != 0, axis=0).mean()) for _, sl in gr.HEAD_GROUPS]
    # (object level: every Gaussian is in front of the camera; at P = 1100 the pixels saturate after a few hundred entries even so)
    assert min(live) > (0.9 if level == "object" and P <= 257 else 0.1), ("share of the rows that carry gradient, per group", live)


@pytest.mark.parametrize("V", gr.VIEW_COUNTS)
@pytest.mark.parametrize("level", ["object", "scene"])
def test_yardstick_view_counts(oracle_mod, level, V):
    pairs = gr.view_pairs(oracle_mod, gr.view_scene(level, V), ("views", level, V))
    o32, o64 = gr.summed_pair(pairs)
    assert_yardstick(o32, o64, what=f"{level} V={V}")
    if V == 9:
        for v in gr.ISOLATED_VIEWS:
            assert_yardstick(pairs[v][0], pairs[v][1], what=f"{level} V=9, view {v} alone")


@pytest.mark.parametrize("level", ["object", "scene"])
def test_branch_scene_is_what_it_claims(oracle_mod, level):
    b = gr.branch_scene(level)
    o32, o64 = gr.summed_pair(gr.view_pairs(oracle_mod, b, ("branch", level)))
    assert_yardstick(o32, o64, what=f"{level} branches")
    check_branch_rows(o64, level, "fp64 arbiter")
    check_branch_rows(o32, level, "fp32 restatement")
    vis = [gr.visible_views(oracle_mod, b, i)[0] for i in range(12)]
    assert not vis[BRANCH["behind"]] and all(v for i, v in enumerate(vis) if i != BRANCH["behind"]), vis


def check_branch_rows(x, level, who):
    """The expectations of gradient_rows.branch_scene on a (23, 12) gradient (shared with the GPU test)."""
    nz = lambda a: bool(np.all(a != 0))
    z = lambda a: not np.any(a != 0)
    i = BRANCH["scale_below"]
    assert z(x[4:7, i]) and nz(x[0:4, i]), (who, "scaling below the clamp", x[0:7, i])
    i = BRANCH["scale_at_clamp"]
    assert nz(x[4:7, i]), (who, "scaling exactly on the clamp", x[4:7, i])
    i = BRANCH["scale_one_axis"]
    assert z(x[5, i]) and nz(x[[4, 6], i]), (who, "one clamped axis", x[4:7, i])
    for i, n in ((BRANCH["dc_one"], 1), (BRANCH["dc_two"], 2), (BRANCH["dc_three"], 3)):
        sh = x[11:23, i].reshape(4, 3)        # (coefficient, colour channel)
        assert z(sh[:, :n]) and nz(sh[:, n:]) and nz(x[0:4, i]), (who, f"{n} clamped colour channels", sh)
    # (object level: the across-point quaternion normalisation hands EVERY Gaussian the column term -x_i (sum_j x_j g_j) / n^3, a culled
    # one too; its other 19 entries are exactly zero.  Scene level: all 23.)
    i = BRANCH["behind"]
    assert z(x[0:7, i]) and z(x[11:23, i]) and (nz(x[7:11, i]) if level == "object" else z(x[7:11, i])), (who, "behind the camera", x[:, i])
    i = BRANCH["far_mean"]
    assert nz(x[0:11, i]) and np.abs(x[0:3, i]).max() > 1e-3 * np.abs(x[0:3]).max(), (who, "far mean takes part", x[:, i])
    if level == "scene":
        rows = np.linalg.norm(x[7:11], axis=0)
        # both were placed where they receive gradient: g / eps and g / n make theirs the largest rotation rows by far
        typical = np.median(np.delete(rows, [BRANCH["quat_eps"], BRANCH["quat_small"], BRANCH["behind"]]))
        assert rows[BRANCH["quat_eps"]] > 1e4 * typical and rows[BRANCH["quat_small"]] > 1e2 * typical, (who, "small quaternions", rows)


@pytest.mark.parametrize("level", ["object", "scene"])
def test_two_view_scene_is_what_it_claims(oracle_mod, level):
    b = gr.two_view_scene(level)
    i = gr.TWO_VIEW_GAUSSIAN
    assert gr.visible_views(oracle_mod, b, i) == [True, False, False, False, True]
    pairs = gr.view_pairs(oracle_mod, b, ("two_view", level))
    o32, o64 = gr.summed_pair(pairs)
    assert_yardstick(o32, o64, what=f"{level} two views")
    for v in (1, 2, 3):
        for a in pairs[v]:      # (object level: the rotation entries carry the across-point column term, see check_branch_rows)
            assert not np.any(a[0:7, i]) and not np.any(a[11:23, i]) and (level == "object" or not np.any(a[7:11, i]))
    assert np.all(pairs[0][1][0:7, i] != 0) and np.all(pairs[4][1][0:7, i] != 0)
    assert row_error(o32[:, i], o64[:, i]) <= gr.YARDSTICK_MAX


def row_error(a, ref):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - ref) / np.linalg.norm(ref))


def test_yardstick_isotropic(oracle_mod):
    o32, o64 = gr.summed_pair(gr.view_pairs(oracle_mod, gr.isotropic_scene(), ("isotropic",), isotropic=True))
    assert_yardstick(o32, o64, what="isotropic head")
    assert not np.any(o64[5:7]) and np.mean(o64[4] != 0) > 0.5


@pytest.mark.parametrize("case", range(6))
def test_yardstick_operator_level(oracle_mod, case):
    from scenes import SMALL_CASES, cotangents, scene
    P, H, W, level, compact, deg, seed = SMALL_CASES[case]
    sc = scene(P, H, W, seed, level, compact, deg)
    dcol, dinv = cotangents(H, W)
    o32, o64, groups = gr.operator_pair(oracle_mod, sc, dcol, dinv)
    assert_yardstick(o32, o64, groups, what=f"operator case {case}")
