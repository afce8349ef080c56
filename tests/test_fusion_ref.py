"""CPU half of the z-buffer fusion edge tests (tests/test_gpu_fusion_edges.py is the GPU half): the scalar-loop reference of
tests/fusion_ref.py, oracle/fusion_oracle.py and golden G15 (the reference's own module on the edge set) agree bit for bit, the scene
builders place what they claim, and the backward refuses buffers its 16-byte accesses cannot take."""
import ctypes

import numpy as np
import pytest

import fusion_ref as R
from oracle import fusion_oracle as fo

UNIT = (1.0, 1.0, 0.0, 0.0)       # fx, fy, cx, cy of every built scene
pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")   # the edge set's subnormal depths, in the oracle


def _both_orders(cam):
    return np.stack([cam, cam[::-1]])


@pytest.mark.parametrize("H,W", R.SIZES)
def test_loop_reference_equals_the_oracle_on_the_edge_set(H, W):
    rng = np.random.RandomState(H * 16 + W)
    for cam in (_both_orders(R.edge_points(H, W)), R.with_nonfinite(R.edge_points(H, W), H, W)[0]):
        feat = rng.randn(2, 5, H, W).astype(np.float32)
        mapped, sel, table = R.zbuffer_loop(cam, feat, *UNIT)
        m2, s2 = fo.mapped_features(cam, feat, *UNIT)
        assert np.array_equal(mapped, m2) and np.array_equal(sel, s2) and sel.dtype == s2.dtype
        for b in range(2):                                   # the table names, per pixel, the first of the points whose sel is that pixel
            assert set(table[b]) == set(sel[b][sel[b] >= 0].tolist())
            for s, (bits, first) in table[b].items():
                assert first == np.nonzero(sel[b] == s)[0][0] and bits == R.depth_bits(cam[b, first, 2])


def test_loop_reference_equals_the_oracle_on_g7(golden):
    g = golden("g7_feature_fusion.npz")
    for tag in ("sq", "rect"):
        intr = g[f"{tag}_intr"]
        k = (intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2])
        cam = fo.camera_points(g[f"{tag}_center"], g[f"{tag}_c2w"])
        mapped, sel, _ = R.zbuffer_loop(cam, g[f"{tag}_feat"], *k)
        m2, s2 = fo.mapped_features(cam, g[f"{tag}_feat"], *k)
        assert np.array_equal(mapped, m2) and np.array_equal(sel, s2) and (sel >= 0).sum() > 20
        Cx = g[f"{tag}_x"].shape[2]
        assert np.array_equal(mapped, g[f"{tag}_out"][:, -mapped.shape[1]:, Cx:])


@pytest.mark.parametrize("H,W", R.SIZES)
def test_grad_loop_equals_the_oracle_for_an_integer_cotangent(H, W):
    cam = _both_orders(R.edge_points(H, W))
    feat = np.zeros((2, 5, H, W), np.float32)
    _, sel, _ = R.zbuffer_loop(cam, feat, *UNIT)
    gm = R.integer_cotangent((2, cam.shape[1], 5), seed=H)
    ref = R.grad_loop(gm, sel, 2, 5, H, W)
    assert ref.dtype == np.float64 and np.array_equal(ref.astype(np.float32), fo.mapped_grad(gm, sel, 2, 5, H, W))
    cnt, _ = R.grad_terms(gm, sel, 2, 5, H, W)
    assert cnt.max() == 70 and cnt.sum() == (sel >= 0).sum()
    R.assert_grad_any_order(ref.astype(np.float32), gm, sel, 2, 5, H, W)
    wrong = ref.astype(np.float32); wrong[0, 0, 5, 2] += 1                       # the 70-tie's pixel, one row dropped or doubled
    with pytest.raises(AssertionError):
        R.assert_grad_any_order(wrong, gm, sel, 2, 5, H, W)


@pytest.mark.parametrize("H,W", R.SIZES)
def test_golden_g15_equals_both_cpu_statements(golden, H, W):
    g, tag = golden("g15_fusion_edges.npz"), f"{H}x{W}"
    center, feat, intr = g[f"{tag}_center"], g[f"{tag}_feat"], g["intr"]
    B, N = center.shape[:2]
    C, Cx = feat.shape[1], g[f"{tag}_x"].shape[2]
    assert np.array_equal(center[0], R.edge_points(H, W)[:, :3]) and np.array_equal(center[1], center[0][::-1])
    cam = fo.camera_points(center, np.tile(np.eye(4, dtype=np.float32), (B, 1, 1)))
    assert np.array_equal(cam[..., :3].view(np.uint32), center.view(np.uint32)) or np.array_equal(cam[..., :3], center)   # (-0.0 + 0.0 = 0.0)
    mapped, sel, _ = R.zbuffer_loop(cam, feat, *UNIT)
    assert (sel >= 0).sum() > 150
    for kind, lo in (("cls", 0), ("plain", 1)):
        x, out = g[f"{tag}_x"][:, lo:], g[f"{tag}_out_{kind}"]
        assert np.array_equal(fo.fuse(x, center, feat, np.tile(np.eye(4, dtype=np.float32), (B, 1, 1)), intr), out)
        assert np.array_equal(out[:, -N:, Cx:], mapped) and np.array_equal(out[:, -N:, :Cx], x[:, -N:])
        if kind == "cls":
            assert np.array_equal(out[:, 0, :Cx], x[:, 0]) and not out[:, 0, Cx:].any()
        wi = g[f"{tag}_wi"].astype(np.float32)[:, -N:, Cx:]
        assert np.array_equal(fo.mapped_grad(wi, sel, B, C, H, W), g[f"{tag}_gfeat_int_{kind}"])
        assert np.array_equal(R.grad_loop(wi, sel, B, C, H, W).astype(np.float32), g[f"{tag}_gfeat_int_{kind}"])
        R.assert_grad_any_order(g[f"{tag}_gfeat_{kind}"], g[f"{tag}_w"][:, -N:, Cx:], sel, B, C, H, W)


@pytest.mark.parametrize("H,W", R.SIZES)
def test_edge_set_places_what_it_claims(H, W):
    cam = R.edge_points(H, W)
    assert cam.shape == (117, 4) and cam.dtype == np.float32 and (cam[:, 3] == 1).all()
    _, sel, table = R.zbuffer_loop(cam[None], np.zeros((1, 1, H, W), np.float32), *UNIT)
    sel, table, claims = sel[0], table[0], {c[0]: c for c in R.edge_claims(H, W)}
    assert sum(c[2] for c in claims.values()) == len(cam)
    for name, at, n, pixel, wins in claims.values():
        s = sel[at:at + n]
        if wins is not None:
            assert ((s >= 0) == wins).all(), name
        if pixel is not None and wins:
            assert (s == pixel[0] * W + pixel[1]).all(), name
    for a, b in (("ulp_far", "ulp_near"), ("far3", "tie3"), ("far70", "tie70")):          # the loser is on the winners' pixel, farther, earlier
        (_, fa, _, pix, _), (_, ta, tn, _, _) = claims[a], claims[b]
        assert fa < ta and cam[fa, 2] > cam[ta, 2] and table[pix[0] * W + pix[1]] == (R.depth_bits(cam[ta, 2]), ta)
        assert round(float(cam[fa, 0] / cam[fa, 2])) == pix[0] and round(float(cam[fa, 1] / cam[fa, 2])) == pix[1]
    assert cam[claims["ulp_far"][1], 2].view(np.uint32) - cam[claims["ulp_near"][1], 2].view(np.uint32) == 1
    for name in ("behind", "zero_depth"):                                                   # outside by the depth alone / by the quotient alone
        _, at, n, _, _ = claims[name]
        assert (cam[at:at + n, 2] <= 0).all()
    _, at, n, _, _ = claims["behind"]
    q = cam[at:at + n, :2] / cam[at:at + n, 2:3]
    assert (q >= 0).all() and (q[:, 0] < min(H, W)).all() and (q[:, 1] < min(H, W)).all()
    _, at, n, _, _ = claims["subnormal"]
    with np.errstate(over="ignore"):
        assert (cam[at:at + n, 2] > 0).all() and (cam[at:at + n, 2] < np.finfo(np.float32).tiny).all() and np.isinf(cam[at:at + n, 0] / cam[at:at + n, 2]).all()
    # half-integer pixels and the borders: Python's round() is half to even too, and px is held against H, py against W
    for name in ("half", "border", "corner", "minus_half"):
        _, at, n, _, _ = claims[name]
        for i in range(at, at + n):
            px, py = round(float(cam[i, 0])), round(float(cam[i, 1]))
            inside = 0 <= px < H and 0 <= py < W
            assert (sel[i] >= 0) == inside or (inside and table[px * W + py][0] < R.depth_bits(1.0)), (name, i)
            if sel[i] >= 0:
                assert sel[i] == px * W + py
    _, at, n, _, _ = claims["half"]
    assert {float(v) % 1 for v in cam[at:at + n, :2].reshape(-1)} == {0.0, 0.5}
    _, at, n, _, _ = claims["border"]
    b = sel[at:at + n].reshape(6, 2) >= 0                   # rows a = H-0.5, H-1, H, W-0.5, W-1, W; columns (a, 0) and (0, a)
    for r, a in enumerate((H - 0.5, H - 1, H, W - 0.5, W - 1, W)):
        assert b[r, 0] == (round(a) < H) and b[r, 1] == (round(a) < W), (r, a)
    assert b[1, 0] and not b[2, 0] and b[4, 1] and not b[5, 1]
    assert b[0, 0] == (H % 2 == 1) and b[3, 1] == (W % 2 == 1)      # H - 0.5 goes to the even one of H - 1 and H
    if H < W:                                                # in the band between H and W a coordinate is inside as py only
        assert not b[4, 0] and b[4, 1] and b[2, 1]
    else:
        assert b[1, 0] and not b[1, 1] and b[5, 0]
    # the accidental tie on pixel 0: 0.5 -> 0 and -0.5 -> -0.0 at one depth
    assert (sel == 0).sum() == 3 and sel[claims["minus_half"][1] + 2] == 0 and cam[claims["minus_half"][1] + 2, 0] == -0.5
    # what the non-finite variant adds
    cam2, inf_at = R.with_nonfinite(cam, H, W)
    _, sel2, table2 = R.zbuffer_loop(cam2, np.zeros((2, 1, H, W), np.float32), *UNIT)
    assert np.isinf(cam2[:, inf_at, 2]).all() and np.isnan(cam2[:, inf_at - 3:inf_at]).sum() == 2 * 3
    assert (sel2[:, inf_at - 3:inf_at] == -1).all() and sel2[0, inf_at] == -1 and sel2[1, inf_at] == 0
    assert table2[0][0][0] == R.depth_bits(1.0) and table2[1][0] == (0x7F800000, inf_at) and (sel2[1] == 0).sum() == 1


def test_structured_scenes_place_what_they_claim():
    zero = lambda B, H, W: np.zeros((B, 1, H, W), np.float32)   # noqa: E731
    # launch classes
    for B, N in ((1, 1), (1, 3), (1, 4), (1, 5), (1, 255), (1, 256), (1, 257), (2, 515)):
        H, W = R.image_for((2 * N + 2) // 3)
        cam, claims = R.launch_scene(B, N, H, W, seed=N)
        _, sel, table = R.zbuffer_loop(cam, zero(B, H, W), *UNIT)
        for b in range(B):
            winners, losers, tied = claims[b]
            assert (sel[b] >= 0).sum() == winners and (sel[b] < 0).sum() == losers and winners + losers == N
            assert len(table[b]) == max(1, (2 * N + 2) // 3) and winners - len(table[b]) == tied
            assert (tied > 0) == (N >= 3) and (losers > 0) == (N >= 255)
        if B > 1:
            assert not np.array_equal(cam[0], cam[1])
    assert {R.image_for(n)[0] * R.image_for(n)[1] % 4 == 0 for n in (1, 2, 3, 4, 170, 171, 172, 344)} == {True, False}
    # ties
    for k in (2, 3, 64, 65, 300):
        N = max(320, 2 * k + 20)
        for variant in ("plain", "nearer_late", "farther_early"):
            for H, W in ((5, 7), (4, 8)):
                cam, idx, T = R.tie_scene(k, variant, 2, N, H, W)
                _, sel, table = R.zbuffer_loop(cam, zero(2, H, W), *UNIT)
                assert len(idx) == k and idx[-1] - idx[0] > 256 and idx[0] // 256 != idx[-1] // 256 and (N + idx[0]) // 256 != (N + idx[-1]) // 256
                assert np.array_equal(sel[0], sel[1]) and sel[0, 1] == 0
                if variant == "nearer_late":
                    assert (sel[0, idx] == -1).all() and sel[0, N - 1] == T and table[0][T] == (R.depth_bits(1), N - 1) and N - 1 > idx[-1]
                    assert (sel[0] >= 0).sum() == 2
                else:
                    assert (sel[0, idx] == T).all() and table[0][T] == (R.depth_bits(2), idx[0]) and (sel[0] >= 0).sum() == k + 1
                    assert sel[0, 0] == -1 and (variant == "plain" or (cam[0, 0, 2] == 4 and 0 < idx[0]))
                assert set(table[0]) == {0, T}
    # backward scenes
    for H, W in ((2, 2), (4, 4), (32, 32), (36, 29), (1, 1), (3, 3), (15, 17), (1, 257), (7, 37)):
        HW = H * W
        scenes = R.backward_scenes(2, H, W)
        assert (len(scenes) == 4 + 4 * len({0, HW // 4 - 1})) if HW % 4 == 0 else len(scenes) == 4
        for name, cam in scenes.items():
            _, sel, table = R.zbuffer_loop(cam, zero(2, H, W), *UNIT)
            won = [sorted(t) for t in table]
            if name == "permutation":
                assert cam.shape[1] == HW and won == [list(range(HW))] * 2 and all(sorted(s.tolist()) == list(range(HW)) for s in sel)
                assert HW < 3 or not np.array_equal(sel[0], sel[1])
            elif name == "none":
                assert won == [[], []] and (sel == -1).all()
            else:
                want = {"first": 0, "last": HW - 1}.get(name)
                if want is None:
                    q, j = (int(v) for v in name.replace("quad", "").split("_pos"))
                    want = 4 * q + j
                assert won == [[want]] * 2 and (sel >= 0).sum() == 2
    assert [(H * W) // 4 for H, W in ((2, 2), (4, 4), (32, 32), (36, 29))] == [1, 4, 256, 261]
    # items differ
    cam, (winners, losers, tied) = R.items_differ_scene(40, 5, 7)
    _, sel, table = R.zbuffer_loop(cam, zero(3, 5, 7), *UNIT)
    assert (sel[1] == -1).all() and table[1] == {} and np.array_equal(sel[0], sel[2]) and (sel[0] >= 0).sum() == winners and tied > 0
    # cotangents
    gi = R.integer_cotangent((3, 40, 5))
    assert gi.dtype == np.float32 and np.array_equal(gi, np.rint(gi)) and np.abs(gi).max() == 8


def test_backward_refuses_misaligned_plane_buffers():
    """H*W a multiple of 4: zbuf and grad_features are read and written 16 bytes at a time, so a pointer 4 or 8 bytes off a 16-byte boundary is
    an invalid argument (1), found on the host before anything is launched.  The pointers are made up and never dereferenced; only refused
    combinations are passed."""
    from unipre3d_amd import fusion
    lib = fusion.load()
    p = lambda v: ctypes.c_void_p(v)   # noqa: E731
    gm, sel, zb, gf, null = 0x10000, 0x20000, 0x30000, 0x40000, p(0)
    for H, W in ((4, 4), (2, 6), (1, 4)):
        for off in (4, 8, 12):
            assert lib.u3d_zbuffer_fusion_backward(1, 4, 2, H, W, p(gm), p(sel), p(zb), p(gf + off), null) == 1
            assert lib.u3d_zbuffer_fusion_backward(1, 4, 2, H, W, p(gm), p(sel), p(zb + off), p(gf), null) == 1
            assert lib.u3d_zbuffer_fusion_backward(2, 4, 2, H, W, p(gm), p(sel), p(zb + off), p(gf + off), null) == 1
    # the unsupported-shape code still comes first, and nothing is looked at when there is nothing to do
    assert lib.u3d_zbuffer_fusion_backward(65536, 4, 2, 4, 4, p(gm), p(sel), p(zb + 8), p(gf), null) == 2
    assert lib.u3d_zbuffer_fusion_backward(0, 4, 2, 4, 4, p(gm), p(sel), p(zb + 8), p(gf + 4), null) == 0
    import re
    from conftest import ROOT
    hdr = open(f"{ROOT}/include/unipre3d_fusion.h").read()
    assert re.search(r"16-byte aligned", hdr)
