"""The five kernels of unipre3d_amd/csrc/u3d_fusion.hip (zbuf_min, gather, grad_plane, grad_dense1<8>, tie_add) at their edges, against the
scalar-loop reference of tests/fusion_ref.py, oracle/fusion_oracle.py and golden G15 (tests/test_fusion_ref.py holds those three against each
other on the CPU and asserts that every scene used here places what it claims).

Forward results are copies and integers: compared bit for bit.  Backward: with an integer cotangent (|values| <= 8) every sum is exact in
fp32 in any order, so the result equals the fp64 scatter-add bit for bit and a dropped or doubled tied row shows as an integer difference;
with a Gaussian cotangent an element fed by at most one row is a copy (bit for bit) and one fed by k rows lies within k * 2^-24 * sum |g_i| of
the fp64 sum (fusion_ref.assert_grad_any_order).  Most tests call the C ABI directly into buffers pre-filled with NaN / 0x7fffffff / a junk
winner table, so that an element the library leaves unwritten shows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fusion_ref as R
from oracle import fusion_oracle as fo

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")]
UNIT = (1.0, 1.0, 0.0, 0.0)
NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def forward_raw(cam, feat, zbuf=None, k=UNIT):
    """u3d_zbuffer_fusion_forward into pre-filled outputs -> (mapped, sel, zbuf) device tensors"""
    from unipre3d_amd import _lib, fusion
    cp, ft = torch.as_tensor(cam).to(_dev()).contiguous(), torch.as_tensor(feat).to(_dev()).contiguous()
    (B, N, _), (_, C, H, W) = cp.shape, ft.shape
    mapped = torch.full((B, N, C), NAN, device=_dev())
    sel = torch.full((B, N), 0x7FFFFFFF, dtype=torch.int32, device=_dev())
    if zbuf is None:
        zbuf = torch.full((B * H * W,), 0x0123456789ABCDEF, dtype=torch.int64, device=_dev())
    assert zbuf.numel() * 8 == fusion.load().u3d_zbuffer_fusion_zbuf_bytes(B, H, W)
    rc = fusion.load().u3d_zbuffer_fusion_forward(B, N, C, H, W, *k, _lib.ptr(cp), _lib.ptr(ft), _lib.ptr(mapped), _lib.ptr(sel),
                                                  _lib.ptr(zbuf), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return mapped, sel, zbuf


def backward_raw(gm, sel, zbuf, C, H, W):
    """u3d_zbuffer_fusion_backward into a NaN-filled gradient -> (B, C, H, W) numpy"""
    from unipre3d_amd import _lib, fusion
    g = torch.as_tensor(gm).to(_dev()).contiguous()
    B, N = sel.shape
    gf = torch.full((B, C, H, W), NAN, device=_dev())
    rc = fusion.load().u3d_zbuffer_fusion_backward(B, N, C, H, W, _lib.ptr(g), _lib.ptr(sel), _lib.ptr(zbuf), _lib.ptr(gf), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return gf.cpu().numpy()


def words(zbuf, B):
    return zbuf.cpu().numpy().view(np.uint64).reshape(B, -1)


def check_all(cam, feat, seed=0, what=""):
    """One scene through the C ABI: mapped, sel and the winner words against the loop reference (and the oracle), the backward with an
    integer cotangent bit for bit and with a Gaussian one within the any-order bound.  -> dict of what was computed"""
    cam, feat = np.asarray(cam, np.float32), np.asarray(feat, np.float32)
    (B, N, _), (_, C, H, W) = cam.shape, feat.shape
    ref_mapped, ref_sel, table = R.zbuffer_loop(cam, feat, *UNIT)
    mapped, sel, zbuf = forward_raw(cam, feat)
    got_mapped, got_sel, got_words = mapped.cpu().numpy(), sel.cpu().numpy(), words(zbuf, B)
    assert np.array_equal(got_sel, ref_sel), what
    assert np.array_equal(got_mapped, ref_mapped), what
    o_mapped, o_sel = fo.mapped_features(cam, feat, *UNIT)
    assert np.array_equal(got_sel, o_sel) and np.array_equal(got_mapped, o_mapped), what
    # header contract: high half = bits of the pixel's minimum depth, low half = smallest index among the points whose sel is the pixel
    assert np.array_equal(got_words, R.winner_words(table, H, W)), what
    for b in range(B):
        for s in np.unique(got_sel[b][got_sel[b] >= 0]):
            first = int(np.nonzero(got_sel[b] == s)[0][0])
            assert int(got_words[b, s]) == (R.depth_bits(cam[b, first, 2]) << 32 | first), what
        assert (got_words[b][np.setdiff1d(np.arange(H * W), got_sel[b])] == np.uint64(R.EMPTY)).all(), what
    gi = R.integer_cotangent((B, N, C), seed=seed + 1)
    grad_i = backward_raw(gi, sel, zbuf, C, H, W)
    assert np.array_equal(grad_i, R.grad_loop(gi, ref_sel, B, C, H, W).astype(np.float32)), what
    gg = np.random.RandomState(seed + 2).randn(B, N, C).astype(np.float32)
    grad_g = backward_raw(gg, sel, zbuf, C, H, W)
    R.assert_grad_any_order(grad_g, gg, ref_sel, B, C, H, W)
    return dict(mapped=got_mapped, sel=got_sel, words=got_words, grad_int=grad_i, grad_gauss=grad_g, dev=(mapped, sel, zbuf), gauss=gg)


def _feat(B, C, H, W, seed=0):
    return np.random.RandomState(seed).randn(B, C, H, W).astype(np.float32)


# ---- forward semantics -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g15_sel(H, W):
    cam = np.ones((2, 117, 4), np.float32)
    cam[0, :, :3] = R.edge_points(H, W)[:, :3]; cam[1] = cam[0, ::-1]
    return R.zbuffer_loop(cam, np.zeros((2, 1, H, W), np.float32), *UNIT)[1]


@pytest.mark.parametrize("kind", ["cls", "plain"])
@pytest.mark.parametrize("H,W", R.SIZES)
def test_g15_through_feature_fusion(golden, H, W, kind):
    """The reference's own outputs on the edge set: half-to-even pixels, the swapped border test, -0.5 -> pixel 0, depths one ulp apart,
    a 3-tie and a 70-tie, both widths of x."""
    from unipre3d_amd.fusion import FeatureFusion
    g, tag, lo = golden("g15_fusion_edges.npz"), f"{H}x{W}", 0 if kind == "cls" else 1
    t = lambda a: torch.tensor(a).to(_dev())   # noqa: E731
    center, feat = t(g[f"{tag}_center"]), t(g[f"{tag}_feat"]).requires_grad_(True)
    B, N = center.shape[:2]
    C, Cx = feat.shape[1], g[f"{tag}_x"].shape[2]
    y = FeatureFusion(torch.nn.Identity())(t(g[f"{tag}_x"][:, lo:]), center, feat, torch.eye(4, device=_dev()).repeat(B, 1, 1), g["intr"])
    assert np.array_equal(y.detach().cpu().numpy(), g[f"{tag}_out_{kind}"])
    w, wi = g[f"{tag}_w"][:, lo:], g[f"{tag}_wi"][:, lo:].astype(np.float32)
    (gi,) = torch.autograd.grad((y * t(wi)).sum(), feat, retain_graph=True)
    assert np.array_equal(gi.cpu().numpy(), g[f"{tag}_gfeat_int_{kind}"])
    (gw,) = torch.autograd.grad((y * t(w)).sum(), feat)
    gw, gold, sel = gw.cpu().numpy(), g[f"{tag}_gfeat_{kind}"], _g15_sel(H, W)
    R.assert_grad_any_order(gw, w[:, -N:, Cx:], sel, B, C, H, W)
    # against the recorded gradient itself: both lie within the bound of the fp64 sum, so within twice the bound of each other
    cnt, mag = R.grad_terms(w[:, -N:, Cx:], sel, B, C, H, W)
    single = np.broadcast_to(cnt <= 1, gold.shape)
    assert np.array_equal(gw[single], gold[single])
    assert np.all(np.abs(gw.astype(np.float64) - gold) <= 2 * cnt * R.U24 * mag)


@pytest.mark.parametrize("H,W", R.SIZES)
def test_edge_set_with_nonfinite_points_through_the_autograd_function(H, W):
    """+inf depth alone on a pixel wins it, +inf depth behind a finite point loses, NaN in x, y or z is outside"""
    from unipre3d_amd.fusion import _ZBufferGather
    cam, inf_at = R.with_nonfinite(R.edge_points(H, W), H, W)
    feat = _feat(2, 5, H, W, seed=H)
    mapped, sel = _ZBufferGather.apply(torch.tensor(cam).to(_dev()), torch.tensor(feat).to(_dev()), *UNIT)
    mapped, sel = mapped.cpu().numpy(), sel.cpu().numpy()
    ref_mapped, ref_sel, _ = R.zbuffer_loop(cam, feat, *UNIT)
    o_mapped, o_sel = fo.mapped_features(cam, feat, *UNIT)
    assert np.array_equal(sel, ref_sel) and np.array_equal(mapped, ref_mapped)
    assert np.array_equal(sel, o_sel) and np.array_equal(mapped, o_mapped)
    assert sel[0, inf_at] == -1 and sel[1, inf_at] == 0 and np.array_equal(mapped[1, inf_at], feat[1, :, 0, 0])


@pytest.mark.parametrize("H,W", R.SIZES)
def test_winner_words_follow_the_header_contract_on_the_edge_set(H, W):
    cam, inf_at = R.with_nonfinite(R.edge_points(H, W), H, W)
    r = check_all(cam, _feat(2, 5, H, W, seed=W), seed=H)
    assert int(r["words"][1, 0]) == (0x7F800000 << 32 | inf_at) and (r["words"] == np.uint64(R.EMPTY)).any()
    both = np.stack([cam[0, :117], cam[0, :117][::-1]])                     # the same points in reverse order name other first winners
    r2 = check_all(both, _feat(2, 5, H, W, seed=W), seed=H)
    assert np.array_equal(r2["words"][0] >> np.uint64(32), r2["words"][1] >> np.uint64(32)) and not np.array_equal(r2["words"][0], r2["words"][1])


@pytest.mark.parametrize("B,N", [(1, 1), (1, 3), (1, 4), (1, 5), (1, 255), (1, 256), (1, 257), (2, 515)])
def test_launch_classes_over_the_number_of_points(B, N):
    """B*N around the 256-thread blocks of zbuf_min_kernel and the 4-points-per-block gather_kernel and tie_add_kernel"""
    H, W = R.image_for((2 * N + 2) // 3)
    cam, _ = R.launch_scene(B, N, H, W, seed=N)
    check_all(cam, _feat(B, 3, H, W, seed=N), seed=N)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_launch_classes_over_the_channels(C):
    """the 64-lane channel loops of gather_kernel and tie_add_kernel: one partial trip, one full, a second, a third"""
    for H, W in ((5, 7), (4, 8)):
        cam, _ = R.launch_scene(2, 40, H, W, seed=C)
        check_all(cam, _feat(2, C, H, W, seed=C), seed=C, what=f"{H}x{W}")


@pytest.mark.parametrize("variant", ["plain", "nearer_late", "farther_early"])
@pytest.mark.parametrize("k", [2, 3, 64, 65, 300])
def test_ties(k, variant):
    """k tied points spread over more than 256 indices in each of two items: every one is kept, and added once"""
    N, C = max(320, 2 * k + 20), 70 if k == 3 else 3
    for H, W in ((5, 7), (4, 8)):
        cam, idx, T = R.tie_scene(k, variant, 2, N, H, W)
        r = check_all(cam, _feat(2, C, H, W, seed=k), seed=k, what=f"{H}x{W}")
        tied = r["sel"][:, idx]
        assert (tied == (-1 if variant == "nearer_late" else T)).all()
        if variant != "nearer_late":
            assert (r["words"][:, T] == np.uint64(R.depth_bits(2) << 32 | int(idx[0]))).all()


def test_items_differ():
    """B = 3, the middle item without a single inside point, the outer two with the same points but other features and cotangent rows:
    a missing b*N*C or b*HW offset cannot cancel"""
    for H, W in ((5, 7), (4, 8)):
        cam, _ = R.items_differ_scene(40, H, W, seed=3)
        r = check_all(cam, _feat(3, 6, H, W, seed=5), seed=7, what=f"{H}x{W}")
        assert (r["sel"][1] == -1).all() and not r["mapped"][1].any() and (r["words"][1] == np.uint64(R.EMPTY)).all()
        assert not r["grad_int"][1].any() and not r["grad_gauss"][1].any()
        assert np.array_equal(r["sel"][0], r["sel"][2]) and np.array_equal(r["words"][0], r["words"][2])
        won = r["sel"][0] >= 0
        assert won.sum() > 20 and (r["mapped"][0][won] != r["mapped"][2][won]).all()
        assert not np.array_equal(r["grad_int"][0], r["grad_int"][2])


def test_buffers_need_no_preparation():
    from unipre3d_amd import _lib, fusion
    for H, W in ((4, 4), (3, 5)):
        # all losers: mapped, sel and the gradient come back all zero, all -1, all zero from NaN / 0x7fffffff / NaN
        cam = R.single_scene(2, 5, H, W, None)
        mapped, sel, zbuf = forward_raw(cam, _feat(2, 3, H, W))
        assert (mapped == 0).all() and (sel == -1).all() and (words(zbuf, 2) == np.uint64(R.EMPTY)).all()
        assert not backward_raw(np.ones((2, 5, 3), np.float32), sel, zbuf, 3, H, W).any()
        # the same winner table again: farther points on the pixels that nearer points of the first call won
        s = np.arange(0, H * W, 2)
        near, far = R.points_at(s, 1, W)[None], R.points_at(s[::-1], 2, W)[None]
        feat = _feat(1, 3, H, W, seed=1)
        _, _, zb = forward_raw(near, feat)
        assert (words(zb, 1)[0, s] >> np.uint64(32) == np.uint64(R.depth_bits(1))).all()
        reused, fresh = forward_raw(far, feat, zbuf=zb), forward_raw(far, feat)
        for a, b in zip(reused, fresh):
            assert torch.equal(a, b)
        assert (reused[1] >= 0).all() and (words(reused[2], 1)[0, s] >> np.uint64(32) == np.uint64(R.depth_bits(2))).all()
    # H*W not a multiple of 4: 8-byte words and 4-byte floats are read and written one at a time, so the element's alignment is enough
    H, W, C = 3, 5, 3
    cam, _ = R.launch_scene(1, 12, H, W, seed=2)
    mapped, sel, zbuf = forward_raw(cam, _feat(1, C, H, W))
    zoff = torch.zeros(H * W + 1, dtype=torch.int64, device=_dev()); zoff[1:] = zbuf
    goff = torch.full((C * H * W + 1,), NAN, device=_dev())
    gi = torch.tensor(R.integer_cotangent((1, 12, C), seed=4)).to(_dev())
    assert zoff.data_ptr() % 16 == 0 and goff.data_ptr() % 16 == 0
    rc = fusion.load().u3d_zbuffer_fusion_backward(1, 12, C, H, W, _lib.ptr(gi), _lib.ptr(sel), ctypes.c_void_p(zoff.data_ptr() + 8),
                                                   ctypes.c_void_p(goff.data_ptr() + 4), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(goff[1:].cpu().numpy().reshape(1, C, H, W), backward_raw(gi, sel, zbuf, C, H, W))


def test_wrapper_inputs():
    """What fusion.py promises around the kernels: any layout and floating dtype of the feature map, the gradient in the input's dtype,
    intrinsics as anything indexable, and view 0 of a 4-dimensional c2w"""
    from unipre3d_amd.fusion import FeatureFusion
    H, W, C = 8, 12, 5
    pts = R.edge_points(H, W)[:, :3]
    center = torch.tensor(np.stack([pts, pts[::-1]])).to(_dev())
    B, N = center.shape[:2]
    c2w = torch.eye(4, device=_dev()).repeat(B, 1, 1)
    intr = np.zeros((3, 4)); intr[0, 0] = intr[1, 1] = intr[2, 2] = 1.0
    ff = FeatureFusion(torch.nn.Identity())
    gi = torch.tensor(R.integer_cotangent((B, N, C), seed=9)).to(_dev())

    def run(feat, c2w=c2w, intr=intr):
        feat = feat.detach().requires_grad_(True)
        mapped = ff.mapped_features(center, feat, c2w, intr)
        (mapped * gi).sum().backward()
        return mapped.detach(), feat.grad

    half = torch.tensor(_feat(B, C, H, W, seed=8)).to(_dev()).half()
    plain = half.float()                                              # every value is an fp16 value: the casts below are exact
    m0, g0 = run(plain)
    assert m0.dtype == torch.float32 and g0.dtype == torch.float32 and (m0 != 0).any() and (g0 != 0).any()
    cl = plain.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    m1, g1 = run(cl)
    assert torch.equal(m1, m0) and g1.dtype == torch.float32 and torch.equal(g1, g0)
    m2, g2 = run(half)
    assert torch.equal(m2, m0) and g2.dtype == torch.float16 and torch.equal(g2, g0.half()) and torch.equal(g2.float(), g0)
    for form in (torch.tensor(intr), intr.tolist(), torch.tensor(intr, dtype=torch.float32)):
        m3, g3 = run(plain, intr=form)
        assert torch.equal(m3, m0) and torch.equal(g3, g0)
    other = c2w.clone(); other[:, 3, :3] = 5.0                        # view 1 looks elsewhere: it must not be the one used
    m4, g4 = run(plain, c2w=torch.stack([c2w, other], dim=1))
    assert torch.equal(m4, m0) and torch.equal(g4, g0)
    assert not torch.equal(run(plain, c2w=other)[0], m0)


def test_two_runs_are_bit_identical():
    H, W = 8, 12
    cam, _ = R.with_nonfinite(R.edge_points(H, W), H, W)
    feat = _feat(2, 5, H, W)
    a, b = forward_raw(cam, feat), forward_raw(cam, feat)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # backward: with at most two tied points on a pixel there is one add onto one written value, so the order cannot matter
    for H, W in ((8, 12), (9, 7)):
        cam, claims = R.launch_scene(2, 60, H, W, seed=1)
        mapped, sel, zbuf = forward_raw(cam, _feat(2, 5, H, W))
        assert np.unique(sel.cpu().numpy()[0], return_counts=True)[1][1:].max() == 2
        gg = np.random.RandomState(3).randn(2, 60, 5).astype(np.float32)
        assert np.array_equal(backward_raw(gg, sel, zbuf, 5, H, W), backward_raw(gg, sel, zbuf, 5, H, W))


# ---- backward sweeps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (4, 4), (32, 32), (36, 29)])
def test_backward_plane_path(H, W):
    """H*W a multiple of 4 (grad_plane_kernel): H*W / 4 = 1, 4, 256 (one full trip of the 256-thread loop) and 261 (a second, partial trip)"""
    for C in (1, 5):
        for name, cam in R.backward_scenes(2, H, W).items():
            r = check_all(cam, _feat(2, C, H, W, seed=C), seed=H, what=f"{name} C={C}")
            if name == "permutation":                                  # the gradient is a permutation of the cotangent
                assert np.array_equal(np.sort(r["grad_gauss"].reshape(2, C, -1), axis=2), np.sort(r["gauss"].transpose(0, 2, 1), axis=2))
            elif name != "none":
                assert (r["grad_gauss"] != 0).reshape(2, C, -1).any(1).sum() == 2


@pytest.mark.parametrize("H,W", [(1, 1), (3, 3), (15, 17), (1, 257), (7, 37)])
def test_backward_dense_path(H, W):
    """H*W not a multiple of 4 (grad_dense1_kernel<8>): partial channel groups and the last partial block of 256 pixels"""
    for C in (1, 7, 8, 9, 17):
        for name, cam in R.backward_scenes(2, H, W).items():
            r = check_all(cam, _feat(2, C, H, W, seed=C), seed=W, what=f"{name} C={C}")
            if name == "permutation":
                assert np.array_equal(np.sort(r["grad_gauss"].reshape(2, C, -1), axis=2), np.sort(r["gauss"].transpose(0, 2, 1), axis=2))


@pytest.mark.parametrize("B,C", [(65536, 1), (1, 65536)])
def test_backward_refuses_more_than_65535_items_or_channels(B, C):
    """the backward's grids carry B and C in dimensions limited to 65535: the forward runs, the backward returns 2 before any launch"""
    from unipre3d_amd.fusion import _ZBufferGather
    cam = torch.tensor(R.points_at([0], 1, 1)).to(_dev()).repeat(B, 1, 1)
    feat = torch.ones(B, C, 1, 1, device=_dev(), requires_grad=True)
    mapped, sel = _ZBufferGather.apply(cam, feat, *UNIT)
    assert (sel == 0).all() and (mapped == 1).all()
    with pytest.raises(RuntimeError, match=r"u3d_zbuffer_fusion_backward failed with code 2"):
        mapped.sum().backward()
    torch.cuda.synchronize()
    assert feat.grad is None
