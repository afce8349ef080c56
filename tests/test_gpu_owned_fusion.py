"""libunipre3d_fusion.so writes every element it owns and nothing else: its two launching entry points called directly, with every pointer
inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: fusion._ZBufferGather on ordinary tensors AND the scalar
loops of tests/fusion_ref.py, bit for bit (the backward's cotangent is fusion_ref.integer_cotangent, so the sum over tied rows is exact in
any order and the result equals grad_loop).

The forward must initialise `zbuf` itself.  Its "empty" word is all-ones, which is what the 0xFF poison leaves there anyway, so only the 0x5A
run can show a missing clear; zbuf is therefore compared with fusion_ref.winner_words in BOTH runs.  The backward's `grad_features` is
placed uninitialised: the library promises to write every element of it exactly once.

  entry point                   cases
  u3d_zbuffer_fusion_forward    image sizes fusion_ref.SIZES = (6, 9), (9, 6), (8, 12): H < W, H > W, H * W a multiple of 4 (asserted); C = 9,
  u3d_zbuffer_fusion_backward   one past the dense backward's eight channels per thread.  Scenes: "edge" = with_nonfinite(edge_points): B = 2,
                                points behind the camera, outside the image, on half-integer pixels, tied depths, NaN and +inf;
                                tie_scene with 5 tied points, variants plain / nearer_late / farther_early, B = 2, N = 300.
                                Outputs: mapped (B,N,C), sel (B,N), zbuf of exactly u3d_zbuffer_fusion_zbuf_bytes bytes, and
                                grad_features (B,C,H,W), computed from the arena's own sel and zbuf.
  u3d_zbuffer_fusion_backward   (8, 12) only: grad_features, and then zbuf, 4 bytes past a 16-byte boundary.  The call returns 1 and the
                                arena is untouched (grad_features owns no byte in these cases).
"""
import numpy as np
import pytest
import torch

import fusion_ref as R
from guarded import run_twice, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:divide by zero encountered:RuntimeWarning")]
UNIT = (1.0, 1.0, 0.0, 0.0)
C = 9
SCENES = ("edge", "tie_plain", "tie_nearer_late", "tie_farther_early")


def _scene(name, H, W):
    if name == "edge":
        return R.with_nonfinite(R.edge_points(H, W), H, W)[0]
    return R.tie_scene(5, name[4:], 2, 300, H, W)[0]


def _feat(B, H, W):
    return np.random.RandomState(H * W).randn(B, C, H, W).astype(np.float32)


def test_sizes_are_the_three_classes():
    (h0, w0), (h1, w1), (h2, w2) = R.SIZES
    assert h0 < w0 and h1 > w1 and (h0 * w0) % 4 and (h1 * w1) % 4 and (h2 * w2) % 4 == 0


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("H, W", R.SIZES)
def test_zbuffer_fusion_writes_what_it_owns(H, W, scene):
    from unipre3d_amd import _lib, fusion
    lib = fusion.load()
    cam = np.ascontiguousarray(_scene(scene, H, W), dtype=np.float32)
    B, N = cam.shape[:2]
    feat = _feat(B, H, W)
    gm = R.integer_cotangent((B, N, C), seed=N + H)
    zbytes = int(lib.u3d_zbuffer_fusion_zbuf_bytes(B, H, W))
    assert zbytes == B * H * W * 8

    def case(arena):
        cp, ft, g = (arena.inp(torch.from_numpy(a), name=nm) for a, nm in ((cam, "camera_points"), (feat, "image_features"), (gm, "grad_mapped")))
        mapped = arena.out((B, N, C), torch.float32, name="mapped")
        sel = arena.out((B, N), torch.int32, name="sel")
        zbuf = arena.out((zbytes // 8,), torch.int64, name="zbuf")
        gf = arena.out((B, C, H, W), torch.float32, name="grad_features")
        assert zbuf.data_ptr() % 16 == 0 and gf.data_ptr() % 16 == 0
        st = _lib.stream_ptr(gf.device)
        p = _lib.ptr
        assert lib.u3d_zbuffer_fusion_forward(B, N, C, H, W, *UNIT, p(cp), p(ft), p(mapped), p(sel), p(zbuf), st) == 0
        assert lib.u3d_zbuffer_fusion_backward(B, N, C, H, W, p(g), p(sel), p(zbuf), p(gf), st) == 0
        return [mapped, sel, zbuf, gf]

    runs = run_twice(case, "cuda")
    ref_mapped, ref_sel, table = R.zbuffer_loop(cam, feat, *UNIT)
    words = R.winner_words(table, H, W)
    ref_grad = R.grad_loop(gm, ref_sel, B, C, H, W)
    assert np.array_equal(ref_grad.astype(np.float32).astype(np.float64), ref_grad)
    ft = torch.from_numpy(feat).cuda().requires_grad_(True)
    w_mapped, w_sel = fusion._ZBufferGather.apply(torch.from_numpy(cam).cuda(), ft, *UNIT)
    w_mapped.backward(torch.from_numpy(gm).cuda())
    for which, (mapped, sel, zbuf, gf) in zip(("poison 0xFF", "poison 0x5A"), runs):
        assert same_bits(mapped, w_mapped.detach()) and same_bits(sel, w_sel), which
        assert same_bits(mapped, torch.from_numpy(ref_mapped)) and same_bits(sel, torch.from_numpy(ref_sel)), which
        assert np.array_equal(zbuf.numpy().view(np.uint64).reshape(B, H * W), words), which
        assert same_bits(gf, ft.grad) and same_bits(gf, torch.from_numpy(ref_grad.astype(np.float32))), which


@pytest.mark.parametrize("off", ["grad_features", "zbuf"])
def test_backward_refuses_a_misaligned_plane_pointer_before_any_launch(off):
    from unipre3d_amd import _lib, fusion
    lib = fusion.load()
    H, W = R.SIZES[2]
    assert (H * W) % 4 == 0
    cam = np.ascontiguousarray(_scene("tie_plain", H, W), dtype=np.float32)
    B, N = cam.shape[:2]
    _, sel_np, table = R.zbuffer_loop(cam, np.zeros((B, 1, H, W), np.float32), *UNIT)
    words = torch.from_numpy(R.winner_words(table, H, W).view(np.int64).reshape(-1).copy())
    gm = R.integer_cotangent((B, N, C), seed=3)

    def case(arena):
        g, sel = arena.inp(torch.from_numpy(gm), name="grad_mapped"), arena.inp(torch.from_numpy(sel_np), name="sel")
        zbuf = arena.inp(words.view(torch.uint8), misalign=4 if off == "zbuf" else 0, name="zbuf")
        gf = arena.out((B, C, H, W), torch.float32, misalign=4 if off == "grad_features" else 0, name="grad_features")
        arena.own(gf, 0)
        assert (zbuf.data_ptr() % 16, gf.data_ptr() % 16) == ((4, 0) if off == "zbuf" else (0, 4))
        p = _lib.ptr
        assert lib.u3d_zbuffer_fusion_backward(B, N, C, H, W, p(g), p(sel), p(zbuf), p(gf), _lib.stream_ptr(gf.device)) == 1
        return []

    run_twice(case, "cuda")
