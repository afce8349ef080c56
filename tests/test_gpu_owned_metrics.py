"""libunipre3d_metrics.so writes every element it owns and nothing else: its entry points called directly, with every pointer inside a
poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors, bit for bit
(tests/test_gpu_metrics.py holds the wrapper to the fp64 restatement).

  entry point                 cases
  u3d_metrics_forward         (N, C, H, W) = (2, 3, 33, 35): 2 x 2 tiles of 32 x 32 per plane, the last one 1 x 3 pixels; (1, 1, 1, 1);
                              each with dmaps and with dmaps = NULL.  `partial` (scratch) is an owned output: every tile writes its row.
  u3d_metrics_ssim_backward   the same two shapes
"""
import numpy as np
import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 33, 35), (1, 1, 1, 1)]


def _images(shape):
    rng = np.random.default_rng(sum(shape))
    a = torch.from_numpy(rng.random(shape, dtype=np.float32))
    b = torch.from_numpy(rng.random(shape, dtype=np.float32))
    if shape[0] > 1:
        b[1] = 0.0            # all_zero takes both values
    return a, b


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_writes_what_it_owns(shape, save):
    from unipre3d_amd import _lib, metrics
    n, c, h, w = shape
    a_cpu, b_cpu = _images(shape)
    lib = metrics.load()
    tiles = lib.u3d_metrics_tiles(c, h, w)
    assert tiles == c * -(-h // 32) * -(-w // 32)

    def case(arena):
        a, b = arena.inp(a_cpu, name="img1"), arena.inp(b_cpu, name="img2")
        partial = arena.out((n * tiles, 3), torch.float32, name="partial")
        ssim, sqsum = arena.out((n,), torch.float32, name="ssim"), arena.out((n,), torch.float32, name="sqsum")
        all_zero = arena.out((n,), torch.int32, name="all_zero")
        dmaps = arena.out((3, n, c, h, w), torch.float32, name="dmaps") if save else None
        assert lib.u3d_metrics_forward(n, c, h, w, _lib.ptr(a), _lib.ptr(b), _lib.ptr(partial), _lib.ptr(ssim), _lib.ptr(sqsum),
                                       _lib.ptr(all_zero), _lib.ptr(dmaps), _lib.stream_ptr(a.device)) == 0
        return [ssim, sqsum, all_zero, partial] + ([dmaps] if save else [])

    run, _ = run_twice(case, "cuda")
    want = metrics._forward(torch.device("cuda:0"), a_cpu.cuda(), b_cpu.cuda(), save)
    for got, exp in zip(run[:3] + run[4:], [w_ for w_ in want if w_ is not None]):
        assert same_bits(got, exp)
    assert torch.isfinite(run[3]).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_ssim_backward_writes_what_it_owns(shape):
    from unipre3d_amd import _lib, metrics
    n, c, h, w = shape
    a_cpu, b_cpu = _images(shape)
    weight_cpu = torch.linspace(-1.0, 2.0, n)
    a_dev = a_cpu.cuda().requires_grad_(True)
    dmaps_cpu = metrics._forward(a_dev.device, a_dev.detach(), b_cpu.cuda(), True)[3].cpu()
    (metrics.ssim(a_dev, b_cpu.cuda(), size_average=False) * weight_cpu.cuda()).sum().backward()

    def case(arena):
        a, b = arena.inp(a_cpu, name="img1"), arena.inp(b_cpu, name="img2")
        dmaps, weight = arena.inp(dmaps_cpu, name="dmaps"), arena.inp(weight_cpu, name="weight")
        dimg1 = arena.out(shape, torch.float32, name="dimg1")
        assert metrics.load().u3d_metrics_ssim_backward(n, c, h, w, _lib.ptr(a), _lib.ptr(b), _lib.ptr(dmaps), _lib.ptr(weight),
                                                        _lib.ptr(dimg1), _lib.stream_ptr(a.device)) == 0
        return [dimg1]

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], a_dev.grad)
