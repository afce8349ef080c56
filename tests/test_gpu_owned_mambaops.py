"""libunipre3d_mambaops.so writes every element it owns and nothing else: its entry points called directly, with every pointer inside a
poisoned arena (tests/guarded.py), under two poisons.  Expected values: the modules' own wrappers on ordinary tensors, bit for bit
(tests/test_gpu_mambaops.py holds the wrappers to the fp64 restatement).

  entry point        cases
  u3d_cconv_fwd      (B, D, L) = (2, 5, 3), (2, 5, 65), (2, 5, 257): a row shorter than a wave, one step into the second lane group, one
  u3d_cconv_bwd      step past four 64-lane loads; W = 4 and W = 2 (dweight (D, W): exactly W taps per channel), and once W = 3 at
                     (1, 3, 130), two steps into the third lane group; with bias and without (bias, dbias NULL); x dense, and x as the
                     second half of a (B, 2D, L) placement through the strides, the first half holding other data.  The backward's
                     scratch is a guarded placement, 256-byte aligned.
  u3d_addnorm_fwd    (M, N) = (5, 4), (5, 65), (5, 384): one float4 per row, a row with a one-element tail, six float4 per lane; and
  u3d_addnorm_bwd    the ends of the range, (2, 1) and (3, 1024) (sixteen dwords or four float4 per lane); every float pointer at
                     misalign 0 (the float4 kernels for N % 4 == 0) and at misalign 4 (the dword kernels); LayerNorm and RMSNorm (mean
                     NULL); with residual, bias, r_out and dres, and with all of them NULL (then dbias is NULL too).
"""
import ctypes

import numpy as np
import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu


def _randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("B, D, L, W", [(2, 5, 3, 4), (2, 5, 3, 2), (2, 5, 65, 4), (2, 5, 65, 2), (2, 5, 257, 4), (2, 5, 257, 2), (1, 3, 130, 3)])
def test_cconv_writes_what_it_owns(B, D, L, W, has_bias, strided):
    from unipre3d_amd import _lib, causal_conv1d
    lib = causal_conv1d.load()
    rng = np.random.default_rng(B * 1000 + D * 100 + L + W)
    xz_cpu = _randn(rng, B, 2 * D, L)
    xz_cpu[:, :D] *= 1e3                                  # the half the kernel must not read
    x_cpu = xz_cpu[:, D:].contiguous()
    w_cpu, b_cpu, dout_cpu = _randn(rng, D, W), (_randn(rng, D) if has_bias else None), _randn(rng, B, D, L)
    nbytes = int(lib.u3d_cconv_bwd_scratch_bytes(B, D))

    def case(arena):
        if strided:
            xz = arena.inp(xz_cpu, name="xz")
            x_ptr, sb, sc = ctypes.c_void_p(xz.data_ptr() + D * L * 4), 2 * D * L, L
        else:
            x = arena.inp(x_cpu, name="x")
            x_ptr, sb, sc = _lib.ptr(x), D * L, L
        w = arena.inp(w_cpu, name="weight")
        b = arena.inp(b_cpu, name="bias") if has_bias else None
        dout = arena.inp(dout_cpu, name="dout")
        out = arena.out((B, D, L), torch.float32, name="out")
        dx, dw = arena.out((B, D, L), torch.float32, name="dx"), arena.out((D, W), torch.float32, name="dweight")
        db = arena.out((D,), torch.float32, name="dbias") if has_bias else None
        scratch = arena.out((max(nbytes, 1),), torch.uint8, name="scratch")
        assert scratch.data_ptr() % 256 == 0
        st = _lib.stream_ptr(w.device)
        assert lib.u3d_cconv_fwd(x_ptr, _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), sb, sc, B, D, L, W, 1, st) == 0
        assert lib.u3d_cconv_bwd(x_ptr, _lib.ptr(w), _lib.ptr(b), _lib.ptr(dout), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(scratch),
                                 nbytes, sb, sc, B, D, L, W, 1, st) == 0
        return [out, dx, dw] + ([db] if has_bias else [])

    run, _ = run_twice(case, "cuda")
    x, w = x_cpu.cuda().requires_grad_(True), w_cpu.cuda().requires_grad_(True)
    b = b_cpu.cuda().requires_grad_(True) if has_bias else None
    out = causal_conv1d.causal_conv1d_fn(x, w, b, "silu")
    out.backward(dout_cpu.cuda())
    want = [out.detach(), x.grad, w.grad] + ([b.grad] if has_bias else [])
    for got, exp, name in zip(run, want, ("out", "dx", "dweight", "dbias")):
        assert same_bits(got, exp), name


def _on_device(t, misalign):
    """A contiguous device copy of t whose first byte lies `misalign` bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + misalign // 4, dtype=torch.float32, device="cuda")
    view = buf[misalign // 4:].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("is_rms", [False, True])
@pytest.mark.parametrize("M, N, misalign", [(5, 4, 0), (5, 4, 4), (5, 65, 0), (5, 384, 0), (5, 384, 4), (2, 1, 0), (3, 1024, 0), (3, 1024, 4)])
def test_addnorm_writes_what_it_owns(M, N, misalign, is_rms, full):
    from unipre3d_amd import _lib, causal_conv1d, layernorm
    lib = causal_conv1d.load()
    rng = np.random.default_rng(M * 1000 + N + misalign)
    x_cpu, w_cpu, dy_cpu = _randn(rng, M, N) + 0.5, _randn(rng, N), _randn(rng, M, N)
    res_cpu, b_cpu, dres_cpu = (_randn(rng, M, N), _randn(rng, N), _randn(rng, M, N)) if full else (None, None, None)
    eps = 1e-5
    nbytes = int(lib.u3d_addnorm_bwd_scratch_bytes(M, N))

    # the wrapper on ordinary tensors: what the forward saves is what the backward call below is given
    # (at misalign 4 x and weight are handed to the wrapper 4 bytes past a 16-byte boundary as well, so that it takes the same dword
    # kernels: the float4 kernels add a row's elements in another order, and their sums differ in the last bit)
    x, w = _on_device(x_cpu, misalign).requires_grad_(True), _on_device(w_cpu, misalign).requires_grad_(True)
    assert x.data_ptr() % 16 == misalign and w.data_ptr() % 16 == misalign and x.is_contiguous()
    b = b_cpu.cuda().requires_grad_(True) if full else None
    res = res_cpu.cuda() if full else None
    ret = layernorm.layer_norm_fn(x, w, b, res, eps, prenorm=full, is_rms_norm=is_rms)
    y, r = ret if full else (ret, None)
    r_saved, _, mean_saved, rstd_saved = y.grad_fn.saved_tensors
    if full:
        torch.autograd.backward([y, r], [dy_cpu.cuda(), dres_cpu.cuda()])
    else:
        y.backward(dy_cpu.cuda())
    r_cpu = r_saved.detach().cpu()
    mean_cpu = None if is_rms else mean_saved.cpu()
    rstd_cpu = rstd_saved.cpu()

    def case(arena):
        a = misalign
        xd, wd = arena.inp(x_cpu, a, name="x"), arena.inp(w_cpu, a, name="weight")
        resd = arena.inp(res_cpu, a, name="residual") if full else None
        bd = arena.inp(b_cpu, a, name="bias") if full else None
        yd = arena.out((M, N), torch.float32, a, name="y")
        rd = arena.out((M, N), torch.float32, a, name="r_out") if full else None
        meand = None if is_rms else arena.out((M,), torch.float32, a, name="mean")
        rstdd = arena.out((M,), torch.float32, a, name="rstd")
        st = _lib.stream_ptr(xd.device)
        assert lib.u3d_addnorm_fwd(_lib.ptr(xd), _lib.ptr(resd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(yd), _lib.ptr(rd), _lib.ptr(meand),
                                   _lib.ptr(rstdd), M, N, eps, int(is_rms), st) == 0
        assert misalign == 0 or all(t.data_ptr() % 16 == 4 for t in (xd, wd, yd))
        # backward: from the wrapper's saved tensors, so that it does not depend on the forward call above
        dyd, r_in = arena.inp(dy_cpu, a, name="dy"), arena.inp(r_cpu, a, name="r")
        dresd = arena.inp(dres_cpu, a, name="dres") if full else None
        mean_in = None if is_rms else arena.inp(mean_cpu, a, name="mean_in")
        rstd_in = arena.inp(rstd_cpu, a, name="rstd_in")
        dxd, dwd = arena.out((M, N), torch.float32, a, name="dx"), arena.out((N,), torch.float32, a, name="dweight")
        dbd = arena.out((N,), torch.float32, a, name="dbias") if full else None
        scratch = arena.out((max(nbytes, 1),), torch.uint8, name="scratch")
        assert scratch.data_ptr() % 256 == 0
        assert lib.u3d_addnorm_bwd(_lib.ptr(dyd), _lib.ptr(dresd), _lib.ptr(r_in), _lib.ptr(wd), _lib.ptr(mean_in), _lib.ptr(rstd_in),
                                   _lib.ptr(dxd), _lib.ptr(dwd), _lib.ptr(dbd), _lib.ptr(scratch), nbytes, M, N, int(is_rms), st) == 0
        return [t for t in (yd, rstdd, dxd, dwd, rd, meand, dbd) if t is not None]

    run, _ = run_twice(case, "cuda")
    want = [y.detach(), rstd_saved, x.grad, w.grad, r.detach() if full else None, mean_saved if not is_rms else None, b.grad if full else None]
    names = ("y", "rstd", "dx", "dweight", "r_out", "mean", "dbias")
    pairs = [(n, e) for n, e in zip(names, want) if e is not None]
    assert len(pairs) == len(run)
    for got, (name, exp) in zip(run, pairs):
        assert same_bits(got, exp.reshape(got.shape)), name
