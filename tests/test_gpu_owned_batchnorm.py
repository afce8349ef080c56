"""libunipre3d_batchnorm.so writes every element it owns and nothing else: its six compute entry points called directly in the order of a
training step (or of an eval-mode forward + backward), with every pointer inside a poisoned arena (tests/guarded.py), under two
poisons.  Expected values: the module's own wrapper on ordinary tensors, bit for bit (tests/test_gpu_batchnorm.py holds the wrapper to
the reference's fp64 record).

  entry point        owned outputs (none pre-zeroed: they hold the poison before the call)
  u3d_bn_stats       partials (parts, 2C) f64; num_batches_tracked (advanced in place)
  u3d_bn_finalize    block (1 + 2C) f64, mean_invstd (2C), running_mean / running_var (updated in place); once more from a block alone
  u3d_bn_sum         block (1 + 2C) f64, dbeta (C), dgamma (C)
  u3d_bn_apply       y (N, C)
  u3d_bn_bwd_reduce  partials (parts, 2C) f64
  u3d_bn_bwd_apply   dx (N, C), dresidual (N, C)
  u3d_bn_abi_version, u3d_bn_row_chunk   host only: called here for their values

Cases (N, C, act, residual, training, misalign of the row tensors in bytes): three chunks and a tail on the 16-byte path; the same rows 4
bytes off (C % 4 == 0 on the scalar path); C = 100 (scalar, two row lanes) with a ragged last chunk; C = 1024 read 4 bytes off (four
column passes); gelu; eval mode (no statistics pass, the running statistics folded in the prologue).
A pointer 2 bytes off, a null output, C = 1025, N = 0: the call returns 1 or 2 and not one byte of the arena changes."""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

CASES = [(3 * 128 + 5, 32, "relu", True, True, 0), (3 * 128 + 5, 32, "relu", True, True, 4), (77, 100, "none", True, True, 0),
         (40, 1024, "relu", False, True, 4), (300, 12, "gelu", False, True, 0), (200, 32, "relu", True, False, 4), (2, 1, "none", False, True, 0)]
EPS, MOMENTUM, NBT0 = 1e-3, 0.1, 3


def _inputs(N, C, residual):
    rng = np.random.default_rng(N * 7 + C)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return dict(x=f(N, C) * 1.5 + 0.5, res=f(N, C) if residual else None, dy=f(N, C), gamma=f(C) * 0.2 + 1.0, beta=f(C) * 0.3,
                rm=f(C) * 0.3, rv=torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))


def _wrapper(d, act, training):
    from unipre3d_amd import batchnorm
    c = lambda k, grad=False: None if d[k] is None else d[k].clone().cuda().requires_grad_(grad)
    x, res, gamma, beta, rm, rv = c("x", True), c("res", True), c("gamma", True), c("beta", True), c("rm"), c("rv")
    nbt = torch.tensor(NBT0, device="cuda")
    y = batchnorm.batch_norm_act(x, gamma, beta, rm, rv, nbt if training else None, training=training, momentum=MOMENTUM, eps=EPS, act=act,
                                 residual=res)
    y.backward(c("dy"))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=x.grad, dres=None if res is None else res.grad, dgamma=gamma.grad, dbeta=beta.grad, rm=rm, rv=rv,
                nbt=nbt.reshape(1))


@pytest.mark.parametrize("N,C,act,residual,training,mis", CASES)
def test_batchnorm_writes_what_it_owns(N, C, act, residual, training, mis):
    from unipre3d_amd import _lib, batchnorm
    lib = batchnorm.load()
    assert lib.u3d_bn_abi_version() == batchnorm.ABI_VERSION
    chunk = lib.u3d_bn_row_chunk(C)
    assert chunk == batchnorm.row_chunk(C) and lib.u3d_bn_row_chunk(0) == 0 and lib.u3d_bn_row_chunk(1025) == 0
    parts = -(-N // chunk)
    d = _inputs(N, C, residual)
    want = _wrapper(d, act, training)
    A, ev = batchnorm.ACTS[act], int(not training)
    P = _lib.ptr
    f32, f64 = torch.float32, torch.float64

    def case_fn(arena):
        st = _lib.stream_ptr(arena.buf.device)
        x, dy = arena.inp(d["x"], mis, name="x"), arena.inp(d["dy"], mis, name="dy")
        res = arena.inp(d["res"], mis, name="res") if residual else None
        gamma, beta = arena.inp(d["gamma"], 4, name="gamma"), arena.inp(d["beta"], 8, name="beta")
        run = {}
        for k in ("rm", "rv", "rm2", "rv2"):                      # updated in place: owned outputs that start from the module's buffers
            run[k] = arena.out((C,), f32, 4, name=k)
            run[k].copy_(d[k[:2]])
        nbt = arena.out((1,), torch.int64, 8, name="nbt")
        nbt.fill_(NBT0)
        outs = []
        if training:
            partials, block = arena.out((parts, 2 * C), f64, 8, name="partials"), arena.out((1 + 2 * C,), f64, 8, name="block")
            mi = arena.out((2 * C,), f32, 4, name="mean_invstd")
            assert lib.u3d_bn_stats(P(x), N, C, P(nbt), P(partials), st) == 0
            assert lib.u3d_bn_finalize(P(partials), parts, float(N), P(block), C, EPS, MOMENTUM, P(run["rm"]), P(run["rv"]), P(nbt), P(mi), st) == 0
            # the two-step form of the same: the sum alone, then a finalize that reads the block
            block2, mi2 = arena.out((1 + 2 * C,), f64, name="block2"), arena.out((2 * C,), f32, name="mean_invstd2")
            assert lib.u3d_bn_sum(P(partials), parts, C, float(N), P(block2), None, None, st) == 0
            assert lib.u3d_bn_finalize(None, 0, 0.0, P(block2), C, EPS, MOMENTUM, P(run["rm2"]), P(run["rv2"]), P(nbt), P(mi2), st) == 0
            mean, second = mi[:C], mi[C:]
            outs = [partials, block, mi, block2, mi2]
        else:
            mean, second = run["rm"], run["rv"]
        y = arena.out((N, C), f32, mis, name="y")
        assert lib.u3d_bn_apply(P(x), P(res), N, C, A, ev, EPS, P(mean), P(second), P(gamma), P(beta), P(y), st) == 0
        pb, bb = arena.out((parts, 2 * C), f64, 8, name="partials_b"), arena.out((1 + 2 * C,), f64, 8, name="block_b")
        dbeta, dgamma = arena.out((C,), f32, 4, name="dbeta"), arena.out((C,), f32, 8, name="dgamma")
        yb = y if act == "relu" else None
        assert lib.u3d_bn_bwd_reduce(P(dy), P(x), P(yb), N, C, A, ev, EPS, P(mean), P(second), P(gamma), P(beta), P(pb), st) == 0
        assert lib.u3d_bn_sum(P(pb), parts, C, float(N), P(bb), P(dbeta), P(dgamma), st) == 0
        dx = arena.out((N, C), f32, mis, name="dx")
        dres = arena.out((N, C), f32, mis, name="dres") if residual and act != "none" else None
        assert lib.u3d_bn_bwd_apply(P(dy), P(x), P(yb), N, C, A, ev, EPS, P(mean), P(second), P(gamma), P(beta), P(bb) if training else None,
                                    P(dx), P(dres), st) == 0
        named = [y, dx, dgamma, dbeta, run["rm"], run["rv"], nbt, run["rm2"], run["rv2"]]
        return named + ([dres] if dres is not None else []) + [pb, bb] + outs

    run_a, _ = run_twice(case_fn, "cuda", capacity=48 << 20)
    names = ("y", "dx", "dgamma", "dbeta", "rm", "rv", "nbt", "rm", "rv") + (("dres",) if residual and act != "none" else ())
    for got, name in zip(run_a, names):
        if got.is_floating_point():
            assert torch.isfinite(got).all(), name                # the poison (NaN / 1.5e16) is gone everywhere
        w = want[name] if training or name != "nbt" else torch.tensor([NBT0])
        assert same_bits(got, w.detach().cpu().reshape(got.shape)), name
    for got in run_a[len(names):]:
        assert torch.isfinite(got).all()
    if training:                                                  # the one-step and the two-step finalize agree bit for bit
        block, mi, block2, mi2 = run_a[-4:]
        assert same_bits(block, block2) and same_bits(mi, mi2) and block[0].item() == N


@pytest.mark.parametrize("which", ["x_off2", "partials_off4", "y_null", "C1025", "N0", "gelu_residual"])
def test_batchnorm_refuses_and_writes_nothing(which):
    from unipre3d_amd import _lib, batchnorm
    lib = batchnorm.load()
    N, C = 70, 32
    d = _inputs(N, C, True)
    arena = Arena("cuda", 0x5A, 16 << 20)
    P = _lib.ptr
    st = _lib.stream_ptr(arena.buf.device)
    x, res = arena.inp(d["x"], name="x"), arena.inp(d["res"], name="res")
    gamma, beta, rm, rv = (arena.inp(d[k], name=k) for k in ("gamma", "beta", "rm", "rv"))
    parts = -(-N // batchnorm.row_chunk(C))
    partials = arena.out((parts, 2 * C), torch.float64, owned=0, name="partials")
    y = arena.out((N, C), torch.float32, owned=0, name="y")
    big = arena.out((4, 1025), torch.float32, owned=0, name="big")
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    calls = {
        "x_off2": (lambda: lib.u3d_bn_stats(off(x, 2), N - 1, C, None, P(partials), st), 1),
        "partials_off4": (lambda: lib.u3d_bn_stats(P(x), N, C, None, off(partials, 4), st), 1),
        "y_null": (lambda: lib.u3d_bn_apply(P(x), P(res), N, C, 1, 1, EPS, P(rm), P(rv), P(gamma), P(beta), None, st), 1),
        "C1025": (lambda: lib.u3d_bn_apply(P(x), None, 2, 1025, 1, 1, EPS, P(rm), P(rv), P(gamma), P(beta), P(big), st), 2),
        "N0": (lambda: lib.u3d_bn_apply(P(x), None, 0, C, 1, 1, EPS, P(rm), P(rv), P(gamma), P(beta), P(y), st), 1),
        "gelu_residual": (lambda: lib.u3d_bn_apply(P(x), P(res), N, C, 2, 1, EPS, P(rm), P(rv), P(gamma), P(beta), P(y), st), 2),
    }
    fn, code = calls[which]
    assert fn() == code
    torch.cuda.synchronize()
    arena.check_guards()
