"""libunipre3d_batchnorm_cf.so writes every element it owns and nothing else: its four compute entry points called directly in the order
of a training step (or of an eval-mode forward + backward), in the dense and in the pooled form, with every pointer inside a poisoned
arena (tests/guarded.py), under two poisons.  The sum and the finalize between them are libunipre3d_batchnorm.so's (u3d_bn_sum,
u3d_bn_finalize), as in the module.  Expected values: the module's own wrapper on ordinary tensors, bit for bit
(tests/test_gpu_batchnorm_cf.py holds the wrapper to the reference's fp64 record).

  entry point          owned outputs (none pre-zeroed: they hold the poison before the call)
  u3d_bncf_stats       partials (parts, 2C) f64; num_batches_tracked (advanced in place)
  u3d_bncf_apply       dense: y (B, C, L); pooled: pooled and arg in the S layout, (B, C) or (B / S, C, S)
  u3d_bncf_bwd_reduce  partials (parts, 2C) f64, from (dy, x, y) or from (dpooled, x, pooled, arg)
  u3d_bncf_bwd_apply   dx (B, C, L), dresidual (B, C, L): in the pooled form every element once, the zeros included
  u3d_bncf_abi_version, u3d_bncf_plan, u3d_bncf_parts   host only: called here for their values

Cases (B, C, L, act, residual, training, misalign of the (B, C, L) tensors in bytes, pooled, S): K = 24 (6 of 8 lanes) over three batch
chunks and a tail; the same 4 bytes off (one float per lane, 32 lanes); L = 50 (L % 4 != 0); 300 floats per row in two sweeps with C = 5
(a channel tile with an idle row slot); gelu; eval mode; the pooled form with S = 1 and with S = 7, dense and pooled in eval mode; B = 1.
A pointer 2 bytes off, y and pooled both given, C = 1025, B = 0, B % S != 0: the call returns 1 or 2 and not one byte of the arena changes."""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

CASES = [(35, 40, 24, "relu", True, True, 0, False, 1), (35, 40, 24, "relu", True, True, 4, False, 1), (7, 3, 50, "none", True, True, 0, False, 1),
         (9, 5, 300, "relu", False, True, 0, False, 1), (6, 12, 33, "gelu", False, True, 0, False, 1), (20, 8, 32, "relu", True, False, 4, False, 1),
         (35, 40, 24, "relu", True, True, 0, True, 1), (21, 6, 24, "relu", True, True, 4, True, 7), (14, 9, 32, "gelu", False, True, 0, True, 7),
         (12, 8, 24, "none", True, False, 0, True, 1), (1, 1, 2, "none", False, True, 0, False, 1), (1, 2, 1, "relu", False, False, 0, True, 1)]
EPS, MOMENTUM, NBT0 = 1e-5, 0.1, 3


def _inputs(B, C, L, residual):
    rng = np.random.default_rng(B * 7 + C * 3 + L)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return dict(x=f(B, C, L) * 1.5 + 0.5, res=f(B, C, L) if residual else None, dy=f(B, C, L), dpooled=f(B, C), gamma=f(C) * 0.2 + 1.0,
                beta=f(C) * 0.3, rm=f(C) * 0.3, rv=torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))


def _grouped(t, S):
    return t if S == 1 else t.reshape(t.shape[0] // S, S, t.shape[1]).permute(0, 2, 1).contiguous()


def _wrapper(d, act, training, pool, S):
    from unipre3d_amd import batchnorm_cf
    c = lambda k, grad=False: None if d[k] is None else d[k].clone().cuda().requires_grad_(grad)
    x, res, gamma, beta, rm, rv = c("x", True), c("res", True), c("gamma", True), c("beta", True), c("rm"), c("rv")
    nbt = torch.tensor(NBT0, device="cuda")
    out = batchnorm_cf.batch_norm_act_cf(x, gamma, beta, rm, rv, nbt if training else None, training=training, momentum=MOMENTUM, eps=EPS,
                                         act=act, residual=res, pool="max" if pool else None, pool_groups=S, return_arg=pool)
    y, arg = out if pool else (out, None)
    y.backward(_grouped(c("dpooled"), S) if pool else c("dy"))
    torch.cuda.synchronize()
    return dict(y=y.detach(), arg=arg, dx=x.grad, dres=None if res is None else res.grad, dgamma=gamma.grad, dbeta=beta.grad, rm=rm, rv=rv,
                nbt=nbt.reshape(1))


@pytest.mark.parametrize("B,C,L,act,residual,training,mis,pool,S", CASES)
def test_batchnorm_cf_writes_what_it_owns(B, C, L, act, residual, training, mis, pool, S):
    from unipre3d_amd import _lib, batchnorm, batchnorm_cf
    lib, bn = batchnorm_cf.load(), batchnorm.load()
    assert lib.u3d_bncf_abi_version() == batchnorm_cf.ABI_VERSION
    out = [ctypes.c_int() for _ in range(4)]
    assert lib.u3d_bncf_plan(C, L, int(mis == 0), *[ctypes.byref(o) for o in out]) == 0
    p = batchnorm_cf.plan(C, L, mis == 0)
    assert tuple(o.value for o in out) == tuple(p[:4]) and p.vec == (4 if L % 4 == 0 and mis == 0 else 1)
    assert lib.u3d_bncf_plan(1025, L, 1, None, None, None, None) == 2 and lib.u3d_bncf_plan(C, 0, 1, None, None, None, None) == 2
    parts = lib.u3d_bncf_parts(B, C, L)
    assert parts == -(-B // p.batch_chunk) == batchnorm_cf.parts(B, C, L) and lib.u3d_bncf_parts(0, C, L) == 0 and lib.u3d_bncf_parts(B, 1025, L) == 0
    d = _inputs(B, C, L, residual)
    want = _wrapper(d, act, training, pool, S)
    A, ev = batchnorm.ACTS[act], int(not training)
    P = _lib.ptr
    f32, f64 = torch.float32, torch.float64
    pshape = (B, C) if S == 1 else (B // S, C, S)

    def case_fn(arena):
        st = _lib.stream_ptr(arena.buf.device)
        x = arena.inp(d["x"], mis, name="x")
        dy = arena.inp(_grouped(d["dpooled"], S), 4, name="dpooled") if pool else arena.inp(d["dy"], mis, name="dy")
        res = arena.inp(d["res"], mis, name="res") if residual else None
        gamma, beta = arena.inp(d["gamma"], 4, name="gamma"), arena.inp(d["beta"], 8, name="beta")
        run = {}
        for k in ("rm", "rv"):                                    # updated in place: owned outputs that start from the module's buffers
            run[k] = arena.out((C,), f32, 4, name=k)
            run[k].copy_(d[k])
        nbt = arena.out((1,), torch.int64, 8, name="nbt")
        nbt.fill_(NBT0)
        outs = []
        if training:
            partials, block = arena.out((parts, 2 * C), f64, 8, name="partials"), arena.out((1 + 2 * C,), f64, 8, name="block")
            mi = arena.out((2 * C,), f32, 4, name="mean_invstd")
            assert lib.u3d_bncf_stats(P(x), B, C, L, P(nbt), P(partials), st) == 0
            assert bn.u3d_bn_finalize(P(partials), parts, float(B * L), P(block), C, EPS, MOMENTUM, P(run["rm"]), P(run["rv"]), P(nbt), P(mi), st) == 0
            mean, second = mi[:C], mi[C:]
            outs = [partials, block, mi]
        else:
            mean, second = run["rm"], run["rv"]
        if pool:
            y, arg = arena.out(pshape, f32, 4, name="pooled"), arena.out(pshape, torch.int32, 8, name="arg")
            assert lib.u3d_bncf_apply(P(x), P(res), B, C, L, A, ev, EPS, P(mean), P(second), P(gamma), P(beta), None, P(y), P(arg), S, st) == 0
        else:
            y, arg = arena.out((B, C, L), f32, mis, name="y"), None
            assert lib.u3d_bncf_apply(P(x), P(res), B, C, L, A, ev, EPS, P(mean), P(second), P(gamma), P(beta), P(y), None, None, 1, st) == 0
        pb, bb = arena.out((parts, 2 * C), f64, 8, name="partials_b"), arena.out((1 + 2 * C,), f64, 8, name="block_b")
        dbeta, dgamma = arena.out((C,), f32, 4, name="dbeta"), arena.out((C,), f32, 8, name="dgamma")
        yb = y if act == "relu" else None
        assert lib.u3d_bncf_bwd_reduce(P(dy), P(x), P(yb), P(arg), B, C, L, A, ev, EPS, P(mean), P(second), P(gamma), P(beta), S, P(pb), st) == 0
        assert bn.u3d_bn_sum(P(pb), parts, C, float(B * L), P(bb), P(dbeta), P(dgamma), st) == 0
        dx = arena.out((B, C, L), f32, mis, name="dx")
        dres = arena.out((B, C, L), f32, mis, name="dres") if residual and (act != "none" or pool) else None
        assert lib.u3d_bncf_bwd_apply(P(dy), P(x), P(yb), P(arg), B, C, L, A, ev, EPS, P(mean), P(second), P(gamma), P(beta),
                                      P(bb) if training else None, S, P(dx), P(dres), st) == 0
        named = [y, dx, dgamma, dbeta, run["rm"], run["rv"], nbt] + ([arg] if pool else [])
        return named + ([dres] if dres is not None else []) + [pb, bb] + outs

    run_a, _ = run_twice(case_fn, "cuda", capacity=48 << 20)
    names = ("y", "dx", "dgamma", "dbeta", "rm", "rv", "nbt") + (("arg",) if pool else ()) + (("dres",) if residual and (act != "none" or pool) else ())
    for got, name in zip(run_a, names):
        if got.is_floating_point():
            assert torch.isfinite(got).all(), name                # the poison (NaN / 1.5e16) is gone everywhere
        w = want[name] if training or name != "nbt" else torch.tensor([NBT0])
        assert same_bits(got, w.detach().cpu().reshape(got.shape)), name
    for got in run_a[len(names):]:
        assert torch.isfinite(got).all()
    if pool:                                                      # g is zero off l = arg: B C non-zero elements of dresidual at the most
        arg = run_a[names.index("arg")]
        assert int(arg.min()) >= 0 and int(arg.max()) < L
        if "dres" in names:
            assert int((run_a[names.index("dres")] != 0).sum()) <= B * C


@pytest.mark.parametrize("which", ["x_off2", "partials_off4", "y_and_pooled", "neither", "arg_null", "C1025", "B0", "gelu_residual", "S_not_dividing"])
def test_batchnorm_cf_refuses_and_writes_nothing(which):
    from unipre3d_amd import _lib, batchnorm_cf
    lib = batchnorm_cf.load()
    B, C, L = 10, 8, 24
    d = _inputs(B, C, L, True)
    arena = Arena("cuda", 0x5A, 16 << 20)
    P = _lib.ptr
    st = _lib.stream_ptr(arena.buf.device)
    x, res = arena.inp(d["x"], name="x"), arena.inp(d["res"], name="res")
    gamma, beta, rm, rv = (arena.inp(d[k], name=k) for k in ("gamma", "beta", "rm", "rv"))
    partials = arena.out((batchnorm_cf.parts(B, C, L), 2 * C), torch.float64, owned=0, name="partials")
    y = arena.out((B, C, L), torch.float32, owned=0, name="y")
    pooled, arg = arena.out((B, C), torch.float32, owned=0, name="pooled"), arena.out((B, C), torch.int32, owned=0, name="arg")
    big = arena.out((2, 1025, 4), torch.float32, owned=0, name="big")
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    tail = (EPS, P(rm), P(rv), P(gamma), P(beta))
    calls = {
        "x_off2": (lambda: lib.u3d_bncf_stats(off(x, 2), B - 1, C, L, None, P(partials), st), 1),
        "partials_off4": (lambda: lib.u3d_bncf_stats(P(x), B, C, L, None, off(partials, 4), st), 1),
        "y_and_pooled": (lambda: lib.u3d_bncf_apply(P(x), P(res), B, C, L, 1, 1, *tail, P(y), P(pooled), P(arg), 1, st), 1),
        "neither": (lambda: lib.u3d_bncf_apply(P(x), P(res), B, C, L, 1, 1, *tail, None, None, None, 1, st), 1),
        "arg_null": (lambda: lib.u3d_bncf_apply(P(x), P(res), B, C, L, 1, 1, *tail, None, P(pooled), None, 1, st), 1),
        "C1025": (lambda: lib.u3d_bncf_apply(P(x), None, 2, 1025, 4, 1, 1, *tail, P(big), None, None, 1, st), 2),
        "B0": (lambda: lib.u3d_bncf_apply(P(x), None, 0, C, L, 1, 1, *tail, P(y), None, None, 1, st), 1),
        "gelu_residual": (lambda: lib.u3d_bncf_apply(P(x), P(res), B, C, L, 2, 1, *tail, P(y), None, None, 1, st), 2),
        "S_not_dividing": (lambda: lib.u3d_bncf_apply(P(x), P(res), B, C, L, 1, 1, *tail, None, P(pooled), P(arg), 3, st), 2),
    }
    fn, code = calls[which]
    assert fn() == code
    torch.cuda.synchronize()
    arena.check_guards()
