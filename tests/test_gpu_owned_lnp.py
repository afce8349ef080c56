"""libunipre3d_lnp.so writes every element it owns and nothing else: its three compute entry points called directly, with every pointer
inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors, bit for bit
(tests/test_gpu_lnp.py holds the wrapper to the reference's fp64 record), and tests/lnp_ref.py's inverse lists.

  entry point          cases (B, G, C, K)
  u3d_lnp_neighbours   (1, 1024, 4, 2): the most rows, the fewest channels (one lane of a wave loads);  (1, 7, 260, 3): a lane's second
  u3d_lnp_fwd          float4 group, a workgroup with one idle wave;  (1, 33, 512, 32): the largest C and K;  (2, 514, 4, 2): x read
  u3d_lnp_bwd          through a batch stride of (G + 1) C, and more rows than the 256 partials of mu and s take in one pass.
                       Outputs: ptr (B,G+1), ent (B,G K), out (B,G,2C), lse (B,G,C), stats (4), dx (B,G,C), dalpha and dbeta (2C), and the
                       scratch of each pass, whose every byte u3d_lnp_scratch_bytes counts is written; none pre-zeroed: they hold the
                       poison before the call.
                       A pointer 4 bytes past a 16-byte boundary: the call returns 1 and not one byte of the arena changes.
"""
import numpy as np
import pytest
import torch

import lnp_ref as LR
from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1024, 4, 2), (1, 7, 260, 3), (1, 33, 512, 32), (2, 514, 4, 2)]
EPS = 1e-5


def _inputs(B, G, C, K, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, G, (B, G, K)).astype(np.int32)
    idx[:, :, 0] = np.arange(G)
    idx[0, G // 2, 1] = -1                                   # one index out of range: never dereferenced
    return (torch.from_numpy(rng.uniform(-1, 1, (B, G + 1, C)).astype(np.float32)), torch.from_numpy(idx),
            torch.from_numpy(rng.uniform(0.5, 1.5, 2 * C).astype(np.float32)), torch.from_numpy(rng.uniform(-0.5, 0.5, 2 * C).astype(np.float32)),
            torch.from_numpy(rng.uniform(-1, 1, (B, G, 2 * C)).astype(np.float32)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lnp_writes_what_it_owns(shape):
    from unipre3d_amd import _lib, lnp
    lib = lnp.load()
    B, G, C, K = shape
    full_cpu, idx_cpu, alpha_cpu, beta_cpu, dout_cpu = _inputs(B, G, C, K, G + C)
    xs = (G + 1) * C                                         # x is rows 1 .. G of every batch element of `full`

    full = full_cpu.cuda().requires_grad_(True)
    a, b = alpha_cpu.cuda().requires_grad_(True), beta_cpu.cuda().requires_grad_(True)
    nb = lnp.neighbours_from_idx(idx_cpu.cuda())
    out = lnp.local_norm_pool(full[:, 1:, :], nb, a, b)
    lse, stats = out.grad_fn.saved_tensors[4:6]
    out.backward(dout_cpu.cuda())
    out_cpu, lse_cpu, stats_cpu = out.detach().cpu(), lse.cpu(), stats.cpu()
    ptr_ref, ent_ref = LR.inverse_lists(idx_cpu.numpy())
    fwd_bytes, bwd_bytes = lib.u3d_lnp_scratch_bytes(B, G, K, C, 0), lib.u3d_lnp_scratch_bytes(B, G, K, C, 1)
    assert fwd_bytes > 0 and bwd_bytes > 0 and fwd_bytes % 16 == 0 and bwd_bytes % 16 == 0

    def case_fn(arena):
        fl, idx = arena.inp(full_cpu, name="x"), arena.inp(idx_cpu, name="idx")
        al, be, dout = arena.inp(alpha_cpu, name="alpha"), arena.inp(beta_cpu, name="beta"), arena.inp(dout_cpu, name="dout")
        x_ptr = _lib.ptr(fl[:, 1:, :])
        st = _lib.stream_ptr(fl.device)
        ptr = arena.out((B, G + 1), torch.int32, name="ptr")
        ent = arena.out((B, G * K), torch.int32, name="ent")
        assert lib.u3d_lnp_neighbours(_lib.ptr(idx), _lib.ptr(ptr), _lib.ptr(ent), B, G, K, st) == 0
        o = arena.out((B, G, 2 * C), torch.float32, name="out")
        l = arena.out((B, G, C), torch.float32, name="lse")
        s = arena.out((4,), torch.float32, name="stats")
        sf = arena.out((fwd_bytes,), torch.uint8, name="scratch_fwd")
        assert lib.u3d_lnp_fwd(x_ptr, xs, _lib.ptr(idx), _lib.ptr(al), _lib.ptr(be), _lib.ptr(o), _lib.ptr(l), _lib.ptr(s), _lib.ptr(sf),
                               B, G, K, C, EPS, st) == 0
        o_in, l_in, s_in = arena.inp(out_cpu, name="out_in"), arena.inp(lse_cpu, name="lse_in"), arena.inp(stats_cpu, name="stats_in")
        p_in, e_in = arena.inp(torch.from_numpy(ptr_ref), name="ptr_in"), arena.inp(torch.from_numpy(ent_ref), name="ent_in")
        dx = arena.out((B, G, C), torch.float32, name="dx")
        da = arena.out((2 * C,), torch.float32, name="dalpha")
        db = arena.out((2 * C,), torch.float32, name="dbeta")
        sb = arena.out((bwd_bytes,), torch.uint8, name="scratch_bwd")
        assert lib.u3d_lnp_bwd(x_ptr, xs, _lib.ptr(idx), _lib.ptr(p_in), _lib.ptr(e_in), _lib.ptr(al), _lib.ptr(be), _lib.ptr(o_in),
                               _lib.ptr(l_in), _lib.ptr(s_in), _lib.ptr(dout), _lib.ptr(dx), _lib.ptr(da), _lib.ptr(db), _lib.ptr(sb),
                               B, G, K, C, st) == 0
        return [ptr, ent, o, l, s, dx, da, db, sf, sb]

    run, _ = run_twice(case_fn, "cuda")
    want = (torch.from_numpy(ptr_ref), torch.from_numpy(ent_ref), out.detach(), lse, stats, full.grad[:, 1:, :].contiguous(), a.grad, b.grad)
    for got, exp, name in zip(run, want, ("ptr", "ent", "out", "lse", "stats", "dx", "dalpha", "dbeta")):
        if got.is_floating_point():
            assert torch.isfinite(got).all(), name            # the poison (NaN / 1.5e16) is gone everywhere
        assert same_bits(got, exp), name
    assert not full.grad[:, 0].any()


@pytest.mark.parametrize("which", ["x", "idx", "ptr", "ent", "alpha", "out", "lse", "stats", "dout", "dx", "dbeta", "scratch"])
def test_lnp_refuses_a_pointer_off_16_bytes_and_writes_nothing(which):
    from unipre3d_amd import _lib, lnp
    lib = lnp.load()
    B, G, C, K = SHAPES[1]
    full_cpu, idx_cpu, alpha_cpu, beta_cpu, dout_cpu = _inputs(B, G, C, K, 3)
    arena = Arena("cuda", 0x5A)
    off = lambda name: 4 if name == which else 0
    x = arena.inp(full_cpu[:, 1:, :], off("x"), name="x")
    idx = arena.inp(idx_cpu, off("idx"), name="idx")
    al, be = arena.inp(alpha_cpu, off("alpha"), name="alpha"), arena.inp(beta_cpu, name="beta")
    dout = arena.inp(dout_cpu, off("dout"), name="dout")
    ptr_ref, ent_ref = LR.inverse_lists(idx_cpu.numpy())
    # owned=0: nothing of these outputs may be written by a refused call
    ptr = arena.out((B, G + 1), torch.int32, off("ptr"), owned=0, name="ptr")
    ent = arena.out((B, G * K), torch.int32, off("ent"), owned=0, name="ent")
    o = arena.out((B, G, 2 * C), torch.float32, off("out"), owned=0, name="out")
    l = arena.out((B, G, C), torch.float32, off("lse"), owned=0, name="lse")
    s = arena.out((4,), torch.float32, off("stats"), owned=0, name="stats")
    dx = arena.out((B, G, C), torch.float32, off("dx"), owned=0, name="dx")
    da = arena.out((2 * C,), torch.float32, owned=0, name="dalpha")
    db = arena.out((2 * C,), torch.float32, off("dbeta"), owned=0, name="dbeta")
    sc = arena.out((lib.u3d_lnp_scratch_bytes(B, G, K, C, 1),), torch.uint8, off("scratch"), owned=0, name="scratch")
    st = _lib.stream_ptr(o.device)
    moved = {"x": x, "idx": idx, "ptr": ptr, "ent": ent, "alpha": al, "out": o, "lse": l, "stats": s, "dout": dout, "dx": dx, "dbeta": db,
             "scratch": sc}[which]
    assert moved.data_ptr() % 16 == 4
    codes = {}
    if which in ("idx", "ptr", "ent"):
        codes["neighbours"] = lib.u3d_lnp_neighbours(_lib.ptr(idx), _lib.ptr(ptr), _lib.ptr(ent), B, G, K, st)
    if which in ("x", "idx", "alpha", "out", "lse", "stats", "scratch"):
        codes["fwd"] = lib.u3d_lnp_fwd(_lib.ptr(x), G * C, _lib.ptr(idx), _lib.ptr(al), _lib.ptr(be), _lib.ptr(o), _lib.ptr(l), _lib.ptr(s),
                                       _lib.ptr(sc), B, G, K, C, EPS, st)
    # (the backward reads out, lse, stats, ptr and ent: the same placements serve, their bytes are never looked at by a refused call)
    codes["bwd"] = lib.u3d_lnp_bwd(_lib.ptr(x), G * C, _lib.ptr(idx), _lib.ptr(ptr), _lib.ptr(ent), _lib.ptr(al), _lib.ptr(be), _lib.ptr(o),
                                   _lib.ptr(l), _lib.ptr(s), _lib.ptr(dout), _lib.ptr(dx), _lib.ptr(da), _lib.ptr(db), _lib.ptr(sc),
                                   B, G, K, C, st)
    torch.cuda.synchronize()
    assert set(codes.values()) == {1}, codes
    arena.check_guards()
