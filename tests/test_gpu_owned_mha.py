"""libunipre3d_mha.so writes every element it owns and nothing else: its two entry points called directly, with every pointer inside a
poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors, bit for bit
(tests/test_gpu_mha.py holds the wrapper to the reference's fp64 record).

  entry point   cases (B, N, H)
  u3d_mha_fwd   (2, 17, 3): one partial key block, one query wave with one row in its second 16;  (1, 65, 1): a full key block and one
  u3d_mha_bwd   of a single row, a second workgroup whose one live wave has one row;  (1, 129, 2): the reference's token count;
                (1, 64, 2): full blocks only -- the host code has one dispatch class (one grid shape per kernel), the kernels two
                key-block forms (full, partial).
                Outputs: out (B,N,H,64), lse (B,H,N), dqkv (B,N,3,H,64), none pre-zeroed: they hold the poison before the call.
                qkv, out, dout or dqkv 4 bytes past a 16-byte boundary: the call returns 1 and not one byte of the arena changes.
"""
import numpy as np
import pytest
import torch

from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

D = 64
SHAPES = [(2, 17, 3), (1, 65, 1), (1, 129, 2), (1, 64, 2)]


def _inputs(B, N, H, seed):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.standard_normal((B, N, 3, H, D)).astype(np.float32)),
            torch.from_numpy(rng.standard_normal((B, N, H, D)).astype(np.float32)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mha_writes_what_it_owns(shape):
    from unipre3d_amd import _lib, mha
    lib = mha.load()
    B, N, H = shape
    qkv_cpu, dout_cpu = _inputs(B, N, H, N)
    scale = float(D ** -0.5)

    q = qkv_cpu.cuda().requires_grad_(True)
    out = mha.attention_qkvpacked(q)
    lse = out.grad_fn.saved_tensors[2]
    out.backward(dout_cpu.cuda())
    out_cpu, lse_cpu = out.detach().cpu(), lse.cpu()

    def case_fn(arena):
        qkv, dout = arena.inp(qkv_cpu, name="qkv"), arena.inp(dout_cpu, name="dout")
        o = arena.out((B, N, H, D), torch.float32, name="out")
        l = arena.out((B, H, N), torch.float32, name="lse")
        st = _lib.stream_ptr(o.device)
        assert lib.u3d_mha_fwd(_lib.ptr(qkv), _lib.ptr(o), _lib.ptr(l), B, N, H, D, scale, st) == 0
        o_in, l_in = arena.inp(out_cpu, name="out_in"), arena.inp(lse_cpu, name="lse_in")
        dqkv = arena.out((B, N, 3, H, D), torch.float32, name="dqkv")
        assert lib.u3d_mha_bwd(_lib.ptr(qkv), _lib.ptr(o_in), _lib.ptr(dout), _lib.ptr(l_in), _lib.ptr(dqkv), B, N, H, D, scale, st) == 0
        return [o, l, dqkv]

    run, _ = run_twice(case_fn, "cuda")
    for got, exp, name in zip(run, (out.detach(), lse, q.grad), ("out", "lse", "dqkv")):
        assert torch.isfinite(got).all(), name        # the poison (NaN / 1.5e16) is gone everywhere
        assert same_bits(got, exp), name


@pytest.mark.parametrize("which", ["qkv", "out", "dout", "dqkv"])
def test_mha_refuses_a_pointer_off_16_bytes_and_writes_nothing(which):
    from unipre3d_amd import _lib, mha
    lib = mha.load()
    B, N, H = SHAPES[0]
    qkv_cpu, dout_cpu = _inputs(B, N, H, 3)
    scale = float(D ** -0.5)
    arena = Arena("cuda", 0x5A)
    off = lambda name: 4 if name == which else 0
    qkv, dout = arena.inp(qkv_cpu, off("qkv"), name="qkv"), arena.inp(dout_cpu, off("dout"), name="dout")
    o_in = arena.inp(torch.zeros(B, N, H, D), off("out"), name="out_in")
    l_in = arena.inp(torch.zeros(B, H, N), name="lse_in")
    # owned=0: nothing of these outputs may be written by a refused call
    o = arena.out((B, N, H, D), torch.float32, off("out"), owned=0, name="out")
    l = arena.out((B, H, N), torch.float32, owned=0, name="lse")
    dqkv = arena.out((B, N, 3, H, D), torch.float32, off("dqkv"), owned=0, name="dqkv")
    st = _lib.stream_ptr(o.device)
    assert {"qkv": qkv, "out": o, "dout": dout, "dqkv": dqkv}[which].data_ptr() % 16 == 4
    fwd = lib.u3d_mha_fwd(_lib.ptr(qkv), _lib.ptr(o), _lib.ptr(l), B, N, H, D, scale, st)
    bwd = lib.u3d_mha_bwd(_lib.ptr(qkv), _lib.ptr(o_in), _lib.ptr(dout), _lib.ptr(l_in), _lib.ptr(dqkv), B, N, H, D, scale, st)
    torch.cuda.synchronize()
    assert bwd == 1 and fwd == (1 if which in ("qkv", "out") else 0)
    if fwd == 0:          # dout / dqkv are no arguments of the forward: it ran, and owns out and lse
        arena.own(o, B), arena.own(l, B)
    arena.check_guards()
