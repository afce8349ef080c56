"""libunipre3d_attention.so writes every element it owns and nothing else: its entry points called directly, with every pointer inside a
poisoned arena (tests/guarded.py), under two poisons.  Expected values: the modules' own wrappers on ordinary tensors, bit for bit
(tests/test_gpu_attention.py and tests/test_gpu_scatter.py hold the wrappers to the fp64 restatement).

  entry point           cases
  u3d_attn_varlen_fwd   H = 3 throughout (the one-wave path packs four heads per workgroup: one slot is empty).
  u3d_attn_varlen_bwd   short: lengths (0, 1, 17, 16) + 2 tail rows at max_seqlen 17 (one wave per head; a 16-row block with one row);
                        long: lengths (65, 0, 1, 33) + 3 tail rows at max_seqlen 65 (four waves per head);
                        overlong: one sequence of 70 rows at max_seqlen 48 (rows 48 .. 69 are written as zeros);
                        all_tail: cu_seqlens = [0], T = 5 (only the uint4 zero-fill of the tail runs);
                        eight_waves, sixteen_waves: the two wider workgroups the host picks from max_seqlen (257: capacity 272 > 256;
                        513 > 512), each one row past the class below it.
                        Outputs: out (T,H,16) fp16, lse (H,T), dqkv (T,3,H,16) fp16.
                        qkv, out, dout or dqkv 4 bytes past a 16-byte boundary: the call returns 1 and not one byte of the arena changes.
  u3d_segment_csr_fwd   N = 13, C = 3, indptr = [2, 2, 7, 10]: an empty segment, rows 0-1 and 10-12 in no segment (dsrc is written
  u3d_segment_csr_bwd   there all the same); sum, mean (arg NULL), max, min (arg (M,C) int64)
"""
import numpy as np
import pytest
import torch

from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

H, D = 3, 16
CASES = {"short": ((0, 1, 17, 16), 2, 17), "long": ((65, 0, 1, 33), 3, 65), "overlong": ((70,), 0, 48), "all_tail": ((), 5, 17),
         "eight_waves": ((257, 2), 1, 257), "sixteen_waves": ((513,), 2, 513)}


def _inputs(lengths, tail, seed):
    rng = np.random.default_rng(seed)
    T = sum(lengths) + tail
    qkv = torch.from_numpy(rng.standard_normal((T, 3, H, D)).astype(np.float16))
    dout = torch.from_numpy(rng.standard_normal((T, H, D)).astype(np.float16))
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))
    return T, qkv, dout, cu


@pytest.mark.parametrize("case", list(CASES))
def test_attention_writes_what_it_owns(case):
    from unipre3d_amd import _lib, attention
    lib = attention.load()
    lengths, tail, max_seqlen = CASES[case]
    T, qkv_cpu, dout_cpu, cu_cpu = _inputs(lengths, tail, len(case))
    S, scale = len(lengths), float(D ** -0.5)

    q = qkv_cpu.cuda().requires_grad_(True)
    out = attention.flash_attn_varlen_qkvpacked_func(q, cu_cpu.cuda(), max_seqlen)
    lse = out.grad_fn.saved_tensors[3]
    out.backward(dout_cpu.cuda())
    out_cpu, lse_cpu = out.detach().cpu(), lse.cpu()

    def case_fn(arena):
        qkv, cu, dout = arena.inp(qkv_cpu, name="qkv"), arena.inp(cu_cpu, name="cu_seqlens"), arena.inp(dout_cpu, name="dout")
        o = arena.out((T, H, D), torch.float16, name="out")
        l = arena.out((H, T), torch.float32, name="lse")
        st = _lib.stream_ptr(o.device)
        assert lib.u3d_attn_varlen_fwd(_lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(o), _lib.ptr(l), T, S, H, D, max_seqlen, scale, st) == 0
        o_in, l_in = arena.inp(out_cpu, name="out_in"), arena.inp(lse_cpu, name="lse_in")
        dqkv = arena.out((T, 3, H, D), torch.float16, name="dqkv")
        assert lib.u3d_attn_varlen_bwd(_lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(o_in), _lib.ptr(dout), _lib.ptr(l_in), _lib.ptr(dqkv),
                                       T, S, H, D, max_seqlen, scale, st) == 0
        return [o, l, dqkv]

    run, _ = run_twice(case_fn, "cuda")
    for got, exp, name in zip(run, (out.detach(), lse, q.grad), ("out", "lse", "dqkv")):
        assert same_bits(got, exp), name
    if case in ("overlong", "all_tail"):
        first = max_seqlen if case == "overlong" else 0
        assert (run[0][first:] == 0).all() and (run[1][:, first:] == 0).all() and (run[2][first:] == 0).all()


@pytest.mark.parametrize("which", ["qkv", "out", "dout", "dqkv"])
def test_attention_refuses_a_pointer_off_16_bytes_and_writes_nothing(which):
    from unipre3d_amd import _lib, attention
    lib = attention.load()
    lengths, tail, max_seqlen = CASES["short"]
    T, qkv_cpu, dout_cpu, cu_cpu = _inputs(lengths, tail, 3)
    S, scale = len(lengths), float(D ** -0.5)
    arena = Arena("cuda", 0x5A)
    off = lambda name: 4 if name == which else 0
    qkv, cu = arena.inp(qkv_cpu, off("qkv"), name="qkv"), arena.inp(cu_cpu, name="cu_seqlens")
    dout = arena.inp(dout_cpu, off("dout"), name="dout")
    o_in = arena.inp(torch.zeros(T, H, D, dtype=torch.float16), off("out"), name="out_in")
    l_in = arena.inp(torch.zeros(H, T), name="lse_in")
    # owned=0: nothing of these outputs may be written by a refused call
    o = arena.out((T, H, D), torch.float16, off("out"), owned=0, name="out")
    l = arena.out((H, T), torch.float32, owned=0, name="lse")
    dqkv = arena.out((T, 3, H, D), torch.float16, off("dqkv"), owned=0, name="dqkv")
    st = _lib.stream_ptr(o.device)
    assert {"qkv": qkv, "out": o, "dout": dout, "dqkv": dqkv}[which].data_ptr() % 16 == 4
    fwd = lib.u3d_attn_varlen_fwd(_lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(o), _lib.ptr(l), T, S, H, D, max_seqlen, scale, st)
    bwd = lib.u3d_attn_varlen_bwd(_lib.ptr(qkv), _lib.ptr(cu), _lib.ptr(o_in), _lib.ptr(dout), _lib.ptr(l_in), _lib.ptr(dqkv),
                                  T, S, H, D, max_seqlen, scale, st)
    torch.cuda.synchronize()
    assert bwd == 1 and fwd == (1 if which in ("qkv", "out") else 0)
    if fwd == 0:          # dout / dqkv are no arguments of the forward: it ran, and owns out and lse
        arena.own(o, T), arena.own(l, H)
    arena.check_guards()


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_segment_csr_writes_what_it_owns(reduce):
    from unipre3d_amd import _lib, attention, scatter
    lib = attention.load()
    N, C, M = 13, 3, 3
    rng = np.random.default_rng(5)
    src_cpu = torch.from_numpy(rng.integers(-3, 4, (N, C)).astype(np.float32))          # ties: the lowest row is the argument
    indptr_cpu = torch.tensor([2, 2, 7, 10], dtype=torch.int64)
    dout_cpu = torch.from_numpy(rng.standard_normal((M, C)).astype(np.float32))
    code = scatter.REDUCE[reduce]

    s = src_cpu.cuda().requires_grad_(True)
    out = scatter.segment_csr(s, indptr_cpu.cuda(), reduce=reduce)
    arg = out.grad_fn.saved_tensors[1]
    out.backward(dout_cpu.cuda())
    assert (arg is None) == (code < 2)
    arg_cpu = None if arg is None else arg.cpu()

    def case(arena):
        src, indptr, dout = arena.inp(src_cpu, name="src"), arena.inp(indptr_cpu, name="indptr"), arena.inp(dout_cpu, name="dout")
        o = arena.out((M, C), torch.float32, name="out")
        a = arena.out((M, C), torch.int64, name="arg") if code >= 2 else None
        st = _lib.stream_ptr(o.device)
        assert lib.u3d_segment_csr_fwd(_lib.ptr(src), _lib.ptr(indptr), _lib.ptr(o), _lib.ptr(a), N, M, C, code, st) == 0
        a_in = arena.inp(arg_cpu, name="arg_in") if code >= 2 else None
        dsrc = arena.out((N, C), torch.float32, name="dsrc")
        assert lib.u3d_segment_csr_bwd(_lib.ptr(dout), _lib.ptr(indptr), _lib.ptr(a_in), _lib.ptr(dsrc), N, M, C, code, st) == 0
        return [o, dsrc] + ([a] if code >= 2 else [])

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], out.detach()) and same_bits(run[1], s.grad)
    assert (run[1][:2] == 0).all() and (run[1][10:] == 0).all()
    if code >= 2:
        assert same_bits(run[2], arg)
