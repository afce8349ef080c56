"""libunipre3d_serialization.so writes every element it owns and nothing else: its entry points called directly, with every pointer
inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrappers on ordinary tensors, bit for
bit (tests/test_gpu_serialization.py holds the wrappers to the numpy restatement).

  entry point             cases
  u3d_ser_encode          N = 1 and N = 4097 (one point past a whole number of scatter tiles), K = 1 (hilbert) and K = 4 (all orders),
  u3d_ser_sort            depth 10, a batch of 2 items (31-bit keys: four radix passes, outputs written by (pass, tile) scatter); the
  u3d_ser_serialize       scratch is a guarded placement.  grid_coord int32 with batch int64; and at N = 4097, K = 1 the other widths the
                          entry points read: grid_coord int64 with batch int32, and batch NULL (30-bit keys)
  u3d_ser_pool_count      the same codes, pooling depth 2; meta is a (4,) placement of which the library owns word 0 (= M, read between
  u3d_ser_pool_emit       the two calls, equal across the runs); idx_ptr (M+1,), head_indices (M,), pooled code / order / inverse (K,M)
  u3d_ser_patch_padding   items of (1, 49, 95) rows at patch 48: one row, one row past a patch, one row short of two patches
"""
import numpy as np
import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

DEPTH, POOL, BATCH = 10, 2, 2
ORDERS = {1: ("hilbert",), 4: ("z", "z-trans", "hilbert", "hilbert-trans")}
I32, I64 = torch.int32, torch.int64


@pytest.mark.parametrize("N, K, coord_dtype, batch_dtype", [(1, 1, I32, I64), (1, 4, I32, I64), (4097, 1, I32, I64), (4097, 4, I32, I64),
                                                            (4097, 1, I64, I32), (4097, 1, I32, None)])
def test_serialization_writes_what_it_owns(N, K, coord_dtype, batch_dtype):
    from unipre3d_amd import _lib, serialization as ser
    lib = ser.load()
    rng = np.random.default_rng(N + K)
    # a coarse lattice: repeated sites (the stable order among equal codes) and clusters of several points
    grid_cpu = torch.from_numpy((rng.integers(0, 24, (N, 3)) * 37 % 1024).astype(np.int32)).to(coord_dtype)
    batch_cpu = None if batch_dtype is None else (torch.arange(N) >= N // 2).to(batch_dtype)
    batch_dev, batch_size = (None, 1) if batch_dtype is None else (batch_cpu.cuda(), BATCH)
    coord64, batch64 = int(coord_dtype == I64), int(batch_dtype == I64)
    _, bits = ser._order_bits(ORDERS[K])
    key_bits, pool_bits = 3 * DEPTH + (batch_size - 1).bit_length(), 3 * (DEPTH - POOL) + (batch_size - 1).bit_length()
    nbytes = int(lib.u3d_ser_scratch_bytes(K, N))

    want_code = ser.encode(grid_cpu.cuda(), batch_dev, DEPTH, list(ORDERS[K]))
    code_cpu = want_code.cpu()
    counts = []

    def case(arena):
        p, st = _lib.ptr, _lib.stream_ptr(torch.device("cuda:0"))
        new = lambda shape, name, **kw: arena.out(shape, torch.int64, name=name, **kw)
        grid, code_in = arena.inp(grid_cpu, name="grid_coord"), arena.inp(code_cpu, name="code_in")
        batch = None if batch_cpu is None else arena.inp(batch_cpu, name="batch")
        code = new((K, N), "code")
        assert lib.u3d_ser_encode(N, p(grid), coord64, p(batch), batch64, DEPTH, K, bits, p(code), st) == 0
        order, inverse = new((K, N), "order"), new((K, N), "inverse")
        scratch = arena.out((nbytes,), torch.uint8, name="sort scratch")
        assert lib.u3d_ser_sort(K, N, key_bits, p(code_in), p(order), p(inverse), p(scratch), st) == 0
        code2, order2, inverse2 = new((K, N), "serialize code"), new((K, N), "serialize order"), new((K, N), "serialize inverse")
        scratch2 = arena.out((nbytes,), torch.uint8, name="serialize scratch")
        assert lib.u3d_ser_serialize(N, p(grid), coord64, p(batch), batch64, DEPTH, K, bits, key_bits, p(code2), p(order2), p(inverse2), p(scratch2), st) == 0
        meta = arena.out((4,), torch.int32, owned=1, name="meta")
        scratch3 = arena.out((nbytes,), torch.uint8, name="pool scratch")
        assert lib.u3d_ser_pool_count(K, N, 3 * POOL, pool_bits, p(code_in), p(meta), p(scratch3), st) == 0
        M = int(meta[0].item())
        counts.append(M)
        assert 1 <= M <= N
        cluster, indices, idx_ptr, head = new((N,), "cluster"), new((N,), "indices"), new((M + 1,), "idx_ptr"), new((M,), "head_indices")
        pcode, porder, pinverse = new((K, M), "pooled code"), new((K, M), "pooled order"), new((K, M), "pooled inverse")
        assert lib.u3d_ser_pool_emit(K, N, M, 3 * POOL, pool_bits, p(code_in), p(cluster), p(indices), p(idx_ptr), p(head), p(pcode),
                                     p(porder), p(pinverse), p(scratch3), st) == 0
        return [code, order, inverse, code2, order2, inverse2, meta[:1], cluster, indices, idx_ptr, head, pcode, porder, pinverse]

    run, _ = run_twice(case, "cuda")
    assert counts[0] == counts[1] and run[6].tolist() == [counts[0]]
    want_order, want_inverse = ser.sort_codes(want_code, key_bits)
    want = [want_code, want_order, want_inverse, *ser.serialize(grid_cpu.cuda(), batch_dev, DEPTH, list(ORDERS[K]), batch_size=batch_size)]
    pooled = ser.pool_clusters(want_code, POOL, depth=DEPTH, batch_size=batch_size)
    assert pooled[3].numel() == counts[0]
    names = ["code", "order", "inverse", "serialize code", "serialize order", "serialize inverse", "cluster", "indices", "idx_ptr",
             "head_indices", "pooled code", "pooled order", "pooled inverse"]
    for got, exp, name in zip(run[:6] + run[7:], want + list(pooled), names):
        assert same_bits(got, exp), name


def test_patch_padding_writes_what_it_owns():
    from unipre3d_amd import _lib, serialization as ser
    lib = ser.load()
    sizes, patch = (1, 49, 95), 48
    ends = np.cumsum(sizes).tolist()
    padded = [n if n <= patch else -(-n // patch) * patch for n in sizes]
    seqs = [1 if n <= patch else -(-n // patch) for n in sizes]
    B, T, T_pad, S = len(sizes), sum(sizes), sum(padded), sum(seqs)
    assert (T, T_pad, S) == (145, 193, 5)
    meta_cpu = torch.tensor([[0] + ends, [0] + np.cumsum(padded).tolist(), [0] + np.cumsum(seqs).tolist()], dtype=torch.int64)

    def case(arena):
        meta = arena.inp(meta_cpu, name="meta")
        pad, unpad = arena.out((T_pad,), torch.int64, name="pad"), arena.out((T,), torch.int64, name="unpad")
        cu = arena.out((S + 1,), torch.int32, name="cu_seqlens")
        assert lib.u3d_ser_patch_padding(B, patch, T, T_pad, S, _lib.ptr(meta), _lib.ptr(pad), _lib.ptr(unpad), _lib.ptr(cu),
                                         _lib.stream_ptr(pad.device)) == 0
        return [pad, unpad, cu]

    run, _ = run_twice(case, "cuda")
    for got, exp, name in zip(run, ser.patch_padding(ends, patch), ("pad", "unpad", "cu_seqlens")):
        assert same_bits(got, exp), name
