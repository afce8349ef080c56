"""Offset-batched point operators without a GPU: the header against the module's binding table, every entry point's argument checks
and empty calls (host code only: the pointers are never dereferenced), and the CPU restatement (tests/offsetops_ref.py) -- its
lexicographic kNN against its own transcription of the reference's max-heap on tie-free ragged batches, its tie rule on a lattice,
and its ball query against a brute-force loop."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import offsetops_ref as OR
from conftest import ROOT

_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)
SUPPORT_SIZES = (1, 7, 0, 64, 130, 33)
QUERY_SIZES = (3, 17, 2, 0, 20, 5)                                  # queries of an empty segment; a segment without queries


def _declared_functions():
    """{name: [parameter type, ...]} of every function include/unipre3d_offsetops.h declares (all return int; a pointer parameter's
    type ends in '*')."""
    hdr = open(os.path.join(ROOT, "include", "unipre3d_offsetops.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    out = {}
    for ret, name, params in _DECLARATION.findall(hdr):
        assert " ".join(ret.split()) == "int" and name not in out, name
        out[name] = [p[:p.rindex("*") + 1].replace(" ", "") if "*" in p else " ".join(p.split()[:-1]) for p in (q.strip() for q in params.split(","))]
    return out


def test_header_and_binding_agree():
    ops = importlib.import_module("unipre3d_amd.offset_ops")
    declared = _declared_functions()
    assert set(declared) == set(ops.EXPORTS) and len(set(ops.EXPORTS)) == len(ops.EXPORTS) == 10
    assert declared["u3d_offset_knn"] == ["int"] * 4 + ["constfloat*", "constfloat*", "constint32_t*", "constint32_t*", "float*", "int32_t*", "void*"]
    assert declared["u3d_offset_ballquery"][:5] == ["int", "int", "int", "float", "int"]
    handle = ops.load()
    for name, params in declared.items():
        fn = getattr(handle, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for c_type, bound in zip(params, fn.argtypes):
            want = ctypes.c_void_p if c_type.endswith("*") else {"int": ctypes.c_int, "float": ctypes.c_float}[c_type]
            assert bound is want, (name, c_type, bound)
    knn_hdr = open(os.path.join(ROOT, "include", "unipre3d_knn.h")).read()
    assert int(re.search(r"^#define U3D_KNN_MAX_K (\d+)", knn_hdr, re.M).group(1)) == ops.MAX_K


ONE, NULL = ctypes.c_void_p(256), ctypes.c_void_p(0)                  # never dereferenced: every call below returns first


def _lib():
    from unipre3d_amd import offset_ops
    return offset_ops.load()


@pytest.mark.parametrize("entry", ["u3d_offset_knn", "u3d_offset_ballquery"])
def test_search_argument_checks(entry):
    fn = getattr(_lib(), entry)
    if entry == "u3d_offset_knn":
        call = lambda b, n, m, k, p=(ONE, ONE, ONE, ONE, NULL, ONE): fn(b, n, m, k, *p, NULL)
        mandatory = (0, 1, 2, 3, 5)
    else:
        call = lambda b, n, m, k, p=(ONE, ONE, ONE, ONE, ONE): fn(b, n, m, 0.5, k, *p, NULL)
        mandatory = (0, 1, 2, 3, 4)
    assert (call(-1, 8, 4, 2), call(1, -8, 4, 2), call(1, 8, -4, 2)) == (1, 1, 1)             # negative sizes
    assert (call(1, 8, 4, 0), call(1, 8, 4, -1), call(1, 8, 4, 65)) == (1, 1, 1)              # k / nsample outside 1..64
    assert (call(0, 8, 4, 0), call(1, 8, 0, 65)) == (1, 1)                                    # ... in an empty call too
    assert call(1, 2**31 - 1, 4, 2) == 1                                                      # n beyond the 32-bit row counter
    for hole in mandatory:                                                                    # NULL mandatory pointers
        ptrs = [ONE] * (6 if entry == "u3d_offset_knn" else 5)
        if entry == "u3d_offset_knn":
            ptrs[4] = NULL
        ptrs[hole] = NULL
        assert call(2, 8, 4, 2, tuple(ptrs)) == 1, hole
    none = (NULL,) * (6 if entry == "u3d_offset_knn" else 5)
    assert (call(0, 8, 4, 2, none), call(3, 8, 0, 64, none), call(0, 0, 0, 1, none)) == (0, 0, 0)   # empty calls: no launch


def test_operator_argument_checks():
    lib = _lib()
    three, four, five, nine = ([ONE] * k for k in (3, 4, 5, 9))
    # (function, valid sizes, pointers): a negative size in every position, then every pointer NULL in turn
    table = [(lib.u3d_offset_group_forward, (5, 4, 8, 9), three), (lib.u3d_offset_group_backward, (5, 4, 8, 9), three),
             (lib.u3d_offset_interpolate_forward, (5, 8, 3, 9), four), (lib.u3d_offset_interpolate_backward, (5, 8, 3, 9), four),
             (lib.u3d_offset_subtract_forward, (5, 4, 8), four), (lib.u3d_offset_subtract_backward, (5, 4, 8), four),
             (lib.u3d_offset_aggregate_forward, (5, 4, 8, 2), five), (lib.u3d_offset_aggregate_backward, (5, 4, 8, 2), nine[:8])]
    for fn, sizes, ptrs in table:
        for at in range(len(sizes)):
            bad = list(sizes)
            bad[at] = -1
            assert fn(*bad, *ptrs, NULL) == 1, (fn.__name__, at)
        for hole in range(len(ptrs)):
            holed = list(ptrs)
            holed[hole] = NULL
            assert fn(*sizes, *holed, NULL) == 1, (fn.__name__, hole)
        for at in range(len(sizes)):                                   # empty calls: 0, nothing launched, pointers unused
            if fn.__name__.startswith("u3d_offset_aggregate") and at == 3:
                continue                                               # (w_c = 0 is invalid, below)
            if fn.__name__ in ("u3d_offset_subtract_backward", "u3d_offset_aggregate_forward", "u3d_offset_aggregate_backward") and at == 1:
                continue                                               # (nsample = 0 still writes the (n,c) outputs)
            if fn.__name__ in ("u3d_offset_group_forward", "u3d_offset_interpolate_forward") and at == 3:
                continue                                               # (no source rows: the output is written as zeros)
            if fn.__name__ == "u3d_offset_interpolate_forward" and at == 2:
                continue                                               # (k = 0: zeros)
            empty = list(sizes)
            empty[at] = 0
            assert fn(*empty, *([NULL] * len(ptrs)), NULL) == 0, (fn.__name__, at)
    for fn, ptrs in ((lib.u3d_offset_aggregate_forward, five), (lib.u3d_offset_aggregate_backward, nine[:8])):
        assert fn(5, 4, 8, 3, *ptrs, NULL) == 1                        # c % w_c != 0
        assert fn(5, 4, 8, 0, *ptrs, NULL) == 1 and fn(5, 4, 8, -2, *ptrs, NULL) == 1
        assert fn(0, 4, 8, 3, *ptrs, NULL) == 1                        # ... in an empty call too
    assert lib.u3d_offset_group_forward(2**30, 2**10, 2**10, 9, *three, NULL) == 1    # 2^50 elements: more workgroups than a grid holds


def _tie_free_batch(seed, k):
    """A seeded ragged batch whose queries all see an fp64 gap between consecutive distances among their first k + 1 -- the guard of
    tests/golden/make_g16_knn.py; a seed that fails it is replaced by the next, never excused."""
    while True:
        xyz, offset = OR.ragged(SUPPORT_SIZES, seed)
        new_xyz, new_offset = OR.ragged(QUERY_SIZES, seed + 1000)
        if OR.min_gap(k, xyz, new_xyz, offset, new_offset) > 1e-6:
            return xyz, new_xyz, offset, new_offset
        seed += 7919


@pytest.mark.parametrize("k", [1, 3, 16, 64])
def test_lexicographic_contract_equals_the_reference_heap_on_tie_free_batches(k):
    for seed in range(3):
        xyz, new_xyz, offset, new_offset = _tie_free_batch(seed, k)
        d2, idx = OR.knn(k, xyz, new_xyz, offset, new_offset)
        hd, hi = OR.knn_heap(k, xyz, new_xyz, offset, new_offset)
        assert d2.dtype == hd.dtype == np.float32 and idx.dtype == hi.dtype == np.int32
        assert np.array_equal(idx, hi) and np.array_equal(d2.view(np.uint32), hd.view(np.uint32)), (k, seed)    # order and fill included
        rng = OR.ranges(len(new_xyz), len(xyz), offset, new_offset)
        for j, (a, e) in enumerate(rng):
            got = min(k, e - a)
            assert (idx[j, :got] >= a).all() and (idx[j, :got] < e).all() and len(set(idx[j, :got])) == got
            assert (idx[j, got:] == (a if e > a else -1)).all() and (d2[j, got:] == OR.FILL_D2).all()


def test_segment_rule_and_fill():
    xyz, offset = OR.ragged((4, 0, 3), 5)
    new_xyz = np.zeros((9, 3), np.float32)
    new_offset = np.array([2, 5, 7], np.int32)                          # rows 7, 8 belong to no segment
    assert OR.ranges(9, 7, offset, new_offset).tolist() == [[0, 4]] * 2 + [[4, 4]] * 3 + [[4, 7]] * 2 + [[0, 0]] * 2
    d2, idx = OR.knn(5, xyz, new_xyz, offset, new_offset)
    assert (idx[2:5] == -1).all() and (idx[7:] == -1).all() and (d2[2:5] == OR.FILL_D2).all()
    assert sorted(idx[0, :4]) == [0, 1, 2, 3] and idx[0, 4] == 0 and d2[0, 4] == OR.FILL_D2
    assert sorted(idx[5, :3]) == [4, 5, 6] and (idx[5, 3:] == 4).all()
    # offsets that lie: clamped to [0, n], end < start empty
    assert OR.ranges(3, 7, np.array([-5, 99, 2]), np.array([1, 2, 3])).tolist() == [[0, 0], [0, 7], [7, 7]]


def test_tie_rule_on_a_lattice():
    """Equal distances go to the lower index; the heap agrees on the distances but not on which tied point stays."""
    g = np.arange(4, dtype=np.float32)
    cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(64, 3)
    xyz = np.concatenate([cube, cube[:10], cube + np.float32(10)])        # segment 0: the lattice and 10 duplicates; segment 1: a copy
    offset = np.array([74, 138], np.int32)
    d2, idx = OR.knn(8, xyz, xyz, offset, offset)
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    assert (np.diff(key.astype(object), axis=-1) > 0).all()
    assert idx[0].tolist() == [0, 64, 1, 4, 16, 65, 68, 5] and d2[0].tolist() == [0, 0, 1, 1, 1, 1, 1, 2]
    assert idx[74].tolist() == [74, 75, 78, 90, 79, 91, 94, 95] and (idx[74:] >= 74).all() and (idx[:74] < 74).all()
    hd, hi = OR.knn_heap(8, xyz, xyz, offset, offset)
    assert np.array_equal(hd, d2) and not np.array_equal(hi, idx)


@pytest.mark.parametrize("nsample", [1, 16, 32])
def test_ball_query_against_brute_force(nsample):
    radius, seed = 0.9, 11
    while True:
        xyz, offset = OR.ragged(SUPPORT_SIZES, seed)
        new_xyz, new_offset = OR.ragged(QUERY_SIZES, seed + 1)
        if OR.ball_margin(radius, xyz, new_xyz, offset, new_offset) > 1e-5:
            break
        seed += 7919
    got = OR.ballquery(radius, nsample, xyz, new_xyz, offset, new_offset)
    rng = OR.ranges(len(new_xyz), len(xyz), offset, new_offset)
    counts = []
    for j, (a, e) in enumerate(rng):
        row, cnt = [0] * nsample, 0
        for i in range(a, e):                                          # fp64: the margin makes the decision format-free
            if float(((new_xyz[j].astype(np.float64) - xyz[i].astype(np.float64)) ** 2).sum()) < radius * radius:
                if cnt == 0:
                    row = [i] * nsample
                row[cnt] = i
                cnt += 1
                if cnt >= nsample:
                    break
        counts.append(cnt)
        assert got[j].tolist() == row, j
    assert 0 in counts and max(counts) == nsample and (nsample == 1 or any(0 < c < nsample for c in counts))


def test_float_restatements_agree_with_torch_autograd():
    """The fp64 forms and their gradients against torch's own indexing and autograd in fp64 (an independent derivation)."""
    import torch
    rng = np.random.default_rng(3)
    n, ns, c, w_c = 12, 4, 6, 3
    idx = rng.integers(0, n, (n, ns))
    x, x2, p, w = rng.standard_normal((n, c)), rng.standard_normal((n, c)), rng.standard_normal((n, ns, c)), rng.standard_normal((n, ns, w_c))
    g2, g3, wk = rng.standard_normal((n, c)), rng.standard_normal((n, ns, c)), rng.uniform(0.1, 1, (n, ns))
    T = lambda a: torch.from_numpy(a).requires_grad_(True)
    ti = torch.from_numpy(idx)
    tx, tx2, tp, tw = T(x), T(x2), T(p), T(w)
    out = ((tx[ti] + tp) * tw.repeat(1, 1, c // w_c)).sum(1)
    assert np.allclose(OR.aggregate_forward(x, p, w, idx)[0], out.detach().numpy(), rtol=1e-12, atol=1e-12)
    out.backward(torch.from_numpy(g2))
    for got, want in zip(OR.aggregate_backward(x, p, w, idx, g2), (tx.grad, tp.grad, tw.grad)):
        assert np.allclose(got[0], want.numpy(), rtol=1e-12, atol=1e-12)
    tx, tx2 = T(x), T(x2)
    (tx[:, None, :] - tx2[ti]).backward(torch.from_numpy(g3))
    (g1, _, _), (gb, _, _) = OR.subtract_backward(g3, idx)
    assert np.allclose(g1, tx.grad.numpy(), atol=1e-12) and np.allclose(gb, tx2.grad.numpy(), atol=1e-12)
    assert np.array_equal(OR.subtract_forward(x, x2, idx), (x.astype(np.float32)[:, None] - x2.astype(np.float32)[idx]))
    tx = T(x)
    tx[ti].backward(torch.from_numpy(g3))
    assert np.allclose(OR.group_backward(g3, idx, n)[0], tx.grad.numpy(), atol=1e-12)
    tx = T(x)
    out = (tx[ti] * torch.from_numpy(wk)[..., None]).sum(1)
    assert np.allclose(OR.interpolate_forward(x, idx, wk)[0], out.detach().numpy(), atol=1e-12)
    out.backward(torch.from_numpy(g2))
    assert np.allclose(OR.interpolate_backward(g2, idx, wk, n)[0], tx.grad.numpy(), atol=1e-12)
    # an index outside its tensor: the term is dropped (group: zeros), the other rows do not change
    bad = idx.copy()
    bad[3, 1], bad[7, 0] = n, -1
    assert (OR.group_forward(x, bad)[3, 1] == 0).all() and np.array_equal(OR.group_forward(x, bad)[0], OR.group_forward(x, idx)[0])
    full, part = OR.aggregate_forward(x, p, w, idx), OR.aggregate_forward(x, p, w, bad)
    keep = np.ones(n, bool)
    keep[[3, 7]] = False
    assert np.array_equal(full[0][keep], part[0][keep]) and part[2][3, 0] == ns - 1 and np.isfinite(part[0]).all()
