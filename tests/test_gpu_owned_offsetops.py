"""libunipre3d_offsetops.so writes every element it owns and nothing else: its entry points called directly, with every pointer inside a
poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrappers on ordinary tensors, bit for bit
(tests/test_gpu_offsetops.py holds the wrappers to the restatement); the four scatter-add outputs, which go through float atomics, are
held in BOTH runs to offsetops_ref.bound against the fp64 restatement, as test_gpu_offsetops._within does.

  entry point                        cases
  u3d_offset_knn                     supports (5, 0, 7, 65), queries (4, 3, 0, 17) + 2 rows past the last segment: k = 1 and k = 12 (more
                                     than two segments hold: fill slots; an empty segment: -1; `lane < k` stores); dist2 NULL at k = 12
  u3d_offset_ballquery               the same layout, nsample = 1 and 16
  u3d_offset_group_forward           n = 41, m = 37, nsample = 5 (185 and 205 rows: the last workgroup is partial); c = 3 (w_c 1 and 3:
  u3d_offset_group_backward (+)      the one-float kernels) and c = 8 (w_c 1 and 8) twice: every float pointer 16-byte aligned (the
  u3d_offset_interpolate_forward     Vec<4> kernels), and every float OUTPUT at 4 bytes past a 16-byte boundary, where the host must fall
  u3d_offset_interpolate_backward(+) back to Vec<1> (no torch allocation is ever so placed, so no wrapper test takes that branch).
  u3d_offset_subtract_forward        One index each of `rows`, -1 and 2^31 - 1 in every index tensor.
  u3d_offset_subtract_backward (+ grad_in2)
  u3d_offset_aggregate_forward
  u3d_offset_aggregate_backward (+ grad_input)
"""
import numpy as np
import pytest
import torch

import offsetops_ref as OR
from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

SUPPORT, QUERY, EXTRA = (5, 0, 7, 65), (4, 3, 0, 17), 2


def _layout():
    xyz, offset = OR.ragged(SUPPORT, 11)
    q, new_offset = OR.ragged(QUERY, 12)
    q = np.concatenate([q, np.random.default_rng(13).uniform(-1, 1, (EXTRA, 3)).astype(np.float32)])
    return tuple(torch.from_numpy(a) for a in (xyz, q, offset, new_offset))


@pytest.mark.parametrize("k, with_dist2", [(1, True), (12, True), (12, False)])
def test_offset_knn_writes_what_it_owns(k, with_dist2):
    from unipre3d_amd import _lib, offset_ops as ops
    xyz, q, off, noff = _layout()
    n, m, b = len(xyz), len(q), len(off)

    def case(arena):
        t = [arena.inp(a, name=nm) for a, nm in ((xyz, "xyz"), (q, "new_xyz"), (off, "offset"), (noff, "new_offset"))]
        d = arena.out((m, k), torch.float32, name="dist2") if with_dist2 else None
        idx = arena.out((m, k), torch.int32, name="idx")
        assert ops.load().u3d_offset_knn(b, n, m, k, *(_lib.ptr(a) for a in t), _lib.ptr(d), _lib.ptr(idx), _lib.stream_ptr(idx.device)) == 0
        return [idx] + ([d] if with_dist2 else [])

    run, _ = run_twice(case, "cuda")
    want_d, want_i = ops.knn_query_raw(k, xyz.cuda(), q.cuda(), off.cuda(), noff.cuda())
    assert same_bits(run[0], want_i) and (run[0][-EXTRA:] == -1).all() and (run[0][4:7] == -1).all()
    if with_dist2:
        assert same_bits(run[1], want_d)


@pytest.mark.parametrize("nsample", [1, 16])
def test_offset_ballquery_writes_what_it_owns(nsample):
    from unipre3d_amd import _lib, offset_ops as ops
    xyz, q, off, noff = _layout()
    n, m, b = len(xyz), len(q), len(off)
    radius = 0.6

    def case(arena):
        t = [arena.inp(a, name=nm) for a, nm in ((xyz, "xyz"), (q, "new_xyz"), (off, "offset"), (noff, "new_offset"))]
        idx = arena.out((m, nsample), torch.int32, name="idx")
        assert ops.load().u3d_offset_ballquery(b, n, m, radius, nsample, *(_lib.ptr(a) for a in t), _lib.ptr(idx), _lib.stream_ptr(idx.device)) == 0
        return [idx]

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], ops.ballquery(radius, nsample, xyz.cuda(), q.cuda(), off.cuda(), noff.cuda()))


def _within(got, ref, what):
    val, S, D = ref
    err, lim = np.abs(got.numpy().astype(np.float64) - val), OR.bound(D, S)
    print(f"{what}: largest error {err.max():.3e}, largest error / bound {float((err / np.maximum(lim, 1e-300)).max()):.3f}")
    assert got.shape == val.shape and np.isfinite(err).all() and (err <= lim).all(), what


@pytest.mark.parametrize("c, w_c, misalign", [(3, 1, 0), (3, 3, 0), (8, 1, 0), (8, 8, 0), (8, 1, 4), (8, 8, 4)])
def test_index_addressed_operators_write_what_they_own(c, w_c, misalign):
    from unipre3d_amd import _lib, offset_ops as ops
    lib = ops.load()
    n, m, ns = 41, 37, 5
    rng = np.random.default_rng(c * 10 + w_c)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))

    def holes(rows_of_idx, rows):
        idx = rng.integers(0, rows, (rows_of_idx, ns)).astype(np.int32)
        idx[3, 1], idx[7, 0], idx[11, 3] = rows, -1, 2**31 - 1
        return torch.from_numpy(idx)

    gidx, iidx, nidx = holes(m, n), holes(n, m), holes(n, n)        # group: (m,ns) into n rows; interpolate: (n,ns) into m rows; the rest
    x, x2, src = f(n, c), f(n, c), f(m, c)
    pos, w = f(n, ns, c), f(n, ns, w_c)
    wk = torch.from_numpy(rng.uniform(0.1, 1, (n, ns)).astype(np.float32))
    g_m3, g_n3, g_n2 = f(m, ns, c), f(n, ns, c), f(n, c)

    def case(arena):
        I = lambda t, nm: arena.inp(t, name=nm)
        O = lambda shape, nm: arena.out(shape, torch.float32, misalign, name=nm)
        p, st = _lib.ptr, _lib.stream_ptr(torch.device("cuda:0"))
        d = {nm: I(t, nm) for nm, t in (("x", x), ("x2", x2), ("src", src), ("pos", pos), ("w", w), ("wk", wk), ("g_m3", g_m3),
                                        ("g_n3", g_n3), ("g_n2", g_n2), ("gidx", gidx), ("iidx", iidx), ("nidx", nidx))}
        o = {"group": O((m, ns, c), "group out"), "group_b": O((n, c), "group grad_in"),
             "interp": O((n, c), "interpolate out"), "interp_b": O((m, c), "interpolate grad_input"),
             "sub": O((n, ns, c), "subtract out"), "sub_b1": O((n, c), "subtract grad_in1"), "sub_b2": O((n, c), "subtract grad_in2"),
             "agg": O((n, c), "aggregate out"), "agg_bx": O((n, c), "aggregate grad_input"),
             "agg_bp": O((n, ns, c), "aggregate grad_position"), "agg_bw": O((n, ns, w_c), "aggregate grad_weight")}
        if misalign:
            assert all(t.data_ptr() % 16 == 4 for t in o.values()) and all(t.data_ptr() % 16 == 0 for t in d.values())
        else:
            assert all(t.data_ptr() % 16 == 0 for t in list(o.values()) + list(d.values()))
        assert lib.u3d_offset_group_forward(m, ns, c, n, p(d["x"]), p(d["gidx"]), p(o["group"]), st) == 0
        assert lib.u3d_offset_group_backward(m, ns, c, n, p(d["g_m3"]), p(d["gidx"]), p(o["group_b"]), st) == 0
        assert lib.u3d_offset_interpolate_forward(n, c, ns, m, p(d["src"]), p(d["iidx"]), p(d["wk"]), p(o["interp"]), st) == 0
        assert lib.u3d_offset_interpolate_backward(n, c, ns, m, p(d["g_n2"]), p(d["iidx"]), p(d["wk"]), p(o["interp_b"]), st) == 0
        assert lib.u3d_offset_subtract_forward(n, ns, c, p(d["x"]), p(d["x2"]), p(d["nidx"]), p(o["sub"]), st) == 0
        assert lib.u3d_offset_subtract_backward(n, ns, c, p(d["nidx"]), p(d["g_n3"]), p(o["sub_b1"]), p(o["sub_b2"]), st) == 0
        assert lib.u3d_offset_aggregate_forward(n, ns, c, w_c, p(d["x"]), p(d["pos"]), p(d["w"]), p(d["nidx"]), p(o["agg"]), st) == 0
        assert lib.u3d_offset_aggregate_backward(n, ns, c, w_c, p(d["x"]), p(d["pos"]), p(d["w"]), p(d["nidx"]), p(d["g_n2"]),
                                                 p(o["agg_bx"]), p(o["agg_bp"]), p(o["agg_bw"]), st) == 0
        return list(o.values())

    names = ["group", "group_b", "interp", "interp_b", "sub", "sub_b1", "sub_b2", "agg", "agg_bx", "agg_bp", "agg_bw"]
    atomic = {"group_b", "interp_b", "sub_b2", "agg_bx"}
    runs = run_twice(case, "cuda", deterministic=[i for i, nm in enumerate(names) if nm not in atomic])

    # the wrappers on ordinary (aligned) tensors
    T = lambda t: t.cuda().requires_grad_(True)
    want = {}
    want["group"] = ops.grouping(x.cuda(), gidx.cuda())
    want["interp"] = ops._WeightedGather.apply(src.cuda(), iidx.cuda(), wk.cuda())
    ta, tb = T(x), T(x2)
    out = ops.subtraction(ta, tb, nidx.cuda())
    want["sub"] = out.detach()
    out.backward(g_n3.cuda())
    want["sub_b1"] = ta.grad
    tx, tp, tw = T(x), T(pos), T(w)
    out = ops.aggregation(tx, tp, tw, nidx.cuda())
    want["agg"] = out.detach()
    out.backward(g_n2.cuda())
    want["agg_bp"], want["agg_bw"] = tp.grad, tw.grad
    ref = {"group_b": OR.group_backward(g_m3, gidx, n), "interp_b": OR.interpolate_backward(g_n2, iidx, wk, m),
           "sub_b2": OR.subtract_backward(g_n3, nidx)[1], "agg_bx": OR.aggregate_backward(x, pos, w, nidx, g_n2)[0]}
    for which, run in zip(("poison 0xFF", "poison 0x5A"), runs):
        got = dict(zip(names, run))
        for nm in names:
            if nm in atomic:
                _within(got[nm], ref[nm], f"{nm}, {which}")
            else:
                assert same_bits(got[nm], want[nm]), (nm, which)
