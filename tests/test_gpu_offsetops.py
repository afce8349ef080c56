"""HIP offset-batched point operators (include/unipre3d_offsetops.h) against the CPU restatement tests/offsetops_ref.py.

Searches: indices AND squared distances bit for bit -- at support segments of one to three LDS tiles and both sides of every edge, with
16-query workgroups that straddle one and two segment boundaries, with k above several segments' sizes (the fill), with empty
segments of either kind, on a lattice full of exact ties, and against the dense u3d_knn the selection core is shared with.
Gathers: bit for bit.  Float sums: against the fp64 restatement within (D + 2) * 2^-23 * sum |term| per element (offsetops_ref.bound:
the recursive-summation bound, valid for any order of addition and so for the atomics)."""
import numpy as np
import pytest
import torch

import offsetops_ref as OR

pytestmark = pytest.mark.gpu

SUPPORT_SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4100)               # one to three LDS tiles of 2048, both sides of each edge
QUERY_SIZES = (3, 17, 16, 1, 33, 5, 16, 40)                           # 16-query workgroups straddle one and two boundaries
KS = (1, 3, 16, 64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(k, xyz, new_xyz, offset, new_offset):
    from unipre3d_amd import offset_ops
    d2, idx = offset_ops.knn_query_raw(k, _dev(xyz), _dev(new_xyz), _dev(offset), _dev(new_offset))
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(new_xyz), k)
    return d2.cpu().numpy(), idx.cpu().numpy()


def _assert_exact(got, want, what):
    (gd, gi), (wd, wi) = got, want
    print(f"{what}: rows with a differing index {int((gi != wi).any(-1).sum())} of {wi.shape[0]}, "
          f"differing d2 words {int((gd.view(np.uint32) != wd.view(np.uint32)).sum())}")
    assert np.array_equal(gi, wi), what
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


@pytest.fixture(scope="module")
def layout():
    """The segment layout and its restatement at k = 64, computed once (a smaller k is its first k columns: the fill follows the
    neighbours).  Every third query is a support point of its own segment."""
    xyz, offset = OR.ragged(SUPPORT_SIZES, 21)
    new_xyz, new_offset = OR.ragged(QUERY_SIZES, 22)
    rng = OR.ranges(len(new_xyz), len(xyz), offset, new_offset)
    for j in range(0, len(new_xyz), 3):
        new_xyz[j] = xyz[rng[j, 0] + (j * 7) % (rng[j, 1] - rng[j, 0])]
    want = OR.knn(64, xyz, new_xyz, offset, new_offset)
    assert (want[1][:3, 1:] == 0).all() and (want[0][:3, 1:] == OR.FILL_D2).all()      # segment 0 has one point: 63 fill slots
    return xyz, new_xyz, offset, new_offset, want


@pytest.mark.parametrize("k", KS)
def test_knn_segment_layout(layout, k):
    xyz, new_xyz, offset, new_offset, (wd, wi) = layout
    _assert_exact(_raw(k, xyz, new_xyz, offset, new_offset), (wd[:, :k], wi[:, :k]), f"segment layout, k = {k}")


def test_knn_offsets_may_be_int64_and_none_means_self(layout):
    from unipre3d_amd import offset_ops
    xyz, _, offset, _, _ = layout
    x, o = _dev(xyz[:300]), _dev(np.array([1, 64, 128, 193, 300], np.int64))
    want = OR.knn(3, xyz[:300], xyz[:300], [1, 64, 128, 193, 300], [1, 64, 128, 193, 300])
    d2, idx = offset_ops.knn_query_raw(3, x, None, o, None)
    _assert_exact((d2.cpu().numpy(), idx.cpu().numpy()), want, "self query, int64 offsets")
    assert (idx[:, 0].cpu().numpy() == np.arange(300)).all()
    idx2, dist = offset_ops.knnquery(3, x, None, o.int(), None)
    assert torch.equal(idx2, idx) and torch.equal(dist, torch.sqrt(d2))


def test_knn_empty_segments():
    """Segment 1: no support, no queries.  Segment 3: queries without support (fill -1 / 1e10).  Segment 4: support without queries
    (a repeated new_offset).  Rows beyond new_offset[-1] belong to no segment."""
    xyz, offset = OR.ragged((5, 0, 7, 0, 3, 9), 31)
    new_xyz, new_offset = OR.ragged((4, 0, 6, 3, 0, 2), 32)
    new_xyz = np.concatenate([new_xyz, new_xyz[:2]])                    # two rows past the last segment
    assert offset.tolist() == [5, 5, 12, 12, 15, 24] and new_offset.tolist() == [4, 4, 10, 13, 13, 15]
    for k in (1, 4, 8):
        want = OR.knn(k, xyz, new_xyz, offset, new_offset)
        got = _raw(k, xyz, new_xyz, offset, new_offset)
        _assert_exact(got, want, f"empty segments, k = {k}")
        assert (got[1][10:13] == -1).all() and (got[0][10:13] == OR.FILL_D2).all() and (got[1][15:] == -1).all()
        assert (got[1][13:15] >= 15).all() and (got[1][13:15] < 24).all()


def test_knn_ties_on_a_lattice():
    g = np.arange(4, dtype=np.float32)
    cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(64, 3)
    xyz = np.concatenate([cube, cube[:10], cube + np.float32(10), cube[:5]])   # 74 with duplicates | 64 | 5
    offset = np.array([74, 138, 143], np.int32)
    rng = OR.ranges(143, 143, offset, offset)
    for k in (8, 64):
        want = OR.knn(k, xyz, xyz, offset, offset)
        d2, idx = _raw(k, xyz, xyz, offset, offset)
        _assert_exact((d2, idx), want, f"lattice, k = {k}")
        for j, (a, e) in enumerate(rng):
            got = min(k, e - a)
            assert (idx[j] >= a).all() and (idx[j] < e).all() and len(set(idx[j, :got].tolist())) == got, j
            assert (idx[j, got:] == a).all() and (d2[j, got:] == OR.FILL_D2).all(), j
    assert idx[0, :8].tolist() == [0, 64, 1, 4, 16, 65, 68, 5]


def test_knn_equals_the_dense_kernel_it_shares_its_core_with():
    from unipre3d_amd import knn, offset_ops
    cloud, _ = OR.ragged((2500,), 41)
    cloud = (np.round(cloud * 16) / 16).astype(np.float32)              # sixteenths: equal distances everywhere
    query, _ = OR.ragged((50,), 42)
    s, q = _dev(cloud), _dev(query)
    for k in (1, 16, 64):
        dd, di = knn.knn_query(k, s[None], q[None])
        rd, ri = offset_ops.knn_query_raw(k, s, q, _dev(np.array([2500], np.int32)), _dev(np.array([50], np.int32)))
        assert torch.equal(ri, di[0]) and torch.equal(rd.view(torch.int32), dd[0].view(torch.int32)), k
    sizes, qsizes = (700, 1000, 800), (10, 25, 15)
    off, qoff = np.cumsum(sizes).astype(np.int32), np.cumsum(qsizes).astype(np.int32)
    rd, ri = offset_ops.knn_query_raw(16, s, q, _dev(off), _dev(qoff))
    a = qa = 0
    for n_s, m_s in zip(sizes, qsizes):
        dd, di = knn.knn_query(16, s[None, a:a + n_s], q[None, qa:qa + m_s])
        assert torch.equal(ri[qa:qa + m_s], di[0] + a) and torch.equal(rd[qa:qa + m_s].view(torch.int32), dd[0].view(torch.int32))
        a, qa = a + n_s, qa + m_s
    _assert_exact((rd.cpu().numpy(), ri.cpu().numpy()), OR.knn(16, cloud, query, off, qoff), "three segments")


def test_the_evaluators_call():
    """pointcept/engines/hooks/evaluator.py: predictions of the grid-sampled voxels carried back to the original points."""
    import unipre3d_amd.offset_ops as pointops
    coord, offset = OR.ragged((900, 1300), 51)                          # two scenes' voxels
    origin_coord, origin_offset = OR.ragged((2100, 2500), 52)
    pred = torch.arange(2200, device="cuda") % 20
    idx, dist = pointops.knn_query(1, _dev(coord), _dev(offset.astype(np.int64)), _dev(origin_coord), _dev(origin_offset.astype(np.int64)))
    assert idx.shape == (4600, 1) and idx.dtype == torch.int32 and dist.shape == (4600, 1)
    wd, wi = OR.knn(1, coord, origin_coord, offset, origin_offset)
    assert np.array_equal(idx.cpu().numpy(), wi) and (wi[:2100] < 900).all() and (wi[2100:] >= 900).all()
    root = np.sqrt(wd)
    assert (np.abs(dist.cpu().numpy().astype(np.float64) - root) <= 2 * np.spacing(np.maximum(root, np.float32(1e-30)))).all()
    assert torch.equal(pred[idx.flatten().long()].cpu(), (torch.arange(2200) % 20)[torch.from_numpy(wi).flatten().long()])


@pytest.fixture(scope="module")
def ball(layout):
    """The radius and the hit count of every query of the layout: some queries without a hit, some with fewer than 16, some with more
    than 32; no |d2 - r^2| below 1e-5 r^2 in fp64, so rounding cannot flip a decision."""
    xyz, new_xyz, offset, new_offset, _ = layout
    radius = 0.26
    assert OR.ball_margin(radius, xyz, new_xyz, offset, new_offset) > 1e-5
    r2 = np.float32(radius) * np.float32(radius)
    counts = np.array([int((OR.dist2_rows(new_xyz[j], xyz[a:e]) < r2).sum())
                       for j, (a, e) in enumerate(OR.ranges(len(new_xyz), len(xyz), offset, new_offset))])
    print("ball query: hits per query", np.bincount(np.minimum(counts, 33)).tolist())
    assert (counts == 0).any() and ((counts > 0) & (counts < 16)).any() and (counts > 32).any()
    return radius


@pytest.mark.parametrize("nsample", [1, 16, 32])
def test_ball_query(layout, ball, nsample):
    from unipre3d_amd import offset_ops
    xyz, new_xyz, offset, new_offset, _ = layout
    got = offset_ops.ballquery(ball, nsample, _dev(xyz), _dev(new_xyz), _dev(offset), _dev(new_offset))
    want = OR.ballquery(ball, nsample, xyz, new_xyz, offset, new_offset)
    assert got.dtype == torch.int32 and got.shape == want.shape
    print(f"ball query, nsample = {nsample}: differing rows {int((got.cpu().numpy() != want).any(-1).sum())} of {len(want)}")
    assert np.array_equal(got.cpu().numpy(), want)


def test_ball_query_empty_segments():
    from unipre3d_amd import offset_ops
    xyz, offset = OR.ragged((5, 0, 7, 0, 3, 9), 31)
    new_xyz, new_offset = OR.ragged((4, 0, 6, 3, 0, 2), 32)
    new_xyz = np.concatenate([new_xyz, new_xyz[:2]])
    got = offset_ops.ballquery(1.5, 4, _dev(xyz), _dev(new_xyz), _dev(offset), _dev(new_offset)).cpu().numpy()
    assert np.array_equal(got, OR.ballquery(1.5, 4, xyz, new_xyz, offset, new_offset))
    assert (got[10:13] == 0).all() and (got[15:] == 0).all()


@pytest.mark.parametrize("c", [1, 3, 32, 67])
def test_gathers_are_bit_exact(c):
    from unipre3d_amd import offset_ops
    rng = np.random.default_rng(c)
    n, m, ns = 41, 37, 5
    x, x2 = rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((n, c)).astype(np.float32)
    gi, si = rng.integers(0, n, (m, ns)).astype(np.int32), rng.integers(0, n, (n, ns)).astype(np.int32)
    got = offset_ops.grouping(_dev(x), _dev(gi))
    assert got.shape == (m, ns, c) and np.array_equal(got.cpu().numpy().view(np.uint32), OR.group_forward(x, gi).view(np.uint32))
    got = offset_ops.subtraction(_dev(x), _dev(x2), _dev(si.astype(np.int64)))
    assert got.shape == (n, ns, c) and np.array_equal(got.cpu().numpy().view(np.uint32), OR.subtract_forward(x, x2, si).view(np.uint32))


def _within(got, ref, what):
    val, S, D = ref
    err, lim = np.abs(got.detach().cpu().numpy().astype(np.float64) - val), OR.bound(D, S)
    worst = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: largest error {err.max() if err.size else 0.0:.3e}, largest error / bound {worst:.3f}, D up to {int(np.max(D))}")
    assert got.shape == val.shape and np.isfinite(err).all() and (err <= lim).all(), what


# (c, w_c): the scalar path with w_c in {1, c}, and the 16-byte path with a shared weight
@pytest.mark.parametrize("c,w_c", [(3, 1), (3, 3), (67, 1), (67, 67), (32, 8)])
@pytest.mark.parametrize("indices", ["random", "one_row"])
def test_float_sums_within_the_summation_bound(c, w_c, indices):
    """Every float sum of the library through its C entry points' Python callers.  `one_row`: every index names row 5, so that row's
    scatter-adds have D = n * nsample addends -- the worst contention."""
    from unipre3d_amd import offset_ops as ops
    rng = np.random.default_rng(c * 100 + w_c)
    n, ns, m = 60, 16, 45
    idx = rng.integers(0, n, (n, ns)).astype(np.int32) if indices == "random" else np.full((n, ns), 5, np.int32)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, p, w, g2, g3, wk = f(n, c), f(n, ns, c), f(n, ns, w_c), f(n, c), f(n, ns, c), rng.uniform(0.05, 1, (n, ns)).astype(np.float32)
    # interpolate: m source rows -> n outputs
    src = f(m, c)
    iidx = idx % m
    t = _dev(src).requires_grad_(True)
    out = ops._WeightedGather.apply(t, _dev(iidx), _dev(wk))
    _within(out, OR.interpolate_forward(src, iidx, wk), "interpolate forward")
    out.backward(_dev(g2))
    _within(t.grad, OR.interpolate_backward(g2, iidx, wk, m), "interpolate backward")
    # aggregate
    tx, tp, tw = (_dev(a).requires_grad_(True) for a in (x, p, w))
    out = ops.aggregation(tx, tp, tw, _dev(idx))
    _within(out, OR.aggregate_forward(x, p, w, idx), "aggregate forward")
    out.backward(_dev(g2))
    for got, ref, what in zip((tx.grad, tp.grad, tw.grad), OR.aggregate_backward(x, p, w, idx, g2), ("input", "position", "weight")):
        _within(got, ref, f"aggregate backward, grad_{what}")
    # group backward: (m, ns) indices into n rows
    tx = _dev(x).requires_grad_(True)
    ops.grouping(tx, _dev(idx[:m])).backward(_dev(g3[:m]))
    _within(tx.grad, OR.group_backward(g3[:m], idx[:m], n), "group backward")
    # subtract backward
    ta, tb = _dev(x).requires_grad_(True), _dev(g2).requires_grad_(True)
    ops.subtraction(ta, tb, _dev(idx)).backward(_dev(g3))
    r1, r2 = OR.subtract_backward(g3, idx)
    _within(ta.grad, r1, "subtract backward, grad_in1")
    _within(tb.grad, r2, "subtract backward, grad_in2")


def test_autograd_functions_against_the_restatement_gradients():
    """Each Function's gradients, through torch.autograd.grad with a random cotangent, at n = 50, nsample = 4, c = 8 in fp32 (there are
    no fp64 kernels, so gradcheck's finite differences are replaced by the restatement's analytic fp64 gradients, same bound)."""
    from unipre3d_amd import offset_ops as ops
    rng = np.random.default_rng(50)
    n, ns, c, w_c = 50, 4, 8, 4
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    xyz, offset = OR.ragged((20, 30), 61)
    idx = OR.knn(ns, xyz, xyz, offset, offset)[1]
    gidx = ops.knnquery(ns, _dev(xyz), None, _dev(offset), None)[0]
    assert np.array_equal(gidx.cpu().numpy(), idx)
    x, x2, p, w, g2, g3 = f(n, c), f(n, c), f(n, ns, c), f(n, ns, w_c), f(n, c), f(n, ns, c)
    T = lambda a: _dev(a).requires_grad_(True)
    tx = T(x)
    (gx,) = torch.autograd.grad(ops.grouping(tx, gidx), tx, _dev(g3))
    _within(gx, OR.group_backward(g3, idx, n), "grouping")
    ta, tb = T(x), T(x2)
    ga, gb = torch.autograd.grad(ops.subtraction(ta, tb, gidx), (ta, tb), _dev(g3))
    r1, r2 = OR.subtract_backward(g3, idx)
    _within(ga, r1, "subtraction, input1")
    _within(gb, r2, "subtraction, input2")
    tx, tp, tw = T(x), T(p), T(w)
    grads = torch.autograd.grad(ops.aggregation(tx, tp, tw, gidx), (tx, tp, tw), _dev(g2))
    for got, ref, what in zip(grads, OR.aggregate_backward(x, p, w, idx, g2), ("input", "position", "weight")):
        _within(got, ref, f"aggregation, {what}")
    # interpolation2: 20 + 30 coarse rows -> 2 x 40 fine rows, k = 3
    fine, fine_offset = OR.ragged((40, 40), 62)
    tf = T(x)
    out = ops.interpolation2(_dev(xyz), _dev(fine), tf, _dev(offset), _dev(fine_offset), 3)
    kidx, weight = ops._interpolation_weights(_dev(xyz), _dev(fine), _dev(offset), _dev(fine_offset), 3)
    wd, wi = OR.knn(3, xyz, fine, offset, fine_offset)
    assert np.array_equal(kidx.cpu().numpy(), wi) and torch.allclose(weight.sum(1), torch.ones(80, device="cuda"), atol=1e-6)
    _within(out, OR.interpolate_forward(x, wi, weight.cpu().numpy()), "interpolation2 forward")
    g80 = f(80, c)
    (gf,) = torch.autograd.grad(out, tf, _dev(g80))
    _within(gf, OR.interpolate_backward(g80, wi, weight.cpu().numpy(), n), "interpolation2 backward")
    assert torch.equal(ops.interpolation(_dev(xyz), _dev(fine), _dev(x), _dev(offset), _dev(fine_offset), 3), out.detach())


def test_indices_outside_their_tensor_are_skipped():
    """Defined behaviour on valid memory: the term an outside index names is dropped, every output stays finite and rows without such
    an index are what they are without it."""
    from unipre3d_amd import offset_ops as ops
    rng = np.random.default_rng(7)
    n, ns, c, w_c = 30, 4, 8, 2
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    idx = rng.integers(0, n, (n, ns)).astype(np.int32)
    bad = idx.copy()
    bad[3, 1], bad[7, 0], bad[11, 3] = n, -1, 2**31 - 1
    clean = np.ones(n, bool)
    clean[[3, 7, 11]] = False
    x, x2, p, w, g2, g3, wk = f(n, c), f(n, c), f(n, ns, c), f(n, ns, w_c), f(n, c), f(n, ns, c), rng.uniform(0.1, 1, (n, ns)).astype(np.float32)
    T = lambda a: _dev(a).requires_grad_(True)
    for name, run in (("grouping", lambda i: ops.grouping(T(x), _dev(i))), ("subtraction", lambda i: ops.subtraction(T(x), T(x2), _dev(i))),
                      ("aggregation", lambda i: ops.aggregation(T(x), T(p), T(w), _dev(i))),
                      ("interpolate", lambda i: ops._WeightedGather.apply(T(x), _dev(i), _dev(wk)))):
        good, holed = run(idx), run(bad)
        assert torch.isfinite(holed).all() and torch.equal(good[_dev(clean)], holed[_dev(clean)]), name
    assert np.array_equal(ops.grouping(_dev(x), _dev(bad)).cpu().numpy(), OR.group_forward(x, bad))
    assert np.array_equal(ops.subtraction(_dev(x), _dev(x2), _dev(bad)).cpu().numpy(), OR.subtract_forward(x, x2, bad))
    tx, tp, tw = T(x), T(p), T(w)
    out = ops.aggregation(tx, tp, tw, _dev(bad))
    _within(out, OR.aggregate_forward(x, p, w, bad), "aggregate forward, holes")
    out.backward(_dev(g2))
    for got, ref, what in zip((tx.grad, tp.grad, tw.grad), OR.aggregate_backward(x, p, w, bad, g2), ("input", "position", "weight")):
        _within(got, ref, f"aggregate backward with holes, grad_{what}")
    ta, tb = T(x), T(x2)
    ops.subtraction(ta, tb, _dev(bad)).backward(_dev(g3))
    r1, r2 = OR.subtract_backward(g3, bad)
    _within(ta.grad, r1, "subtract backward with holes, grad_in1")
    _within(tb.grad, r2, "subtract backward with holes, grad_in2")
    tx = T(x)
    ops.grouping(tx, _dev(bad)).backward(_dev(g3))
    _within(tx.grad, OR.group_backward(g3, bad, n), "group backward with holes")


def test_compositions_and_refusals():
    from unipre3d_amd import offset_ops as ops
    xyz, offset = OR.ragged((40, 25), 71)
    feat = np.random.default_rng(72).standard_normal((65, 6)).astype(np.float32)
    x, o, ft = _dev(xyz), _dev(offset), _dev(feat)
    idx = OR.knn(8, xyz, xyz, offset, offset)[1].astype(np.int64)
    rel = xyz[idx] - xyz[:, None, :]
    out = ops.queryandgroup(8, x, None, ft, None, o, None)
    assert out.shape == (65, 8, 9) and np.array_equal(out.cpu().numpy(), np.concatenate([rel, feat[idx]], -1))
    assert np.array_equal(ops.queryandgroup(8, x, x, ft, _dev(idx), o, o, use_xyz=False).cpu().numpy(), feat[idx])
    gx, gf = ops.querygroup(8, x, None, ft, o, None)
    assert np.array_equal(gx.cpu().numpy(), rel) and np.array_equal(gf.cpu().numpy(), feat[idx])
    bidx = OR.ballquery(0.5, 8, xyz, xyz, offset, offset).astype(np.int64)
    gx, gf = ops.querygroup(8, x, x, None, o, o, radius=0.5, query_method="ballquery")
    assert gf is None and np.array_equal(gx.cpu().numpy(), xyz[bidx] - xyz[:, None, :])
    with pytest.raises(ValueError):
        ops.knnquery(65, x, None, o, None)
    with pytest.raises(ValueError):
        ops.ballquery(0.5, 0, x, None, o, None)
    with pytest.raises(NotImplementedError):
        ops.knnquery(4, torch.zeros(65, 4, device="cuda"), None, o, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knnquery(4, x.cpu(), None, o.cpu(), None)
    with pytest.raises(ValueError):
        ops.aggregation(ft, torch.zeros(65, 8, 6, device="cuda"), torch.zeros(65, 8, 4, device="cuda"), _dev(idx))   # 6 % 4 != 0
    d2, i = ops.knn_query_raw(2, x, torch.zeros(0, 3, device="cuda"), o, torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert d2.shape == i.shape == (0, 2)
    torch.cuda.synchronize()
