"""tests/fps_ref.py against itself and against the dense C oracle (CPU only): the two forms of the ragged restatement agree, each
segment equals oracle/pointops_oracle.c on its slice where the block sizes coincide, and the documented edge cases hold."""
import math

import numpy as np
import pytest

import fps_ref
from oracle import pointops as po

MODES = ("fma_llvm", "fma_chain", "none")


def _lattice(rng, n, side=4, scale=0.25):
    """n rows drawn from {0..side-1}^3 * scale, repeats allowed: equal distances (and coincident rows) everywhere."""
    return (rng.randint(0, side, (n, 3)) * scale).astype(np.float32)


def _offsets(sizes):
    return np.cumsum(np.asarray(sizes, dtype=np.int64)).astype(np.int32)


@pytest.fixture(params=MODES)
def mode(request):
    po.set_contraction(request.param)
    yield request.param
    po.set_contraction("fma_llvm")


def test_fma_is_exactly_rounded():
    """The fp64 route of fps_ref._fma against exact rational arithmetic, including sums that sit on an fp32 rounding boundary."""
    from fractions import Fraction
    rng = np.random.RandomState(0)
    a = rng.randn(4000).astype(np.float32)
    b = rng.randn(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) + rng.randn(4000).astype(np.float32) * np.float32(1e-7)
    a = np.concatenate([a, np.float32([1 + 2 ** -12, 1 + 2 ** -23])])
    b = np.concatenate([b, np.float32([1 + 2 ** -12, 1 - 2 ** -23])])
    c = np.concatenate([c, np.float32([2 ** -60, 2 ** -24])])
    got = fps_ref._fma(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo = np.float32(float(exact))                     # fp64 rounding first can be off by one fp32 step: test the neighbours
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        err = [abs(Fraction(float(v)) - exact) for v in cands]
        best = min(err)
        winners = [float(v) for v, e in zip(cands, err) if e == best]
        if len(winners) == 2:                             # an exact tie: round to even mantissa
            winners = [w for w in winners if (np.float32(w).view(np.uint32) & 1) == 0]
        assert g == winners[0], (x, y, z)


def test_integer_log2_matches_the_double_formula():
    for n in range(1, 4097):
        pow_2 = int(math.log(float(n)) / math.log(2.0))
        want = max(min(1 << pow_2, 1024), 1)
        assert fps_ref.opt_n_threads(n) == want == po.opt_n_threads(n), n
    assert fps_ref.opt_n_threads(0) == 1 and fps_ref.opt_n_threads(10 ** 6) == 1024


@pytest.mark.parametrize("sizes,req", [([64, 17, 40], [64, 9, 30]), ([5, 130, 1], [3, 60, 1]), ([300], [120])])
def test_two_forms_agree_on_lattices_and_random_clouds(sizes, req, mode):
    rng = np.random.RandomState(sum(sizes))
    off, noff = _offsets(sizes), _offsets(req)
    for xyz in (_lattice(rng, sum(sizes)), rng.randn(sum(sizes), 3).astype(np.float32)):
        a = fps_ref.furthestsampling_ref(xyz, off, noff, mode)
        b = fps_ref.furthestsampling_lex(xyz, off, noff, mode)
        assert np.array_equal(a, b)
        for (st, ln, ost, r) in fps_ref.segments(len(xyz), len(a), off, noff):
            assert a[ost] == st and np.all((a[ost:ost + r] >= st) & (a[ost:ost + r] < st + ln))


@pytest.mark.parametrize("sizes", [[40, 63, 33], [1100, 2047, 1024], [300, 511, 256, 400]])
def test_segments_equal_the_dense_oracle_where_block_sizes_coincide(sizes, mode):
    """Every segment's own opt_n_threads equals that of the largest one, so each segment is a dense cloud of the C oracle."""
    assert len({fps_ref.opt_n_threads(s) for s in sizes}) == 1
    rng = np.random.RandomState(len(sizes))
    req = [min(s, 48) for s in sizes]
    for xyz in (_lattice(rng, sum(sizes), side=6), rng.randn(sum(sizes), 3).astype(np.float32)):
        got = fps_ref.furthestsampling_lex(xyz, _offsets(sizes), _offsets(req), mode)
        if max(sizes) <= 600:
            assert np.array_equal(got, fps_ref.furthestsampling_ref(xyz, _offsets(sizes), _offsets(req), mode))
        st = ost = 0
        for s, r in zip(sizes, req):
            want = po.furthest_point_sampling(xyz[None, st:st + s], r)[0] + st
            assert np.array_equal(got[ost:ost + r], want), (s, r)
            st, ost = st + s, ost + r


def test_dense_form_equals_the_dense_oracle(mode):
    rng = np.random.RandomState(5)
    for B, N, M in ((2, 100, 30), (1, 1500, 40), (3, 17, 17)):
        xyz = np.stack([_lattice(rng, N, side=5) for _ in range(B)])
        assert np.array_equal(fps_ref.dense_as_ragged(xyz, M, mode), po.furthest_point_sampling(xyz, M))


def test_a_small_segment_follows_the_largest_segments_block_size():
    """Four coincident-distance rows: which of two equidistant rows wins depends on bs, and bs comes from n_max."""
    pts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])          # rows 1, 2, 3 are all at distance 1 from row 0
    alone = fps_ref.furthestsampling_ref(pts, [4], [2])
    assert alone.tolist() == [0, 2]                                        # bs = 4: slots 0..3, the tree prefers slot 2 to slot 1 and 3
    rng = np.random.RandomState(1)
    big = np.concatenate([pts, rng.randn(1, 3).astype(np.float32)])        # n_max = 5 -> still bs = 4
    assert fps_ref.furthestsampling_ref(big, [4, 5], [2, 3])[:2].tolist() == [0, 2]
    one = np.concatenate([pts[:3], rng.randn(1, 3).astype(np.float32)])    # segments of 3 and 1 rows: bs = 2
    got = fps_ref.furthestsampling_ref(one, [3, 4], [2, 3])
    assert got[:2].tolist() == [0, 2] and np.array_equal(got, fps_ref.furthestsampling_lex(one, [3, 4], [2, 3]))


def test_more_selections_than_points_zero_requests_and_empty_segments(mode):
    rng = np.random.RandomState(9)
    sizes, req = [1, 6, 0, 5, 0, 4], [3, 11, 0, 0, 3, 4]
    xyz = _lattice(rng, sum(sizes), side=3)
    off, noff = _offsets(sizes), _offsets(req)
    a = fps_ref.furthestsampling_ref(xyz, off, noff, mode)
    assert np.array_equal(a, fps_ref.furthestsampling_lex(xyz, off, noff, mode)) and len(a) == sum(req)
    assert a[:3].tolist() == [0, 0, 0]                                     # one row asked three times
    seg1 = a[3:14]
    assert seg1[0] == 1 and set(seg1.tolist()) <= set(range(1, 7))
    # once every distinct position is taken all minima are 0 and the first row of the segment wins every time
    distinct = len({tuple(r) for r in xyz[1:7].tolist()})
    assert np.all(seg1[distinct:] == 1)
    assert a[14:17].tolist() == [-1, -1, -1]                               # empty segment, three requests
    assert sorted(a[17:21].tolist()) == [12, 13, 14, 15] or len({tuple(r) for r in xyz[12:16].tolist()}) < 4
    # zero request: the segment of five rows (7..11) appears nowhere
    assert not np.any((a >= 7) & (a < 12))
    # offsets beyond the tensor are clamped
    b = fps_ref.furthestsampling_ref(xyz, [4, 100], [2, 5], mode)
    assert b[0] == 0 and b[2] == 4 and np.all(b[2:] < len(xyz))
    assert len(fps_ref.furthestsampling_ref(xyz, off, noff, mode, m=sum(req) + 2)) == sum(req) + 2
