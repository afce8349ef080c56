"""The scatter-add gradients of the point operators (u3d_group_points_grad / u3d_gather_points_grad, u3d_three_interpolate_grad) at EVERY
rows-per-workgroup class of their LDS kernels (CB = 1, 2, 4, 8, 16) and in the global-atomic kernel (0), against the plain fp64 references of
tests/pointops_grad_ref.py, on index sets whose runs are placed on purpose (row, wave and step boundaries of the segmented scan).

The library says which kernel a shape launches (u3d_*_grad_rows, host arithmetic), so the shape lists are checked for coverage without a GPU.
These kernels do not depend on the contraction mode of the three-term sums; the file stays apart from test_gpu_pointops.py's mode fixture."""
import numpy as np
import pytest

import pointops_grad_ref as R

gpu = pytest.mark.gpu
CLASSES = [0, 1, 2, 4, 8, 16]

# (b, c, len): len = n of the grouping gradient, m of the interpolation gradient.  c = 3073 with b = 1, 3, 7, 15 are the smallest shapes of the
# classes 2, 4, 8, 16 (b * c >= 3072 * (CB - 1) + 1) and leave a channel tail of ONE row; the second shape of a class has c % CB == 0.
EXACT_SHAPES = [(1, 3, 16385), (2, 37, 48), (1, 3072, 1024), (1, 5, 16384),
                (1, 3073, 48), (1, 3074, 1024), (1, 3073, 8192),
                (3, 3073, 48), (3, 3076, 1024),
                (7, 3073, 48), (7, 3080, 48),
                (15, 3073, 48), (15, 3088, 1024)]
VALUE_SHAPES = [(2, 37, 48), (3, 3073, 48), (15, 3073, 48)]          # CB = 1, 4, 16
NONFINITE_SHAPE = (3, 3073, 48)                                       # CB = 4
INTERP_POINTS = 300                                                   # two steps of 256 threads, the second one partial
ROTATE = 61                                                           # cloud i uses the destinations (d + 61 i) mod n


def _rows():
    from unipre3d_amd import pointops
    lib = pointops.load()
    return lib.u3d_group_points_grad_rows, lib.u3d_three_interpolate_grad_rows


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ---- a. coverage: no GPU ----------------------------------------------------------------------------------------------------------------------
def test_shape_lists_reach_every_kernel_class():
    """plain integer arithmetic through the library's own choice: an edit of the shape lists or of lds_rows cannot lose a class unnoticed"""
    for rows in _rows():
        got = {s: rows(*s) for s in EXACT_SHAPES}
        assert sorted(set(got.values())) == CLASSES, got
        for cb in CLASSES[2:]:
            cs = [c for (b, c, n), v in got.items() if v == cb]
            assert any(c % cb != 0 for c in cs) and any(c % cb == 0 for c in cs), (cb, cs)
        assert [rows(*s) for s in VALUE_SHAPES] == [1, 4, 16] and rows(*NONFINITE_SHAPE) == 4
        # the row count: 3072 rows per doubling
        assert rows(1, 3072, 48) == 1 and rows(1, 3073, 48) == 2 and rows(3072, 1, 48) == 1 and rows(3073, 1, 48) == 2
        assert [rows(b, 3073, 48) for b in (1, 2, 3, 6, 7, 14, 15, 64)] == [2, 2, 4, 4, 8, 8, 16, 16]
        # the row length: CB rows of `len` floats fit 64 KB
        assert rows(64, 3073, 8192) == 2 and rows(64, 3073, 8193) == 1
        assert rows(64, 3073, 16384) == 1 and rows(64, 3073, 16385) == 0 and rows(1, 1, 16385) == 0
        assert rows(64, 3073, 1024) == 16 and rows(64, 3073, 1025) == 8
        assert rows(64, 3073, 4096) == 4 and rows(64, 3073, 4097) == 2


def _segs(idx):
    return [(v, s) for v in R.wave_view(idx) for s in v["segs"]]


def test_structured_index_sets_place_their_runs_where_they_claim():
    sets = R.named_sets()
    assert all(0 <= s.min() and s.max() < R.N_DEST and s.dtype == np.int32 for s in sets.values())
    main = sets["main"]
    assert 590 <= len(main) <= 610
    lengths = {l for s in sets.values() for _, l, _ in R.runs_of(s)}
    assert lengths >= {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300}
    runs, segs = R.runs_of(main), [s for _, s in _segs(main)]
    assert {l for _, l, _ in runs} >= {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65}
    for lo in (15, 31, 47):                                              # a run that crosses this pair of lanes and no other row boundary
        assert any(a <= lo < b and a > lo - 16 and b < lo + 17 for a, b, _ in segs), lo
    assert any(a < 16 and b > 48 for a, b, _ in segs)
    assert any(a < 32 <= b and a >= 16 for a, b, _ in segs) and any(a < 32 <= b and a < 16 for a, b, _ in segs)
    assert any(p % 64 % 16 == 0 and l == 16 for p, l, _ in runs), "a run covering exactly one row"
    assert any(p % 64 == 0 and l == 64 for p, l, _ in runs), "a run covering exactly one wave"
    assert any(p // 64 != (p + l - 1) // 64 and p // 256 == (p + l - 1) // 256 for p, l, _ in runs), "a run over a wave boundary"
    assert any(p // 256 != (p + l - 1) // 256 for p, l, _ in runs), "a run over a step boundary"
    assert any(v["segs"][i][1] + 1 == v["segs"][i + 1][0] and v["segs"][i + 1][0] % 16 == 0 and v["segs"][i][2] != v["segs"][i + 1][2]
               and v["segs"][i][1] > v["segs"][i][0] and v["segs"][i + 1][1] > v["segs"][i + 1][0]
               for v in R.wave_view(main) for i in range(len(v["segs"]) - 1)), "two runs meeting exactly at a row boundary"
    assert any(v["active"] == 64 and not v["scan"] for v in R.wave_view(main)), "a full wave that skips the scan"
    assert any(v["scan"] for v in R.wave_view(main))
    last = R.wave_view(main)[-1 - sum(v["active"] == 0 for v in R.wave_view(main))]
    assert 0 < last["active"] < 64 and last["segs"][-1][1] == last["active"] - 1 and last["segs"][-1][0] < last["segs"][-1][1]
    # the 300-entry run spans whole waves and the step boundary
    (p, l, _), = [r for r in R.runs_of(sets["long300"]) if r[1] == 300]
    assert p // 256 != (p + l - 1) // 256 and sum(v["segs"] == [(0, 63, 0)] for v in R.wave_view(sets["long300"])) >= 3
    alt = sets["alternating"]
    assert len(alt) >= 128 and len(set(alt.tolist())) == 2 and all(l == 1 for _, l, _ in R.runs_of(alt))
    assert not any(v["scan"] for v in R.wave_view(alt))
    for t in R.TOTALS:                                                   # every total ends inside a run (a lone entry is its own)
        s = sets[f"one_destination_{t}"]
        assert len(s) == t and len(R.runs_of(s)) == 1
    assert {len(s) for s in sets.values()} >= set(R.TOTALS[:-1]) and any(590 <= len(s) <= 610 for s in sets.values())
    bq = R.ball_query_set()
    assert bq.shape == (33, 32) and not bq[0].any()
    for h in range(1, 33):
        assert len(set(bq[h, :h].tolist())) == h and np.all(np.diff(bq[h, :h]) > 0) and np.all(bq[h, h:] == bq[h, 0])
    assert max(l for _, l, _ in R.runs_of(bq.reshape(-1))) >= 31
    ov, places = R.overflow_set()
    assert len(ov) == 64 and [p % 16 for p, _, _ in places] == [5, 14, 15]
    for p, d0, d1 in places:
        assert ov[p - 1] != d0 and list(ov[p:p + 7]) == [d0] * 2 + [d1] * 4 + [ov[p + 6]] and ov[p + 6] != d1
        assert np.count_nonzero(ov == d0) == 2 and np.count_nonzero(ov == d1) == 4


def test_references_agree_with_a_scalar_loop():
    """the matmul form against the definition, on a shape small enough to loop over"""
    rng = np.random.RandomState(3)
    go = rng.randn(2, 3, 40); idx = rng.randint(0, 7, (2, 10, 4)); idx[:, :, 2:] = idx[:, :, :1]
    g, cnt, mag = R.group_grad_fp64(go, idx, 9)
    eg, ec, em = np.zeros((2, 3, 9)), np.zeros((2, 1, 9)), np.zeros((2, 3, 9))
    for b in range(2):
        for e, d in enumerate(idx[b].reshape(-1)):
            eg[b, :, d] += go[b, :, e]; em[b, :, d] += np.abs(go[b, :, e]); ec[b, 0, d] += 1
    assert np.allclose(g, eg, rtol=0, atol=1e-13) and np.allclose(mag, em, rtol=0, atol=1e-13) and np.array_equal(cnt, ec)
    assert not g[:, :, 7:].any() and not cnt[:, :, 7:].any()
    go = rng.randn(2, 3, 20); i3 = rng.randint(0, 6, (2, 20, 3)); i3[:, ::3, 1] = i3[:, ::3, 0]; w = rng.rand(2, 20, 3)
    g, cnt, mag = R.interp_grad_fp64(go, i3, w, 8)
    eg, ec, em = np.zeros((2, 3, 8)), np.zeros((2, 1, 8)), np.zeros((2, 3, 8))
    for b in range(2):
        for p in range(20):
            for k in range(3):
                eg[b, :, i3[b, p, k]] += go[b, :, p] * w[b, p, k]; em[b, :, i3[b, p, k]] += np.abs(go[b, :, p]) * w[b, p, k]
                ec[b, 0, i3[b, p, k]] += 1
    assert np.allclose(g, eg, rtol=0, atol=1e-13) and np.allclose(mag, em, rtol=0, atol=1e-13) and np.array_equal(cnt, ec)
    # integer cotangents, weights in eighths: exact
    go = rng.randint(-8, 9, (1, 2, 20)).astype(np.float64); w = rng.randint(0, 9, (1, 20, 3)) / 8.0
    g, _, _ = R.interp_grad_fp64(go, i3[:1], w, 8)
    assert np.array_equal(g * 8, np.round(g * 8))


# ---- helpers of the GPU tests -----------------------------------------------------------------------------------------------------------------
def _rotated(idx1d, b, n):
    return np.stack([(idx1d.astype(np.int64) + ROTATE * i) % n for i in range(b)]).astype(np.int32)


def _same(got, want, what):
    """bit-for-bit equality of two device tensors (NaN equals NaN), with the first mismatch in the message"""
    import torch
    if torch.equal(got, want):
        return
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    if not bool(bad.any()):
        return
    at = tuple(int(x) for x in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: got {got[at].item()!r}, want {want[at].item()!r}")


def _group_grad(go_t, idx_t, out_t, gather=False):
    """the C-ABI call itself, ACCUMULATING into out_t (b, c, n); idx_t (b, total)"""
    from unipre3d_amd import _lib, pointops
    b, c, n = out_t.shape
    total = idx_t.shape[1]
    lib, s = pointops.load(), _lib.stream_ptr(out_t.device)
    if gather:
        rc = lib.u3d_gather_points_grad(b, c, n, total, _lib.ptr(go_t), _lib.ptr(idx_t), _lib.ptr(out_t), s)
    else:
        k = 4 if total % 4 == 0 else 1
        rc = lib.u3d_group_points_grad(b, c, n, total // k, k, _lib.ptr(go_t), _lib.ptr(idx_t), _lib.ptr(out_t), s)
    assert rc == 0


def _interp_grad(go_t, idx_t, w_t, out_t):
    from unipre3d_amd import _lib, pointops
    b, c, m = out_t.shape
    rc = pointops.load().u3d_three_interpolate_grad(b, c, idx_t.shape[1], m, _lib.ptr(go_t), _lib.ptr(idx_t), _lib.ptr(w_t), _lib.ptr(out_t),
                                                    _lib.stream_ptr(out_t.device))
    assert rc == 0


def _exact_f32(ref):
    f = ref.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), ref), "the integer-valued reference must be representable in fp32"
    return f


def _check_group_exact(b, c, n, idx1d, seed):
    import torch
    from unipre3d_amd import pointops
    dev = torch.device("cuda:0")
    idx = _rotated(idx1d, b, n)
    total = idx.shape[1]
    go = np.random.RandomState(seed).randint(-8, 9, (b, c, total)).astype(np.float32)
    ref, cnt, _ = R.group_grad_fp64(go, idx, n, with_mag=False)
    assert (cnt == 0).any() == (len(np.unique(idx1d)) < n) and not ref[np.broadcast_to(cnt == 0, ref.shape)].any()   # untouched destinations: exactly 0
    ref_t, go_t, idx_t = torch.from_numpy(_exact_f32(ref)).to(dev), torch.from_numpy(go).to(dev), torch.from_numpy(idx).to(dev)
    for gather in (False, True):
        acc = torch.zeros(b, c, n, device=dev)
        _group_grad(go_t, idx_t, acc, gather)
        _same(acc, ref_t, f"group_points_grad{' (gather)' if gather else ''} {b}x{c}x{n}, {total} entries")
        _group_grad(go_t, idx_t, acc, gather)                                                # read-modify-write: adds, never overwrites
        _same(acc, 2 * ref_t, f"second accumulation{' (gather)' if gather else ''} {b}x{c}x{n}")
    del acc
    # autograd wrappers (their zero-fill): grouping when the entries split into groups of 4, gather always
    f = torch.full((b, c, n), 3.0, device=dev).requires_grad_(True)
    if total % 4 == 0:
        out = pointops.grouping_operation(f, idx_t.view(b, total // 4, 4))
        out.backward(go_t.view_as(out), retain_graph=True)
        _same(f.grad, ref_t, f"grouping_operation backward {b}x{c}x{n}")
        out.backward(go_t.view_as(out))
        _same(f.grad, 2 * ref_t, f"grouping_operation second backward {b}x{c}x{n}")
        f.grad = None
    out = pointops.gather_operation(f, idx_t)
    out.backward(go_t)
    _same(f.grad, ref_t, f"gather_operation backward {b}x{c}x{n}")


def _interp_inputs(b, c, m, idx, seed, integer):
    rng = np.random.RandomState(seed)
    n = idx.shape[1]
    if integer:
        return rng.randint(-8, 9, (b, c, n)).astype(np.float32), (rng.randint(0, 9, (b, n, 3)) / 8.0).astype(np.float32)
    return rng.standard_normal((b, c, n)).astype(np.float32), rng.rand(b, n, 3).astype(np.float32)


# ---- b. every class, exact --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_id)
def test_group_grad_every_class_exact(shape):
    """Integer cotangents in [-8, 8]: every partial sum is exact, so the result equals the fp64 reference bit for bit in any summation order;
    destinations without a term are exactly 0.  The structured 604-entry set, its destinations rotated per cloud."""
    b, c, n = shape
    print(f"[pointops] group grad {b}x{c}x{n}: rows per workgroup {_rows()[0](b, c, n)}")
    _check_group_exact(b, c, n, R.main_set(), seed=c + n)


@gpu
@pytest.mark.parametrize("name", sorted(R.named_sets()))
@pytest.mark.parametrize("shape", [(2, 37, 48), (3, 3073, 48)], ids=_id)
def test_group_grad_named_sets_exact(shape, name):
    """every named index set (run of 300, a/b/a/b, one destination at every total, ball-query padding) at CB = 1 and at CB = 4 with a tail"""
    b, c, n = shape
    _check_group_exact(b, c, n, R.named_sets()[name], seed=len(name) + c)


@gpu
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_id)
def test_interp_grad_every_class_exact(shape):
    """Integer cotangents, weights in eighths: exact in any order.  Random triples, i0 == i1 == i2, one destination, the crowded pattern."""
    import torch
    from unipre3d_amd import pointops
    b, c, m = shape
    dev = torch.device("cuda:0")
    print(f"[pointops] three_interpolate grad {b}x{c}x{m}: rows per workgroup {_rows()[1](b, c, m)}")
    for name, idx in R.interp_sets(b, INTERP_POINTS, m, seed=c).items():
        go, w = _interp_inputs(b, c, m, idx, seed=m + len(name), integer=True)
        ref, cnt, _ = R.interp_grad_fp64(go, idx, w, m, with_mag=False)
        assert (cnt == 0).any() or name != "one_destination"
        ref_t = torch.from_numpy(_exact_f32(ref)).to(dev)
        go_t, idx_t, w_t = (torch.from_numpy(a).to(dev) for a in (go, idx, w))
        acc = torch.zeros(b, c, m, device=dev)
        _interp_grad(go_t, idx_t, w_t, acc)
        _same(acc, ref_t, f"three_interpolate_grad {b}x{c}x{m} {name}")
        _interp_grad(go_t, idx_t, w_t, acc)
        _same(acc, 2 * ref_t, f"three_interpolate_grad second accumulation {b}x{c}x{m} {name}")
        del acc
        f = torch.full((b, c, m), 3.0, device=dev).requires_grad_(True)
        out = pointops.three_interpolate(f, idx_t, w_t)
        out.backward(go_t, retain_graph=True)
        _same(f.grad, ref_t, f"three_interpolate backward {b}x{c}x{m} {name}")
        out.backward(go_t)
        _same(f.grad, 2 * ref_t, f"three_interpolate second backward {b}x{c}x{m} {name}")


def test_interp_crowded_pattern_is_the_existing_tests():
    idx = R.interp_sets(2, 2048, 512, seed=1)["crowded"]
    assert np.all(idx[:, ::2, 0] == 7) and np.all(idx[:, 1::3, 2] == 7)


# ---- c. Gaussian values, derived bound --------------------------------------------------------------------------------------------------------
def _order_bound_check(got, ref, cnt, mag, extra, what):
    """|got - fp64| <= (count + extra) x 2^-24 x sum |terms| per element: `count - 1` additions (+ `extra + 1` roundings of the terms
    themselves), each off by at most half an ulp = 2^-24 of a partial sum that never exceeds sum |terms| -- whatever the order.  Elements with
    one term are that term rounded once, elements without any are 0.  Returns the worst error / bound."""
    got64 = got.astype(np.float64)
    cnt = np.broadcast_to(cnt, ref.shape)
    assert not got[cnt == 0].any(), f"{what}: a destination without a term is not 0"
    one = cnt == 1
    assert np.array_equal(got[one], ref[one].astype(np.float32)), f"{what}: a single term is not copied exactly"
    err, bound = np.abs(got64 - ref), (cnt + extra) * 2.0 ** -24 * mag
    many = cnt > 1
    ratio = float((err[many] / bound[many]).max()) if many.any() else 0.0
    print(f"[pointops] {what}: worst error / any-order bound {ratio:.3f} (largest count {int(cnt.max())})")
    assert np.all(err[many] <= bound[many]), f"{what}: {ratio:.3f} x the any-order bound"
    return ratio


@gpu
@pytest.mark.parametrize("name", sorted(R.named_sets()))
@pytest.mark.parametrize("shape", VALUE_SHAPES, ids=_id)
def test_group_grad_gaussian_within_the_any_order_bound(shape, name):
    import torch
    b, c, n = shape
    dev = torch.device("cuda:0")
    idx = _rotated(R.named_sets()[name], b, n)
    go = np.random.default_rng(c + len(name)).standard_normal((b, c, idx.shape[1]), dtype=np.float32)
    ref, cnt, mag = R.group_grad_fp64(go, idx, n)
    acc = torch.zeros(b, c, n, device=dev)
    _group_grad(torch.from_numpy(go).to(dev), torch.from_numpy(idx).to(dev), acc)
    _order_bound_check(acc.cpu().numpy(), ref, cnt, mag, 0, f"group grad CB {_rows()[0](b, c, n)} {name}")


@gpu
@pytest.mark.parametrize("shape", VALUE_SHAPES + [(2, 40, 512)], ids=_id)
def test_interp_grad_gaussian_within_the_any_order_bound(shape):
    import torch
    b, c, m = shape
    dev = torch.device("cuda:0")
    n = 2048 if m == 512 else INTERP_POINTS                              # (40, 2048, 512): the crowded case of test_gpu_pointops.py
    for name, idx in R.interp_sets(b, n, m, seed=c + 1).items():
        go, w = _interp_inputs(b, c, m, idx, seed=m + len(name), integer=False)
        ref, cnt, mag = R.interp_grad_fp64(go, idx, w, m)
        acc = torch.zeros(b, c, m, device=dev)
        _interp_grad(*(torch.from_numpy(a).to(dev) for a in (go, idx, w)), acc)
        _order_bound_check(acc.cpu().numpy(), ref, cnt, mag, 1, f"three_interpolate grad CB {_rows()[1](b, c, m)} {name}")


# ---- d. non-finite and overflowing values (grouping) ------------------------------------------------------------------------------------------
def _nonfinite_base(idx1d):
    import torch
    b, c, n = NONFINITE_SHAPE
    idx = _rotated(idx1d, b, n)
    go = np.random.RandomState(17).randint(-8, 9, (b, c, idx.shape[1])).astype(np.float32)
    ref, _, _ = R.group_grad_fp64(go, idx, n, with_mag=False)
    dev = torch.device("cuda:0")
    return dict(idx=idx, go=go, ref=_exact_f32(ref), go_t=torch.from_numpy(go).to(dev), idx_t=torch.from_numpy(idx).to(dev))


@pytest.fixture(scope="module")
def nonfinite_main():
    return _nonfinite_base(R.main_set())


@pytest.fixture(scope="module")
def nonfinite_overflow():
    return _nonfinite_base(R.overflow_set()[0])


CLOUD, CHANNEL = 1, 4 * 100 + 1                                       # one channel of one CB = 4 workgroup
INF, NAN = float("inf"), float("nan")


def _place_and_check(base, placed, what):
    """set grad_out[CLOUD, CHANNEL, position] = value for every (position, value), run the kernel, and expect: the destinations that own a
    placed value hold the IEEE sum of their terms; EVERYTHING else -- the rest of that channel, the other channels of its workgroup (whose
    waves take the select form with it), every other workgroup -- equals the finite reference exactly."""
    import torch
    b, c, n = NONFINITE_SHAPE
    go_t = base["go_t"].clone()
    want = base["ref"].copy()
    row = base["go"][CLOUD, CHANNEL].astype(np.float64)
    for p, v in placed:
        go_t[CLOUD, CHANNEL, p] = v
        row[p] = np.float32(v)
    owners = sorted({int(base["idx"][CLOUD, p]) for p, _ in placed})
    with np.errstate(invalid="ignore", over="ignore"):
        for d in owners:
            want[CLOUD, CHANNEL, d] = np.float32(row[base["idx"][CLOUD] == d].sum())
    assert not np.isfinite(want[CLOUD, CHANNEL, owners]).any() and np.isfinite(want).sum() == want.size - len(owners)
    acc = torch.zeros(b, c, n, device=go_t.device)
    _group_grad(go_t, base["idx_t"], acc)
    torch.cuda.synchronize()                                             # data values, not faults: the kernel completes normally
    _same(acc, torch.from_numpy(want).to(acc.device), what)


_RUN31_LAST, _RUN32_FIRST, _RUN64_INSIDE = 351, 352, 400                 # main_set(): run of 31 on 321-351, of 32 on 352-383, of 64 on 384-447


@gpu
@pytest.mark.parametrize("value", [INF, -INF, NAN], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("where", ["inside_a_long_run", "last_lane_of_a_run", "first_lane_of_the_next_run", "inside_a_run_over_rows"])
def test_group_grad_nonfinite_value_stays_in_its_run(nonfinite_main, where, value):
    m = R.main_set()
    assert m[_RUN31_LAST] != m[_RUN32_FIRST] and m[_RUN31_LAST - 30] == m[_RUN31_LAST] and m[_RUN32_FIRST + 31] == m[_RUN32_FIRST]
    assert m[384] == m[_RUN64_INSIDE] == m[447] and m[129] == m[150] == m[191]
    pos = {"inside_a_long_run": _RUN64_INSIDE, "last_lane_of_a_run": _RUN31_LAST, "first_lane_of_the_next_run": _RUN32_FIRST,
           "inside_a_run_over_rows": 150}[where]
    _place_and_check(nonfinite_main, [(pos, value)], f"{value} {where}")


@gpu
def test_group_grad_opposite_infinities_in_one_run_give_nan(nonfinite_main):
    _place_and_check(nonfinite_main, [(395, INF), (420, -INF)], "+inf and -inf in one run")


@gpu
@pytest.mark.parametrize("place", [0, 1, 2], ids=["inside_a_row", "ending_on_a_row_boundary", "across_a_row_boundary"])
def test_group_grad_overflowing_run_does_not_poison_the_next(nonfinite_overflow, place):
    """3e38 + 3e38 overflows to +inf although both inputs are finite.  The run that follows holds small integers and must come out as their
    exact sum: a 0-multiplier of the scan times the neighbour's +inf would make it NaN."""
    p, d0, d1 = R.overflow_set()[1][place]
    _place_and_check(nonfinite_overflow, [(p, 3e38), (p + 1, 3e38)], f"overflowing pair on lanes {p}, {p + 1}")


# ---- e. ball query edges that feed the gradient -----------------------------------------------------------------------------------------------
def _ball_cloud(n, hit_lists):
    """one cloud of n points and len(hit_lists) queries: query q sits at (10 q, 0, 0) and exactly the points hit_lists[q] lie within 0.5 of it"""
    rng = np.random.RandomState(n)
    xyz = np.full((n, 3), 1000.0, np.float32) + rng.rand(n, 3).astype(np.float32)
    new = np.zeros((len(hit_lists), 3), np.float32)
    for q, hits in enumerate(hit_lists):
        new[q, 0] = 10.0 * q
        assert len(set(hits)) == len(hits)
        xyz[list(hits)] = new[q] + (rng.rand(len(hits), 3).astype(np.float32) - np.float32(0.5)) * np.float32(0.5)
    assert len({h for hits in hit_lists for h in hits}) == sum(len(h) for h in hit_lists)
    return xyz, new


BALL_CASES = [  # (n, nsample, hit lists of the queries)
    (600, 65, [[], [301], list(range(5, 145, 2)), list(range(150, 300, 3)) + list(range(400, 420))]),      # 0, 1, 70 (over three ballots), 70
    (600, 128, [[], [599], list(range(1, 211, 3)), list(range(300, 429)), list(range(440, 568))]),         # 0, 1, 70, 129 (> nsample), 128
    (37, 32, [[], [36], [0, 1, 35], list(range(2, 35))]),                                                  # n < 64; 33 hits > nsample
    (50, 65, [[3, 4, 49], list(range(10, 40))]),                                                           # n < 64 < nsample
    (200, 32, [list(range(0, 40, 2)) + list(range(70, 100)), list(range(40, 64)) + list(range(120, 128)) + list(range(130, 140))]),  # 20 then 30 hits: crosses 32 inside the second ballot; exactly 32 at a ballot's end
    (200, 65, [list(range(0, 40)) + list(range(64, 94)), list(range(40, 64)) + list(range(94, 128)) + list(range(128, 200, 5))]),  # 40 + 30 and 24 + 34 + 15: cross 65 inside the second / third ballot
]


@gpu
@pytest.mark.parametrize("case", range(len(BALL_CASES)))
def test_ball_query_padding_and_ballot_edges(case):
    """Bit for bit against the oracle: nsample beyond one wave (the padding loop strides by 64), clouds smaller than a wave, and hit counts that
    reach nsample in the middle of a 64-point ballot; the index sets then feed the grouping gradient (exact, integer cotangents)."""
    import torch
    from oracle import pointops as po
    from unipre3d_amd import pointops
    n, k, hit_lists = BALL_CASES[case]
    dev = torch.device("cuda:0")
    xyz, new = _ball_cloud(n, hit_lists)
    xyz, new = np.stack([xyz, xyz[::-1].copy()]), np.stack([new, new])                      # second cloud: the same hits in reversed index order
    want = po.ball_query(0.5, k, xyz, new)
    for q, hits in enumerate(hit_lists):                                                     # the construction gives the hit counts it claims
        h = sorted(hits)[:k]
        assert list(want[0, q]) == h + [h[0] if h else 0] * (k - len(h)), (q, want[0, q])
    got = pointops.ball_query(0.5, k, torch.from_numpy(xyz).to(dev), torch.from_numpy(new).to(dev))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    go = np.random.RandomState(case).randint(-8, 9, (2, 5, len(hit_lists) * k)).astype(np.float32)
    ref, _, _ = R.group_grad_fp64(go, want, n, with_mag=False)
    acc = torch.zeros(2, 5, n, device=dev)
    _group_grad(torch.from_numpy(go).to(dev), got.view(2, -1), acc)
    _same(acc, torch.from_numpy(_exact_f32(ref)).to(dev), f"group grad on ball query output, case {case}")
