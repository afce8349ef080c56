"""HIP k-nearest-neighbour search (include/unipre3d_knn.h) against the CPU restatement tests/knn_ref.py: indices AND squared distances
bit for bit, at the sizes where the launch changes shape, on clouds full of exact ties, and through every Python entry point against
the indices recorded from the reference's own functions (tests/golden/g16_knn.npz).

The kernel has one path; what changes with the shape is the number of LDS tiles (u3d_knn_path: U3D_KNN_TILE = 2048 points each), the
number of 64-candidate steps in a tile (one candidate per lane), how many of a workgroup's U3D_KNN_QUERIES = 16 query slots (one per
wave) are live, and -- with the data -- whether a step's candidates are inserted one by one or sorted and merged."""
import numpy as np
import pytest
import torch

import knn_ref as KR

pytestmark = pytest.mark.gpu

RECORDED_SORTED = ("layers_knn_point", "layers_knn_KNN", "group_KNN", "pcm_knn_point")


def _cloud(B, N, seed, quantized=False):
    p = np.random.default_rng(seed).uniform(-1, 1, (B, N, 3)).astype(np.float32)
    return (np.round(p * 8) / 8).astype(np.float32) if quantized else p       # eighths: duplicates and equal distances everywhere


def _run(k, support, query):
    from unipre3d_amd import knn
    d2, idx = knn.knn_query(k, torch.from_numpy(support).cuda(), torch.from_numpy(query).cuda())
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (support.shape[0], query.shape[1], k)
    return d2.cpu().numpy(), idx.cpu().numpy()


def _assert_exact(got, want, what):
    (gd, gi), (wd, wi) = got, want
    print(f"{what}: rows with a differing index {int((gi != wi).any(-1).sum())} of {wi.shape[0] * wi.shape[1]}, "
          f"differing d2 words {int((gd.view(np.uint32) != wd.view(np.uint32)).sum())}")
    assert np.array_equal(gi, wi), what
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


# (b, n, m, k, quantized): n around the 64-candidate step (63 | 64 | 65), around the LDS tile (2047 | 2048 | 2049) and its second
# boundary (4097); k over {1, 2, 12, 31, 32, 33, 63, 64} incl. k == n; m around the workgroup's 16 query slots; b 1 and 3
SHAPES = [(1, 1, 1, 1, False), (3, 2, 1, 2, False), (1, 2, 17, 1, False), (1, 63, 15, 63, False), (3, 63, 16, 12, True),
          (1, 64, 17, 64, False), (1, 64, 77, 31, True), (3, 65, 1, 64, False), (1, 65, 15, 33, True), (1, 65, 5, 2, False),
          (1, 2047, 16, 32, False), (3, 2047, 17, 12, True), (1, 2048, 77, 63, True), (1, 2048, 15, 1, False), (3, 2049, 16, 64, True),
          (1, 2049, 77, 12, False), (1, 2049, 1, 33, False), (1, 4097, 17, 31, True), (1, 8200, 17, 32, False)]


@pytest.mark.parametrize("b,n,m,k,quantized", SHAPES)
def test_bit_exact_at_every_boundary(b, n, m, k, quantized):
    from unipre3d_amd import knn
    assert knn.load().u3d_knn_path(n, k) == (n + knn.TILE - 1) // knn.TILE
    support = _cloud(b, n, seed=n * 131 + k, quantized=quantized)
    query = _cloud(b, m, seed=m * 17 + 1, quantized=quantized)
    take = np.arange(0, m, 3)                                                 # every third query is a support point itself
    query[:, take] = support[:, (take * 7) % n]
    _assert_exact(_run(k, support, query), KR.knn(k, support, query), f"(b, n, m, k) = {(b, n, m, k)}")


def test_every_candidate_enters():
    """Support points in order of DEcreasing distance from the query: each one is below the bar when it arrives, so every step of both
    tiles takes the sort-and-merge route (a uniform cloud takes it on the first steps only)."""
    p = _cloud(1, 2049, seed=9)
    order = np.argsort(-KR.dist2(p, np.zeros((1, 1, 3), np.float32))[0, 0], kind="stable")
    support, query = np.ascontiguousarray(p[:, order]), np.zeros((1, 5, 3), np.float32)
    _assert_exact(_run(32, support, query), KR.knn(32, support, query), "descending distances")


@pytest.mark.parametrize("below", [0, 1, 8, 9, 64])
def test_both_sides_of_the_merge_threshold(below):
    """The second step of 64 candidates holds exactly `below` points under the bar: up to 8 are inserted one by one, 9 and more are
    sorted and merged (csrc/u3d_knn.hip: KNN_MERGE_ABOVE).  k = 64 keeps the bar at the farthest point of the first step."""
    rng = np.random.default_rng(below)
    unit = rng.standard_normal((1, 128, 3))
    unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
    radius = np.concatenate([rng.uniform(2, 3, 64), rng.permutation(np.r_[rng.uniform(0.1, 1, below), rng.uniform(4, 5, 64 - below)])])
    support = (unit * radius[None, :, None]).astype(np.float32)
    query = np.zeros((1, 3, 3), np.float32)
    got, want = _run(64, support, query), KR.knn(64, support, query)
    assert int((want[1][0, 0] >= 64).sum()) == below
    _assert_exact(got, want, f"{below} candidates below the bar")


@pytest.mark.parametrize("cloud", ["lattice", "duplicated", "identical"])
def test_ties_go_to_the_lower_index(cloud):
    p = {"lattice": KR.lattice, "duplicated": KR.duplicated, "identical": lambda: np.full((2, 70, 3), 0.25, np.float32)}[cloud]()
    d2, idx = _run(8, p, p)
    _assert_exact((d2, idx), KR.knn(8, p, p), cloud)
    assert (np.diff(KR.keys(d2, idx).astype(object), axis=-1) > 0).all()
    if cloud == "identical":
        assert (idx == np.arange(8)).all() and (d2 == 0).all()


@pytest.fixture(scope="module")
def g16(golden):
    """[(k, support, query, {recorded name: idx}, restatement (d2, idx))] of the four recorded cases, computed once."""
    z = golden("g16_knn.npz")
    out = []
    for i, (B, N, M, k) in enumerate(z["cases"].tolist()):
        support = z[f"c{i}_support"]
        query = np.take_along_axis(support, z[f"c{i}_qsel"].astype(np.int64)[:, :, None], 1)
        rec = {n: z[f"c{i}_{n}"].astype(np.int64) for n in RECORDED_SORTED + ("pointmlp_knn_point",)}
        out.append((k, support, query, rec, KR.knn(k, support, query)))
    return out


def _assert_root_within_2ulp(dist, d2_ref, what):
    want = np.sqrt(d2_ref.astype(np.float32))
    err = np.abs(dist.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(want, np.float32(1e-30)))
    print(f"{what}: largest distance error {err.max():.2f} ulp of sqrt(restatement d2)")
    assert dist.dtype == np.float32 and err.max() <= 2.0, what


@pytest.mark.parametrize("case", range(4))
def test_golden_through_every_entry_point(g16, case):
    """Each Python entry point reproduces, exactly, the indices recorded from the reference function it stands for."""
    from unipre3d_amd import knn
    k, support, query, rec, (d2_ref, idx_ref) = g16[case]
    s, q = torch.from_numpy(support).cuda(), torch.from_numpy(query).cuda()
    d2, idx = knn.knn_query(k, s, q)
    _assert_exact((d2.cpu().numpy(), idx.cpu().numpy()), (d2_ref, idx_ref), f"g16 case {case}")
    # layers/knn.py knn_point and its KNN module (the same call; the module adds .int())
    dist, i64 = knn.knn_point(k, q, s)
    assert i64.dtype == torch.int64 and np.array_equal(i64.cpu().numpy(), rec["layers_knn_point"])
    assert np.array_equal(i64.int().cpu().numpy(), rec["layers_knn_KNN"])
    _assert_root_within_2ulp(dist.cpu().numpy(), d2_ref, "knn_point")
    # layers/group.py KNN
    dist, i32 = knn.OpenpointsKNN(k)(s, q)
    assert i32.dtype == torch.int32 and i32.is_contiguous() and np.array_equal(i32.cpu().numpy(), rec["group_KNN"])
    assert dist.shape == (s.shape[0], k, q.shape[1])
    _assert_root_within_2ulp(dist.transpose(1, 2).cpu().numpy(), d2_ref, "OpenpointsKNN")
    # PCM_utils.knn_point (both splits) and pointmlp.knn_point (sorted=False: the set)
    for training in (True, False):
        got = knn.xyz_knn_point(k, s, q, training=training)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), rec["pcm_knn_point"])
    assert np.array_equal(np.sort(knn.xyz_knn_point(k, s, q).cpu().numpy(), -1), np.sort(rec["pointmlp_knn_point"], -1))
    # knn_cuda's name: recorded nowhere, so held to the restatement
    dist, i64 = knn.KNN(k, transpose_mode=True)(s, q)
    assert i64.dtype == torch.int64 and np.array_equal(i64.cpu().numpy(), idx_ref)
    _assert_root_within_2ulp(dist.cpu().numpy(), d2_ref, "KNN")
    # self-query form of knn_point (support=None)
    assert np.array_equal(knn.knn_point(k, s)[1].cpu().numpy(), KR.knn(k, support, support)[1])


def test_knn_transpose_modes_agree():
    from unipre3d_amd import knn
    s, q = torch.from_numpy(_cloud(3, 130, 1)).cuda(), torch.from_numpy(_cloud(3, 21, 2)).cuda()
    dt, it = knn.KNN(12, transpose_mode=True)(s, q)
    df, i_f = knn.KNN(12, transpose_mode=False)(s.transpose(1, 2).contiguous(), q.transpose(1, 2).contiguous())
    assert df.shape == i_f.shape == (3, 12, 21) and i_f.dtype == torch.int64 and df.is_contiguous() and i_f.is_contiguous()
    assert torch.equal(i_f.transpose(1, 2), it) and torch.equal(df.transpose(1, 2), dt)
    assert np.array_equal(it.cpu().numpy(), KR.knn(12, s.cpu().numpy(), q.cpu().numpy())[1])


def test_knn_group_is_gather_by_restatement_index():
    from unipre3d_amd import knn
    support, query = _cloud(2, 200, 3), _cloud(2, 37, 4)
    feats = np.random.default_rng(5).standard_normal((2, 6, 200)).astype(np.float32)
    _, idx = KR.knn(12, support, query)
    b = np.arange(2)[:, None, None]
    want_xyz = support[b, idx].transpose(0, 3, 1, 2)                          # (B, 3, M, k)
    want_f = feats.transpose(0, 2, 1)[b, idx].transpose(0, 3, 1, 2)           # (B, C, M, k)
    s, q, f = torch.from_numpy(support).cuda(), torch.from_numpy(query).cuda(), torch.from_numpy(feats).cuda()
    only = knn.KNNGroup(12, return_only_idx=True)(q, s)
    assert only.dtype == torch.int32 and np.array_equal(only.cpu().numpy(), idx)
    gx, gf = knn.KNNGroup(12, relative_xyz=True)(q, s, f)
    assert np.array_equal(gx.cpu().numpy(), want_xyz - query.transpose(0, 2, 1)[:, :, :, None])
    assert np.array_equal(gf.cpu().numpy(), want_f)
    gx, gf = knn.KNNGroup(12, relative_xyz=False)(q, s)
    assert gf is None and np.array_equal(gx.cpu().numpy(), want_xyz)


def test_input_views_and_casts():
    from unipre3d_amd import knn
    wide, query = _cloud(2, 150, 6).repeat(2, axis=2) * np.float32(0.5), _cloud(2, 19, 7)      # (B, N, 6)
    support = np.ascontiguousarray(wide[:, :, :3])
    want = KR.knn(12, support, query)
    view = torch.from_numpy(wide).cuda()[:, :, :3]
    assert not view.is_contiguous()
    d2, idx = knn.knn_query(12, view, torch.from_numpy(query).cuda())
    _assert_exact((d2.cpu().numpy(), idx.cpu().numpy()), want, "non-contiguous view")
    d2, idx = knn.knn_query(12, torch.from_numpy(support).cuda().double(), torch.from_numpy(query).cuda().double())
    _assert_exact((d2.cpu().numpy(), idx.cpu().numpy()), want, "float64 input")


def test_refusals_raise_and_launch_nothing():
    from unipre3d_amd import knn
    s, q = torch.from_numpy(_cloud(1, 100, 8)).cuda(), torch.from_numpy(_cloud(1, 9, 9)).cuda()
    for k in (101, 65, 0, -1):                                                # k > n, k > 64, k < 1
        with pytest.raises(ValueError):
            knn.knn_query(k, s, q)
    with pytest.raises(ValueError):
        knn.knn_query(65, torch.zeros(1, 300, 3, device="cuda"), q)           # k > 64 with k <= n
    with pytest.raises(NotImplementedError):
        knn.knn_query(4, torch.zeros(1, 100, 4, device="cuda"), torch.zeros(1, 9, 4, device="cuda"))
    with pytest.raises(NotImplementedError):
        knn.KNN(4, transpose_mode=True)(torch.zeros(1, 100, 4, device="cuda"), torch.zeros(1, 9, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn.knn_query(4, s.cpu(), q.cpu())
    with pytest.raises(RuntimeError):
        knn.knn_query(4, s, q.cpu())                                          # one tensor on the host, one on the device
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="different devices"):
            knn.knn_query(4, s, q.to("cuda:1"))
    from unipre3d_amd import _lib
    idx = torch.empty(1, 9, 101, dtype=torch.int32, device="cuda")
    assert knn.load().u3d_knn(1, 100, 9, 101, _lib.ptr(s), _lib.ptr(q), _lib.ptr(None), _lib.ptr(idx), _lib.stream_ptr(s.device)) == 1
    torch.cuda.synchronize()                                                  # nothing was launched: no error surfaces later
    assert np.array_equal(knn.knn_query(4, s, q)[1].cpu().numpy(), KR.knn(4, s.cpu().numpy(), q.cpu().numpy())[1])


def test_dist2_may_be_null():
    from unipre3d_amd import _lib, knn
    support, query = _cloud(2, 90, 10), _cloud(2, 18, 11)
    s, q = torch.from_numpy(support).cuda(), torch.from_numpy(query).cuda()
    idx = torch.full((2, 18, 5), -1, dtype=torch.int32, device="cuda")
    assert knn.load().u3d_knn(2, 90, 18, 5, _lib.ptr(s), _lib.ptr(q), _lib.ptr(None), _lib.ptr(idx), _lib.stream_ptr(s.device)) == 0
    assert np.array_equal(idx.cpu().numpy(), KR.knn(5, support, query)[1])


def test_deterministic_and_stream_independent():
    from unipre3d_amd import knn
    support, query = _cloud(2, 2100, 12, quantized=True), _cloud(2, 40, 13, quantized=True)
    s, q = torch.from_numpy(support).cuda(), torch.from_numpy(query).cuda()
    d_a, i_a = knn.knn_query(32, s, q)
    d_b, i_b = knn.knn_query(32, s, q)
    assert torch.equal(i_a, i_b) and torch.equal(d_a.view(torch.int32), d_b.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d_c, i_c = knn.knn_query(32, s, q)
    side.synchronize()
    assert torch.equal(i_a, i_c) and torch.equal(d_a.view(torch.int32), d_c.view(torch.int32))
    _assert_exact((d_a.cpu().numpy(), i_a.cpu().numpy()), KR.knn(32, support, query), "two tiles, quantized")
