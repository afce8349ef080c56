"""unipre3d_amd.serialization on the MI355X against the reference's recorded values (tests/golden/g13_serialization.npz) and the
plain-torch restatement (tests/serialization_ref.py, run on the CPU): every comparison is exact integer equality.
Sort tile = 4096 elements, 8 bits per pass."""
import os

import numpy as np
import pytest
import torch

import serialization_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POOL_NAMES = ("cluster", "indices", "idx_ptr", "head_indices", "code", "order", "inverse")


def _se():
    from unipre3d_amd import serialization
    return serialization


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLDEN, "g13_serialization.npz"), allow_pickle=False)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _points(N, depth, B, seed, spread=None):
    """N points in B items (sorted batch ids); spread < 2**depth bounds the coordinates so that sites repeat."""
    g = torch.Generator().manual_seed(seed)
    hi = min(spread or (1 << depth), 1 << depth)
    coord = torch.randint(0, hi, (N, 3), generator=g, dtype=torch.int32)
    batch = torch.sort(torch.randint(0, B, (N,), generator=g))[0]
    return coord, batch


def _same(got, ref, what):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}[{i}]: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
        assert torch.equal(a.cpu(), b), f"{what}[{i}] differs"


def _check_serialize(coord, batch, depth, orders, batch_size, what):
    got = _se().serialize(coord.to(DEV), None if batch is None else batch.to(DEV), depth, orders, batch_size=batch_size)
    _same(got, R.serialize(coord, batch, depth, orders), what)
    return got


# ---- codes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3, 10, 16])
def test_encode_golden(g13, depth):
    coord, batch, code = _t(g13[f"enc{depth}_coord"]), _t(g13[f"enc{depth}_batch"]), _t(g13[f"enc{depth}_code"])
    S = _se()
    for cd, bd in ((torch.int32, torch.int64), (torch.int64, torch.int32)):
        c, b = coord.to(cd).to(DEV), batch.to(bd).to(DEV)
        all4 = S.encode(c, b, depth, R.ORDERS)
        assert all4.dtype == torch.int64 and torch.equal(all4.cpu(), code), f"depth {depth} {cd}: four orders at once"
        for k, order in enumerate(R.ORDERS):
            one = S.encode(c, b, depth, order)
            assert one.shape == (len(coord),) and torch.equal(one.cpu(), code[k]), f"depth {depth} {order} {cd}"
            assert torch.equal(S.encode(c, None, depth, order).cpu(), code[k] & ((1 << 3 * depth) - 1)), f"depth {depth} {order}: batch=None"


def test_serialize_golden(g13):
    coord, batch, depth = _t(g13["ser_grid_coord"]), _t(g13["ser_batch"]), int(g13["ser_depth"])
    ref = tuple(_t(g13[n]) for n in ("ser_code", "ser_order", "ser_inverse"))
    S = _se()
    _same(S.serialize(coord.to(DEV), batch.to(DEV), depth, R.ORDERS, batch_size=4), ref, "serialize")
    _same(S.serialize(coord.to(DEV), batch.to(DEV), None, R.ORDERS), ref, "serialize, adaptive depth, 63-bit keys")
    assert S.adaptive_depth(coord.to(DEV)) == depth
    _same(S.sort_codes(ref[0].to(DEV), key_bits=3 * depth + 2), ref[1:], "sort_codes")


# ---- the sort ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 4095, 4096, 4097, 9001])
@pytest.mark.parametrize("orders", [("hilbert",), R.ORDERS], ids=["K1", "K4"])
def test_serialize_sizes(N, orders):
    coord, batch = _points(N, 16, 2, N, spread=12)            # 1728 sites per item: ties from 4095 points up
    _check_serialize(coord, batch, 16, orders, 2, f"N={N}")


@pytest.mark.parametrize("depth,B,passes", [(2, 4, 1), (3, 1, 2), (7, 8, 3), (10, 3, 4), (11, 1, 5), (15, 5, 6), (16, 2, 7), (16, None, 8)])
def test_every_pass_count(depth, B, passes):
    width = 63 if B is None else 3 * depth + (B - 1).bit_length()
    assert (width + 7) // 8 == passes
    coord, batch = _points(5000, depth, B or 3, 100 + passes)
    coord[:4] = (1 << depth) - 1                               # the top bits of the key are in use
    batch[-1] = (B or 3) - 1
    _check_serialize(coord, batch, depth, ("z", "hilbert-trans"), B, f"{passes} passes")


def test_depths_1_2_16_with_repeats():
    for depth in (1, 2, 16):
        coord, batch = _points(3000, depth, 3, depth, spread=5)
        _check_serialize(coord, batch, depth, R.ORDERS, 3, f"depth {depth}")


def test_all_codes_equal_sorted_reversed_and_one_site():
    N = 5000
    coord, batch = torch.full((N, 3), 77, dtype=torch.int32), torch.ones(N, dtype=torch.int64)
    code, order, inverse = _check_serialize(coord, batch, 10, R.ORDERS, 2, "all codes equal")
    assert torch.equal(order[0].cpu(), torch.arange(N)) and torch.equal(inverse[3].cpu(), torch.arange(N))
    coord, batch = _points(N, 10, 2, 5, spread=40)
    by_code = torch.argsort(R.encode(coord, batch, 10, "z"), stable=True)
    for name, idx in (("sorted", by_code), ("reversed", by_code.flip(0))):
        _check_serialize(coord[idx].contiguous(), batch[idx].contiguous(), 10, R.ORDERS, 2, name)
    coord, batch = _points(1000, 10, 1, 6)
    coord[100:400] = torch.tensor([513, 2, 1000], dtype=torch.int32)      # 300 rows on one site
    code, order, _ = _check_serialize(coord, batch, 10, R.ORDERS, 1, "300 rows on one site")
    for k in range(4):
        at = torch.nonzero(code[k][order[k]] == code[k][100]).flatten()
        assert torch.equal(order[k][at].cpu(), torch.arange(100, 400)), f"{R.ORDERS[k]}: the site's rows are not in ascending index"


def test_dtypes_and_no_batch():
    coord, batch = _points(4500, 9, 3, 9, spread=20)
    ref = R.serialize(coord, batch, 9, R.ORDERS)
    for cd in (torch.int32, torch.int64):
        for bd in (torch.int32, torch.int64):
            _same(_se().serialize(coord.to(cd).to(DEV), batch.to(bd).to(DEV), 9, R.ORDERS, batch_size=3), ref, f"{cd} {bd}")
    _check_serialize(coord.long(), None, 9, ("z-trans", "hilbert"), None, "batch=None")


def test_serialize_and_pool_above_1024_tiles():
    """1024 * 4096 + 1 rows = 1025 sort tiles: the digit scan walks each digit's line in five trips of 256 tiles with a carry (the last
    trip holds one tile), and the one-workgroup scan of the per-tile head counts owns two entries per thread, most threads past the end"""
    N = 1024 * 4096 + 1
    coord, batch = _points(N, 10, 2, 1025)
    ref = R.serialize(coord, batch, 10, ("hilbert",))
    got = _se().serialize(coord.to(DEV), batch.to(DEV), 10, ("hilbert",), batch_size=2)
    _same(got, ref, "serialize, 1025 tiles")
    _same(_se().pool_clusters(got[0], 1, depth=10, batch_size=2), R.pool_clusters(ref[0], 1), "pool_clusters, 1025 tiles")


def test_two_calls_are_bit_identical():
    coord, batch = _points(9001, 12, 2, 21, spread=15)
    c, b = coord.to(DEV), batch.to(DEV)
    first = _se().serialize(c, b, 12, R.ORDERS, batch_size=2)
    pool1 = _se().pool_clusters(first[0], 1, depth=12, batch_size=2)
    second = _se().serialize(c, b, 12, R.ORDERS, batch_size=2)
    pool2 = _se().pool_clusters(second[0], 1, depth=12, batch_size=2)
    for x, y in zip(first + pool1, second + pool2):
        assert torch.equal(x, y)


def test_serialize_is_capturable_in_a_graph():
    S, N, depth = _se(), 6000, 11
    sets = [_points(N, depth, 2, seed, spread=14) for seed in (31, 32, 33)]
    static_c, static_b = sets[0][0].to(DEV), sets[0][1].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        S.serialize(static_c, static_b, depth, R.ORDERS, batch_size=2)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = S.serialize(static_c, static_b, depth, R.ORDERS, batch_size=2)
    for coord, batch in sets[1:] + sets[:1]:
        static_c.copy_(coord)
        static_b.copy_(batch)
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(out, R.serialize(coord, batch, depth, R.ORDERS), "graph replay")


# ---- patch padding -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["pada", "padb"])
def test_patch_padding_golden(g13, tag):
    ends = np.cumsum(g13[f"{tag}_sizes"])
    ref = tuple(_t(g13[f"{tag}_{n}"]) for n in ("pad", "unpad", "cu_seqlens"))
    P = int(g13["patch_size"])
    for offset in (ends.tolist(), _t(ends), _t(ends).to(DEV), _t(ends).int().to(DEV)):
        _same(_se().patch_padding(offset, P, device=DEV), ref, f"{tag} {type(offset).__name__}")


@pytest.mark.parametrize("P", [48, 1024])
def test_patch_padding_edges(P):
    for sizes in ((P,), (P + 1,), (2 * P - 1,), (1,), (P, P + 1, 2 * P - 1, 1, 3 * P, 1, 5 * P + 7), (1,) * 300):
        ends = np.cumsum(sizes)
        ref = R.patch_padding(ends.tolist(), P)
        _same(_se().patch_padding(ends.tolist(), P, device=DEV), ref, f"P={P} {sizes[:7]} host offset")
        _same(_se().patch_padding(_t(ends).to(DEV), P), ref, f"P={P} {sizes[:7]} device offset")


# ---- pooling -----------------------------------------------------------------------------------------------------------------------
def test_pool_golden(g13):
    ref = tuple(_t(g13["pool_" + n]) for n in POOL_NAMES)
    code = _t(g13["ser_code"]).to(DEV)
    _same(_se().pool_clusters(code, int(g13["pool_depth"])), ref, "pool, 63-bit keys")
    _same(_se().pool_clusters(code, int(g13["pool_depth"]), depth=int(g13["ser_depth"]), batch_size=4), ref, "pool")


def _check_pool(coord, batch, depth, B, pd, what):
    code = R.serialize(coord, batch, depth, R.ORDERS)[0]
    ref = R.pool_clusters(code, pd)
    _same(_se().pool_clusters(code.to(DEV), pd, depth=depth, batch_size=B), ref, what)
    return ref


def test_pool_shapes():
    N = 5000
    cells = torch.randperm(20 ** 3, generator=torch.Generator().manual_seed(3))[:N]
    distinct = torch.stack([cells // 400, cells // 20 % 20, cells % 20], 1).int()
    zeros = torch.zeros(N, dtype=torch.int64)
    ref = _check_pool(distinct, zeros, 5, 1, 0, "pooling_depth 0 on distinct sites: M = N")
    assert len(ref[3]) == N
    ref = _check_pool(distinct % 2, zeros, 5, 1, 1, "one parent voxel: M = 1")
    assert len(ref[3]) == 1
    # sorted positions 3500 .. 4999 are one cluster: it spans the tile boundary at 4096
    coord = torch.cat([distinct[:3500] % 16, torch.tensor([[16, 16, 16]], dtype=torch.int32).repeat(1500, 1), distinct[3500:4500] % 8 + 24])
    perm = torch.randperm(len(coord), generator=torch.Generator().manual_seed(4))
    ref = _check_pool(coord[perm].contiguous(), torch.zeros(len(coord), dtype=torch.int64), 5, 1, 1, "a cluster across the tile boundary")
    assert int((ref[2][1:] - ref[2][:-1]).max()) >= 1500
    coord, batch = _points(9001, 8, 3, 8, spread=30)
    for pd in (0, 1, 2):
        _check_pool(coord, batch, 8, 3, pd, f"pooling_depth {pd}, three items, repeated sites")


# ---- the chain into attention and segment_csr ---------------------------------------------------------------------------------
def test_chain_into_attention_and_segment_csr(g13):
    """G12's shapes: items of 17, 96, 130, 97 at patch 48, 2 heads; patch_padding's cu_seqlens feeds the varlen attention and
    pool_clusters' indices / idx_ptr feed segment_csr; the same calls fed by the restatement give the same bits."""
    from unipre3d_amd import attention, scatter
    S = _se()
    g12 = np.load(os.path.join(GOLDEN, "g12_ptv3_boundary.npz"), allow_pickle=False)
    sizes, P, H = tuple(int(s) for s in g12["item_sizes"]), int(g12["patch_size"]), int(g12["attn_qkv_shape"][2])
    coord, batch, depth = _t(g13["ser_grid_coord"]), _t(g13["ser_batch"]), int(g13["ser_depth"])
    assert len(coord) == sum(sizes)
    ends = np.cumsum(sizes)
    code, order, inverse = S.serialize(coord.to(DEV), batch.to(DEV), depth, R.ORDERS, batch_size=len(sizes))
    pad, unpad, cu = S.patch_padding(_t(ends).to(DEV), P)
    rcode, rorder, rinverse = R.serialize(coord, batch, depth, R.ORDERS)
    rpad, runpad, rcu = R.patch_padding(ends.tolist(), P)
    assert torch.equal(cu.cpu(), _t(g12["attn_cu_seqlens"]))
    gen = torch.Generator().manual_seed(13)
    qkv = torch.randn(len(coord), 3, H, 16, generator=gen).half().to(DEV)
    feat = torch.randn(len(coord), 32, generator=gen).to(DEV)
    scale = float(g12["attn_softmax_scale"])

    def attend(order, inverse, pad, unpad, cu):
        out = attention.flash_attn_varlen_qkvpacked_func(qkv[order][pad].contiguous(), cu, max_seqlen=P, softmax_scale=scale)
        return out[unpad][inverse]

    ours = attend(order[0], inverse[0], pad, unpad, cu)
    theirs = attend(rorder[0].to(DEV), rinverse[0].to(DEV), rpad.to(DEV), runpad.to(DEV), rcu.to(DEV))
    assert ours.shape == (len(coord), H, 16) and torch.equal(ours, theirs) and bool(ours.float().abs().sum() > 0)
    cluster, indices, idx_ptr, head = S.pool_clusters(code, 1, depth=depth, batch_size=len(sizes))[:4]
    rcluster, rindices, ridx_ptr, rhead = R.pool_clusters(rcode, 1)[:4]
    for reduce in ("max", "mean"):
        a = scatter.segment_csr(feat[indices].contiguous(), idx_ptr, reduce=reduce)
        b = scatter.segment_csr(feat[rindices.to(DEV)].contiguous(), ridx_ptr.to(DEV), reduce=reduce)
        assert a.shape == (len(head), 32) and torch.equal(a, b), reduce
        assert torch.equal(a[cluster], b[rcluster.to(DEV)])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    S = _se()
    coord, batch = _points(64, 8, 2, 1)
    c, b = coord.to(DEV), batch.to(DEV)
    for depth in (0, 17, -1, 2.0):
        with pytest.raises(ValueError):
            S.serialize(c, b, depth, ("z",), batch_size=2)
    with pytest.raises(ValueError):                       # 3 * 16 + bit_length(2 ** 15) = 64 bits
        S.serialize(c, b, 16, ("z",), batch_size=1 << 15)
    S.serialize(c, b, 16, ("z",), batch_size=(1 << 15) - 1)
    with pytest.raises(NotImplementedError):              # K > 4
        S.serialize(c, b, 8, ("z",) * 5, batch_size=2)
    with pytest.raises(NotImplementedError):
        S.encode(c, b, 8, ())
    with pytest.raises(ValueError):
        S.encode(c, b, 8, "morton")
    with pytest.raises(ValueError):                       # non-contiguous
        S.encode(c.repeat(1, 2)[:, ::2], b, 8, "z")
    with pytest.raises(ValueError):
        S.encode(c, b.repeat_interleave(2)[::2], 8, "z")
    for bad in (c.float(), c.short()):
        with pytest.raises(NotImplementedError):
            S.encode(bad, b, 8, "z")
    with pytest.raises(NotImplementedError):
        S.encode(c, b.float(), 8, "z")
    with pytest.raises(ValueError):
        S.encode(c[:, :2].contiguous(), b, 8, "z")
    with pytest.raises(ValueError):
        S.encode(c, b[:-1].contiguous(), 8, "z")
    with pytest.raises(RuntimeError):                     # no CPU fallback
        S.encode(coord, batch, 8, "z")
    code = S.encode(c, b, 8, R.ORDERS)
    with pytest.raises(ValueError):
        S.pool_clusters(code[:, ::2], 1)
    with pytest.raises(ValueError):
        S.pool_clusters(code.int(), 1)
    with pytest.raises(NotImplementedError):
        S.pool_clusters(torch.cat([code, code[:1]]), 1)
    with pytest.raises(ValueError):
        S.pool_clusters(code, 17)
    with pytest.raises(ValueError):
        S.pool_clusters(code, 9, depth=8, batch_size=2)
    with pytest.raises(ValueError):
        S.sort_codes(code, key_bits=0)
    for offset in ([5, 5, 9], [0, 4], [], torch.tensor([3, 2]).to(DEV)):
        with pytest.raises(ValueError):
            S.patch_padding(offset, 48, device=DEV)
    with pytest.raises(ValueError):
        S.patch_padding([4, 9], 0, device=DEV)
