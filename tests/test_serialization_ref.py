"""tests/serialization_ref.py (the plain-torch restatement of PTv3's index plumbing) against the reference's recorded values in
tests/golden/g13_serialization.npz, everywhere and exactly, and its own properties on random points.  CPU only.

pool_indices / pool_head_indices in G13 are the reference's values with each cluster's points in ascending index: the reference's
torch.sort(cluster) leaves that order unspecified and is not the stable sort on the CPU at this size (make_g13_serialization.py);
test_pool_matches_reference_up_to_tie_order checks the values as they came out (*_ref) for everything the tie order cannot change."""
import os

import numpy as np
import pytest
import torch

import serialization_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLDEN, "g13_serialization.npz"), allow_pickle=False)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_golden_is_small_and_lists_the_orders(g13):
    assert os.path.getsize(os.path.join(GOLDEN, "g13_serialization.npz")) < 100 * 1024
    assert tuple(str(o) for o in g13["orders"]) == R.ORDERS


@pytest.mark.parametrize("depth", [1, 2, 3, 10, 16])
def test_encode_matches_reference(g13, depth):
    coord, batch, code = _t(g13[f"enc{depth}_coord"]), _t(g13[f"enc{depth}_batch"]), _t(g13[f"enc{depth}_code"])
    top = (1 << depth) - 1
    assert bool((coord[0] == 0).all()) and bool((coord[1] == top).all()) and set(batch.tolist()) == {0, 1, 2}
    if depth == 16:
        assert int(code.max()).bit_length() == 50
    for k, order in enumerate(R.ORDERS):
        got = R.encode(coord, batch, depth, order)
        assert got.dtype == torch.int64 and torch.equal(got, code[k]), f"depth {depth} {order}"
        assert torch.equal(R.encode(coord.long(), None, depth, order), code[k] & ((1 << 3 * depth) - 1)), f"depth {depth} {order}: no batch"


def test_serialize_matches_reference(g13):
    code, order, inverse = R.serialize(_t(g13["ser_grid_coord"]), _t(g13["ser_batch"]), int(g13["ser_depth"]), R.ORDERS)
    assert torch.equal(code, _t(g13["ser_code"]))
    assert torch.equal(order, _t(g13["ser_order"]))
    assert torch.equal(inverse, _t(g13["ser_inverse"]))


@pytest.mark.parametrize("tag", ["pada", "padb"])
def test_patch_padding_matches_reference(g13, tag):
    ends = np.cumsum(g13[f"{tag}_sizes"])
    for offset in (ends.tolist(), _t(ends)):
        pad, unpad, cu = R.patch_padding(offset, int(g13["patch_size"]))
        assert pad.dtype == torch.int64 and unpad.dtype == torch.int64 and cu.dtype == torch.int32
        assert torch.equal(pad, _t(g13[f"{tag}_pad"])) and torch.equal(unpad, _t(g13[f"{tag}_unpad"]))
        assert torch.equal(cu, _t(g13[f"{tag}_cu_seqlens"]))


def test_g12_item_sizes_are_covered(g13):
    g12 = np.load(os.path.join(GOLDEN, "g12_ptv3_boundary.npz"), allow_pickle=False)
    assert np.array_equal(g13["pada_sizes"], g12["item_sizes"]) and int(g13["patch_size"]) == int(g12["patch_size"])
    assert np.array_equal(g13["pada_cu_seqlens"], g12["attn_cu_seqlens"])
    assert tuple(g13["padb_sizes"]) == (1, 48, 49, 95)


def test_pool_matches_reference(g13):
    res = R.pool_clusters(_t(g13["ser_code"]), int(g13["pool_depth"]))
    for got, name in zip(res, ("cluster", "indices", "idx_ptr", "head_indices", "code", "order", "inverse")):
        assert got.dtype == torch.int64 and torch.equal(got, _t(g13["pool_" + name])), name


def test_pool_matches_reference_up_to_tie_order(g13):
    cluster, indices, idx_ptr, head = (_t(g13["pool_" + n]) for n in ("cluster", "indices", "idx_ptr", "head_indices"))
    raw, raw_head = _t(g13["pool_indices_ref"]), _t(g13["pool_head_indices_ref"])
    assert torch.equal(cluster[raw], cluster[indices]) and torch.equal(cluster[raw_head], cluster[head])
    for a, b in zip(idx_ptr[:-1].tolist(), idx_ptr[1:].tolist()):
        assert torch.equal(torch.sort(raw[a:b])[0], indices[a:b])           # the same points, ours in ascending index
        assert int(head[int(cluster[indices[a]])]) == int(indices[a:b].min())


def test_properties_on_random_points():
    g = torch.Generator().manual_seed(2000)
    N, depth = 2000, 6
    coord = torch.randint(0, 9, (N, 3), generator=g)          # 729 sites for 2000 points: repeated sites
    batch = torch.sort(torch.randint(0, 3, (N,), generator=g))[0]
    site = (batch * 16 + coord[:, 0]) * 256 + coord[:, 1] * 16 + coord[:, 2]
    code, order, inverse = R.serialize(coord, batch, depth, R.ORDERS)
    same_site = site[:, None] == site[None, :]
    for k in range(4):
        assert torch.equal(code[k][:, None] == code[k][None, :], same_site), R.ORDERS[k]   # distinct exactly when the sites are
        s = code[k][order[k]]
        assert bool((s[1:] >= s[:-1]).all())
        tie = s[1:] == s[:-1]
        assert bool(tie.any()) and bool((order[k][1:][tie] > order[k][:-1][tie]).all())  # ties in ascending index
        assert torch.equal(inverse[k][order[k]], torch.arange(N))
    cluster, indices, idx_ptr, head, pcode, porder, pinverse = R.pool_clusters(code, 1)
    M = len(head)
    assert bool((cluster[indices][1:] >= cluster[indices][:-1]).all()) and int(idx_ptr[-1]) == N and M < N
    assert torch.equal(cluster[head], torch.arange(M))
    assert torch.equal(pcode, (code >> 3)[:, head]) and torch.equal(pinverse[0][porder[0]], torch.arange(M))


def test_patch_padding_properties():
    for P in (48, 1024):
        sizes = (P, P + 1, 2 * P - 1, 1, 3 * P)
        pad, unpad, cu = R.patch_padding(np.cumsum(sizes).tolist(), P)
        assert torch.equal(pad[unpad], torch.arange(sum(sizes)))            # unpad undoes pad
        lens = (cu[1:] - cu[:-1]).tolist()
        assert lens == [P] + [P] * 2 + [P] * 2 + [1] + [P] * 3 and int(cu[-1]) == len(pad)
        starts = np.concatenate([[0], np.cumsum(sizes)])
        item = np.searchsorted(starts, pad.numpy(), side="right") - 1
        assert bool((np.diff(item) >= 0).all())                             # a padded slot stays inside its item
