"""tests/pcm_order_ref.py (the plain-torch restatement of PCM's order serialization) against the reference's recorded values in
tests/golden/g23_pcm_order.npz, exactly, and the closed form of the axis-order code against the reference's literal loop.  CPU only.

Where codes tie (most points under the axis orders) the reference's plain argsort leaves the order open, so its recorded rows are
compared through what the tie order cannot change: the code along its order is non-decreasing, and the rows are a permutation of the
input's.  In the tie-free case its rows are compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import pcm_order_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_pcm_order.npz")
CASES = ("orders", "tiefree", "boundary", "planar", "onecell")


@pytest.fixture(scope="module")
def g23():
    return np.load(GOLDEN, allow_pickle=False)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _case(g, case):
    return (_t(g[f"{case}/pos"]), _t(g[f"{case}/feat"]), _t(g[f"{case}/x_res"]), [str(o) for o in g[f"{case}/orders"]],
            _t(g[f"{case}/code"]), _t(g[f"{case}/rows"]), float(g["grid_size"]))


def test_golden_is_small_and_holds_the_cases(g23):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert tuple(str(o) for o in g23["orders/orders"]) == R.SHIPPED == tuple(str(o) for o in g23["tiefree/orders"])
    assert g23["orders/pos"].shape == (3, 64, 3) and int(g23["onecell/depth"]) == 0
    assert int(g23["planar/code"][0].min()) < 0                                     # negative codes are recorded


@pytest.mark.parametrize("case", CASES)
def test_code_and_order_match_reference(g23, case):
    pos, feat, x_res, orders, code, rows, gs = _case(g23, case)
    B, N, _ = pos.shape
    src = torch.cat([pos, feat, x_res], 2).flatten(0, 1)
    assert torch.equal(R.grid_cells(pos, gs), (lambda c: c - c.min(dim=1, keepdim=True)[0])(torch.floor(pos / gs).to(torch.int64)))
    for k, order in enumerate(orders):
        index, inverse, got = R.point_order(pos, order, gs)
        assert got.dtype == torch.int64 and torch.equal(got, code[k]), f"{case} {order}: code"
        assert torch.equal(R.point_order(pos, order, gs, literal=True)[2], code[k]), f"{case} {order}: literal code"
        assert torch.equal(index, torch.argsort(code[k], stable=True)) and torch.equal(inverse[index], torch.arange(B * N))
        outs = [feat.clone()]
        moved = R.serialization(pos, feat, x_res, order, outs, gs)
        assert torch.equal(outs[0], moved[1]) and all(m.shape == t.shape for m, t in zip(moved, (pos, feat, x_res)))
        mine = torch.cat(moved, 2).flatten(0, 1)
        assert torch.equal(mine, src[index])
        if code[k].unique().numel() == B * N:                                        # no ties: the reference's rows, bit for bit
            assert torch.equal(mine.view(torch.int32), rows[k].view(torch.int32)), f"{case} {order}: rows"
        else:                                                                        # ties: its order sorts the code, whichever it is
            ref_index = torch.tensor([int(torch.nonzero((src == r).all(1))[0]) for r in rows[k]])
            assert torch.equal(torch.sort(ref_index)[0], torch.arange(B * N)), f"{case} {order}: not a permutation"
            assert bool((code[k][ref_index].diff() >= 0).all()), f"{case} {order}: the recorded order does not sort the code"


def test_tiefree_has_no_ties_and_the_other_cases_what_they_are_for(g23):
    assert all(len(np.unique(c)) == c.size for c in g23["tiefree/code"])
    assert len(np.unique(g23["orders/code"][0])) < 192                               # the axis orders tie
    pos, gs = _t(g23["boundary/pos"]), float(g23["grid_size"])
    recip = torch.floor(pos * np.float32(1.0 / np.float32(gs))).to(torch.int64)     # the other form floors differently somewhere
    assert bool((recip != torch.floor(pos / gs).to(torch.int64)).any())
    planar = _t(g23["planar/code"][0])                                               # xyz: stride 0, the items interleave once sorted
    batch = torch.arange(2).repeat_interleave(48)[torch.argsort(planar, stable=True)]
    assert int((batch.diff() != 0).sum()) > 1


def test_onecell_hilbert_is_the_batch_id(g23):
    pos, gs = _t(g23["onecell/pos"]), float(g23["grid_size"])
    want = torch.arange(2).repeat_interleave(16)
    for order in R.CURVES:                                                           # depth 0: no curve bits, as the reference's z
        assert torch.equal(R.point_order(pos, order, gs)[2], want)
    assert torch.equal(R.point_order(pos, "z", gs)[2], _t(g23["onecell/code"][1]))


def test_closed_form_equals_literal_form():
    g = torch.Generator().manual_seed(7)
    maxima = [0, 1, 2, 3, 4, 5, 62, 63, 65534, 65535]
    c1 = torch.randint(0, 65536, (257,), generator=g)
    batch = torch.randint(0, 16, (257,), generator=g)
    n = 0
    for m1 in maxima:
        for m2 in maxima:
            for m3 in maxima:
                t = [torch.tensor(m) for m in (m1, m2, m3)]
                c = c1 % (m1 + 1)
                assert torch.equal(R.axis_code_closed(c, batch, *t), R.axis_code_literal(c, batch, *t)), (m1, m2, m3)
                n += 1
    assert n == 1000
    c, b = torch.tensor([3]), torch.tensor([2])                                      # a planar cloud: m2 = 0, m3 odd -> negative
    assert int(R.axis_code_closed(c, b, torch.tensor(9), torch.tensor(0), torch.tensor(7))) == -3
