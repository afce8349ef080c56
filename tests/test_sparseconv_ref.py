"""CPU: the restatement tests/spconv_ref.py against dense Conv3d / ConvTranspose3d in fp64 (forward and autograd gradients at the active
sites), its repeated-site semantics and output order, and the spconv-style modules' construction."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spconv_ref as R


def _scene(seed, B=2, D=(7, 6, 8), n=60, dup=0):
    g = np.random.default_rng(seed)
    cells = set()
    while len(cells) < n:
        cells.add((int(g.integers(B)), int(g.integers(D[0])), int(g.integers(D[1])), int(g.integers(D[2]))))
    idx = np.array(sorted(cells), dtype=np.int64)
    idx = idx[g.permutation(len(idx))]
    if dup:
        idx = np.concatenate([idx, idx[g.choice(len(idx), dup, replace=False)]])
    return idx, list(D), B


def _params(Cin, Cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(Cout, k, k, k, Cin, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, generator=g, dtype=torch.float64, requires_grad=True)
    return W, b


@pytest.mark.parametrize("k", [1, 3, 5])
def test_subm_equals_dense_conv3d(k):
    idx, D, B = _scene(k)
    Cin, Cout = 4, 5
    X = torch.randn(len(idx), Cin, dtype=torch.float64, generator=torch.Generator().manual_seed(3), requires_grad=True)
    W, b = _params(Cin, Cout, k, 7)
    T = R.subm_table(idx, D, k)
    Y = R.subm(X, W, b, T)
    G = R.dense_grid(X, idx, D, B)
    Yd = R.sample(F.conv3d(G, W.permute(0, 4, 1, 2, 3), b, padding=k // 2), idx)
    assert torch.allclose(Y, Yd, rtol=1e-12, atol=1e-12)
    gY = torch.randn_like(Y)
    g1 = torch.autograd.grad(Y, (X, W, b), gY)
    g2 = torch.autograd.grad(Yd, (X, W, b), gY)
    for a, c in zip(g1, g2):
        assert torch.allclose(a, c, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("s", [2, 3])
def test_strided_and_inverse_equal_dense(s):
    idx, D, B = _scene(10 + s, D=(7, 8, 9), n=90)
    Cin, Cout = 3, 4
    X = torch.randn(len(idx), Cin, dtype=torch.float64, generator=torch.Generator().manual_seed(1), requires_grad=True)
    W, b = _params(Cin, Cout, s, 2)
    m = R.down_map(idx, D, s)
    assert m["out_shape"] == [(d - s) // s + 1 for d in D]
    Y = R.down(X, W, b, m)
    G = R.dense_grid(X, idx, D, B)
    Yd = R.sample(F.conv3d(G, W.permute(0, 4, 1, 2, 3), b, stride=s), m["out_indices"])
    assert torch.allclose(Y, Yd, rtol=1e-12, atol=1e-12)
    gY = torch.randn_like(Y)
    for a, c in zip(torch.autograd.grad(Y, (X, W, b), gY), torch.autograd.grad(Yd, (X, W, b), gY)):
        assert torch.allclose(a, c, rtol=1e-11, atol=1e-11)
    # the inverse: back to the input rows (in order) from the coarse sites
    Wi, bi = _params(Cout, Cin, s, 5)
    Xc = torch.randn(len(m["out_indices"]), Cout, dtype=torch.float64, generator=torch.Generator().manual_seed(4), requires_grad=True)
    Yi = R.inverse(Xc, Wi, bi, m)
    Gc = R.dense_grid(Xc, m["out_indices"], m["out_shape"], B)
    full = F.conv_transpose3d(Gc, Wi.permute(4, 0, 1, 2, 3), bi, stride=s)
    pad = [0, D[2] - full.shape[4], 0, D[1] - full.shape[3], 0, D[0] - full.shape[2]]
    full = F.pad(full, pad)   # sites the strided conv dropped lie outside the transposed conv's output
    kept = m["row_out"] >= 0
    Yid = R.sample(full, idx)
    assert torch.allclose(Yi[kept], Yid[kept], rtol=1e-12, atol=1e-12)
    assert torch.allclose(Yi[~kept], bi.expand(int((~kept).sum()), -1))
    gYi = torch.randn_like(Yi)
    gYi[~kept] = 0
    for a, c in zip(torch.autograd.grad(Yi, (Xc, Wi), gYi), torch.autograd.grad(Yid, (Xc, Wi), gYi)):
        assert torch.allclose(a, c, rtol=1e-11, atol=1e-11)


def test_down_output_order_and_drops():
    idx = np.array([[1, 0, 0, 0], [0, 3, 3, 3], [0, 2, 2, 2], [0, 0, 1, 0], [1, 4, 0, 0]])
    m = R.down_map(idx, [5, 5, 5], 2)   # out_shape 2: d // 2 == 2 is dropped
    assert m["out_indices"].tolist() == [[0, 0, 0, 0], [0, 1, 1, 1], [1, 0, 0, 0]]
    assert m["row_out"].tolist() == [2, 1, 1, 0, -1]
    assert m["row_tap"].tolist() == [0, 7, 0, 2, -1]


def test_duplicate_semantics():
    idx = np.array([[0, 1, 1, 1], [0, 1, 1, 2], [0, 1, 1, 1], [0, 1, 1, 2], [0, 1, 1, 1]])
    T = R.subm_table(idx, [3, 3, 3], 3)
    assert (T[:, 13] == [0, 1, 0, 1, 0]).all()      # the centre reads the site's lowest row
    assert (T[0, 14] == 1) and (T[2, 14] == 1) and (T[1, 12] == 0)
    X = torch.randn(5, 2, dtype=torch.float64, requires_grad=True)
    W, b = _params(2, 3, 3, 0)
    Y = R.subm(X, W, b, T)
    assert torch.equal(Y[0], Y[2]) and torch.equal(Y[0], Y[4])   # every repeated row gets an output
    gX, = torch.autograd.grad(Y.sum(), X)
    assert (gX[2:] == 0).all() and (gX[:2] != 0).all()           # repeated rows are never read
    m = R.down_map(idx, [4, 4, 4], 2)
    Yd = R.down(X, W[:, :2, :2, :2], None, m)
    assert torch.allclose(Yd[0], X[[0, 2, 4]].sum(0) @ R._w(W[:, :2, :2, :2], 7))   # the strided conv sums every row at a site
    assert torch.allclose(Yd[1], X[[1, 3]].sum(0) @ R._w(W[:, :2, :2, :2], 6))
    Yi = R.inverse(Yd.detach(), W[:, :2, :2, :2].permute(4, 1, 2, 3, 0), None, m)
    assert torch.equal(Yi[0], Yi[2]) and torch.equal(Yi[1], Yi[3])


def test_module_construction_on_cpu():
    from unipre3d_amd import sparseconv as sp
    c = sp.SubMConv3d(6, 32, 5, padding=1, bias=False, indice_key="stem")
    assert c.weight.shape == (32, 5, 5, 5, 6) and c.bias is None
    assert list(c.state_dict()) == ["weight"]
    d = sp.SparseConv3d(32, 64, kernel_size=2, stride=2, bias=False, indice_key="spconv1")
    assert d.weight.shape == (64, 2, 2, 2, 32)
    u = sp.SparseInverseConv3d(64, 32, kernel_size=2, bias=False, indice_key="spconv1")
    assert u.weight.shape == (32, 2, 2, 2, 64)
    p = sp.SubMConv3d(32, 32, 3, bias=True)
    assert list(p.state_dict()) == ["weight", "bias"]
    seq = sp.SparseSequential(sp.SubMConv3d(32, 32, 3, padding=1), torch.nn.BatchNorm1d(32), torch.nn.ReLU())
    assert [k for k in seq.state_dict() if k.startswith("0.")] == ["0.weight", "0.bias"]
    for bad in (lambda: sp.SubMConv3d(4, 4, 2), lambda: sp.SubMConv3d(4, 4, 7), lambda: sp.SubMConv3d(4, 4, 3, dilation=2),
                lambda: sp.SubMConv3d(4, 4, 3, stride=2), lambda: sp.SparseConv3d(4, 4, 3, stride=2),
                lambda: sp.SparseConv3d(4, 4, 2, stride=2, padding=1), lambda: sp.SubMConv3d(4, 4, (3, 3, 1)),
                lambda: sp.SubMConv3d(4, 4, 3, groups=2)):
        with pytest.raises(NotImplementedError):
            bad()
    with pytest.raises(ValueError):
        sp.SparseInverseConv3d(4, 4, 2)


def test_sparse_tensor_on_cpu():
    from unipre3d_amd import sparseconv as sp
    f = torch.arange(6.0).reshape(3, 2)
    idx = torch.tensor([[0, 0, 0, 1], [1, 1, 0, 0], [0, 0, 0, 1]], dtype=torch.int32)
    t = sp.SparseConvTensor(f, idx, [2, 2, 2], 2)
    t.indice_dict["a"] = object()
    r = t.replace_feature(f * 2)
    assert r.indice_dict is t.indice_dict and r.indices is idx and torch.equal(r.features, f * 2)
    d = t.dense()
    assert d.shape == (2, 2, 2, 2, 2) and torch.equal(d[0, :, 0, 0, 1], f[0] + f[2]) and torch.equal(d[1, :, 1, 0, 0], f[1])
    seq = sp.SparseSequential(torch.nn.Identity(), sp.Identity(), torch.nn.ReLU())
    assert torch.equal(seq(t).features, f)


@pytest.mark.parametrize("k", [3, 5])
def test_vectorized_table_equals_dictionary_table(k):
    idx, D, _ = _scene(20 + k, n=150, dup=20)
    assert np.array_equal(R.subm_table_np(idx, D, k), R.subm_table(idx, D, k))


def test_chains_np_against_dictionaries():
    g = np.random.default_rng(5)
    idx = np.concatenate([g.integers(0, 2, size=(400, 1)), g.integers(0, 4, size=(400, 3))], 1)   # 128 cells: long chains
    first, nxt = R.chains_np(idx, (4, 4, 4))
    rows = {}
    for i, s in enumerate(map(tuple, idx)):
        rows.setdefault(s, []).append(i)
    for s, rs in rows.items():
        assert all(first[r] == rs[0] for r in rs)
        assert [int(nxt[r]) for r in rs] == rs[1:] + [-1]
    assert R.chains_np(np.zeros((0, 4), np.int64), (4, 4, 4))[0].shape == (0,)
