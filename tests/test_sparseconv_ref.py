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


# ---- tests/spconv_kernel_ref.py: the C-ABI contractions and the structured tables ------------------------------------------------------------
import spconv_kernel_ref as KR


def _ints(g, *shape):
    return torch.as_tensor(g.integers(-4, 5, size=shape)).double()


def test_kernel_references_agree_with_scalar_loops():
    """gemm (table mode, list mode, mask, out_rows), wgrad (both sides), colsum and dupsum against the header's sentences as Python loops"""
    g = np.random.default_rng(0)
    R, K, Cin, Cout, Ra = 5, 3, 2, 3, 4
    A, W, b = _ints(g, Ra, Cin), _ints(g, K, Cin, Cout), _ints(g, Cout)
    T = g.integers(-1, Ra, size=(R, K))
    mask = np.array([0, 0, 2, 1, 4])
    for bias in (None, b):
        for m in (None, mask):
            want = torch.zeros(R, Cout, dtype=torch.float64)
            for o in range(R):
                for n in range(Cout):
                    s = 0.0 if bias is None else float(bias[n])
                    for k in range(K):
                        if T[o, k] >= 0:
                            for c in range(Cin):
                                s += float(A[T[o, k], c]) * float(W[k, c, n])
                    want[o, n] = 0.0 if (m is not None and m[o] != o) else s
            assert torch.equal(KR.gemm_ref(A, W, bias, T, mask=m), want)
    # list mode: 6 entries into 7 output rows, one entry dropped
    list_row, list_src = np.array([5, 0, 6, 2, 1, 3]), np.array([1 * K + 2, -1, 3 * K + 0, 0 * K + 1, 3 * K + 2, 2 * K + 0])
    mask7 = np.array([0, 1, 0, 3, 4, 5, 2])
    for bias in (None, b):
        for m in (None, mask7):
            want = torch.zeros(7, Cout, dtype=torch.float64)
            for e in range(6):
                o = list_row[e]
                row = torch.zeros(Cout, dtype=torch.float64) if bias is None else bias.clone()
                if list_src[e] >= 0:
                    row = row + A[list_src[e] // K] @ W[list_src[e] % K]
                want[o] = 0 if (m is not None and m[o] != o) else row
            got = KR.gemm_ref(A, W, bias, list_src, list_row=list_row, mask=m, out_rows=7)
            assert torch.equal(got, want) and not got[4].any()          # row 4: no entry writes it
    # wgrad: the gathered side holds Ra rows, the other side R
    for gather_g in (0, 1):
        Aw, Gw = (_ints(g, R, Cin), _ints(g, Ra, Cout)) if gather_g else (_ints(g, Ra, Cin), _ints(g, R, Cout))
        want = torch.zeros(K, Cin, Cout, dtype=torch.float64)
        for k in range(K):
            for o in range(R):
                if T[o, k] >= 0:
                    ia, ig = (o, T[o, k]) if gather_g else (T[o, k], o)
                    for c in range(Cin):
                        for n in range(Cout):
                            want[k, c, n] += float(Aw[ia, c]) * float(Gw[ig, n])
        assert torch.equal(KR.wgrad_ref(Aw, Gw, T, gather_g), want)
    G = _ints(g, 7, 3)
    assert torch.equal(KR.colsum_ref(G), torch.stack([sum(G[o, c] for o in range(7)) for c in range(3)]))
    first, nxt = np.array([0, 1, 0, 5, 1, 5, 0]), np.array([2, 4, 6, -1, -1, 3, -1])   # chains 0-2-6, 1-4, 5-3 (descending)
    want = torch.zeros(7, 3, dtype=torch.float64)
    for r in range(7):
        if first[r] == r:
            j = r
            while j >= 0:
                want[r] += G[j]
                j = nxt[j]
    assert torch.equal(KR.dupsum_ref(G, first, nxt), want) and not want[[2, 3, 4, 6]].any() and want[5].equal(G[5] + G[3])


@pytest.mark.parametrize("per", [32, 64])
@pytest.mark.parametrize("R,K", [(1, 1), (63, 8), (64, 27), (65, 8), (129, 27), (300, 8)])
def test_structured_tables_hold_what_they_claim(R, K, per):
    for pattern in sorted(set(KR.GEMM_PATTERNS + KR.WGRAD_PATTERNS)):
        for n_src in (R, R + 7, max(1, R // 2)):
            T, claim = KR.build_table(pattern, R, K, n_src, per, seed=R + K)
            assert T.dtype == np.int32 and T.shape == (R, K) and T.min() >= -1 and T.max() < n_src, pattern
            assert KR.live_rows(T) == claim["live_rows"], pattern
            assert np.array_equal(KR.block_tap_live(T, per), claim["cells"]), pattern
    nb = -(-R // per)
    T, c = KR.build_table("empty", R, K, R, per)
    assert (T == -1).all() and not c["cells"].any()
    T, c = KR.build_table("block_last_row", R, K, R, per)
    assert c["live_rows"] == [min((j + 1) * per, R) - 1 for j in range(nb)] and all((T[r] >= 0).all() for r in c["live_rows"])
    T, c = KR.build_table("block_tap", R, K, R, per)
    assert all(list(np.nonzero(c["cells"][j])[0]) == [j % K] for j in range(nb))
    T, c = KR.build_table("one_source", R, K, R + 7, per)
    assert len(np.unique(T)) == 1 and T[0, 0] >= 0
    T, c = KR.build_table("step_last_row", R, K, R, per)
    assert c["live_rows"] == [o for o in range(R) if o % per == per - 1]
    T, c = KR.build_table("empty_steps", R, K, R, per)
    assert [bool(c["cells"][j].all()) for j in range(nb)] == [j % 3 == 0 for j in range(nb)] and not c["cells"][1::3].any()
    T, c = KR.build_table("empty_tap", R, K, R, per)
    assert (T[:, K // 2] == -1).all() and not c["cells"][:, K // 2].any()
    T, c = KR.build_table("last_row_only", R, K, R, per)
    assert c["live_rows"] == [R - 1] and (T[R - 1] >= 0).all() and int(c["cells"].sum()) == K
    T, c = KR.build_table("sparse", 300, 27, 300, per)
    assert 0.10 < (T >= 0).mean() < 0.20


@pytest.mark.parametrize("R,K,n_src", [(1, 1, 1), (65, 8, 40), (129, 27, 200)])
def test_structured_lists_masks_and_chains_hold_what_they_claim(R, K, n_src):
    for pattern in KR.LIST_PATTERNS:
        row, src, claim = KR.build_list(pattern, R, K, n_src, seed=R)
        assert row.dtype == src.dtype == np.int32 and sorted(row.tolist()) == list(range(R)) and src.min() >= -1 and src.max() < n_src * K
        assert sorted(int(o) for o, s in zip(row, src) if s >= 0) == claim["live_outputs"]
        taps = [int(s % K) for s in src if s >= 0]
        assert sorted(set(taps)) == claim["taps"]
        if pattern == "empty":
            assert (src == -1).all()
        if pattern == "one_tap":
            assert set(taps) <= {K - 1}
        if pattern in ("tap_major", "one_tap"):
            assert taps == sorted(taps) and (src[len(taps):] == -1).all()
    if R > 64:
        taps = [int(s % K) for s in KR.build_list("shuffled", R, K, n_src, seed=R)[1] if s >= 0]
        assert taps != sorted(taps)
    mask, kept = KR.build_mask(R, seed=K)
    assert kept == [o for o in range(R) if mask[o] == o] and 0 in kept and all(0 <= mask[o] < o for o in range(R) if o not in kept)
    if R > 64:
        assert 0.4 * R < len(kept) < 0.8 * R and (mask[1:] == 0).any()
        for order in ("ascending", "descending"):
            first, nxt, chains = KR.build_chains(R, [1, 2, 40], order, seed=K)
            assert sorted(r for c in chains for r in c) == list(range(R)) and [len(c) for c in chains[:3]] == [1, 2, 40]
            for c in chains:
                assert all(first[r] == c[0] for r in c) and [int(nxt[r]) for r in c] == c[1:] + [-1]
                assert c == sorted(c, reverse=order == "descending")
