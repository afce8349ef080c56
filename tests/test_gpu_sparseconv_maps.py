"""The maps of unipre3d_amd.sparseconv on the MI355X where a radix sort, a scan and a chain walk go wrong: every pass count of the
8-bit sort of site keys (1 to 7, keys up to 2^54), row counts around the 4096-row sort tile, sites at every corner of the grid in
every batch item, long chains of rows on one site, a strided conv that drops every row, graph capture and a side stream.  Maps are
compared bit for bit and values against the fp64 restatement by test_gpu_sparseconv._check."""
import ctypes

import numpy as np
import pytest
import torch

import spconv_ref as R
from test_gpu_sparseconv import _check, _t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bit_len(v):
    return int(v).bit_length()


def _subm_passes(B, D):
    return (_bit_len(B * D[0] * D[1] * D[2] - 1) + 7) // 8


def _down_passes(B, D, s):
    O = [(d - s) // s + 1 for d in D]
    return (_bit_len(B * O[0] * O[1] * O[2] * s ** 3) + 7) // 8


def _corners(B, D):
    out = []
    for b in range(B):
        for m in range(8):
            c = [(D[a] - 1) if (m >> a) & 1 else 0 for a in range(3)]
            inward = [v - 1 if v else 1 for v in c]
            out += [[b] + c, [b] + [min(max(v, 0), D[a] - 1) for a, v in enumerate(inward)], [b, min(inward[0], D[0] - 1), c[1], c[2]]]
    return np.asarray(out, dtype=np.int64)


def _sites(B, D, seed, n=3000, dup=100):
    """clusters of neighbouring sites (one per batch item at least, one against the far corner of the last item), isolated sites, the
    8 corners of every batch item with two inner neighbours each, `dup` repeated rows; rows permuted"""
    g = np.random.default_rng(seed)
    Dn = np.asarray(D, dtype=np.int64)
    ncl = max(B, 6)
    centres = np.concatenate([g.integers(0, Dn, size=(ncl - 1, 3)), (Dn - 2)[None]])
    cb = np.concatenate([np.arange(ncl - 1) % B, [B - 1]])
    per = n // ncl
    pts = np.concatenate([np.concatenate([np.full((per, 1), cb[i]), np.rint(centres[i] + g.normal(0, 2.5, size=(per, 3))).astype(np.int64)], 1)
                          for i in range(ncl)])
    iso = np.concatenate([g.integers(0, B, size=(n // 20, 1)), g.integers(0, Dn, size=(n // 20, 3))], 1)
    idx = np.concatenate([pts, iso, _corners(B, D)])
    idx[:, 1:] = np.clip(idx[:, 1:], 0, Dn - 1)
    idx = np.unique(idx, axis=0)
    idx = idx[g.permutation(len(idx))]
    if dup:
        idx = np.concatenate([idx, idx[g.choice(len(idx), dup, replace=len(idx) < dup)]])
        idx = idx[g.permutation(len(idx))]
    for b in range(B):     # the extremes are there: both ends of every batch item's key range
        assert (idx == [b, 0, 0, 0]).all(1).any() and (idx == [b, D[0] - 1, D[1] - 1, D[2] - 1]).all(1).any()
    return idx


# (n_batch, spatial shape): one shape per pass count of the site-key sort
KEY_SHAPES = [(2, (5, 5, 5)), (2, (20, 18, 22)), (3, (200, 180, 150)), (4, (1000, 900, 800)), (8, (5000, 4000, 3000)),
              (4, (40000, 30000, 20000)), (16, (100000, 90000, 80000))]


def test_key_shapes_cover_every_pass_count():
    """plain integer arithmetic on KEY_SHAPES: an edit of the list cannot lose a pass count"""
    assert sorted(_subm_passes(B, D) for B, D in KEY_SHAPES) == [1, 2, 3, 4, 5, 6, 7]
    for s in (2, 3):
        assert {_down_passes(B, D, s) & 1 for B, D in KEY_SHAPES} == {0, 1}, f"stride {s}: both ping-pong parities"
        assert {_down_passes(B, D, s) for B, D in KEY_SHAPES} >= {1, 2, 3, 4, 5}
    assert max(B * D[0] * D[1] * D[2] for B, D in KEY_SHAPES) > 1 << 48


@pytest.mark.parametrize("kind,k", [("subm", 3), ("down", 2), ("inv", 2), ("down", 3)])
@pytest.mark.parametrize("B,D", KEY_SHAPES)
def test_key_width(B, D, kind, k):
    idx = _sites(B, D, seed=_subm_passes(B, D))
    print(f"[sparseconv] key width: n_batch {B} shape {D}: {_subm_passes(B, D)} passes (SubM), {_down_passes(B, D, k)} (stride {k}); {len(idx)} rows")
    _check(kind, k, 32, 37, idx, list(D), B)


def test_shape_limit_is_refused():
    """one step beyond check_shape's limit (sites * 216 < 9e18): code 2 from every map entry point and nothing written"""
    from unipre3d_amd import _lib
    from unipre3d_amd import sparseconv as sp
    inside, beyond = [340000] * 3, [350000] * 3
    assert inside[0] ** 3 * 216 < 9.0e18 <= beyond[0] ** 3 * 216
    idx = np.asarray([[0, 0, 0, 0], [0, 339999, 339999, 339999], [0, 339999, 339999, 339998], [0, 5, 6, 7]], dtype=np.int64)
    _check("subm", 3, 32, 6, idx, inside, 1)
    _check("down", 2, 32, 6, idx, inside, 1)
    lib, N = sp.load(), len(idx)
    idx_d = _t(idx, torch.int32)
    bufs = [torch.full((N * 27,), -7, dtype=torch.int32, device=DEV) for _ in range(6)]
    meta = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(lib.u3d_spconv_scratch_bytes(N), dtype=torch.uint8, device=DEV)
    p = _lib.ptr
    null = ctypes.c_void_p(0)
    assert lib.u3d_spconv_subm_map(N, p(idx_d), 1, *beyond, 3, p(bufs[0]), p(bufs[1]), p(bufs[2]), p(scratch), null) == 2
    assert lib.u3d_spconv_down_map(N, p(idx_d), 1, *beyond, 2, p(meta), p(scratch), null) == 2
    assert lib.u3d_spconv_down_emit(N, 1, p(idx_d), 1, *beyond, 2, *[p(b) for b in bufs], p(scratch), null) == 2
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs + [meta]) and not scratch.any()
    for conv in (sp.SubMConv3d(4, 4, 3), sp.SparseConv3d(4, 4, 2, stride=2)):
        with pytest.raises(RuntimeError, match="code 2"):
            conv.to(DEV)(sp.SparseConvTensor(torch.zeros(N, 4, device=DEV), idx_d, beyond, 1))


# ---- row counts around the sort tile (4096 rows, 256 threads) ------------------------------------------------------------------
@pytest.mark.parametrize("kind,k", [("subm", 3), ("down", 2)])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_row_counts(N, kind, k):
    B, D = 2, (24, 23, 24)
    g = np.random.default_rng(N)
    cells = g.choice(B * D[0] * D[1] * D[2], size=N, replace=False)
    idx = np.stack([cells // (D[0] * D[1] * D[2]), cells // (D[1] * D[2]) % D[0], cells // D[2] % D[1], cells % D[2]], 1).astype(np.int64)
    _check(kind, k, 6, 32, idx, list(D), B)


def test_maps_above_1024_tiles():
    """1024 * 4096 + 1 rows = 1025 sort tiles: the digit scan walks each digit's line in five trips of 256 tiles with a carry (the last
    trip holds one tile), and the one-workgroup scan of the per-tile head counts owns two entries per thread.  The strided map's answer
    follows from np.unique of output site * 8 + tap (an even grid: no row is dropped)."""
    from unipre3d_amd import sparseconv as sp
    N, B, D, s = 1024 * 4096 + 1, 2, (192, 192, 192), 2
    g = np.random.default_rng(1025)
    idx = np.concatenate([g.integers(0, B, size=(N, 1)), g.integers(0, D[0], size=(N, 3))], 1)
    rf, rn = R.chains_np(idx, D)
    assert (rn >= 0).sum() > 100_000, "sites repeat"
    idx_d = _t(idx, torch.int32)

    m = sp.subm_map(idx_d, D, B, 1)
    first, nxt = m.first.cpu().numpy(), m.next.cpu().numpy()
    assert np.array_equal(first, rf) and np.array_equal(nxt, rn)
    assert np.array_equal(m.table.cpu().numpy()[:, 0], first)
    del m

    O = [d // s for d in D]
    out_site = ((idx[:, 0] * O[0] + idx[:, 1] // s) * O[1] + idx[:, 2] // s) * O[2] + idx[:, 3] // s
    key = out_site * s ** 3 + ((idx[:, 1] % s) * s + idx[:, 2] % s) * s + idx[:, 3] % s
    sites = np.unique(out_site)
    present, lowest = np.unique(key, return_index=True)           # the first occurrence of a key: its lowest row
    table = np.full((len(sites), s ** 3), -1, dtype=np.int64)
    table[np.searchsorted(sites, present // s ** 3), present % s ** 3] = lowest
    out_indices = np.stack([sites // (O[0] * O[1] * O[2]), sites // (O[1] * O[2]) % O[0], sites // O[2] % O[1], sites % O[2]], 1)
    m = sp.down_map(idx_d, D, B, s)
    assert m.out_shape == O and np.array_equal(m.out_indices.cpu().numpy(), out_indices)
    assert np.array_equal(m.table.cpu().numpy(), table)
    assert np.array_equal(m.first.cpu().numpy(), rf) and np.array_equal(m.next.cpu().numpy(), rn)


# ---- long chains of rows on one site -------------------------------------------------------------------------------------------
def _chain_sets():
    g = np.random.default_rng(11)
    D = (12, 12, 12)
    cells = g.choice(2 * 12 ** 3, size=500, replace=False)
    base = np.stack([cells // 1728, cells // 144 % 12, cells // 12 % 12, cells % 12], 1).astype(np.int64)
    many = np.concatenate([base, np.repeat(base[137:138], 1000, 0)])
    return {"one_site_x1000": many[g.permutation(len(many))], "all_rows_one_site": np.repeat(np.asarray([[1, 11, 0, 7]], np.int64), 300, 0),
            "every_site_x3": np.tile(base[:200], (3, 1))[g.permutation(600)]}, D


@pytest.mark.parametrize("kind", ["subm", "down", "inv"])
@pytest.mark.parametrize("name", ["one_site_x1000", "all_rows_one_site", "every_site_x3"])
def test_chains(name, kind):
    sets, D = _chain_sets()
    idx = sets[name]
    conv, X, y = _check(kind, 3 if kind == "subm" else 2, 32, 37, idx, list(D), 2)
    m = y.indice_dict["a" if kind == "subm" else "d"]
    first, nxt = m.first.cpu().numpy().astype(np.int64), m.next.cpu().numpy().astype(np.int64)
    rf, rn = R.chains_np(idx, D)     # an even grid: the strided map drops no row, so its chains are the sites' chains too
    assert np.array_equal(first, rf) and np.array_equal(nxt, rn)
    rows = {}
    for i, s in enumerate(map(tuple, idx)):
        rows.setdefault(s, []).append(i)
    assert max(len(v) for v in rows.values()) == {"one_site_x1000": 1001, "all_rows_one_site": 300, "every_site_x3": 3}[name]
    for rs in rows.values():
        assert all(first[r] == rs[0] for r in rs), "first: the lowest row at the row's site"
        walk, r = [], rs[0]
        while r != -1 and len(walk) <= len(rs):
            walk.append(int(r))
            r = nxt[r]
        assert walk == rs, "next from first visits the site's rows in ascending order and ends in -1"


# ---- a strided conv that drops every row ---------------------------------------------------------------------------------------
def _last_layer_sites(only):
    g = np.random.default_rng(3)
    allc = np.stack(np.meshgrid(np.arange(2), np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 4)
    last = (allc[:, 1:] == 4).any(1)
    idx = allc[last] if only else np.concatenate([allc[last][::2], allc[~last][::3]])
    return idx[g.permutation(len(idx))].astype(np.int64)


@pytest.mark.parametrize("bias", [True, False])
def test_everything_dropped(bias):
    from unipre3d_amd import sparseconv as sp
    idx = _last_layer_sites(True)
    N = len(idx)
    assert N > 0 and len(R.down_map(idx, (5, 5, 5), 2)["out_indices"]) == 0
    torch.manual_seed(0)
    down = sp.SparseConv3d(32, 16, 2, stride=2, bias=bias, indice_key="d").to(DEV)
    up = sp.SparseInverseConv3d(16, 32, 2, indice_key="d", bias=bias).to(DEV)
    X = torch.randn(N, 32, device=DEV, requires_grad=True)
    y = down(sp.SparseConvTensor(X, _t(idx, torch.int32), [5, 5, 5], 2))
    assert y.features.shape == (0, 16) and y.indices.shape == (0, 4) and y.spatial_shape == [2, 2, 2]
    m = y.indice_dict["d"]
    assert bool((m.list_src == -1).all()) and np.array_equal(np.sort(m.list_row.cpu().numpy()), np.arange(N))
    assert torch.equal(m.first.cpu(), torch.arange(N, dtype=torch.int32)) and bool((m.next == -1).all())
    z = up(y)
    assert z.features.shape == (N, 32) and torch.equal(z.indices.cpu(), torch.as_tensor(idx, dtype=torch.int32)) and z.spatial_shape == [5, 5, 5]
    want = up.bias.detach().expand(N, 32) if bias else torch.zeros(N, 32, device=DEV)
    assert torch.equal(z.features.detach(), want), "rows the conv dropped get the bias (or 0)"
    gZ = torch.randn(N, 32, device=DEV)
    z.features.backward(gZ)
    torch.cuda.synchronize()
    assert X.grad is not None and X.grad.shape == (N, 32) and not X.grad.any()
    for conv in (down, up):
        assert conv.weight.grad is not None and conv.weight.grad.shape == conv.weight.shape and not conv.weight.grad.any()
    if bias:
        assert not down.bias.grad.any()
        assert torch.allclose(up.bias.grad, gZ.double().sum(0).float(), rtol=0, atol=1e-5 * float(gZ.abs().sum(0).max()))
    # the strided conv alone: its backward has N rows to write from an empty dY
    X2 = torch.randn(N, 32, device=DEV, requires_grad=True)
    y2 = down(sp.SparseConvTensor(X2, _t(idx, torch.int32), [5, 5, 5], 2))
    y2.features.sum().backward()
    assert X2.grad.shape == (N, 32) and not X2.grad.any()


@pytest.mark.parametrize("kind", ["down", "inv"])
def test_some_rows_dropped(kind):
    idx = _last_layer_sites(False)
    dm = R.down_map(idx, (5, 5, 5), 2)
    assert 0 < (dm["row_out"] < 0).sum() < len(idx)
    _check(kind, 2, 32, 37, idx, [5, 5, 5], 2)


# ---- replay and streams --------------------------------------------------------------------------------------------------------
def _stack(seed=0):
    from unipre3d_amd import sparseconv as sp
    torch.manual_seed(seed)
    return (sp.SubMConv3d(32, 32, 3, padding=1, indice_key="s").to(DEV), sp.SparseConv3d(32, 64, 2, stride=2, indice_key="d").to(DEV),
            sp.SparseInverseConv3d(64, 32, 2, indice_key="d").to(DEV))


def _stack_inputs():
    idx = _sites(2, (21, 19, 23), seed=21, n=2000, dup=50)
    g = torch.Generator().manual_seed(5)
    return idx, torch.randn(len(idx), 32, generator=g), torch.randn(len(idx), 32, generator=g)


def _fwd_bwd(mods, x, X, gY):
    subm, down, up = mods
    y = up(down(subm(x))).features
    return (y,) + torch.autograd.grad(y, [X] + [p for m in mods for p in m.parameters()], gY)


def test_graph_capture_with_cached_maps():
    """With the maps built (the strided one reads its output count once), forward and backward of SubM -> inverse(down(.)) are captured
    into a graph: nothing in them reads the device from the host.  The replay equals the eager call bit for bit."""
    from unipre3d_amd import sparseconv as sp
    idx, X0, gY0 = _stack_inputs()
    mods = _stack()
    X, gY = X0.to(DEV).requires_grad_(True), gY0.to(DEV)
    x = sp.SparseConvTensor(X, _t(idx, torch.int32), [21, 19, 23], 2)
    eager = [t.detach().clone() for t in _fwd_bwd(mods, x, X, gY)]       # builds and caches both maps
    assert set(x.indice_dict) == {"s", "d"}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        _fwd_bwd(mods, x, X, gY)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _fwd_bwd(mods, x, X, gY)
    for t in outs:
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(outs, eager)):
        assert torch.equal(a.detach(), b), f"graph replay differs from the eager call (output {i})"
    assert eager[0].abs().sum() > 0 and eager[1].abs().sum() > 0


def test_side_stream_equals_default_stream():
    from unipre3d_amd import sparseconv as sp
    idx, X0, gY0 = _stack_inputs()
    res = []
    for stream in (None, torch.cuda.Stream()):
        mods = _stack()
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            X, gY = X0.to(DEV).requires_grad_(True), gY0.to(DEV)
            x = sp.SparseConvTensor(X, _t(idx, torch.int32), [21, 19, 23], 2)     # fresh tensor: the maps are built on this stream
            out = _fwd_bwd(mods, x, X, gY)
            maps = [x.indice_dict["s"].table, x.indice_dict["d"].table, x.indice_dict["d"].list_src]
        if stream is not None:
            torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        res.append([t.detach().clone() for t in out] + maps)
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), f"side stream differs from the default stream (tensor {i})"
