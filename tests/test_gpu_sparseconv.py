"""Sparse 3D convolution on the MI355X: unipre3d_amd.sparseconv against the fp64 restatement tests/spconv_ref.py (maps bit-exact; values
within 2e-6 (forward, input gradient) and 1e-5 (weight gradient) of sum|products| per element), edge cases, repeatability, PointFusion ->
fuseTo3d, and a SpUNet-shaped stack on a surface-like scene of more than 200 k voxels."""
import numpy as np
import pytest
import torch

import spconv_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_X, TOL_W = 2e-6, 1e-5


def _scene(seed, B=2, D=(20, 18, 22), n=2500, dup=0, empty_item=False):
    g = np.random.default_rng(seed)
    # a blob of neighbouring sites plus isolated ones
    pts = np.concatenate([g.normal(np.array(D) / 2, np.array(D) / 6, size=(n, 3)), g.uniform(0, np.array(D), size=(n // 20, 3))])
    pts = np.clip(np.floor(pts), 0, np.array(D) - 1).astype(np.int64)
    b = g.integers(0, 1 if empty_item else B, size=(len(pts), 1))
    idx = np.unique(np.concatenate([b, pts], 1), axis=0)
    idx = idx[g.permutation(len(idx))]
    if dup:
        idx = np.concatenate([idx, idx[g.choice(len(idx), dup, replace=False)]])
    return idx, list(D), B


def _t(a, dt=torch.float32):
    return torch.as_tensor(a).to(DEV, dt)


def _module(kind, Cin, Cout, k, seed):
    from unipre3d_amd import sparseconv as sp
    torch.manual_seed(seed)
    if kind == "subm":
        m = sp.SubMConv3d(Cin, Cout, k, padding=k // 2, bias=True, indice_key="a")
    elif kind == "down":
        m = sp.SparseConv3d(Cin, Cout, k, stride=k, bias=True, indice_key="d")
    else:
        m = sp.SparseInverseConv3d(Cin, Cout, k, indice_key="d", bias=True)
    with torch.no_grad():   # O(1) parameters so that the bias does not hide the products
        m.weight.normal_()
        m.bias.normal_()
    return m.to(DEV)


def _ref(kind, X, W, b, idx, D, k, dm):
    if kind == "subm":
        return R.subm(X, W, b, R.subm_table_np(idx, D, k))
    if kind == "down":
        return R.down(X, W, b, dm)
    return R.inverse(X, W, b, dm)


def _within(got, ref, bound, tol, what):
    err = (got.double() - ref).abs()
    lim = tol * bound + 1e-30
    bad = err > lim
    assert not bad.any(), f"{what}: {int(bad.sum())} elements out of bound, worst err/bound {float((err / (bound + 1e-30)).max()):.2e}"


def _check(kind, k, Cin, Cout, idx, D, B, seed=0):
    from unipre3d_amd import sparseconv as sp
    g = torch.Generator().manual_seed(seed)
    dm = R.down_map(idx, D, k) if kind != "subm" else None
    rows = len(dm["out_indices"]) if kind == "inv" else len(idx)
    X64 = torch.randn(rows, Cin, generator=g, dtype=torch.float64)
    conv = _module(kind, Cin, Cout, k, seed)
    X = X64.to(DEV, torch.float32).requires_grad_(True)
    x = sp.SparseConvTensor(X, _t(idx, torch.int32), D, B)
    if kind == "inv":   # the inverse needs its strided conv's map under the same key
        src = sp.SparseConvTensor(torch.zeros(len(idx), 1, device=DEV), _t(idx, torch.int32), D, B)
        down = sp.SparseConv3d(1, Cin, k, stride=k, indice_key="d").to(DEV)(src)
        x = down.replace_feature(X)
    y = conv(x)
    gY = torch.randn(y.features.shape, generator=g, dtype=torch.float64)
    y.features.backward(gY.to(DEV, torch.float32))
    torch.cuda.synchronize()
    # maps and output sites
    if kind == "subm":
        assert np.array_equal(x.indice_dict["a"].table.cpu().numpy(), R.subm_table_np(idx, D, k))
        assert torch.equal(y.indices.cpu(), torch.as_tensor(idx, dtype=torch.int32))
    elif kind == "down":
        m = x.indice_dict["d"]
        assert np.array_equal(m.out_indices.cpu().numpy(), dm["out_indices"]) and y.spatial_shape == dm["out_shape"]
        assert np.array_equal(m.table.cpu().numpy(), dm["table"])
        src = m.list_src.cpu().numpy()
        lr = m.list_row.cpu().numpy()
        kept = src >= 0
        assert np.array_equal(np.sort(lr), np.arange(len(idx)))
        assert np.array_equal(src[kept] // k ** 3, dm["row_out"][lr[kept]]) and np.array_equal(src[kept] % k ** 3, dm["row_tap"][lr[kept]])
        assert (dm["row_out"][lr[~kept]] == -1).all()
    else:
        assert torch.equal(y.indices.cpu(), torch.as_tensor(idx, dtype=torch.int32)) and y.spatial_shape == D
    # values: fp64 restatement on the device, bounds from |X|, |W|, |b|, |dY|
    W64, b64 = conv.weight.detach().double(), conv.bias.detach().double()
    Xd, Wd, bd = X64.to(DEV).requires_grad_(True), W64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    ref = _ref(kind, Xd, Wd, bd, idx, D, k, dm)
    gref = torch.autograd.grad(ref, (Xd, Wd, bd), gY.to(DEV))
    Xa, Wa = X64.abs().to(DEV).requires_grad_(True), W64.abs().requires_grad_(True)
    bound = _ref(kind, Xa, Wa, b64.abs(), idx, D, k, dm)
    gbound = torch.autograd.grad(bound, (Xa, Wa), gY.abs().to(DEV))
    _within(y.features.detach(), ref.detach(), bound.detach(), TOL_X, "forward")
    _within(X.grad, gref[0], gbound[0], TOL_X, "input gradient")
    _within(conv.weight.grad, gref[1], gbound[1], TOL_W, "weight gradient")
    _within(conv.bias.grad, gref[2], gY.abs().sum(0).to(DEV), TOL_W, "bias gradient")
    return conv, X, y


CHANNELS = [(3, 32), (6, 37), (37, 32), (32, 128), (128, 256), (256, 6)]


@pytest.mark.parametrize("Cin,Cout", CHANNELS)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_subm_against_restatement(k, Cin, Cout):
    idx, D, B = _scene(k * 7 + Cin, n=1200 if k == 5 else 2500)
    _check("subm", k, Cin, Cout, idx, D, B)


@pytest.mark.parametrize("Cin,Cout", CHANNELS)
@pytest.mark.parametrize("kind", ["down", "inv"])
def test_strided_and_inverse_against_restatement(kind, Cin, Cout):
    idx, D, B = _scene(Cout + 3, D=(21, 19, 23))   # odd shapes: the last layer of sites is dropped
    _check(kind, 2, Cin, Cout, idx, D, B)


@pytest.mark.parametrize("kind,k", [("subm", 3), ("down", 3), ("inv", 3)])
def test_stride_three(kind, k):
    _check(kind, k, 32, 37, *_scene(5, D=(20, 17, 22)))


@pytest.mark.parametrize("kind", ["subm", "down", "inv"])
def test_repeated_sites(kind):
    idx, D, B = _scene(9, dup=300)
    conv, X, y = _check(kind, 3 if kind == "subm" else 2, 32, 37, idx, D, B)
    if kind == "subm":   # a repeated row has an output equal to its site's first row, and no input gradient
        n0 = len(idx) - 300
        first = {}
        for i, r in enumerate(map(tuple, idx)):
            first.setdefault(r, i)
        rep = np.arange(n0, len(idx))
        f = np.array([first[tuple(idx[i])] for i in rep])
        assert torch.equal(y.features[rep], y.features[f])
        assert (X.grad[rep] == 0).all()


@pytest.mark.parametrize("kind", ["subm", "down", "inv"])
def test_edge_cases(kind):
    # a single site, an empty batch item, isolated sites only
    isolated = [[b, 4 * i, 4 * j, 4 * l] for b in range(2) for i in range(3) for j in range(3) for l in range(2)]
    for idx, D, B in (([[0, 3, 4, 5]], [8, 8, 8], 1), _scene(1, n=300, empty_item=True), (isolated[::-1], [12, 12, 8], 2)):
        _check(kind, 3 if kind == "subm" else 2, 32, 6, np.asarray(idx, dtype=np.int64).reshape(-1, 4), D, B)


def test_empty_input():
    from unipre3d_amd import sparseconv as sp
    idx = torch.zeros(0, 4, dtype=torch.int32, device=DEV)
    X = torch.zeros(0, 32, device=DEV, requires_grad=True)
    x = sp.SparseConvTensor(X, idx, [8, 8, 8], 2)
    for conv in (sp.SubMConv3d(32, 16, 3, indice_key="s"), sp.SparseConv3d(32, 16, 2, stride=2, indice_key="d")):
        y = conv.to(DEV)(x)
        assert y.features.shape == (0, 16)
        y.features.sum().backward()
        assert (conv.weight.grad == 0).all() and (conv.bias.grad == 0).all()
    up = sp.SparseInverseConv3d(16, 32, 2, indice_key="d").to(DEV)(y)
    assert up.features.shape == (0, 32) and up.indices.shape == (0, 4)


def test_repeated_calls_are_bit_identical():
    from unipre3d_amd import sparseconv as sp
    idx, D, B = _scene(4, dup=100)
    out = []
    for _ in range(2):
        torch.manual_seed(0)
        net = sp.SparseSequential(sp.SubMConv3d(6, 32, 5, indice_key="s0"), sp.SparseConv3d(32, 64, 2, stride=2, indice_key="d"),
                                  sp.SubMConv3d(64, 64, 3), sp.SparseInverseConv3d(64, 32, 2, indice_key="d")).to(DEV)
        X = torch.randn(len(idx), 6, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
        y = net(sp.SparseConvTensor(X, _t(idx, torch.int32), D, B))
        y.features.backward(torch.randn(y.features.shape, generator=torch.Generator().manual_seed(2)).to(DEV))
        out.append([y.features.detach().clone(), X.grad.clone()] + [p.grad.clone() for p in net.parameters()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_point_fusion_into_fuse_to_3d():
    from unipre3d_amd import sparseconv as sp
    from unipre3d_amd import synthetic
    from unipre3d_amd.pointfusion import PointFusion
    sc = synthetic.point_fusion_scene(V=4, H=60, W=80, C=32, seed=3)
    coord = sc["init_coord"].to(DEV)
    grid = torch.floor((coord - coord.min(0).values) / 0.02).int()
    uniq = torch.unique(grid, dim=0)
    feat3d = sp.SparseConvTensor(torch.randn(uniq.shape[0], 32, device=DEV, requires_grad=True),
                                 torch.cat([torch.zeros(uniq.shape[0], 1, dtype=torch.int32, device=DEV), uniq], 1).contiguous(),
                                 (uniq.max(0).values + 64).tolist(), 1)
    torch.manual_seed(0)
    fuse = sp.SparseSequential(sp.SubMConv3d(32, 32, 3, padding=1, bias=False), torch.nn.BatchNorm1d(32), torch.nn.ReLU()).to(DEV)
    pf = PointFusion(fuse, fea2d_dim=32, viewNum=4)
    feat2d = sc["feat_2d_all"].to(DEV).requires_grad_(True)
    data = {"coord": coord}
    out = pf(feat2d, feat3d, sc["unprojected_coord"].to(DEV), data, 0.02)
    assert isinstance(out, sp.SparseConvTensor) and out.features.shape[1] == 32
    out.features.square().sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(feat2d.grad).all() and feat2d.grad.abs().sum() > 0 and feat3d.features.grad.abs().sum() > 0
    # the SubM layer alone against the restatement on the combined (repeated-site) tensor
    comb_idx = data["grid_coord"]
    idx = torch.cat([data["batch"][:, None], comb_idx], 1).cpu().numpy()
    assert len(np.unique(idx, axis=0)) < len(idx)          # fused pixels share sites with 3D voxels
    _check("subm", 3, 32, 32, idx, feat3d.spatial_shape, 1)


def test_spunet_stack_at_c5_scale():
    """Stem k5 6->32, one level down (k2 s2) / encoder block / up (inverse) / decoder block with the skip concat, final k1; fp64
    restatement of the whole stack on the device, forward and backward."""
    from unipre3d_amd import sparseconv as sp
    from unipre3d_amd import synthetic
    sc = synthetic.sparse_voxel_scene(batch=2, seed=0)
    idx_t = sc["indices"].to(DEV)
    idx, D, B = sc["indices"].numpy().astype(np.int64), sc["spatial_shape"], sc["batch_size"]
    assert len(idx) >= 200_000
    torch.manual_seed(0)
    stem = sp.SubMConv3d(6, 32, 5, padding=1, bias=False, indice_key="stem").to(DEV)
    down = sp.SparseConv3d(32, 64, 2, stride=2, bias=False, indice_key="spconv1").to(DEV)
    enc = sp.SubMConv3d(64, 64, 3, padding=1, bias=False, indice_key="subm1").to(DEV)
    up = sp.SparseInverseConv3d(64, 32, 2, indice_key="spconv1", bias=False).to(DEV)
    dec = sp.SubMConv3d(64, 32, 3, padding=1, bias=False, indice_key="subm0").to(DEV)
    final = sp.SubMConv3d(32, 13, 1, bias=True).to(DEV)
    X = sc["features"].to(DEV).requires_grad_(True)
    x0 = stem(sp.SparseConvTensor(X, idx_t, D, B))
    x1 = enc(down(x0))
    u = up(x1)
    y = final(dec(u.replace_feature(torch.cat([u.features, x0.features], 1))))
    gY = torch.randn(y.features.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    params = [stem.weight, down.weight, enc.weight, up.weight, dec.weight, final.weight]
    got = torch.autograd.grad(y.features, [X] + params, gY.to(DEV, torch.float32))
    # restatement
    T5, T3, T1 = (R.subm_table_np(idx, D, k) for k in (5, 3, 1))
    dm = R.down_map(idx, D, 2)
    assert np.array_equal(x1.indices.cpu().numpy(), dm["out_indices"])
    T3c = R.subm_table_np(dm["out_indices"], dm["out_shape"], 3)

    def net(Xr, Ws, b):
        a0 = R.subm(Xr, Ws[0], None, T5)
        a1 = R.subm(R.down(a0, Ws[1], None, dm), Ws[2], None, T3c)
        a2 = R.inverse(a1, Ws[3], None, dm)
        return R.subm(R.subm(torch.cat([a2, a0], 1), Ws[4], None, T3), Ws[5], b, T1)

    Xd = X.detach().double().requires_grad_(True)
    Wd = [p.detach().double().requires_grad_(True) for p in params]
    ref = net(Xd, Wd, final.bias.detach().double())
    gref = torch.autograd.grad(ref, [Xd] + Wd, gY.to(DEV))
    # a stack has no per-element product bound: relative errors against fp32-level expectations
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    assert rel(y.features.detach(), ref.detach()) < 1e-5
    for i, (a, b) in enumerate(zip(got, gref)):
        assert rel(a, b) < 1e-5, (i, rel(a, b))
