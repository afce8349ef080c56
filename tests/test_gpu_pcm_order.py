"""unipre3d_amd.pcm_order on the MI355X against the plain-torch restatement (tests/pcm_order_ref.py, run on the CPU) and the reference's
recorded values (tests/golden/g23_pcm_order.npz): integers and copies, so every comparison is bit for bit -- code, order, inverse,
every reordered tensor and every gradient.  One-workgroup sort up to 8192 rows, eight signed radix passes above."""
import os

import numpy as np
import pytest
import torch

import pcm_order_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_pcm_order.npz")
GS = 0.02


def _po():
    from unipre3d_amd import pcm_order
    return pcm_order


@pytest.fixture(scope="module")
def g23():
    return np.load(GOLDEN, allow_pickle=False)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _bits(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} against {want.dtype} {tuple(want.shape)}"
    view = torch.int32 if got.dtype == torch.float32 else got.dtype
    assert torch.equal(got.contiguous().view(view), want.contiguous().view(view)), f"{what} differs"


def _cloud(B, N, seed, extent=0.4):
    """Points on a lattice finer than the grid, so that cells repeat and some coordinates sit on cell boundaries."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, int(extent / 0.005), (B, N, 3), generator=g).float() * 0.005 - 0.1


def _check_order(pos, order, what):
    index, inverse, code = _po().point_order(pos.to(DEV), order, GS)
    ri, rv, rc = R.point_order(pos, order[0] if isinstance(order, list) else order, GS)
    _bits(code, rc, f"{what}: code")
    _bits(index, ri, f"{what}: order")
    _bits(inverse, rv, f"{what}: inverse")
    assert torch.equal(inverse[index].cpu(), torch.arange(pos.shape[0] * pos.shape[1]))
    return index, inverse, code


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257])
def test_point_order_all_orders(B, N):
    pos = _cloud(B, N, 100 * B + N)
    for order in R.ORDERS:
        _check_order(pos, order, f"B={B} N={N} {order}")
    _check_order(pos, ["hilbert"], "a list of one order")


@pytest.mark.parametrize("case, B, N, C, L, with_res", [(0, 1, 1, 1, 0, True), (1, 3, 2, 3, 1, True), (2, 1, 63, 5, 8, True),
                                                        (3, 3, 64, 384, 9, True), (4, 1, 65, 3, 9, False), (5, 3, 257, 5, 1, False),
                                                        (6, 3, 65, 1, 0, False), (7, 1, 257, 384, 8, True), (8, 3, 63, 3, 1, True)])
def test_serialization_forward_and_gradients(case, B, N, C, L, with_res):
    """Every (B, N) pair appears in test_point_order_all_orders; here each N, each C and 0 / 1 / 8 / 9 list entries appear at least
    once, x_res=None among them; case k runs the k-th of the nine shipped orders, so each is gathered and differentiated once."""
    P = _po()
    order = R.SHIPPED[case]
    g = torch.Generator().manual_seed(N * 7 + C)
    pos = _cloud(B, N, N + C)
    chans = [C, C + 1 if with_res else 0] + [(C, 1, 3, 5, 2, 4, 7, 6, 384)[i % 9] for i in range(L)]
    host = [torch.randn(B, N, c, generator=g) for c in chans if c]
    dev = [t.to(DEV).requires_grad_(True) for t in host]
    ref = [t.clone().requires_grad_(True) for t in host]
    k = 2 if with_res else 1
    outs_d, outs_r = list(dev[k:]), list(ref[k:])
    got = P.serialization(pos.to(DEV), dev[0], dev[1] if with_res else None, order, outs_d, GS)
    want = R.serialization(pos, ref[0], ref[1] if with_res else None, order, outs_r, GS)
    assert (got[2] is None) == (not with_res) and len(outs_d) == L and all(o is not t for o, t in zip(outs_d, dev[k:]))
    flat_d = [t for t in got if t is not None] + outs_d
    flat_r = [t for t in want if t is not None] + outs_r
    for i, (a, b) in enumerate(zip(flat_d, flat_r)):
        assert a.is_contiguous()
        _bits(a, b.detach(), f"{order}: output {i}")
    grads = [torch.randn(t.shape, generator=g) for t in flat_r[1:]]
    torch.autograd.backward(flat_d[1:], [x.to(DEV) for x in grads])
    torch.autograd.backward(flat_r[1:], grads)
    for i, (a, b) in enumerate(zip(dev, ref)):
        _bits(a.grad, b.grad, f"{order}: gradient {i}")


def test_partial_gradients_and_reorder():
    """Only some outputs used downstream, a tensor without requires_grad, and reorder on its own with (rows, C) tensors."""
    P = _po()
    g = torch.Generator().manual_seed(5)
    pos = _cloud(2, 65, 9)
    index, inverse, _ = P.point_order(pos.to(DEV), "zyx", GS)
    a, b, c = (torch.randn(130, ch, generator=g) for ch in (5, 4, 2048))
    da, db, dc = a.to(DEV).requires_grad_(True), b.to(DEV), c.to(DEV).requires_grad_(True)
    ya, yb, yc = P.reorder(index, inverse, da, db, dc)
    ix = index.cpu()
    _bits(ya, a[ix], "a"), _bits(yb, b[ix], "b"), _bits(yc, c[ix], "c")
    assert not yb.requires_grad
    w = torch.randn(130, 5, generator=g)
    (ya * w.to(DEV)).sum().backward()                       # yc unused: its gradient never materialises
    want = torch.zeros(130, 5)
    want[ix] = w
    _bits(da.grad, want, "da")
    assert dc.grad is None
    assert P.reorder(index, inverse) == ()


def test_non_contiguous_feat_is_copied():
    P = _po()
    g = torch.Generator().manual_seed(6)
    pos = _cloud(3, 64, 11)
    wide = torch.randn(3, 64, 10, generator=g)
    host = wide[:, :, 1:10:2].clone().requires_grad_(True)
    dwide = wide.to(DEV).requires_grad_(True)
    view = dwide[:, :, 1:10:2]
    assert not view.is_contiguous()
    got = P.serialization(pos.to(DEV), view, None, "hilbert", [], GS)
    want = R.serialization(pos, host, None, "hilbert", [], GS)
    _bits(got[1], want[1].detach(), "feat")
    w = torch.randn(3, 64, 5, generator=g)
    (got[1] * w.to(DEV)).sum().backward()
    (want[1] * w).sum().backward()
    full = torch.zeros(3, 64, 10)
    full[:, :, 1:10:2] = host.grad
    _bits(dwide.grad, full, "gradient through the view")
    tr = torch.randn(64, 3, 4, generator=g)                  # (N, B, C) seen as (B, N, C)
    got = P.serialization(pos.to(DEV), tr.to(DEV).transpose(0, 1), None, "xyz", [], GS)
    _bits(got[1], R.serialization(pos, tr.transpose(0, 1), None, "xyz", [], GS)[1], "transposed feat")


@pytest.mark.parametrize("case", ["orders", "tiefree", "boundary", "planar", "onecell"])
def test_golden_cases(g23, case):
    P = _po()
    pos, feat, x_res = (_t(g23[f"{case}/{n}"]) for n in ("pos", "feat", "x_res"))
    gs = float(g23["grid_size"])
    B, N, _ = pos.shape
    for k, order in enumerate(str(o) for o in g23[f"{case}/orders"]):
        code = _t(g23[f"{case}/code"][k])
        index, inverse, got = P.point_order(pos.to(DEV), order, gs, check=True)
        _bits(got, code, f"{case} {order}: code against the reference's")
        _bits(index, torch.argsort(code, stable=True), f"{case} {order}: order")
        moved = P.serialization(pos.to(DEV), feat.to(DEV), x_res.to(DEV), order, [], gs)
        rows = torch.cat([m.cpu() for m in moved], 2).flatten(0, 1)
        _bits(rows, torch.cat([pos, feat, x_res], 2).flatten(0, 1)[index.cpu()], f"{case} {order}: rows")
        if code.unique().numel() == B * N:
            _bits(rows, _t(g23[f"{case}/rows"][k]), f"{case} {order}: rows against the reference's")
    if case == "onecell":
        _bits(P.point_order(pos.to(DEV), "hilbert", gs)[2], torch.arange(B).repeat_interleave(N), "depth 0 hilbert")


def test_signed_sort_takes_any_int64_on_both_paths():
    """u3d_ser_sort_signed directly: extreme and negative keys, ties, at one row, at the one-workgroup limit and one past it."""
    from unipre3d_amd import _lib, serialization as ser
    lib = ser.load()
    rng = np.random.default_rng(8)
    for n in (1, 255, 8192, 8193):
        code = torch.from_numpy(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True))
        code[::3] = code[::3] >> 40                                   # small magnitudes of both signs: constant upper digits, ties
        code[::7] = torch.tensor([-2**63, 2**63 - 1, 0, -1])[torch.arange(len(code[::7])) % 4]
        d = code.to(DEV)
        order, inverse = torch.empty_like(d), torch.empty_like(d)
        scratch = torch.empty(lib.u3d_ser_scratch_bytes(1, n), dtype=torch.uint8, device=DEV)
        assert lib.u3d_ser_sort_signed(n, _lib.ptr(d), _lib.ptr(order), _lib.ptr(inverse), _lib.ptr(scratch), _lib.stream_ptr(DEV)) == 0
        ro, rv = R.order_inverse(code)
        _bits(order, ro, f"n={n}: order"), _bits(inverse, rv, f"n={n}: inverse")
    same = torch.full((300,), -5, dtype=torch.int64, device=DEV)      # every pass constant: the identity
    order, inverse = torch.empty_like(same), torch.empty_like(same)
    scratch = torch.empty(lib.u3d_ser_scratch_bytes(1, 300), dtype=torch.uint8, device=DEV)
    assert lib.u3d_ser_sort_signed(300, _lib.ptr(same), _lib.ptr(order), _lib.ptr(inverse), _lib.ptr(scratch), _lib.stream_ptr(DEV)) == 0
    assert torch.equal(order.cpu(), torch.arange(300)) and torch.equal(inverse.cpu(), torch.arange(300))


def test_large_batch_takes_the_multi_launch_sort():
    pos = _cloud(3, 2731, 12, extent=1.0)                              # 8193 rows
    for order in ("xyz", "hilbert"):
        _check_order(pos, order, f"8193 rows {order}")


def test_graph_capture_and_replay():
    P = _po()
    g = torch.Generator().manual_seed(13)
    B, N, C = 3, 65, 5
    pos, feat, x_res = _cloud(B, N, 14).to(DEV), torch.randn(B, N, C, generator=g).to(DEV), torch.randn(B, N, 3, generator=g).to(DEV)
    feat.requires_grad_(True)
    extra = torch.randn(B, N, 2, generator=g).to(DEV)
    dy = torch.randn(B, N, C, generator=g).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm-up outside the capture: the library is loaded
        P.serialization(pos, feat, x_res, "xzy", [extra], GS)[1].backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    feat.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [extra]
        moved = P.serialization(pos, feat, x_res, "xzy", outs, GS)
        (dfeat,) = torch.autograd.grad(moved[1], feat, dy)
    for seed in (15, 16):
        h = torch.Generator().manual_seed(seed)
        new = [_cloud(B, N, seed), torch.randn(B, N, C, generator=h), torch.randn(B, N, 3, generator=h), torch.randn(B, N, 2, generator=h),
               torch.randn(B, N, C, generator=h)]
        with torch.no_grad():
            for dst, src in zip((pos, feat, x_res, extra, dy), new):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        rf = new[1].clone().requires_grad_(True)
        routs = [new[3]]
        want = R.serialization(new[0], rf, new[2], "xzy", routs, GS)
        for a, b, what in zip((*moved, outs[0]), (*want, routs[0]), ("pos", "feat", "x_res", "layers_outputs[0]")):
            _bits(a, b.detach(), f"replay {seed}: {what}")
        _bits(dfeat, torch.autograd.grad(want[1], rf, new[4])[0], f"replay {seed}: d feat")


def test_error_paths_and_check_flag():
    P = _po()
    pos, feat = _cloud(2, 8, 17), torch.zeros(2, 8, 4)
    with pytest.raises(ValueError, match="order="):
        P.serialization(pos, feat, None, "xyzz", [], GS)               # CPU tensors: the order is refused before the device is looked at
    with pytest.raises(ValueError, match="order="):
        P.point_order(pos.to(DEV), "morton", GS)
    with pytest.raises(NotImplementedError, match="list of 2"):
        P.serialization(pos.to(DEV), feat.to(DEV), None, ["z", "hilbert"], [], GS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.serialization(pos, feat, None, "z", [], GS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.point_order(pos, "z", GS)
    with pytest.raises(ValueError, match="grid_size"):
        P.point_order(pos.to(DEV), "z", 0.0)
    with pytest.raises(ValueError, match="rows of channels"):
        P.serialization(pos.to(DEV), feat[:, :7].to(DEV), None, "z", [], GS)
    with pytest.raises(NotImplementedError, match="dtype"):
        P.serialization(pos.to(DEV), feat.double().to(DEV), None, "z", [], GS)
    far = pos.clone()
    far[0, 0, 0] = 0.02 * 70000                                       # a cell past 16 bits: flagged on the device, raised on request
    index, inverse, _ = P.point_order(far.to(DEV), "hilbert", GS)
    assert torch.equal(torch.sort(index.cpu())[0], torch.arange(16))   # still a permutation, every store in bounds
    with pytest.raises(ValueError, match="16 bits"):
        P.point_order(far.to(DEV), "hilbert", GS, check=True)
    far[0, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="16 bits"):
        P.point_order(far.to(DEV), "xyz", GS, check=True)
    P.point_order(pos.to(DEV), "xyz", GS, check=True)
