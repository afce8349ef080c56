"""unipre3d_amd/feature_propagation.py on the device: the golden record of the reference's own two PointNetFeaturePropagation classes
(tests/golden/g22_feature_propagation.npz) through neighbours, propagate and both modules; the smallest shapes at which the kernels can go
wrong against the fp64 restatement; an out-of-range override, duplicated support points, reproducibility, graph capture and the argument
checks.

The rule (profiles/feature_propagation/tolerance.json, tests/feature_propagation_ref.py): bar = 2 x floor per quantity, in
max|x - fp64| / max|fp64|, the floor being the CPU-measured distance of the fp32 restatement from the fp64 record; idx and the lists are
held bit for bit, dpoints1 to be the dout[:, :D1] view.  The whole-module cases go through torch's convolutions and BatchNorm on both
sides and keep bar = 2 x yardstick + floor.

Shapes (B, N, S, D1, D2) of test_smallest_shapes; T = 1024 is the search's staging tile (U3D_FEATURE_PROPAGATION_TILE):
  (1, 1, 3, 4, 4)          a single query
  (1, 65, 3, 1, 1)         a lane past one wave, one channel each
  (1, 130, 1025, 0, 5)     T + 1 support points: a second staging pass of one point; no points1; odd channel count; a query past the
                           search's 128 per workgroup
  (1, 8, 4, 512, 1024)     the decoder's largest channel counts
  (1, 300, 4, 4, 8)        one support point at the centroid and three far away: list 0 holds an entry of every query
  (1, 64, 1, 4, 8)         S = 1
  (3, 32, 16, 8, 8)        scales 1 / 10 / 100
  (2, 1040, 520, 68, 36)   no kernel here loops over workgroups, so this is the shape at which every launch has several workgroups and a
                           partial last one: 9 of 128 queries in the search, 5 of 256 queries x 7 tiles of 16 channels in the forward (the
                           fifth tile holds points1's last 4 channels and the first 12 interpolated ones, the seventh 8), 3 of 256 support
                           points x 5 tiles of 8 channels in the backward (the fifth holds 4), whose LDS staging takes a second tile of
                           16 queries after the first 1024, 3120 entries and 521 bins under the 1024 threads of the list build,
                           131 workgroups of 4 lists in the ranking"""
import numpy as np
import pytest
import torch

import feature_propagation_ref as FR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 3, 4, 4, "independent"), (1, 65, 3, 1, 1, "subset"), (1, 130, 1025, 0, 5, "independent"), (1, 8, 4, 512, 1024, "subset"),
          (1, 300, 4, 4, 8, "centroid"), (1, 64, 1, 4, 8, "subset"), (3, 32, 16, 8, 8, "scales"), (2, 1040, 520, 68, 36, "subset")]


@pytest.fixture(scope="module")
def golden():
    return np.load(FR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def tol():
    return FR.tolerance()


def _dev(a, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _inputs(B, N, S, D1, D2, kind, seed):
    rng = np.random.default_rng(seed)
    xyz1 = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    if kind == "independent":
        xyz2 = rng.uniform(-1, 1, (B, S, 3)).astype(np.float32)
    elif kind == "centroid":
        far = np.array([[40, 0, 0], [0, 50, 0], [0, 0, 60]], np.float32)
        xyz2 = np.concatenate([xyz1.mean(1, keepdims=True), np.broadcast_to(far, (B, 3, 3))], axis=1).astype(np.float32)
    else:
        xyz2 = np.stack([xyz1[b, np.sort(rng.permutation(N)[:S])] for b in range(B)])
    p1 = rng.uniform(-1, 1, (B, D1, N)).astype(np.float32) if D1 else None
    p2 = rng.uniform(-1, 1, (B, D2, S)).astype(np.float32)
    if kind == "scales":
        sc = (10.0 ** np.arange(B)).astype(np.float32).reshape(B, 1, 1)
        xyz1, xyz2, p1, p2 = xyz1 * sc, xyz2 * sc, p1 * sc, p2 * sc
    return xyz1, xyz2, p1, p2, rng.uniform(-1, 1, (B, D1 + D2, N)).astype(np.float32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def _run(xyz1, xyz2, p1, p2, dout, neighbours=None):
    """{out, dpoints2, idx, weight} of neighbours + propagate, after holding dpoints1 to be the view of dout."""
    from unipre3d_amd import feature_propagation as fp
    a1, a2, g = _dev(p1, True), _dev(p2, True), _dev(dout)
    x1, x2 = _dev(xyz1), _dev(xyz2)
    nb = fp.neighbours(x1, x2) if neighbours is None else tuple(_dev(a) for a in neighbours)
    out = fp.propagate(x1, x2, a1, a2, neighbours=None if neighbours is None else nb)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == dout.shape
    if a1 is not None:
        g1, g2 = torch.autograd.grad(out, (a1, a2), g)
        assert g1.data_ptr() == g.data_ptr() and g1.stride() == g.stride() and tuple(g1.shape) == p1.shape       # the view: no copy
        assert torch.equal(out[:, :p1.shape[1]], a1)
    else:
        (g2,) = torch.autograd.grad(out, (a2,), g)
    torch.cuda.synchronize()
    assert g2.is_contiguous() and tuple(g2.shape) == p2.shape
    return {"out": out.detach().cpu().numpy(), "dpoints2": g2.cpu().numpy(), "idx": nb[0].cpu().numpy(), "weight": nb[1].cpu().numpy()}


def _check_lists(idx, S):
    """The library's lists of idx, bit for bit the restatement's."""
    from unipre3d_amd import _lib, feature_propagation as fp
    lib = fp.load()
    B, N, _ = idx.shape
    t = _dev(idx.astype(np.int32))
    ptr, ent = torch.empty(B, S + 1, dtype=torch.int32, device="cuda"), torch.empty(B, 3 * N, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.u3d_feature_propagation_scratch_bytes(B, N, S), dtype=torch.uint8, device="cuda")
    assert lib.u3d_feature_propagation_lists(_lib.ptr(t), _lib.ptr(ptr), _lib.ptr(ent), _lib.ptr(scratch), B, N, S, _lib.stream_ptr(t.device)) == 0
    rptr, rent = FR.inverse_lists(idx, S)
    assert np.array_equal(ptr.cpu().numpy(), rptr) and np.array_equal(ent.cpu().numpy(), rent)


def _check_search(got, xyz1, xyz2, r32, r64):
    from unipre3d_amd import knn
    S = xyz2.shape[1]
    assert got["idx"].dtype == np.int32 and np.array_equal(got["idx"], r32["idx"]) and np.array_equal(got["idx"], r64["idx"])
    if S >= 3:
        assert np.array_equal(got["idx"], knn.knn_query(3, _dev(xyz2), _dev(xyz1))[1].cpu().numpy())
    # d2 (three roundings that count), + 1e-8, two divisions and two sums: at most eight half-ulp steps on a value of at most 1
    assert np.abs(got["weight"].astype(np.float64) - r64["weight"]).max() <= 8 * 2.0 ** -24
    _check_lists(got["idx"], S)


@pytest.mark.parametrize("case", [str(n) for n in np.load(FR.GOLDEN, allow_pickle=False)["names"]])
def test_golden_cases(golden, tol, case):
    from unipre3d_amd import feature_propagation as fp
    c = FR.golden_case(golden, case)
    args = (c["xyz1"], c["xyz2"], c["points1"], c["points2"], c["dout"])
    got = _run(*args)
    D1 = 0 if c["points1"] is None else c["points1"].shape[1]
    assert np.array_equal(got["idx"], c["idx64"])
    _check_search(got, c["xyz1"], c["xyz2"], FR.restatement(*args, FR.f32), FR.restatement(*args, FR.f64))
    cut, bars = FR.recorded(got, c["cut"], D1), FR.bars(tol)
    d = {q: FR.dist(cut[q], golden[f"{case}_out64" if q == "out" else f"{case}_{q}_64"]) for q in FR.QUANTITIES}
    print(f"\nfeature_propagation golden {case}: " + "  ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in FR.QUANTITIES))
    for q in FR.QUANTITIES:
        assert np.isfinite(got[q]).all() and d[q] <= bars[q], q
    # PointMLP's module without its MLP is propagate itself
    with torch.no_grad():
        m = fp.PointNetFeaturePropagation(D1 + c["points2"].shape[1], 4, has_MLP=False)
        assert _same_bits(m(_dev(c["xyz1"]), _dev(c["xyz2"]), _dev(c["points1"]), _dev(c["points2"])).cpu().numpy(), got["out"])


@pytest.mark.parametrize("case", [str(n) for n in np.load(FR.GOLDEN, allow_pickle=False)["module_names"]])
def test_modules_against_the_record(golden, tol, case):
    from unipre3d_amd import feature_propagation as fp
    d = FR.module_dists(golden, case, FR.module_run(golden, case, fp.propagate, device="cuda"))
    bars = FR.module_bars(case, tol)
    print(f"\nfeature_propagation golden {case}: " + "  ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in FR.MODULE_QUANTITIES))
    for q in FR.MODULE_QUANTITIES:
        assert d[q] <= bars[q], q


def test_pcm_module_in_eval_mode_takes_the_same_path(golden):
    from unipre3d_amd import feature_propagation as fp
    name = "mod_pcm"
    m = fp.PCMPointNetFeaturePropagation(24, 16, blocks=1)
    m.load_state_dict({str(k): torch.from_numpy(golden[f"{name}_sd_{i}"]) for i, k in enumerate(golden[f"{name}_sd_names"])}, strict=True)
    m = m.cuda().eval()
    a = [_dev(golden[f"{name}_{k}"]) for k in ("xyz1", "xyz2", "points1", "points2")]
    with torch.no_grad():
        out = m(*a, k=3)
        assert torch.equal(out, m.extraction(m.fuse(fp.propagate(*a)))) and out.shape == (2, 16, 16)
    with pytest.raises(ValueError, match="k=4"):
        m(*a, k=4)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_smallest_shapes(tol, shape):
    B, N, S, D1, D2, kind = shape
    args = _inputs(*shape, seed=sum(shape[:5]))
    r32, r64 = FR.restatement(*args, FR.f32), FR.restatement(*args, FR.f64)
    got = _run(*args)
    _check_search(got, args[0], args[1], r32, r64)
    bars = FR.bars(tol)
    d = {q: FR.dist(got[q], r64[q]) for q in FR.QUANTITIES}
    print(f"\nfeature_propagation {shape}: " + "  ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e}, restatement {FR.dist(r32[q], r64[q]):.3e})"
                                                         for q in FR.QUANTITIES))
    for q in FR.QUANTITIES:
        assert np.isfinite(got[q]).all() and d[q] <= bars[q], q
    if kind == "centroid":
        assert (got["idx"][:, :, 0] == 0).all()
    if S == 1:
        assert _same_bits(got["out"][:, D1:], np.ascontiguousarray(np.broadcast_to(args[3], (B, D2, N))))


def test_override_with_an_index_out_of_range(tol):
    """An overridden index outside [0, S) is never dereferenced: its term is 0 and it receives no gradient, exactly as if its weight were 0."""
    B, N, S, D1, D2 = 2, 70, 9, 4, 12
    xyz1, xyz2, p1, p2, dout = _inputs(B, N, S, D1, D2, "subset", seed=21)
    idx, w = FR.search(xyz1, xyz2, FR.f32)
    bad = idx.copy()
    for (b, n, j), v in {(0, 5, 1): -1, (1, 69, 0): S, (0, 0, 2): 2 ** 31 - 1, (1, 33, 2): -2 ** 31}.items():
        bad[b, n, j] = v
    bad[1, :, 1] = np.where(bad[1, :, 1] == 3, S + 7, bad[1, :, 1])           # support point 3 of batch element 1 loses a column of entries
    safe, w0 = np.clip(bad, 0, S - 1), np.where((bad < 0) | (bad >= S), 0, w).astype(np.float32)
    a, b = _run(xyz1, xyz2, p1, p2, dout, neighbours=(bad, w)), _run(xyz1, xyz2, p1, p2, dout, neighbours=(safe, w0))
    for q in FR.QUANTITIES:
        assert _same_bits(a[q], b[q]) and np.isfinite(a[q]).all(), q
    _check_lists(bad, S)
    ref, bars = FR.restatement(xyz1, xyz2, p1, p2, dout, FR.f64, neighbours=(bad, w)), FR.bars(tol)
    for q in FR.QUANTITIES:
        assert FR.dist(a[q], ref[q]) <= bars[q], q
    # a support point no entry names gets exactly 0
    lone = np.zeros_like(idx)
    lone[:, :, 1], lone[:, :, 2] = 1, 2
    got = _run(xyz1, xyz2, p1, p2, dout, neighbours=(lone, w))
    assert (got["dpoints2"][:, :, 3:].view(np.int32) == 0).all() and got["dpoints2"][:, :, :3].all()
    # int64 indices, as torch's own searches return them
    assert _same_bits(_run(xyz1, xyz2, p1, p2, dout, neighbours=(idx.astype(np.int64), w))["out"], _run(xyz1, xyz2, p1, p2, dout)["out"])


def test_duplicated_support_points(tol):
    rng = np.random.default_rng(22)
    B, N, D1, D2 = 2, 40, 4, 8
    xyz1 = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    base = xyz1[:, :5]
    xyz2 = np.concatenate([base, base[:, ::-1], base], axis=1)               # every support point three times; queries 0 .. 4 sit on them
    S = xyz2.shape[1]
    p1, p2 = rng.uniform(-1, 1, (B, D1, N)).astype(np.float32), rng.uniform(-1, 1, (B, D2, S)).astype(np.float32)
    dout = rng.uniform(-1, 1, (B, D1 + D2, N)).astype(np.float32)
    r32, r64 = FR.restatement(xyz1, xyz2, p1, p2, dout, FR.f32), FR.restatement(xyz1, xyz2, p1, p2, dout, FR.f64)
    got = _run(xyz1, xyz2, p1, p2, dout)
    _check_search(got, xyz1, xyz2, r32, r64)
    i = got["idx"]
    assert (i[:, :, 0] < 5).all() and np.array_equal(i[:, :, 1], 9 - i[:, :, 0]) and np.array_equal(i[:, :, 2], 10 + i[:, :, 0])      # lower index first
    assert _same_bits(got["weight"][:, :, 0], got["weight"][:, :, 1]) and _same_bits(got["weight"][:, :, 0], got["weight"][:, :, 2])
    for q in FR.QUANTITIES:
        assert FR.dist(got[q], r64[q]) <= FR.bars(tol)[q], q


def test_two_calls_give_the_same_bits():
    args = _inputs(3, 200, 100, 68, 7, "subset", seed=23)
    a, b = _run(*args), _run(*args)
    for q in a:
        assert _same_bits(a[q], b[q]), q


def test_graph_capture_replays_to_the_eager_bits():
    from unipre3d_amd import feature_propagation as fp
    B, N, S, D1, D2 = 2, 256, 128, 16, 32
    xyz1, xyz2, p1, p2, dout = _inputs(B, N, S, D1, D2, "subset", seed=24)
    x1, x2, s1, s2, sd = _dev(xyz1), _dev(xyz2), _dev(p1, True), _dev(p2, True), _dev(dout)
    run = lambda a1, a2, g: torch.autograd.grad(fp.propagate(x1, x2, a1, a2), (a2,), g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s1, s2, sd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_out = fp.propagate(x1, x2, s1, s2)
        (c_g2,) = torch.autograd.grad(c_out, (s2,), sd)
    g = torch.Generator().manual_seed(4)
    n1, n2, nd = (torch.randn(t.shape, generator=g).cuda() for t in (s1, s2, sd))
    with torch.no_grad():
        s1.copy_(n1)
        s2.copy_(n2)
        sd.copy_(nd)
    graph.replay()
    torch.cuda.synchronize()
    e1, e2 = n1.clone().requires_grad_(True), n2.clone().requires_grad_(True)
    e_out = fp.propagate(x1, x2, e1, e2)
    (e_g2,) = torch.autograd.grad(e_out, (e2,), nd)
    assert torch.equal(c_out.detach().view(torch.int32), e_out.detach().view(torch.int32)) and torch.isfinite(c_out).all()
    assert torch.equal(c_g2.view(torch.int32), e_g2.view(torch.int32)) and torch.isfinite(c_g2).all()


def test_autograd_node_keeps_the_lists_and_the_weights_alone():
    from unipre3d_amd import feature_propagation as fp
    B, N, S, D1, D2 = 2, 64, 32, 8, 16
    xyz1, xyz2, p1, p2, _ = _inputs(B, N, S, D1, D2, "subset", seed=25)
    out = fp.propagate(_dev(xyz1), _dev(xyz2), _dev(p1, True), _dev(p2, True))
    saved = out.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [(B, S + 1), (B, 3 * N), (B, N, 3)]
    assert fp.propagate(_dev(xyz1), _dev(xyz2), _dev(p1), _dev(p2)).grad_fn is None


def test_device_argument_checks():
    from unipre3d_amd import feature_propagation as fp
    z = lambda *s: torch.zeros(*s, device="cuda")
    xyz1, xyz2, p1, p2 = z(1, 16, 3), z(1, 4, 3), z(1, 2, 16), z(1, 5, 4)
    assert fp.propagate(xyz1, xyz2, p1, p2).shape == (1, 7, 16) and fp.propagate(xyz1, xyz2, None, p2).shape == (1, 5, 16)
    with pytest.raises(ValueError, match="S = 2"):
        fp.propagate(xyz1, z(1, 2, 3), p1, z(1, 5, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        fp.propagate(xyz1.cpu(), xyz2, p1, p2)
    with pytest.raises(RuntimeError, match="HIP device"):
        fp.propagate(xyz1, xyz2, p1, p2.cpu())
    with pytest.raises(NotImplementedError, match="requires_grad"):
        fp.propagate(xyz1.clone().requires_grad_(True), xyz2, p1, p2)
    with pytest.raises(NotImplementedError, match="requires_grad"):
        fp.neighbours(xyz1, xyz2.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="k=1"):
        fp.PCMPointNetFeaturePropagation(7, 4).cuda()(xyz1, xyz2, p1, p2, k=1)
    with pytest.raises(NotImplementedError, match="D1="):
        fp.propagate(xyz1, xyz2, p1, z(1, fp.MAX_CHANNELS + 1, 4))
    with pytest.raises(NotImplementedError, match="N="):
        fp.neighbours(z(1, fp.MAX_POINTS + 1, 3), xyz2)
    # other floating types and strided inputs are cast or copied
    g = torch.Generator().manual_seed(3)
    x1, x2 = torch.randn(1, 16, 3, generator=g).cuda(), torch.randn(1, 4, 3, generator=g).cuda()
    q1, q2 = torch.randn(1, 2, 16, generator=g).cuda(), torch.randn(1, 5, 4, generator=g).cuda()
    want = fp.propagate(x1, x2, q1, q2)
    assert torch.equal(fp.propagate(x1.double(), x2.permute(0, 2, 1).contiguous().permute(0, 2, 1), q1.double(),
                                    q2.permute(0, 2, 1).contiguous().permute(0, 2, 1)), want)
