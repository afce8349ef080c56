"""unipre3d_amd/local_grouper.py on the device: the golden record of the reference's own two LocalGrouper classes
(tests/golden/g21_local_grouper.npz) through local_group and both modules, in both input layouts and both output layouts; the smallest
shapes at which something can go wrong against the fp64 restatement; one list that holds every entry, duplicate anchors, out-of-range
indices, a std of zero, the whole-module path without overrides, reproducibility, graph capture and the argument checks.

The rule (profiles/local_grouper/tolerance.json, tests/local_grouper_ref.py): bar = 2 x yardstick + floor per quantity, in
max|x - fp64| / max|fp64|; the yardstick is the reference's own fp32 error against fp64 (recorded for the golden cases, computed on the
spot on the CPU elsewhere), the floor the CPU-measured distance of the fp32 restatement in the kernels' order.

Shapes (B, N, S, D, K) of test_smallest_shapes:
  (2, 16, 8, 8, 4)      every mode x use_xyz; C = 2 D + 3 = 19, so rows are off a float4
  (1, 12, 12, 4, 3)     S == N with no fps_idx
  (1, 64, 32, 12, 24)   use_xyz = False
  (1, 64, 32, 4, 64)    K == N: every list has S entries
  (1, 8, 4, 512, 2)     the largest D
  (3, 32, 16, 8, 4)     per-batch scales of 1 / 10 / 100
  (1, 1040, 520, 68, 3) more anchors than one pass of the 128 x 4 rows of the statistics kernel (and of the 32 x 8 of the first backward
                        kernel) takes; a lane's second channel"""
import numpy as np
import pytest
import torch

import local_grouper_ref as GR

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 8, 8, 4, m, u) for m in (None, "center", "anchor") for u in (True, False)] + [
    (1, 12, 12, 4, 3, "center", True), (1, 64, 32, 12, 24, "anchor", False), (1, 64, 32, 4, 64, "center", True),
    (1, 8, 4, 512, 2, "anchor", True), (3, 32, 16, 8, 4, "anchor", True), (1, 1040, 520, 68, 3, "center", True)]
LAYOUTS = [(False, True), (False, False), (True, True), (True, False)]          # (points transposed, channels_first)
LAYOUT_IDS = ["rows_cf", "rows_cl", "transposed_cf", "transposed_cl"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def tol():
    return GR.tolerance()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _points(points, transposed):
    """(leaf, the (B, N, D) tensor passed): rows contiguous, or the permute(0, 2, 1) view of a (B, D, N) leaf."""
    p = _dev(points)
    if transposed:
        leaf = p.permute(0, 2, 1).contiguous().requires_grad_(True)
        return leaf, leaf.permute(0, 2, 1)
    leaf = p.requires_grad_(True)
    return leaf, leaf


def _dout(dout, cf):
    d = _dev(dout)
    return d.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2) if cf else d


def _check_layouts(out, leaf, transposed, cf):
    B, S, K, C = out.shape
    assert out.stride() == ((S * K * C, C * K, 1, K) if cf else (S * K * C, K * C, C, 1))
    if cf:      # PreExtraction's permute + reshape is a view
        assert out.permute(0, 1, 3, 2).reshape(-1, C, K).data_ptr() == out.data_ptr()
    assert leaf.grad.shape == leaf.shape and leaf.grad.is_contiguous()


def _run(xyz, points, fps, idx, alpha, beta, dout, mode, use_xyz, transposed=False, cf=True):
    """{quantity: host array} of local_group, plus new_xyz and stats."""
    from unipre3d_amd import local_grouper as lg
    leaf, p = _points(points, transposed)
    a = b = None
    if mode is not None:
        a, b = _dev(alpha).requires_grad_(True), _dev(beta).requires_grad_(True)
    new_xyz, out, stats = lg.local_group_with_stats(_dev(xyz), p, _dev(fps), _dev(idx), a, b, mode, use_xyz, channels_first=cf)
    out.backward(_dout(dout, cf))
    torch.cuda.synchronize()
    _check_layouts(out, leaf, transposed, cf)
    res = {"out": out.detach().contiguous().cpu().numpy(), "dpoints": (leaf.grad.permute(0, 2, 1) if transposed else leaf.grad).cpu().numpy(),
           "new_xyz": new_xyz.cpu().numpy(), "stats": stats.cpu().numpy()}
    if mode is not None:
        res["dalpha"], res["dbeta"] = a.grad.cpu().numpy(), b.grad.cpu().numpy()
    return res


def _inputs(B, N, S, D, K, mode, use_xyz, seed, scales=False):
    rng = np.random.default_rng(seed)
    Cn = D + (3 if use_xyz else 0)
    xyz, points = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32), rng.uniform(-1, 1, (B, N, D)).astype(np.float32)
    if scales:
        sc = (10.0 ** np.arange(B)).astype(np.float32).reshape(B, 1, 1)
        xyz, points = xyz * sc, points * sc
    dout = rng.uniform(-1, 1, (B, S, K, D + Cn)).astype(np.float32)
    alpha = (rng.uniform(0.5, 1.5, Cn) * rng.choice([-1.0, 1.0], Cn)).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, Cn).astype(np.float32)
    fps = None if S == N else np.stack([rng.permutation(N)[:S] for _ in range(B)]).astype(np.int32)
    idx = np.stack([np.stack([rng.permutation(N)[:K] for _ in range(S)]) for _ in range(B)]).astype(np.int32)
    idx[:, :, 0] = np.arange(S) if fps is None else fps            # an anchor is its own first neighbour
    return xyz, points, fps, idx, alpha, beta, dout


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _args(c):
    return c["xyz"], c["points"], c["fps"], GR.used_idx(c), c["alpha"], c["beta"], c["dout"]


@pytest.fixture(scope="module")
def golden_runs(golden):
    """{(case, layout id): result of _run}, each computed once."""
    cache = {}

    def get(case, layout):
        if (case, layout) not in cache:
            c = GR.golden_case(golden, case)
            transposed, cf = LAYOUTS[LAYOUT_IDS.index(layout)]
            cache[(case, layout)] = _run(*_args(c), c["mode"], c["use_xyz"], transposed, cf)
        return cache[(case, layout)]
    return get


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("case", [str(n) for n in np.load(GR.GOLDEN, allow_pickle=False)["names"]])
def test_golden_cases(golden, tol, golden_runs, case, layout):
    c = GR.golden_case(golden, case)
    got = golden_runs(case, layout)
    qs = GR.quantities(c["mode"])
    assert got["out"].shape == c["dout"].shape and got["dpoints"].shape == c["points"].shape
    assert all(got[q].dtype == np.float32 and np.isfinite(got[q]).all() for q in qs)
    cut, bars = GR.recorded(got, c["cut"]), GR.case_bars(case, tol)
    d = {q: GR.dist(cut[q], golden[f"{case}_{q}64"]) for q in qs}
    print(f"\nlocal_grouper golden {case} {layout}: " + "  ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in qs))
    for q in qs:
        assert d[q] <= bars[q], q
    assert np.array_equal(got["new_xyz"], golden[f"{case}_new_xyz64"].astype(np.float32))
    if c["mode"] is not None:
        _, _, mu64, s64 = GR.forward_f64(*_args(c)[:6], c["mode"], c["use_xyz"])
        mu, s, r, c0 = got["stats"].T
        assert (np.abs(s - s64) <= 2.0 ** -23 * s64).all() and (np.abs(mu - mu64) <= 2.0 ** -23 * s64).all()
        assert np.allclose(r, 1.0 / (s.astype(np.float64) + 1e-5), rtol=2.0 ** -22, atol=0)
    else:
        assert got["stats"].shape == (0, 4)


@pytest.mark.parametrize("case", ["center_xyz", "anchor_noxyz", "none_xyz", "pcm_stride", "stage1"])
def test_layouts_give_the_same_bits(golden_runs, case):
    """The two output layouts hold the same values, and neither they nor the input's layout change one bit of any result."""
    first = golden_runs(case, LAYOUT_IDS[0])
    for layout in LAYOUT_IDS[1:]:
        other = golden_runs(case, layout)
        for q in first:
            assert _same_bits(first[q], other[q]), (layout, q)


@pytest.mark.parametrize("case", [str(n) for n in np.load(GR.GOLDEN, allow_pickle=False)["names"]])
def test_modules_against_the_record(golden, tol, case):
    """The case's own module (PointMLP's or PCM's) with the recorded fps_idx and idx as overrides, points as its callers pass them."""
    from unipre3d_amd import local_grouper as lg
    c = GR.golden_case(golden, case)
    B, N, D = c["points"].shape
    K = c["idx"].shape[2]
    if c["module"] == "pcm":
        m = lg.PCMLocalGrouper(D, c["sample_ratio"], K, use_xyz=c["use_xyz"], normalize=c["mode"], k_stride=c["k_stride"])
    else:
        m = lg.LocalGrouper(D, c["sample_ratio"], K, use_xyz=c["use_xyz"], normalize=c["mode"])
    if c["mode"] is not None:
        m.load_state_dict({"affine_alpha": torch.from_numpy(c["alpha"]).view(1, 1, 1, -1), "affine_beta": torch.from_numpy(c["beta"]).view(1, 1, 1, -1)})
    m = m.cuda()
    leaf, p = _points(c["points"], True)
    extra = (_dev(c["points_res"]),) if c["module"] == "pcm" else ()
    res = m(_dev(c["xyz"]), p, *extra, fps_idx=_dev(c["fps"]), idx=_dev(c["idx"]))
    res[1].backward(_dout(c["dout"], True))
    torch.cuda.synchronize()
    _check_layouts(res[1], leaf, True, True)
    got = {"out": res[1].detach().contiguous().cpu().numpy(), "dpoints": leaf.grad.permute(0, 2, 1).cpu().numpy()}
    if c["mode"] is not None:
        got["dalpha"], got["dbeta"] = m.affine_alpha.grad.cpu().numpy().reshape(-1), m.affine_beta.grad.cpu().numpy().reshape(-1)
    cut, bars = GR.recorded(got, c["cut"]), GR.case_bars(case, tol)
    for q in GR.quantities(c["mode"]):
        assert GR.dist(cut[q], golden[f"{case}_{q}64"]) <= bars[q], q
    assert np.array_equal(res[0].cpu().numpy(), golden[f"{case}_new_xyz64"].astype(np.float32))
    if c["module"] == "pcm":
        assert np.array_equal(res[2].cpu().numpy(), golden[f"{case}_res64"].astype(np.float32))


@pytest.mark.parametrize("case", ["anchor_xyz", "pcm_stride", "stage1"])
def test_modules_without_overrides_find_the_recorded_groups(golden, tol, case):
    """No overrides: the project's own furthest point sampling and search.  On these tie-free clouds they select the recorded anchors and,
    after sorting along K, the recorded neighbours; PCM's search is recorded in ascending order, so there the whole result is held to the
    record, and for PointMLP (whose topk leaves the order open) its maximum over K, which is what every consumer takes."""
    from unipre3d_amd import knn, local_grouper as lg, pointops
    c = GR.golden_case(golden, case)
    B, N, D = c["points"].shape
    S, K = c["idx"].shape[1:]
    xyz = _dev(c["xyz"])
    fps = pointops.furthest_point_sample(xyz, S)
    if c["module"] == "pcm":
        fps = torch.sort(fps.long(), dim=-1)[0]
    assert np.array_equal(fps.cpu().numpy(), c["fps"])
    idx = knn.knn_query(K, xyz, torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)))[1].cpu().numpy()
    assert np.array_equal(np.sort(idx, -1), np.sort(c["idx"], -1))
    if c["module"] == "pcm":
        assert np.array_equal(idx, c["idx"])
        m = lg.PCMLocalGrouper(D, c["sample_ratio"], K, use_xyz=c["use_xyz"], normalize=c["mode"], k_stride=c["k_stride"])
    else:
        m = lg.LocalGrouper(D, c["sample_ratio"], K, use_xyz=c["use_xyz"], normalize=c["mode"])
    m.load_state_dict({"affine_alpha": torch.from_numpy(c["alpha"]).view(1, 1, 1, -1), "affine_beta": torch.from_numpy(c["beta"]).view(1, 1, 1, -1)})
    m = m.cuda()
    extra = (_dev(c["points_res"]),) if c["module"] == "pcm" else ()
    with torch.no_grad():
        out = m(xyz, _dev(c["points"]), *extra)[1].contiguous().cpu().numpy()
    want = golden[f"{case}_out64"]
    bar = GR.case_bars(case, tol)["out"]
    if c["module"] == "pcm":
        assert GR.dist(out, want) <= bar
    else:
        cut = GR.recorded({"out": out, "dpoints": c["points"]}, c["cut"])["out"]
        assert np.abs(cut.max(2) - want.max(2)).max() <= bar * np.abs(want).max()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_smallest_shapes(tol, shape):
    B, N, S, D, K, mode, use_xyz = shape
    args = _inputs(*shape, seed=sum(shape[:5]), scales=(B == 3))
    ref, bars = GR.spot_bars(*args, mode, use_xyz, tol)
    for transposed, cf in ((True, True), (False, False)):
        got = _run(*args, mode, use_xyz, transposed, cf)
        d = {q: GR.dist(got[q], ref[q]) for q in ref}
        print(f"\nlocal_grouper {shape} transposed={transposed} cf={cf}: " + "  ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in ref))
        for q in ref:
            assert np.isfinite(got[q]).all() and d[q] <= bars[q], q


def test_one_list_holds_every_entry(tol):
    """Every idx entry names point 5: its list has S K entries, every other list is empty, and dpoints is exactly 0 where no list names a
    point (with normalize = center the anchors' rows only get the cat's half)."""
    B, N, S, D, K = 2, 24, 6, 8, 4
    xyz, points, fps, idx, alpha, beta, dout = _inputs(B, N, S, D, K, "center", True, seed=11)
    idx[:] = 5
    for mode in ("center", "anchor", None):
        ref, bars = GR.spot_bars(xyz, points, fps, idx, alpha, beta, dout, mode, True, tol)
        got = _run(xyz, points, fps, idx, alpha, beta, dout, mode, True)
        named = np.zeros((B, N), bool)
        named[:, 5] = True
        np.put_along_axis(named, fps.astype(np.int64), True, axis=1)
        assert named.sum() == B * (S + 1) - (fps == 5).sum()
        assert (got["dpoints"][~named].view(np.int32) == 0).all()
        for q in ref:
            if mode == "center" and q in ("out", "dpoints", "dalpha"):
                continue                                   # d = 0 everywhere: s_b = 0, covered by test_coinciding_points_...
            assert GR.dist(got[q], ref[q]) <= bars[q], (mode, q)


def test_duplicate_anchors_and_out_of_range_indices(tol):
    B, N, S, D, K = 2, 20, 6, 8, 3
    xyz, points, fps, idx, alpha, beta, dout = _inputs(B, N, S, D, K, "anchor", True, seed=12)
    fps[0, 3] = fps[0, 1]
    fps[1, :] = 7                                        # FPS on a cloud of repeated points returns duplicates
    idx[:, :, 0] = fps
    for mode in ("anchor", "center"):
        ref, bars = GR.spot_bars(xyz, points, fps, idx, alpha, beta, dout, mode, True, tol)
        got = _run(xyz, points, fps, idx, alpha, beta, dout, mode, True)
        for q in ref:
            assert GR.dist(got[q], ref[q]) <= bars[q], (mode, q)
    # out of range: idx counts as the anchor, fps as point s; never dereferenced
    bad_idx, bad_fps = idx.copy(), fps.copy()
    for (b, s, k), v in {(0, 2, 1): -1, (1, 5, 0): N, (0, 0, 2): 2 ** 31 - 1, (1, 4, 2): -2 ** 31}.items():
        bad_idx[b, s, k] = v
    bad_fps[0, 4], bad_fps[1, 2] = N + 3, -5
    sfps, sidx = (a.astype(np.int32) for a in GR.sanitize(bad_fps, bad_idx, N))
    assert sfps[0, 4] == 4 and sfps[1, 2] == 2 and sidx[0, 2, 1] == sfps[0, 2] and (sidx != bad_idx).sum() == 4
    a, b = _run(xyz, points, bad_fps, bad_idx, alpha, beta, dout, "anchor", True), _run(xyz, points, sfps, sidx, alpha, beta, dout, "anchor", True)
    for q in a:
        assert _same_bits(a[q], b[q]), q
    ref, bars = GR.spot_bars(xyz, points, sfps, sidx, alpha, beta, dout, "anchor", True, tol)
    for q in ref:
        assert GR.dist(a[q], ref[q]) <= bars[q], q


def test_coinciding_points_give_zero_std_and_finite_results():
    """Batch element 1's points coincide: s_b = 0 there, out = beta in the normalised channels and every gradient is finite (the variance
    term is taken as 0, where the reference's gradient is NaN); batch element 0 is an ordinary cloud."""
    B, N, S, D, K = 2, 16, 8, 8, 4
    for mode in ("center", "anchor"):
        xyz, points, fps, idx, alpha, beta, dout = _inputs(B, N, S, D, K, mode, True, seed=13)
        xyz[1], points[1] = 0.25, 0.75
        got = _run(xyz, points, fps, idx, alpha, beta, dout, mode, True)
        assert (got["stats"][1] == np.array([0, 0, 1e5, 0], np.float32)).all() and got["stats"][0, 1] > 0.1
        assert np.array_equal(got["out"][1, :, :, :D + 3], np.broadcast_to(beta, (S, K, D + 3)))
        assert np.array_equal(got["out"][1, :, :, D + 3:], np.full((S, K, D), 0.75, np.float32))
        for q in ("out", "dpoints", "dalpha", "dbeta"):
            assert np.isfinite(got[q]).all(), (mode, q)
        # the closed form with the variance term dropped where s_b == 0
        want = GR.backward_f64(xyz, points, fps, idx, alpha, beta, dout, mode, True)
        for q, w in zip(("dpoints", "dalpha", "dbeta"), want):
            assert np.isfinite(w).all() and np.abs(got[q] - w).max() <= 1e-5 * max(1.0, np.abs(w).max()), (mode, q)


def test_two_calls_give_the_same_bits():
    args = _inputs(3, 200, 100, 68, 7, "center", True, seed=14)
    args[3][:, :, 1] = 9                                            # a long list
    a, b = _run(*args, "center", True, True, True), _run(*args, "center", True, True, True)
    for q in a:
        assert _same_bits(a[q], b[q]), q


def test_graph_capture_replays_to_the_eager_bits():
    from unipre3d_amd import local_grouper as lg
    B, N, S, D, K = 2, 256, 128, 64, 16
    xyz, points, fps, idx, alpha, beta, dout = _inputs(B, N, S, D, K, "anchor", True, seed=15)
    xyz_t, fps_t, idx_t = _dev(xyz), _dev(fps), _dev(idx)
    a, b = _dev(alpha).requires_grad_(True), _dev(beta).requires_grad_(True)
    sp = _dev(points).permute(0, 2, 1).contiguous().requires_grad_(True)          # (B, D, N), as the callers hold it
    sd = _dout(dout, True)
    run = lambda p, d: torch.autograd.grad(lg.local_group(xyz_t, p.permute(0, 2, 1), fps_t, idx_t, a, b, "anchor", True)[1], (p, a, b), d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sp, sd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_out = lg.local_group(xyz_t, sp.permute(0, 2, 1), fps_t, idx_t, a, b, "anchor", True)[1]
        c_grads = torch.autograd.grad(c_out, (sp, a, b), sd)
    g = torch.Generator().manual_seed(4)
    nx, nd = torch.randn(B, D, N, generator=g).cuda(), torch.randn(sd.shape, generator=g).cuda()
    with torch.no_grad():
        sp.copy_(nx)
        sd.copy_(nd)
    graph.replay()
    torch.cuda.synchronize()
    ex = nx.clone().requires_grad_(True)
    e_out = lg.local_group(xyz_t, ex.permute(0, 2, 1), fps_t, idx_t, a, b, "anchor", True)[1]
    e_grads = torch.autograd.grad(e_out, (ex, a, b), sd)
    assert torch.equal(c_out.detach().contiguous().view(torch.int32), e_out.detach().contiguous().view(torch.int32))
    for c, e in zip(c_grads, e_grads):
        assert torch.equal(c.view(torch.int32), e.view(torch.int32)) and torch.isfinite(c).all()


def test_autograd_node_keeps_nothing_of_the_outputs_size():
    from unipre3d_amd import local_grouper as lg
    B, N, S, D, K = 2, 64, 32, 16, 8
    xyz, points, fps, idx, alpha, beta, _ = _inputs(B, N, S, D, K, "center", True, seed=16)
    p = _dev(points).requires_grad_(True)
    out = lg._LocalGroup.apply(_dev(xyz), p, _dev(alpha), _dev(beta), _dev(fps), _dev(idx), 1, True, 1e-5, True)[0]
    saved = out.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [(B, N, 3), (B, N, D), (D + 3,), (B, S, D + 3), (B, 4)]
    assert saved[1].data_ptr() == p.data_ptr() and all(t.numel() * K <= out.numel() for t in saved)


def test_device_argument_checks():
    from unipre3d_amd import local_grouper as lg
    xyz, pts = torch.zeros(1, 16, 3, device="cuda"), torch.zeros(1, 16, 8, device="cuda")
    fps, idx = torch.zeros(1, 8, dtype=torch.int64, device="cuda"), torch.zeros(1, 8, 4, dtype=torch.int64, device="cuda")
    a, b = torch.ones(1, 1, 1, 11, device="cuda"), torch.zeros(1, 1, 1, 11, device="cuda")
    new_xyz, out = lg.local_group(xyz, pts, fps, idx, a, b, "center", True)                     # int64 indices, [1, 1, 1, D + A] parameters
    assert new_xyz.shape == (1, 8, 3) and out.shape == (1, 8, 4, 19)
    assert lg.local_group(xyz, pts, fps, idx, None, None, None, False)[1].shape == (1, 8, 4, 16)
    # any other stride pattern is made contiguous first
    wide = torch.arange(16 * 16, dtype=torch.float32, device="cuda").view(1, 16, 16)
    assert torch.equal(lg.local_group(xyz, wide[:, :, :8], fps, idx, a, b, None, True)[1],
                       lg.local_group(xyz, wide[:, :, :8].contiguous(), fps, idx, a, b, None, True)[1])
    with pytest.raises(NotImplementedError, match="xyz.requires_grad"):
        lg.local_group(xyz.clone().requires_grad_(True), pts, fps, idx, a, b, "center", True)
    with pytest.raises(RuntimeError):
        lg.local_group(xyz.cpu(), pts, fps, idx, a, b, "center", True)
    with pytest.raises(NotImplementedError, match="dtype"):
        lg.local_group(xyz, pts.double(), fps, idx, a, b, "center", True)
    for shape_idx in (torch.zeros(1, 8, 1, dtype=torch.int32, device="cuda"), torch.zeros(1, 8, 65, dtype=torch.int32, device="cuda")):
        with pytest.raises(NotImplementedError, match="K="):
            lg.local_group(xyz, pts, fps, shape_idx, a, b, "center", True)
    with pytest.raises(NotImplementedError, match="D="):
        lg.local_group(xyz, torch.zeros(1, 16, 6, device="cuda"), fps, idx, torch.ones(9, device="cuda"), torch.zeros(9, device="cuda"), "center", True)
    with pytest.raises(NotImplementedError, match="N="):
        lg.local_group(xyz, pts, torch.zeros(1, 17, dtype=torch.int32, device="cuda"), torch.zeros(1, 17, 4, dtype=torch.int32, device="cuda"),
                       a, b, "center", True)
    with pytest.raises(NotImplementedError, match="N="):
        lg.local_group(torch.zeros(1, 16385, 3, device="cuda"), torch.zeros(1, 16385, 8, device="cuda"), fps, idx, a, b, "center", True)
