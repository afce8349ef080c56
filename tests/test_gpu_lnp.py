"""unipre3d_amd/lnp.py on the device: the golden record of the reference's own K_Norm + K_Pool and LNPBlock (tests/golden/g20_lnp.npz),
every dispatch class of the kernels against the fp64 restatement, the hub graph and out-of-range indices, a std of zero, reproducibility,
graph capture, the strided view and the memory kept.

The rule (profiles/lnp/tolerance.json, tests/lnp_ref.py): bar = 2 x yardstick + floor per quantity, in max|x - fp64| / max|fp64|; the
yardstick is the reference's own fp32 error against fp64 (recorded for the golden cases, computed on the spot on the CPU elsewhere), the
floor the CPU-measured distance of the fp32 restatement in the kernels' order.

Dispatch classes (csrc/u3d_lnp.hip), one case on each side of every boundary, as (B, G, C, K):
  a lane's second float4 group     C = 256 (64 groups, one per lane) | C = 260                  (1, 8, 256, 3)    | (1, 7, 260, 3)
  four rows per workgroup          B G = 8 (full workgroups) | 7 (a workgroup with one idle wave)     the same two
  at most 256 partials of mu, s    B G = 1024 (256 workgroups, one pass) | 1028 (a second pass)       (1, 1024, 4, 2)   | (2, 514, 4, 2)
  at most 512 partials of t, dalpha, dbeta; a thread of the dx kernel sums one or two of them
                                   B G = 4096 (512 workgroups of 8 rows) | 4104 (a second pass)       (4, 1024, 4, 2)   | (8, 513, 4, 2)
  parameter-reduce workgroups      C = 16 (one workgroup of 16 float4 columns) | C = 20 (two)         (1, 256, 16, 2)   | (1, 257, 20, 2)
  lists per thread of the neighbours kernel   G = 256 (one) | G = 257 (two for thread 0)              the same two
  the largest C and K              (1, 33, 512, 32)"""
import numpy as np
import pytest
import torch

import lnp_ref as LR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1024, 4, 2), (1, 7, 260, 3), (1, 33, 512, 32), (1, 8, 256, 3), (2, 514, 4, 2), (4, 1024, 4, 2), (8, 513, 4, 2),
          (1, 256, 16, 2), (1, 257, 20, 2)]
BLOCK_KEYS = ("lga.affine_alpha_feat", "lga.affine_beta_feat", "mlp.share_mlp.weight", "mlp.share_mlp.bias", "pre_norm_ft.weight",
              "pre_norm_ft.bias")


@pytest.fixture(scope="module")
def golden():
    return np.load(LR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def tol():
    return LR.tolerance()


def _run(x, idx, alpha, beta, dout, view=False):
    """{quantity: host array} of the wrapper, plus lse and stats.  view=True passes x as the [:, 1:, :] view of a (B, G+1, C) tensor."""
    from unipre3d_amd import lnp
    nb = lnp.neighbours_from_idx(torch.from_numpy(np.ascontiguousarray(idx)).cuda())
    xt = torch.from_numpy(x).cuda()
    if view:
        xt = torch.cat((torch.full_like(xt[:, :1], 7.0), xt), dim=1)
    xt.requires_grad_(True)
    a, b = torch.from_numpy(alpha).cuda().requires_grad_(True), torch.from_numpy(beta).cuda().requires_grad_(True)
    out = lnp.local_norm_pool(xt[:, 1:, :] if view else xt, nb, a, b)
    saved = out.grad_fn.saved_tensors
    out.backward(torch.from_numpy(dout).cuda())
    torch.cuda.synchronize()
    dx = xt.grad[:, 1:, :] if view else xt.grad
    if view:
        assert not xt.grad[:, 0].any()
    return {"out": out.detach().cpu().numpy(), "dx": dx.cpu().numpy(), "dalpha": a.grad.cpu().numpy(), "dbeta": b.grad.cpu().numpy(),
            "lse": saved[4].cpu().numpy(), "stats": saved[5].cpu().numpy()}


def _inputs(B, G, C, K, seed):
    rng = np.random.default_rng(seed)
    x, dout = rng.uniform(-1, 1, (B, G, C)).astype(np.float32), rng.uniform(-1, 1, (B, G, 2 * C)).astype(np.float32)
    alpha = (rng.uniform(0.5, 1.5, 2 * C) * rng.choice([-1.0, 1.0], 2 * C)).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, 2 * C).astype(np.float32)
    idx = rng.integers(0, G, (B, G, K)).astype(np.int32)
    idx[:, :, 0] = np.arange(G)
    return x, idx, alpha, beta, dout


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("case", LR.CASES)
def test_golden_cases(golden, tol, case):
    x, idx, alpha, beta, dout, cols = LR.golden_case(golden, case)
    got = _run(x, idx, alpha, beta, dout)
    assert got["out"].shape == dout.shape and got["dx"].shape == x.shape and got["dalpha"].shape == got["dbeta"].shape == alpha.shape
    assert all(got[q].dtype == np.float32 and np.isfinite(got[q]).all() for q in LR.QUANTITIES)
    cut, bars = LR.recorded(got, cols), LR.case_bars(case, tol)
    d = {q: LR.dist(cut[q], golden[f"{case}_{q}64"]) for q in LR.QUANTITIES}
    print(f"\nlnp golden {case}: " + "  ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in LR.QUANTITIES))
    for q in LR.QUANTITIES:
        assert d[q] <= bars[q], q
    _, lse64, mu64, s64 = LR.forward_f64(x, idx, alpha, beta)
    assert np.abs(got["lse"] - lse64).max() <= 8 * 2.0 ** -23 * max(1.0, np.abs(lse64).max())
    mu, s, r, c0 = got["stats"]
    assert abs(s - s64) <= 2.0 ** -23 * s64 and abs(mu - mu64) <= 2.0 ** -23 * s64 and r == pytest.approx(1.0 / (float(s) + 1e-5), rel=2.0 ** -22)


@pytest.mark.parametrize("given", [True, False], ids=["neighbours_given", "neighbours_none"])
def test_block_against_the_whole_block_record(golden, tol, given):
    """y and every gradient of LNPBlock within 2 x the reference block's own fp32 distance + the operator's floor (out's for y, the
    largest gradient floor for the gradients: the LayerNorm, the linear map and SiLU around the operator are torch's in both)."""
    from unipre3d_amd import lnp
    B, G, C, K = 2, 16, 8, 4
    blk = lnp.LNPBlock(lga_out_dim=2 * C, k_group_size=K, alpha=100, beta=1000, mlp_in_dim=2 * C, mlp_out_dim=C, num_group=G)
    blk.load_state_dict({k: torch.from_numpy(golden[f"block_w_{k}"]) for k in BLOCK_KEYS}, strict=True)
    blk = blk.cuda()
    center = torch.from_numpy(golden["tiny_center"]).cuda()
    feat = torch.from_numpy(golden["block_feat"]).cuda().requires_grad_(True)
    nb = lnp.neighbours(center, K) if given else None
    if given:
        assert np.array_equal(nb.idx.cpu().numpy(), golden["tiny_idx"])          # the device search selects the recorded neighbours
        ptr, ent = LR.inverse_lists(golden["tiny_idx"])
        assert np.array_equal(nb.ptr.cpu().numpy(), ptr) and np.array_equal(nb.ent.cpu().numpy(), ent)
    y = blk(center, feat, nb) if given else blk(center, feat)
    y.backward(torch.from_numpy(golden["block_dy"]).cuda())
    torch.cuda.synchronize()
    gfloor = max(tol["floors"][q] for q in ("dx", "dalpha", "dbeta"))
    checks = [("y", y.detach(), golden["block_y64"], golden["block_yard_y"], tol["floors"]["out"]),
              ("dfeat", feat.grad, golden["block_dfeat64"], golden["block_yard_dfeat"], gfloor)]
    checks += [(k, p.grad, golden[f"block_g64_{k}"], golden[f"block_yard_{k}"], gfloor) for k, p in blk.named_parameters()]
    assert {c[0] for c in checks[2:]} == set(BLOCK_KEYS)
    for name, got, want, yard, floor in checks:
        d = LR.dist(got.cpu().numpy().reshape(want.shape), want)
        print(f"\nlnp block {name}: {d:.3e} (bar {2 * float(yard) + floor:.3e})")
        assert d <= 2 * float(yard) + floor, name
    assert torch.equal(y[:, 0], feat[:, 0])


def test_strided_view_gives_the_bits_of_a_contiguous_copy(golden):
    x, idx, alpha, beta, dout, _ = LR.golden_case(golden, "k8")
    a, b = _run(x, idx, alpha, beta, dout), _run(x, idx, alpha, beta, dout, view=True)
    for q in LR.QUANTITIES + ("lse", "stats"):
        assert _same_bits(a[q], b[q]), q


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_dispatch_class(tol, shape):
    x, idx, alpha, beta, dout = _inputs(*shape, seed=sum(shape))
    ref, bars = LR.spot_bars(x, idx, alpha, beta, dout, tol)
    got = _run(x, idx, alpha, beta, dout)
    d = {q: LR.dist(got[q], ref[q]) for q in LR.QUANTITIES}
    print(f"\nlnp {shape}: " + "  ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in LR.QUANTITIES))
    for q in LR.QUANTITIES:
        assert np.isfinite(got[q]).all() and d[q] <= bars[q], q


def _hub(B=2, G=12, C=20, K=4):
    x, idx, alpha, beta, dout = _inputs(B, G, C, K, seed=99)
    idx[:, :, 0] = 3                       # row 3 is every row's neighbour (twice), rows 1, 2, 4 .. G - 2 are nobody's
    idx[:, :, 1:] = np.array(([3, 0, G - 1] * K)[:K - 1])
    return x, idx, alpha, beta, dout


def test_hub_graph(tol):
    from unipre3d_amd import lnp
    x, idx, alpha, beta, dout = _hub()
    nb = lnp.neighbours_from_idx(torch.from_numpy(idx).cuda())
    ptr, ent = LR.inverse_lists(idx)
    assert np.array_equal(nb.ptr.cpu().numpy(), ptr) and np.array_equal(nb.ent.cpu().numpy(), ent)
    assert ptr[0, 4] - ptr[0, 3] == 2 * 12 and ptr[0, 1] == ptr[0, 2] == ptr[0, 3]
    ref, bars = LR.spot_bars(x, idx, alpha, beta, dout, tol)
    got = _run(x, idx, alpha, beta, dout)
    for q in LR.QUANTITIES:
        assert LR.dist(got[q], ref[q]) <= bars[q], q


def test_out_of_range_index_counts_as_the_row_itself(tol):
    from unipre3d_amd import lnp
    x, idx, alpha, beta, dout = _inputs(2, 9, 12, 3, seed=5)
    bad = idx.copy()
    for (b, g, k), v in {(0, 2, 1): -1, (1, 5, 0): 9, (0, 0, 2): 2 ** 31 - 1, (1, 8, 2): -2 ** 31, (0, 4, 0): 1 << 20}.items():
        bad[b, g, k] = v
    fixed = LR.sanitize(bad).astype(np.int32)
    assert (fixed != bad).sum() == 5 and fixed[0, 2, 1] == 2 and fixed[1, 5, 0] == 5
    nb = lnp.neighbours_from_idx(torch.from_numpy(bad).cuda())
    ptr, ent = LR.inverse_lists(fixed)
    assert np.array_equal(nb.ptr.cpu().numpy(), ptr) and np.array_equal(nb.ent.cpu().numpy(), ent)
    a, b = _run(x, bad, alpha, beta, dout), _run(x, fixed, alpha, beta, dout)
    for q in LR.QUANTITIES + ("lse", "stats"):
        assert _same_bits(a[q], b[q]), q
    ref, bars = LR.spot_bars(x, fixed, alpha, beta, dout, tol)
    for q in LR.QUANTITIES:
        assert LR.dist(a[q], ref[q]) <= bars[q], q


def test_constant_rows_give_zero_std_and_finite_results():
    x, idx, alpha, beta, dout = _inputs(2, 10, 24, 4, seed=3)
    x[:] = 0.75
    got = _run(x, idx, alpha, beta, dout)
    assert got["stats"][0] == 0 and got["stats"][1] == 0 and got["stats"][3] == 0 and np.isfinite(got["stats"]).all()
    for q in LR.QUANTITIES + ("lse",):
        assert np.isfinite(got[q]).all(), q
    ref = LR.forward_f64(x, idx, alpha, beta)[0]
    assert LR.dist(got["out"], ref) <= 4 * 2.0 ** -23          # K equal values: the pooled value is beta, alpha x + beta above
    g64 = LR.backward_f64(x, idx, alpha, beta, dout)
    for q, want in zip(("dx", "dalpha", "dbeta"), g64):
        assert np.abs(got[q] - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), q


def test_two_runs_give_the_same_bits():
    x, idx, alpha, beta, dout = _hub(B=3, G=40, C=260, K=5)
    a, b = _run(x, idx, alpha, beta, dout), _run(x, idx, alpha, beta, dout)
    for q in LR.QUANTITIES + ("lse", "stats"):
        assert _same_bits(a[q], b[q]), q


def test_autograd_node_keeps_no_gathered_tensor():
    from unipre3d_amd import lnp
    x, idx, alpha, beta, _ = _inputs(2, 16, 24, 4, seed=8)
    nb = lnp.neighbours_from_idx(torch.from_numpy(idx).cuda())
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    out = lnp.local_norm_pool(xt, nb, torch.from_numpy(alpha).cuda(), torch.from_numpy(beta).cuda())
    saved = out.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [(2, 16, 24), (48,), (48,), (2, 16, 48), (2, 16, 24), (4,)]
    assert saved[0].data_ptr() == xt.data_ptr() and saved[3].data_ptr() == out.data_ptr()


def test_graph_capture_replays_to_the_eager_bits():
    from unipre3d_amd import lnp
    B, G, C, K = 3, 128, 384, 4
    x, idx, alpha, beta, dout = _inputs(B, G, C, K, seed=21)
    nb = lnp.neighbours_from_idx(torch.from_numpy(idx).cuda())
    a, b = torch.from_numpy(alpha).cuda().requires_grad_(True), torch.from_numpy(beta).cuda().requires_grad_(True)
    sx, sd = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(dout).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(lnp.local_norm_pool(sx, nb, a, b), (sx, a, b), sd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_out = lnp.local_norm_pool(sx, nb, a, b)
        c_grads = torch.autograd.grad(c_out, (sx, a, b), sd)
    g = torch.Generator().manual_seed(4)
    nx, nd = torch.randn(B, G, C, generator=g).cuda(), torch.randn(B, G, 2 * C, generator=g).cuda()
    with torch.no_grad():
        sx.copy_(nx)
        sd.copy_(nd)
    graph.replay()
    torch.cuda.synchronize()
    ex = nx.clone().requires_grad_(True)
    e_out = lnp.local_norm_pool(ex, nb, a, b)
    e_grads = torch.autograd.grad(e_out, (ex, a, b), nd)
    assert torch.equal(c_out.detach().view(torch.int32), e_out.detach().view(torch.int32))
    for c, e in zip(c_grads, e_grads):
        assert torch.equal(c.view(torch.int32), e.view(torch.int32)) and torch.isfinite(c).all()


def test_forward_and_backward_keep_less_than_one_gathered_tensor():
    from unipre3d_amd import lnp
    B, G, C, K = 32, 128, 384, 8
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, G, C, generator=g).cuda().requires_grad_(True)
    a, b = torch.ones(2 * C, device="cuda", requires_grad=True), torch.zeros(2 * C, device="cuda", requires_grad=True)
    dout = torch.randn(B, G, 2 * C, generator=g).cuda()
    nb = lnp.neighbours(torch.rand(B, G, 3, generator=g).cuda(), K)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = lnp.local_norm_pool(x, nb, a, b)
    grads = torch.autograd.grad(out, (x, a, b), dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"\nlnp peak above the starting level at {(B, G, C, K)}: {peak / 2 ** 20:.1f} MB; one (B, G, K, C) tensor: {B * G * K * C * 4 / 2 ** 20:.1f} MB")
    assert peak < B * G * K * C * 4
    assert all(torch.isfinite(t).all() for t in grads)


def test_device_argument_checks():
    from unipre3d_amd import lnp
    idx = torch.zeros(1, 8, 4, dtype=torch.int32, device="cuda")
    nb = lnp.neighbours_from_idx(idx)
    a16, b16 = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
    ok = torch.zeros(1, 8, 8, device="cuda")
    assert lnp.local_norm_pool(ok, nb, a16.view(1, 1, 1, 16), b16.view(1, 1, 1, 16)).shape == (1, 8, 16)
    assert lnp.neighbours_from_idx(idx.long()).idx.dtype == torch.int32
    with pytest.raises(RuntimeError):
        lnp.local_norm_pool(ok.cpu(), nb, a16, b16)
    with pytest.raises(ValueError, match="contiguous"):
        lnp.local_norm_pool(torch.zeros(1, 8, 16, device="cuda")[:, :, :8], nb, a16, b16)
    with pytest.raises(ValueError, match="built for"):
        lnp.local_norm_pool(torch.zeros(2, 8, 8, device="cuda"), nb, a16, b16)
    with pytest.raises(NotImplementedError, match="dtype"):
        lnp.local_norm_pool(ok.double(), nb, a16, b16)
    with pytest.raises(NotImplementedError, match="C="):
        lnp.local_norm_pool(torch.zeros(1, 8, 6, device="cuda"), nb, torch.ones(12, device="cuda"), torch.zeros(12, device="cuda"))
