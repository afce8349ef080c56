"""unipre3d_amd/image_fusion.py on the device: the reference's record (golden G25), every dispatch class of the kernels, the selection, the
loser rows, the dense path against the sparse one, reproducibility, graph capture, memory and the refusals.

The rule (profiles/image_fusion/tolerance.json, tests/image_fusion_ref.py): bar = 2 x floor per quantity, in max|x - fp64| / max|fp64|, the
floor being the CPU-measured distance of the fp32 restatement in the kernels' order from the fp64 record over the cases of G25.  A shape
without a recorded case is held to the fp64 restatement with bar = 2 x max(floor of the golden cases, floor of the shape).

Dispatch classes and the constants of csrc/u3d_image_fusion.hip they come from (CHUNK = 8192 floats of a group per workgroup, 256 threads
x float4 = 1024 floats a pass; 64 x 64 product tiles with 32 of the reduction per stage; row splits of the backward in multiples of 32):
  statistics  odd_group    105 floats a group (5 x 7, 3 channels): groups start off 16 bytes -> scalar head and tail; shorter than one pass
              split_group  8427 floats a group: two workgroups, the last one ragged (235 floats) and misaligned; B = 1
              dims (G25)   1024 floats a group, aligned: the float4 body alone
  rows        every shape  R is no multiple of 64 (46, 7, 3, 70, 18, 300, 80)
              odd_group    Cout = 6, Cin = 12: one ragged column tile, one ragged reduction stage
              ragged_tiles Cout = 70, Cin = 40: two column tiles and two stages, the last of each ragged
              dims (G25)   Cout = 384, Cin = 128: six column tiles, four full stages
              one_point    N = 1        all_win  every row a winner        none_win  none (zeros out, zero gradients)
              two_splits   300 rows: two row splits (160 + 140) in the backward, five row tiles in the forward"""
import numpy as np
import pytest
import torch

import image_fusion_ref as IR

pytestmark = pytest.mark.gpu


def _conv(inp, G):
    from unipre3d_amd.image_fusion import ImageConv
    Cout, Cin = inp["weight"].shape
    conv = ImageConv(Cin, Cout, num_groups=G, eps=IR.EPS).cuda()
    with torch.no_grad():
        for t, k in zip(conv.parameters(), ("gamma", "beta", "weight", "bias")):
            t.copy_(torch.from_numpy(inp[k]).reshape(t.shape))
    return conv


def _run(inp, cam, G, fx, fy, cx, cy, cot=None):
    """-> {out, sel, dW, dbias, dgamma, dbeta} as numpy, through sample_at_points and autograd"""
    from unipre3d_amd.image_fusion import sample_at_points
    conv = _conv(inp, G)
    out, sel = sample_at_points(conv, torch.from_numpy(inp["map"]).cuda(), torch.from_numpy(cam).cuda(), fx, fy, cx, cy)
    assert not sel.requires_grad and sel.dtype == torch.int32
    cot = inp["cot"] if cot is None else cot
    dgamma, dbeta, dW, dbias = torch.autograd.grad(out, list(conv.parameters()), torch.from_numpy(cot).cuda())
    torch.cuda.synchronize()
    return {"out": out.detach().cpu().numpy(), "sel": sel.cpu().numpy(), "dW": dW.cpu().numpy().reshape(inp["weight"].shape),
            "dbias": dbias.cpu().numpy(), "dgamma": dgamma.cpu().numpy(), "dbeta": dbeta.cpu().numpy()}


def _intr(g, tag):
    i = g[f"{tag}_intr"]
    return float(i[0][0]), float(i[1][1]), float(i[0][2]), float(i[1][2])


def _zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


@pytest.mark.parametrize("tag", list(IR.CASES))
def test_golden_cases(golden, tag):
    g, cfg, inp = golden("g25_image_fusion.npz"), IR.CASES[tag], IR.case_inputs(tag)
    assert np.array_equal(IR.checksum(inp), g[f"{tag}_checksum"])
    bars = IR.tolerance()["bars"]
    got = _run(inp, g[f"{tag}_cam"], cfg["G"], *_intr(g, tag))
    assert np.array_equal(got["sel"], g[f"{tag}_sel"])
    d = {q: IR.distance(got[q], g[f"{tag}_{q}_f64"]) for q in IR.QUANTITIES}
    print(f"[image_fusion] {tag}: " + ", ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in IR.QUANTITIES))
    for q in IR.QUANTITIES:
        assert d[q] <= bars[q], (tag, q, d[q], bars[q])
    assert _zero_bits(got["out"][got["sel"] < 0])
    if tag == "nowin":
        assert not got["out"][1].any()


@pytest.mark.parametrize("name", list(IR.EDGE_SHAPES))
def test_dispatch_classes(name):
    from unipre3d_amd import image_fusion
    B, N, Cin, G, Cout, H, W, _ = IR.EDGE_SHAPES[name]
    inp, cam, sel = IR.edge_inputs(name)
    lib = image_fusion.load()
    assert lib.u3d_imgfus_stats_chunks(Cin, G, H, W) == IR.stats_chunks(Cin, G, H, W) == (2 if name == "split_group" else 1)
    assert lib.u3d_imgfus_row_splits(B * N) == IR.row_splits(B * N) == (2 if name == "two_splits" else 1)
    rec = IR.tolerance()["edge_cases"][name]
    assert rec["shape_BNCinGCoutHW"] == [B, N, Cin, G, Cout, H, W] and rec["winners"] == int((sel >= 0).sum())
    got = _run(inp, cam, G, 1.0, 1.0, 0.0, 0.0)
    assert np.array_equal(got["sel"], sel)
    want = {"out": IR.forward(inp["map"], sel, inp, G), **IR.backward(inp["map"], sel, inp, G, inp["cot"])}
    d = {q: IR.distance(got[q], want[q]) for q in IR.QUANTITIES}
    print(f"[image_fusion] {name}: " + ", ".join(f"{q} {d[q]:.3e} (bar {rec['bars'][q]:.3e})" for q in IR.QUANTITIES))
    stats = image_fusion.group_stats(torch.from_numpy(inp["map"]).cuda(), G, IR.EPS).cpu().numpy()
    mean, rstd = IR.group_stats(inp["map"], G)
    assert np.array_equal(stats[..., 0], mean.astype(np.float32))             # f64 sums rounded once: the mean is the rounded f64 mean
    assert np.max(np.abs(stats[..., 1] / rstd - 1)) < 2.0 ** -22
    if name == "none_win":
        assert all(_zero_bits(got["out"]) and not got[q].any() for q in IR.QUANTITIES)
        return
    if name == "all_win":
        assert (sel >= 0).all()
    for q in IR.QUANTITIES:
        assert d[q] <= rec["bars"][q], (name, q, d[q], rec["bars"][q])
    assert _zero_bits(got["out"][sel < 0])


def test_selection_is_the_dense_paths(golden):
    """sel bit for bit that of fusion._ZBufferGather on the dense tensor, which is what the reference's module is pinned to"""
    from unipre3d_amd import fusion
    g, inp = golden("g25_image_fusion.npz"), IR.case_inputs("dims")
    got = _run(inp, g["dims_cam"], 32, *_intr(g, "dims"))
    with torch.no_grad():
        dense = _conv(inp, 32)(torch.from_numpy(inp["map"]).cuda())
        mapped, sel = fusion._ZBufferGather.apply(torch.from_numpy(g["dims_cam"]).cuda(), dense, *_intr(g, "dims"))
    assert np.array_equal(sel.cpu().numpy(), got["sel"])
    assert np.array_equal(mapped.cpu().numpy() != 0, got["out"] != 0)


def test_loser_rows_are_zero_and_their_cotangent_is_never_read(golden):
    g, inp = golden("g25_image_fusion.npz"), IR.case_inputs("sq")
    sel = g["sq_sel"]
    lose = sel < 0
    assert lose.any() and (~lose).any()
    clean, wild = inp["cot"].copy(), inp["cot"].copy()
    clean[lose] = 0.0
    wild[lose] = np.where(np.arange(wild.shape[2]) % 2 == 0, np.float32(3e38), np.float32(np.nan))[None]
    a = _run(inp, g["sq_cam"], 2, *_intr(g, "sq"), cot=clean)
    b = _run(inp, g["sq_cam"], 2, *_intr(g, "sq"), cot=wild)
    assert _zero_bits(a["out"][lose])                                        # +0.0, not -0.0
    for q in IR.QUANTITIES:
        assert np.isfinite(b[q]).all() and np.array_equal(a[q].view(np.uint32), b[q].view(np.uint32)), q


@pytest.mark.parametrize("cls", [False, True], ids=["plain", "cls"])
def test_dense_path_against_sparse_path(golden, cls):
    """ImageConv.forward + fusion.FeatureFusion (torch's fp32 dense path, what a user switches from) against ImageConv.deferred +
    image_fusion.FeatureFusion at the reference's channel counts: outputs and all four gradients.

    These are two fp32 evaluations and their errors add, so the bar is two-sided (profiles/image_fusion/tolerance.json,
    dense32_against_sparse_bars): the sparse bar + 2 x the dims case's yardstick, the dense path's own recorded distance from fp64.  The
    one-sided bars do not apply to this pair: measured on one MI355X, dbeta is 3.9e-07 (plain) and 4.6e-07 (cls) against the one-sided
    3.2e-07 and the two-sided 7.0e-07, while the sparse path is 1.4e-07 from the fp64 dense path.  The dense path evaluated in fp64
    (ImageConv.double()) is held to the one-sided bars next to it."""
    from unipre3d_amd import fusion, image_fusion
    g, inp = golden("g25_image_fusion.npz"), IR.case_inputs("dims")
    cfg = IR.CASES["dims"]
    B, N, Cout = cfg["B"], cfg["N"], cfg["Cout"]
    bars = IR.tolerance()["bars"]
    center, c2w = torch.from_numpy(g["dims_center"]).cuda(), torch.from_numpy(g["dims_c2w"]).cuda()
    x = torch.from_numpy(np.random.RandomState(5).randn(B, N + int(cls), 7).astype(np.float32)).cuda()
    w = torch.from_numpy(np.random.RandomState(6).randn(B, N + int(cls), 7 + Cout).astype(np.float32)).cuda()
    xmap = torch.from_numpy(inp["map"]).cuda()
    res = {}
    for mode in ("dense64", "dense32", "sparse"):
        conv = _conv(inp, cfg["G"])
        if mode == "sparse":
            feats = conv.deferred(xmap)
            assert feats.shape == (B, Cout, cfg["H"], cfg["W"]) and feats.device == xmap.device and feats.dtype == torch.float32
            y = image_fusion.FeatureFusion(torch.nn.Identity())(x, center, feats, c2w, g["dims_intr"])
            assert feats.stats() is feats.stats()                           # computed once, kept on the handle
            assert torch.equal(feats.materialize(), conv(xmap))
        elif mode == "dense64":
            conv = conv.double()
            y = fusion.FeatureFusion(torch.nn.Identity())(x, center, conv(xmap.double()), c2w, g["dims_intr"])
        else:
            y = fusion.FeatureFusion(torch.nn.Identity())(x, center, conv(xmap), c2w, g["dims_intr"])
        grads = torch.autograd.grad((y * w).sum(), list(conv.parameters()))
        res[mode] = [y.detach().cpu().numpy()[..., 7:]] + [t.cpu().numpy() for t in (grads[2], grads[3], grads[0], grads[1])]
        assert np.array_equal(y.detach().cpu().numpy()[..., :7], x.cpu().numpy())
    d = {q: IR.distance(s, dn) for q, dn, s in zip(IR.QUANTITIES, res["dense64"], res["sparse"])}
    d32 = {q: IR.distance(s, dn) for q, dn, s in zip(IR.QUANTITIES, res["dense32"], res["sparse"])}
    print(f"[image_fusion] dense fp64 vs sparse (cls={cls}): " + ", ".join(f"{q} {d[q]:.3e} (bar {bars[q]:.3e})" for q in IR.QUANTITIES))
    bars32 = IR.tolerance()["dense32_against_sparse_bars"]
    print(f"[image_fusion] dense fp32 vs sparse (cls={cls}): " + ", ".join(f"{q} {d32[q]:.3e} (bar {bars32[q]:.3e})" for q in IR.QUANTITIES))
    if cls:
        assert _zero_bits(res["sparse"][0][:, 0])
    assert np.array_equal(res["dense32"][0] != 0, res["sparse"][0] != 0)
    for q in IR.QUANTITIES:
        assert d32[q] <= bars32[q], ("dense fp32", q, d32[q], bars32[q])
        assert d[q] <= bars[q], ("dense fp64", q, d[q], bars[q])


def test_two_runs_are_bitwise_equal():
    inp, cam, _ = IR.edge_inputs("two_splits")
    a, b = _run(inp, cam, 4, 1.0, 1.0, 0.0, 0.0), _run(inp, cam, 4, 1.0, 1.0, 0.0, 0.0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_graph_capture_and_replay_equal_eager_bitwise():
    from unipre3d_amd.image_fusion import sample_at_points
    inp, cam, _ = IR.edge_inputs("two_splits")
    conv = _conv(inp, 4)
    xmap, cp, cot = (torch.from_numpy(a).cuda() for a in (inp["map"], cam, inp["cot"]))

    def step():
        out, sel = sample_at_points(conv, xmap, cp, 1.0, 1.0, 0.0, 0.0)
        return (out, sel) + torch.autograd.grad(out, list(conv.parameters()), cot)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    names = ("out", "sel", "dgamma", "dbeta", "dW", "dbias")
    for replay in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        differ = [f"{n} (replay {replay})" for n, a, b in zip(names, eager, captured) if not torch.equal(a, b)]
        assert not differ, differ


def test_no_image_sized_tensor_is_made():
    """(B = 2, Cin = 128, Cout = 384, 64 x 64, N = 128): forward + backward raise the peak by less than a quarter of one (B, Cout, H, W)
    fp32 tensor (12.6 MB); the path's own tensors (rows, out, winner table, partials, gradients) total about 1 MB."""
    from unipre3d_amd.image_fusion import ImageConv, sample_at_points
    import fusion_ref
    B, Cin, Cout, H, N = 2, 128, 384, 64, 128
    conv = ImageConv(Cin, Cout).cuda()
    xmap = torch.randn(B, Cin, H, H, device="cuda")
    cp = torch.from_numpy(fusion_ref.launch_scene(B, N, H, H, seed=1)[0]).cuda()
    cot = torch.randn(B, N, Cout, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, sel = sample_at_points(conv, xmap, cp, 1.0, 1.0, 0.0, 0.0)
    grads = torch.autograd.grad(out, list(conv.parameters()), cot)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    dense = B * Cout * H * H * 4
    print(f"[image_fusion] peak rise {rise} bytes against {dense} for one dense output")
    assert int((sel >= 0).sum()) > N and all(torch.isfinite(t).all() for t in grads)
    assert rise < dense // 4


def test_refusals_on_the_device():
    from unipre3d_amd import image_fusion as IF
    conv = IF.ImageConv(8, 6, num_groups=2).cuda()
    x = torch.randn(2, 8, 4, 4, device="cuda")
    cam = torch.ones(2, 3, 4, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        conv.deferred(x.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="contiguous"):
        IF.sample_at_points(conv, x.transpose(2, 3), cam, 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(NotImplementedError, match="frozen"):
        conv.deferred(x.clone().requires_grad_(True))
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError, match="fp32"):
            conv.deferred(x.to(dt))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.deferred(x.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IF.sample_at_points(conv, x, cam.cpu(), 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="one image"):
        IF.sample_at_points(conv, x, cam[:1], 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="one image"):
        IF.FeatureFusion(torch.nn.Identity())(torch.zeros(3, 3, 0, device="cuda"), torch.zeros(3, 3, 3, device="cuda"), conv.deferred(x),
                                              torch.eye(4, device="cuda").repeat(3, 1, 1), np.eye(3, 4))
    with pytest.raises(ValueError, match="fit"):
        IF.sample_at_points(IF.ImageConv(4, 6, num_groups=2).cuda(), x, cam, 1.0, 1.0, 0.0, 0.0)
    out, sel = IF.sample_at_points(conv, x, cam, 1.0, 1.0, 0.0, 0.0)         # and the call these refuse does run
    assert out.shape == (2, 3, 6) and sel.shape == (2, 3)
    off = torch.ones(2 * 3 * 4 + 1, device="cuda")[1:].view(2, 3, 4)          # camera points 4 bytes off a 16-byte boundary: copied
    assert off.data_ptr() % 16 == 4
    out2, sel2 = IF.sample_at_points(conv, x, off, 1.0, 1.0, 0.0, 0.0)
    assert torch.equal(out2, out) and torch.equal(sel2, sel)
    (g,) = torch.autograd.grad(out.sum(), [conv[1].bias], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):   # no double backward: it raises, no silent zeros
        torch.autograd.grad(g.sum(), [conv[1].weight])
