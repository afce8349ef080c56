"""unipre3d_amd.metrics on the MI355X: the golden cases of tests/golden/g18_metrics.npz (what the reference's own `ssim` and PSNR line
returned on the CPU), every tile class of the kernels against the fp64 restatement of tests/metrics_ref.py, the gradient, the exact
outputs (valid flag, +inf), NaN isolation, determinism, HIP-graph capture, the aggregation and the argument errors.

Tolerances (profiles/metrics/tolerance.json, tests/metrics_ref.py `bars`): bar = 2 x yardstick + floor, the yardstick being the
reference's own fp32 result against its fp64 record and the floor the fp32 restatement's largest distance from that record on the CPU.
Shapes without a recorded case are held to the largest bar of the non-degenerate golden cases.  Every figure is printed before it is
asserted (`pytest -s` shows them).  The fp64 analytic gradient these tests compare with is itself pinned by finite differences on the
CPU (tests/test_metrics_ref.py)."""
import numpy as np
import pytest
import torch

import metrics_ref as MR

pytestmark = pytest.mark.gpu

CASES = ("noise", "smooth", "render", "identical", "constant_constant", "constant_zero", "one_channel", "small", "pixel")
T = 32                                                        # unipre3d_amd.metrics.TILE (asserted below)
_EDGES = (1, 5, 10, 11, T - 1, T, T + 1, 2 * T + 3)
# every value on each axis once (the widths are the heights rotated by three); N in {1, 5} and C in {1, 3} in every combination
TILE_CLASSES = [(n, c, h, w) for (h, w), (n, c) in zip(zip(_EDGES, _EDGES[3:] + _EDGES[:3]), [(1, 1), (5, 3), (1, 3), (5, 1)] * 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from unipre3d_amd import metrics
    assert metrics.TILE == T and metrics.HALO == 5
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def general_bars(golden):
    """The largest bar of the non-degenerate golden cases, per quantity."""
    z = golden("g18_metrics.npz")
    per_case = [MR.bars(c, z) for c in CASES if c not in MR.DEGENERATE]
    return {k: max(b[k] for b in per_case) for k in ("ssim", "psnr", "grad")}


def _pair(shape, seed):
    """Half the images noise against noise, the others a smooth image against itself plus noise."""
    rng = np.random.default_rng(seed)
    n, c, h, w = shape
    a, b = rng.uniform(0, 1, shape), rng.uniform(0, 1, shape)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    for i in range(1, n, 2):
        a[i] = 0.5 + 0.4 * np.sin(5 * x + i) * np.cos(3 * y - i)
        b[i] = np.clip(a[i] + rng.normal(0, 0.05, (c, h, w)), 0, 1)
    return a.astype(np.float32), b.astype(np.float32)


@pytest.fixture(scope="module")
def tile_refs():
    """{shape: (img1, img2, ssim64 (N,), psnr64 (N,), unit gradient64 (N,C,H,W))}, computed once and left unchanged."""
    out = {}
    for k, shape in enumerate(TILE_CLASSES):
        a, b = _pair(shape, 100 + k)
        out[shape] = (a, b, MR.ssim_f64(a, b), MR.psnr(a, b), MR.ssim_grad(a, b))
    return out


def _np(t):
    return t.detach().cpu().numpy()


def _check(what, got, bar):
    print(f"[metrics] {what}: {got:.3e} (bar {bar:.3e})")
    assert got <= bar, (what, got, bar)


@pytest.mark.parametrize("case", CASES)
def test_golden_cases(golden, dev, case):
    from unipre3d_amd import metrics
    z = golden("g18_metrics.npz")
    bar = MR.bars(case, z)
    a = torch.from_numpy(z[f"{case}_img1"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(z[f"{case}_img2"]).to(dev)
    per_image = metrics.ssim(a, b, size_average=False)
    per_image.sum().backward()
    assert per_image.shape == (a.size(0),) and a.grad.shape == a.shape
    p = metrics.psnr(a.detach(), b)
    d = MR.distances(case, _np(per_image), _np(p), _np(a.grad), z)
    for k in ("ssim", "psnr", "grad"):
        _check(f"golden {case} {k}", d[k], bar[k])
    if case in MR.DEGENERATE:                                 # true SSIM 1, true gradient 0, PSNR +inf
        _check(f"golden {case} |ssim - 1|", float(np.abs(_np(per_image).astype(np.float64) - 1).max()), bar["ssim"])
        assert torch.isposinf(p).all()
    mean = metrics.ssim(a.detach(), b)
    assert mean.dim() == 0
    _check(f"golden {case} mean ssim", abs(float(mean) - float(z[f"{case}_ssim64"].mean())), bar["ssim"])
    m = metrics.image_metrics(a.detach(), b)
    assert torch.equal(m["ssim"], per_image.detach()) and torch.equal(m["psnr"], p)
    assert m["valid"].dtype == torch.bool and m["valid"].tolist() == (~MR.all_zero(z[f"{case}_img2"])).tolist()
    if a.size(0) == 1:                                        # (C,H,W) is one image
        assert torch.equal(metrics.ssim(a.detach()[0], b[0]), mean) and torch.equal(metrics.psnr(a.detach()[0], b[0]), p)


@pytest.mark.parametrize("shape", TILE_CLASSES, ids=lambda s: "x".join(map(str, s)))
def test_tile_classes_forward(dev, tile_refs, general_bars, shape):
    from unipre3d_amd import metrics
    a, b, s64, p64, _ = tile_refs[shape]
    m = metrics.image_metrics(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    _check(f"tile {shape} ssim", float(np.abs(_np(m["ssim"]) - s64).max()), general_bars["ssim"])
    _check(f"tile {shape} psnr", float(np.abs(_np(m["psnr"]) - p64).max()), general_bars["psnr"])
    assert m["valid"].all()


@pytest.mark.parametrize("shape", TILE_CLASSES, ids=lambda s: "x".join(map(str, s)))
def test_tile_classes_gradient(dev, tile_refs, general_bars, shape):
    """`ssim(...).backward()` (every image weighs 1 / N) and size_average=False with a non-uniform grad_output of shape (N,)."""
    from unipre3d_amd import metrics
    a, b, _, _, g64 = tile_refs[shape]
    n = shape[0]
    b_d = torch.from_numpy(b).to(dev)
    x = torch.from_numpy(a).to(dev).requires_grad_(True)
    metrics.ssim(x, b_d).backward()
    _check(f"tile {shape} grad of the mean", MR.rel_l2(_np(x.grad), g64 / n), general_bars["grad"])
    w = np.linspace(-1.5, 2.0, n) if n > 1 else np.array([0.625])
    x = torch.from_numpy(a).to(dev).requires_grad_(True)
    metrics.ssim(x, b_d, size_average=False).backward(torch.from_numpy(w.astype(np.float32)).to(dev))
    _check(f"tile {shape} grad, weighted", MR.rel_l2(_np(x.grad), w.astype(np.float32).astype(np.float64).reshape(-1, 1, 1, 1) * g64),
           general_bars["grad"])


@pytest.mark.parametrize("shape", [(4, 3, 128, 128), (2, 3, 120, 160)], ids=lambda s: "x".join(map(str, s)))
def test_full_shapes(dev, general_bars, shape):
    from unipre3d_amd import metrics
    a, b = _pair(shape, 7)
    m = metrics.image_metrics(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    _check(f"full {shape} ssim", float(np.abs(_np(m["ssim"]) - MR.ssim_f64(a, b)).max()), general_bars["ssim"])
    _check(f"full {shape} psnr", float(np.abs(_np(m["psnr"]) - MR.psnr(a, b)).max()), general_bars["psnr"])


def test_exact_outputs(dev):
    from unipre3d_amd import metrics
    h, w = 2 * T + 3, T + 1                                   # the last tile is one pixel wide and three high
    g = torch.Generator().manual_seed(2)
    a = torch.rand(4, 3, h, w, generator=g).to(dev)
    a[1] = a[0]
    b = torch.zeros(4, 3, h, w, device=dev)
    b[1] = -0.0
    b[2, 2, h - 1, w - 1] = 1e-20                             # the last pixel of the last tile
    b[3] = a[3]
    m = metrics.image_metrics(a, b)
    assert m["valid"].tolist() == [False, False, True, True]
    assert torch.isposinf(m["psnr"][3]) and torch.isfinite(m["psnr"][:3]).all()
    assert torch.isposinf(metrics.psnr(a[3], a[3])).all()
    assert torch.equal(m["ssim"][0], m["ssim"][1])            # -0.0 and 0.0 are the same target


def test_nan_stays_in_its_image(dev):
    from unipre3d_amd import metrics
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(5, 3, T + 1, 2 * T + 3, generator=g).to(dev), torch.rand(5, 3, T + 1, 2 * T + 3, generator=g).to(dev)
    clean = metrics.image_metrics(a, b)
    x = a.clone().requires_grad_(True)
    metrics.ssim(x, b).backward()
    a2 = a.clone()
    a2[2, 1, T, T] = float("nan")
    dirty = metrics.image_metrics(a2, b)
    x2 = a2.clone().requires_grad_(True)
    metrics.ssim(x2, b).backward()
    keep = [0, 1, 3, 4]
    for k in ("psnr", "ssim", "valid"):
        assert torch.equal(dirty[k][keep], clean[k][keep]), k
    assert torch.isnan(dirty["psnr"][2]) and torch.isnan(dirty["ssim"][2]) and bool(dirty["valid"][2])
    assert torch.equal(x2.grad[keep], x.grad[keep]) and torch.isnan(x2.grad[2]).any()
    b2 = b.clone()
    b2[2, 0, 0, 0] = float("nan")                             # a NaN target is not "all zero"
    assert metrics.image_metrics(a, b2)["valid"].all()


def test_deterministic(dev):
    from unipre3d_amd import metrics
    g = torch.Generator().manual_seed(5)
    a, b = torch.rand(5, 3, 2 * T + 3, T + 1, generator=g).to(dev), torch.rand(5, 3, 2 * T + 3, T + 1, generator=g).to(dev)
    w = torch.linspace(-1, 2, 5, device=dev)
    runs = []
    for _ in range(2):
        x = a.clone().requires_grad_(True)
        s = metrics.ssim(x, b, size_average=False)
        s.backward(w)
        runs.append((s.detach(), x.grad, metrics.psnr(a, b)))
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_graph_capture(dev):
    from unipre3d_amd import metrics
    g = torch.Generator().manual_seed(6)
    shape = (3, 3, T + 1, 2 * T + 3)
    sa, sb = torch.rand(shape, generator=g).to(dev), torch.rand(shape, generator=g).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.image_metrics(sa, sb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = metrics.image_metrics(sa, sb)
    a, b = torch.rand(shape, generator=g).to(dev), torch.rand(shape, generator=g).to(dev)
    b[1] = 0
    sa.copy_(a)
    sb.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    eager = metrics.image_metrics(a, b)
    for k in ("psnr", "ssim", "valid"):
        assert torch.equal(captured[k], eager[k]), k
    assert eager["valid"].tolist() == [True, False, True]


def test_evaluate_views(dev):
    """Three examples of five views, two of them conditioning; an all-zero target among the cond views and one among the novel views."""
    from unipre3d_amd import metrics
    g = torch.Generator().manual_seed(8)
    a, b = torch.rand(15, 3, 20, 24, generator=g).to(dev), torch.rand(15, 3, 20, 24, generator=g).to(dev)
    b[1] = 0                                                  # example 0, cond view 1
    b[5 + 3] = 0                                              # example 1, novel view 3
    m = metrics.image_metrics(a, b)
    assert m["valid"].sum().item() == 13
    want = MR.evaluate_views_lists(m["psnr"].tolist(), m["ssim"].tolist(), m["valid"].tolist(), 5, 2)
    got = metrics.evaluate_views(a, b, 5, 2)
    assert sorted(got) == ["PSNR_cond", "PSNR_novel", "SSIM_cond", "SSIM_novel"]
    for k, v in got.items():
        assert v.dim() == 0 and v.device.type == "cuda"
        assert abs(v.item() - want[k]) <= 4e-6 * abs(want[k]), (k, v.item(), want[k])     # fp32 means of a few fp32 values
    b[0] = 0                                                  # example 0 has no valid cond view: left out of the cond means
    m = metrics.image_metrics(a, b)
    want = MR.evaluate_views_lists(m["psnr"].tolist(), m["ssim"].tolist(), m["valid"].tolist(), 5, 2)
    got = metrics.evaluate_views(a, b, 5, 2)
    for k, v in got.items():
        assert abs(v.item() - want[k]) <= 4e-6 * abs(want[k]), (k, v.item(), want[k])
    assert all(torch.isnan(v) for v in metrics.evaluate_views(a, torch.zeros_like(b), 5, 2).values())


def test_casts_and_views(dev):
    """Other float dtypes and strided views are cast or copied, never reinterpreted."""
    from unipre3d_amd import metrics
    g = torch.Generator().manual_seed(9)
    a, b = torch.rand(2, 3, 12, 40, generator=g).to(dev), torch.rand(2, 3, 12, 40, generator=g).to(dev)
    want = metrics.image_metrics(a[..., ::2].contiguous(), b[..., ::2].contiguous())
    got = metrics.image_metrics(a[..., ::2], b.double()[..., ::2])
    assert torch.equal(got["ssim"], want["ssim"]) and torch.equal(got["psnr"], want["psnr"])
    x = a.double().requires_grad_(True)
    metrics.ssim(x, b).backward()
    y = a.clone().requires_grad_(True)
    metrics.ssim(y, b).backward()
    assert x.grad.dtype == torch.float64 and torch.equal(x.grad.float(), y.grad)
    with torch.no_grad():
        s = metrics.ssim(y, b, size_average=False)            # no gradient asked for: nothing is saved
    assert not s.requires_grad and torch.equal(s, metrics.ssim(a, b, size_average=False))


def test_errors(dev):
    from unipre3d_amd import metrics
    a = torch.rand(2, 3, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.ssim(a.cpu(), a.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.image_metrics(a, a.cpu())
    with pytest.raises(NotImplementedError):
        metrics.ssim(a, a, window_size=7)
    with pytest.raises(NotImplementedError):
        metrics.ssim(a, a.clone().requires_grad_(True))
    for fn in (metrics.ssim, metrics.psnr, metrics.image_metrics):
        with pytest.raises(ValueError):
            fn(a, a[:, :, :7])
        with pytest.raises(ValueError):
            fn(a[0, 0], a[0, 0])
    with pytest.raises(ValueError):
        metrics.evaluate_views(a, a, 3, 1)
