"""unipre3d_amd/mha.py on the device: the golden record of the reference's own Attention.forward (tests/golden/g19_dense_attention.npz),
every row-count class of the kernels, structured inputs that show a transposed or permuted operand, reproducibility and graph capture,
the Attention module against a reference-form module, and the argument checks.

The rule (profiles/mha/tolerance.json, tests/mha_ref.py): bar = 2 x yardstick + floor per quantity, in max|x - fp64| / max|fp64|; the
yardstick is the reference's own fp32 error against fp64 (recorded for the golden cases, computed on the spot on the CPU elsewhere), the
floor the CPU-measured distance of the fp32 restatement in the kernel's order.

Row-count classes: a wave owns 16 rows (15, 16, 17), a workgroup 64 queries and a staged block 64 keys (63, 64, 65; 127, 128, 129; 257:
five blocks), a key block is taken whole or with a masked tail, and N = 1023 / 1024 is the largest the library takes."""
import numpy as np
import pytest
import torch

import mha_ref as MR

pytestmark = pytest.mark.gpu

D = 64
SHAPES = ([(1, n, 1) for n in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)]
          + [(3, 17, 6), (3, 65, 1), (1, 129, 6), (3, 63, 6), (2, 129, 6), (1, 1023, 1), (1, 1024, 1)])


@pytest.fixture(scope="module")
def golden():
    return np.load(MR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def tol():
    return MR.tolerance()


def _lse_bar(lse64):
    """lse = m * scale + log(sum): the 64-term score chain, the product and the log each round at lse's size (16 eps of it covers them),
    and the N rounded terms of the sum add errors like sqrt(N) eps; eps = 2^-23."""
    eps = 2.0 ** -23
    return 16 * eps * max(1.0, float(np.abs(lse64).max())) + np.sqrt(lse64.shape[-1]) * eps


def _run(qkv_np, dout_np, scale=None):
    """(out, lse, dqkv) of the wrapper as host arrays."""
    from unipre3d_amd import mha
    q = torch.from_numpy(qkv_np).cuda().requires_grad_(True)
    out = mha.attention_qkvpacked(q, scale)
    lse = out.grad_fn.saved_tensors[2]
    out.backward(torch.from_numpy(dout_np).cuda())
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), lse.cpu().numpy(), q.grad.cpu().numpy()


@pytest.mark.parametrize("case", MR.CASES)
def test_golden_cases(golden, tol, case):
    qkv, dout = golden[f"{case}_qkv"], golden[f"{case}_dout"]
    out, lse, dqkv = _run(qkv, dout)
    assert out.shape == dout.shape and out.dtype == np.float32 and dqkv.shape == qkv.shape and dqkv.dtype == np.float32
    d_out, d_g = MR.dist(out, golden[f"{case}_out64"]), MR.dist(dqkv, golden[f"{case}_dqkv64"])
    bar_out, bar_g = MR.case_bars(case, tol)
    lse64 = MR.forward_f64(qkv)[1]
    d_lse = float(np.abs(lse - lse64).max())
    print(f"\nmha golden {case}: out {d_out:.3e} (bar {bar_out:.3e})  dqkv {d_g:.3e} (bar {bar_g:.3e})  lse abs {d_lse:.3e} (bar {_lse_bar(lse64):.3e})")
    assert d_out <= bar_out and d_g <= bar_g
    assert d_lse <= _lse_bar(lse64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_row_class(tol, shape):
    B, N, H = shape
    rng = np.random.default_rng(1000 * B + 10 * N + H)
    qkv = rng.uniform(-1, 1, (B, N, 3, H, D)).astype(np.float32)
    qkv[:, :, :2] *= 2.0                                  # probabilities well away from uniform
    dout = rng.uniform(-1, 1, (B, N, H, D)).astype(np.float32)
    o64, g64, bar_out, bar_g = MR.spot_bars(qkv, dout, tol=tol)
    out, lse, dqkv = _run(qkv, dout)
    d_out, d_g = MR.dist(out, o64), MR.dist(dqkv, g64)
    print(f"\nmha {shape}: out {d_out:.3e} (bar {bar_out:.3e})  dqkv {d_g:.3e} (bar {bar_g:.3e})")
    assert np.isfinite(out).all() and np.isfinite(dqkv).all() and np.isfinite(lse).all()
    assert d_out <= bar_out and d_g <= bar_g
    lse64 = MR.forward_f64(qkv)[1]
    assert np.abs(lse - lse64).max() <= _lse_bar(lse64)


def test_softmax_scale_argument(tol):
    rng = np.random.default_rng(7)
    qkv = rng.uniform(-1, 1, (2, 33, 3, 2, D)).astype(np.float32)
    dout = rng.uniform(-1, 1, (2, 33, 2, D)).astype(np.float32)
    o64, g64, bar_out, bar_g = MR.spot_bars(qkv, dout, scale=0.7, tol=tol)
    out, _, dqkv = _run(qkv, dout, 0.7)
    assert MR.dist(out, o64) <= bar_out and MR.dist(dqkv, g64) <= bar_g
    assert MR.dist(out, MR.forward_f64(qkv)[0]) > 100 * bar_out          # (and the default scale is another function)


def test_layout_one_key_per_query_is_exact():
    """Query n lies along channel axis n at magnitude 2048, key pi(n) is that axis' unit vector: the matching score is 256 and every
    other 0, exp of the difference underflows to exactly 0 in fp32, so out[n] is v[pi(n)] bit for bit.  v[n, d] = 64 n + d is asymmetric
    in (n, d): a transposed or permuted operand, or a permuted write, shows.  The two heads use different permutations."""
    from unipre3d_amd import mha
    N, H = 37, 2
    rng = np.random.default_rng(37)
    qkv = np.zeros((1, N, 3, H, D), np.float32)
    perms = [rng.permutation(N) for _ in range(H)]
    for h, pi in enumerate(perms):
        qkv[0, np.arange(N), 0, h, np.arange(N)] = 2048.0
        qkv[0, pi, 1, h, np.arange(N)] = 1.0
        qkv[0, :, 2, h] = 64.0 * np.arange(N)[:, None] + np.arange(D)[None, :] + 4096.0 * h
    ref = MR.reference_form(qkv)
    for h, pi in enumerate(perms):
        assert np.array_equal(ref[0, :, h], qkv[0, pi, 2, h])           # the reference's form is exact on this input
    out = mha.attention_qkvpacked(torch.from_numpy(qkv).cuda()).cpu().numpy()
    for h, pi in enumerate(perms):
        assert np.array_equal(out[0, :, h], qkv[0, pi, 2, h]), h


def test_layout_equal_keys_give_the_mean(tol):
    """All keys equal: every query's probabilities are uniform and out is the mean of v, whatever q is."""
    B, N, H = 2, 70, 2
    rng = np.random.default_rng(70)
    qkv = rng.uniform(-1, 1, (B, N, 3, H, D)).astype(np.float32)
    qkv[:, :, 1] = qkv[:, :1, 1]
    dout = rng.uniform(-1, 1, (B, N, H, D)).astype(np.float32)
    o64, g64, bar_out, bar_g = MR.spot_bars(qkv, dout, tol=tol)
    mean = qkv[:, :, 2].astype(np.float64).mean(1, keepdims=True)
    assert MR.dist(o64, np.broadcast_to(mean, o64.shape)) < 1e-12
    out, _, dqkv = _run(qkv, dout)
    assert MR.dist(out, o64) <= bar_out and MR.dist(dqkv, g64) <= bar_g


def test_two_calls_give_the_same_bits():
    from unipre3d_amd import mha
    g = torch.Generator().manual_seed(2)
    qkv_cpu, dout_cpu = torch.randn(3, 129, 3, 6, D, generator=g), torch.randn(3, 129, 6, D, generator=g)
    runs = []
    for _ in range(2):
        q = qkv_cpu.cuda().requires_grad_(True)
        out = mha.attention_qkvpacked(q)
        lse = out.grad_fn.saved_tensors[2]
        out.backward(dout_cpu.cuda())
        runs.append((out.detach().cpu(), lse.cpu(), q.grad.cpu()))
    for a, b, name in zip(runs[0], runs[1], ("out", "lse", "dqkv")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def test_autograd_node_keeps_qkv_out_and_lse_only():
    from unipre3d_amd import mha
    q = torch.randn(2, 65, 3, 2, D, device="cuda", requires_grad=True)
    out = mha.attention_qkvpacked(q)
    saved = out.grad_fn.saved_tensors
    assert [tuple(t.shape) for t in saved] == [(2, 65, 3, 2, D), (2, 65, 2, D), (2, 2, 65)]
    assert saved[0].data_ptr() == q.data_ptr() and saved[1].data_ptr() == out.data_ptr()
    # a gradient that is not contiguous fp32 (sum()'s expanded scalar; an fp64 one) is made so
    out.sum().backward()
    g_sum = q.grad.clone()
    q.grad = None
    out2 = mha.attention_qkvpacked(q)
    out2.backward(torch.ones_like(out2))
    assert torch.equal(g_sum, q.grad)


def test_graph_capture_replays_to_the_eager_bits():
    from unipre3d_amd import mha
    g = torch.Generator().manual_seed(4)
    shape = (2, 129, 3, 6, D)
    sq = torch.randn(shape, generator=g).cuda().requires_grad_(True)
    sd = torch.randn(2, 129, 6, D, generator=g).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(mha.attention_qkvpacked(sq), sq, sd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_out = mha.attention_qkvpacked(sq)
        (c_grad,) = torch.autograd.grad(c_out, sq, sd)
    a, b = torch.randn(shape, generator=g).cuda(), torch.randn(2, 129, 6, D, generator=g).cuda()
    with torch.no_grad():
        sq.copy_(a)
        sd.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    e = a.clone().requires_grad_(True)
    e_out = mha.attention_qkvpacked(e)
    e_out.backward(b)
    assert torch.equal(c_out.detach().view(torch.int32), e_out.detach().view(torch.int32))
    assert torch.equal(c_grad.view(torch.int32), e.grad.view(torch.int32))
    assert torch.isfinite(c_out).all() and torch.isfinite(c_grad).all()


class _ReferenceForm(torch.nn.Module):
    """The op-by-op form of the reference's module: packed qkv Linear, permute, q k^T times the scale, softmax, attn v, transpose, proj."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads, self.scale = num_heads, (dim // num_heads) ** -0.5
        self.qkv = torch.nn.Linear(dim, dim * 3, bias=False)
        self.proj = torch.nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * self.scale).softmax(dim=-1)
        return self.proj((attn @ qkv[2]).transpose(1, 2).reshape(B, N, C))


def test_attention_module_against_the_reference_form(tol):
    from unipre3d_amd import mha
    torch.manual_seed(11)
    ref32 = _ReferenceForm(384, 6).cuda()
    ref64 = _ReferenceForm(384, 6).cuda().double()
    ref64.load_state_dict({k: v.double() for k, v in ref32.state_dict().items()})
    ours = mha.Attention(384, 6).cuda()
    ours.load_state_dict(ref32.state_dict())
    g = torch.Generator().manual_seed(12)
    x_cpu, dy_cpu = torch.randn(2, 129, 384, generator=g), torch.randn(2, 129, 384, generator=g)

    def run(module, dtype):
        x = x_cpu.to("cuda", dtype).requires_grad_(True)
        y = module(x)
        y.backward(dy_cpu.to("cuda", dtype))
        grads = [x.grad, module.qkv.weight.grad, module.proj.weight.grad, module.proj.bias.grad]
        return [t.detach().double().cpu().numpy() for t in [y] + grads]

    r64, r32, got = run(ref64, torch.float64), run(ref32, torch.float32), run(ours, torch.float32)
    for name, a64, a32, a, floor in zip(("y", "dx", "dqkv.weight", "dproj.weight", "dproj.bias"), r64, r32, got,
                                        [tol["floors"]["out"]] + [tol["floors"]["dqkv"]] * 4):
        yard, d = MR.dist(a32, a64), MR.dist(a, a64)
        print(f"\nmha module {name}: {d:.3e} (yardstick {yard:.3e}, bar {2 * yard + floor:.3e})")
        assert d <= 2 * yard + floor, name


def test_argument_checks():
    from unipre3d_amd import mha
    ok = torch.zeros(1, 5, 3, 2, D, device="cuda")
    with pytest.raises(ValueError, match="expected"):
        mha.attention_qkvpacked(ok[0])
    with pytest.raises(ValueError, match="expected"):
        mha.attention_qkvpacked(torch.zeros(1, 5, 2, 2, D, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        mha.attention_qkvpacked(torch.zeros(1, 3, 5, 2, D, device="cuda").transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous"):
        mha.attention_qkvpacked(torch.zeros(1, 5, 3, 2, 2 * D, device="cuda")[..., :D])
    with pytest.raises(ValueError, match="empty"):
        mha.attention_qkvpacked(torch.zeros(1, 0, 3, 2, D, device="cuda"))
    with pytest.raises(ValueError, match="positive"):
        mha.attention_qkvpacked(ok, softmax_scale=-1.0)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError, match="dtype"):
            mha.attention_qkvpacked(ok.to(dtype))
    for d in (16, 32, 128):
        with pytest.raises(NotImplementedError, match="head dim"):
            mha.attention_qkvpacked(torch.zeros(1, 5, 3, 2, d, device="cuda"))
    with pytest.raises(NotImplementedError, match="1024"):
        mha.attention_qkvpacked(torch.zeros(1, 1025, 3, 1, D, device="cuda"))
    with pytest.raises(RuntimeError):
        mha.attention_qkvpacked(ok.cpu())
    assert mha.attention_qkvpacked(ok).shape == (1, 5, 2, D)
