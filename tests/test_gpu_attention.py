"""unipre3d_amd.attention on the MI355X against tests/attention_ref.py: every element of out within 3 * 2^-11 * max|v| of the fp64
restatement, every element of dqkv within the derived bar (attention_ref's docstring), both kernel paths (max_seqlen <= 64: one wave per
(sequence, head); above: one workgroup), ragged lengths, tails, repeatability, graph capture, refusals, a 240 k-token call and one
training step of a module with SerializedAttention's data flow."""
import json
import os

import numpy as np
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fa():
    from unipre3d_amd import attention
    return attention


def _run(qkv, dout, cu, max_seqlen, scale=R.SCALE):
    x = qkv.to(DEV).requires_grad_(True)
    out = _fa().flash_attn_varlen_qkvpacked_func(x, torch.as_tensor(cu).to(DEV), max_seqlen, softmax_scale=scale)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), x.grad


def _compare(name, qkv, dout, cu, out, dqkv, yardstick, scale=R.SCALE, dev="cpu"):
    """every element of out and dqkv against the fp64 restatement (evaluated on `dev`); returns the figures"""
    q, g = qkv.to(dev), dout.to(dev)
    o64, d64 = R.attention_fp64(q, cu, scale, g)
    out, dqkv = out.to(dev), dqkv.to(dev)
    assert out.dtype == torch.float16 and dqkv.dtype == torch.float16 and out.shape == o64.shape and dqkv.shape == d64.shape
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all()), f"{name}: NaN / inf"
    bound = R.fwd_bound(q, cu)
    ferr = (out.double() - o64).abs()
    units = float((ferr / (bound / R.FWD_UNITS).clamp_min(1e-300)).max()) if out.numel() else 0.0
    berr = R.bwd_norm_err(dqkv, d64, R.block_den(q, g, d64, cu, scale))
    bar = R.bwd_bar(yardstick)
    fig = {"case": name, "fwd_units_of_2^-11_maxv": round(units, 3), "fwd_bar_units": R.FWD_UNITS, "bwd_yardstick": yardstick,
           "bwd_bar": bar, "bwd_kernel_worst": berr}
    print("[attention]", json.dumps(fig))
    assert bool((ferr <= bound).all()), f"{name}: forward {units:.2f} units of 2^-11 max|v| (bar {R.FWD_UNITS})"
    assert berr <= bar, f"{name}: backward normalised error {berr:.3e} above the bar {bar:.3e} (yardstick {yardstick:.3e})"
    return fig


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_against_fp64(name):
    lens, tail, H, max_seqlen, sc = R.CASES[name]
    qkv, dout, cu = R.make_inputs(lens, tail, H, sc, R.SEED)
    out, dqkv = _run(qkv, dout, cu, max_seqlen)
    _compare(name, qkv, dout, cu, out, dqkv, R.BWD_YARDSTICK_ULPS[name] * R.ULP16)
    if tail:
        assert not out[-tail:].any() and not dqkv[-tail:].any(), "tail rows must be zero (output and gradient)"


def test_g12_boundary():
    g = np.load(os.path.join(GOLDEN, "g12_ptv3_boundary.npz"), allow_pickle=False)
    cu, H, D = g["attn_cu_seqlens"], int(g["attn_qkv_shape"][2]), int(g["attn_qkv_shape"][3])
    T = int(g["attn_qkv_shape"][0])
    assert str(g["attn_qkv_dtype"]) == "torch.float16" and D == 16 and T == int(cu[-1])
    gen = torch.Generator().manual_seed(12)
    qkv, dout = torch.randn(T, 3, H, D, generator=gen).half(), torch.randn(T, H, D, generator=gen).half()
    scale, max_seqlen = float(g["attn_softmax_scale"]), int(g["attn_max_seqlen"])
    x = qkv.to(DEV).requires_grad_(True)
    out = _fa().flash_attn_varlen_qkvpacked_func(x, torch.as_tensor(cu).to(DEV), max_seqlen=max_seqlen, dropout_p=0, softmax_scale=scale)
    out.backward(dout.to(DEV))
    _, d = R.attention_rounded(qkv, cu, scale, dout)
    _, d64 = R.attention_fp64(qkv, cu, scale, dout)
    yard = R.bwd_norm_err(d, d64, R.block_den(qkv, dout, d64, cu, scale))
    _compare("g12", qkv, dout, cu, out.detach(), x.grad, yard, scale)


def test_default_scale_and_no_grad():
    qkv, dout, cu = R.make_inputs((48, 17, 100), 0, 2, 1.0, 3)
    for ms in (48, 100):
        c = cu if ms == 100 else R.cu_from_lengths((48, 17, 48, 48, 4))
        with torch.no_grad():
            out = _fa().flash_attn_varlen_qkvpacked_func(qkv.to(DEV), torch.as_tensor(c).to(DEV), ms)
        o64 = R.attention_fp64(qkv, c, 16 ** -0.5)
        assert bool(((out.cpu().double() - o64).abs() <= R.fwd_bound(qkv, c)).all())


def test_bit_identical_and_graph_capture():
    for name in ("short_h2_p48", "mixed_h2"):
        lens, tail, H, max_seqlen, sc = R.CASES[name]
        qkv, dout, cu = R.make_inputs(lens, tail, H, sc, 7)
        o1, d1 = _run(qkv, dout, cu, max_seqlen)
        o2, d2 = _run(qkv, dout, cu, max_seqlen)
        assert torch.equal(o1, o2) and torch.equal(d1, d2), f"{name}: two calls differ"
        x = qkv.to(DEV).requires_grad_(True)
        g, c = dout.to(DEV), torch.as_tensor(cu).to(DEV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # warm-up outside the capture
            _fa().flash_attn_varlen_qkvpacked_func(x, c, max_seqlen, softmax_scale=R.SCALE).backward(g)
        torch.cuda.current_stream().wait_stream(side)
        x.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _fa().flash_attn_varlen_qkvpacked_func(x, c, max_seqlen, softmax_scale=R.SCALE)
            (dx,) = torch.autograd.grad(out, x, g)
        out.zero_()
        dx.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, o1) and torch.equal(dx, d1), f"{name}: graph replay differs from the eager call"


def test_refusals():
    f = _fa().flash_attn_varlen_qkvpacked_func
    qkv = torch.zeros(64, 3, 2, 16, dtype=torch.float16, device=DEV)
    cu = torch.tensor([0, 48, 64], dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError, match="max_seqlen"):
        f(qkv, cu, 1025)
    with pytest.raises(NotImplementedError, match="dropout_p"):
        f(qkv, cu, 48, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="causal"):
        f(qkv, cu, 48, causal=True)
    with pytest.raises(NotImplementedError, match="dtype"):
        f(qkv.bfloat16(), cu, 48)
    with pytest.raises(NotImplementedError, match="head dim"):
        f(torch.zeros(64, 3, 2, 32, dtype=torch.float16, device=DEV), cu, 48)
    with pytest.raises(ValueError, match="contiguous"):
        f(torch.zeros(64, 3, 16, 2, dtype=torch.float16, device=DEV).transpose(2, 3), cu, 48)
    with pytest.raises(ValueError, match="cu_seqlens"):
        f(qkv, cu.long(), 48)
    with pytest.raises(RuntimeError, match="device"):
        f(qkv.cpu(), cu.cpu(), 48)


def test_empty_and_overlong():
    f = _fa().flash_attn_varlen_qkvpacked_func
    # no sequence at all: everything is tail
    qkv = torch.randn(5, 3, 2, 16, device=DEV).half().requires_grad_(True)
    out = f(qkv, torch.zeros(1, dtype=torch.int32, device=DEV), 48)
    out.backward(torch.ones_like(out))
    assert not out.any() and not qkv.grad.any()
    assert f(torch.zeros(0, 3, 2, 16, dtype=torch.float16, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), 48).shape == (0, 2, 16)
    # a sequence longer than max_seqlen (a caller error): its first max_seqlen rows attend to one another, the rest are zeros
    for ms, n in ((48, 70), (100, 130)):
        x, dout, _ = R.make_inputs((n, 20), 0, 2, 1.0, 5)
        out, dx = _run(x, dout, R.cu_from_lengths((n, 20)), ms)
        assert not out[ms:n].any() and not dx[ms:n].any()
        keep = torch.cat([torch.arange(ms), torch.arange(n, n + 20)])
        o2, d2 = _run(x[keep], dout[keep], R.cu_from_lengths((ms, 20)), ms)
        assert torch.equal(out[keep], o2) and torch.equal(dx[keep], d2)


def test_240k_tokens_against_fp64_on_device():
    g = torch.Generator().manual_seed(240)
    for H, patch, n_tok in ((4, 48, 240_000), (2, 1024, 60_000)):
        lens = [patch] * (n_tok // patch) + [n_tok % patch or 1, 0, 17]
        T = sum(lens) + 11
        qkv, dout = torch.randn(T, 3, H, 16, generator=g).half(), torch.randn(T, H, 16, generator=g).half()
        cu = R.cu_from_lengths(lens)
        out, dqkv = _run(qkv, dout, cu, patch)
        q, d = qkv.to(DEV), dout.to(DEV)
        _, dr = R.attention_rounded(q, cu, R.SCALE, d)
        _, d64 = R.attention_fp64(q, cu, R.SCALE, d)
        yard = R.bwd_norm_err(dr, d64, R.block_den(q, d, d64, cu, R.SCALE))
        _compare(f"tokens{n_tok}_h{H}_p{patch}", qkv, dout, cu, out, dqkv, yard, dev=DEV)
        assert not out[-11:].any() and not dqkv[-11:].any()


class _SerializedAttentionLike(torch.nn.Module):
    """linear -> gather by order -> varlen attention -> gather by inverse -> linear (fp32 parameters, fp16 attention)"""

    def __init__(self, C, H, attn):
        super().__init__()
        self.qkv, self.proj, self.H, self.attn = torch.nn.Linear(C, 3 * C), torch.nn.Linear(C, C), H, attn

    def forward(self, feat, order, inverse, cu, max_seqlen):
        C = feat.shape[1]
        qkv = self.qkv(feat)[order].half().reshape(-1, 3, self.H, C // self.H)
        o = self.attn(qkv, cu, max_seqlen, (C // self.H) ** -0.5).reshape(-1, C).to(feat.dtype)
        return self.proj(o[inverse])


class _RoundedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cu, scale):
        ctx.save_for_backward(qkv)
        ctx.args = (cu, scale)
        return R.attention_rounded(qkv, cu, scale)

    @staticmethod
    def backward(ctx, dout):
        (qkv,) = ctx.saved_tensors
        return R.attention_rounded(qkv, ctx.args[0], ctx.args[1], dout.half())[1], None, None


def test_module_trains_one_step():
    C, H, patch = 64, 4, 48
    sizes = (17, 96, 130, 97)
    cu, padded = R.ptv3_padding(sizes, patch)
    N = sum(sizes)
    g = torch.Generator().manual_seed(4)
    # order: a permutation inside every item, padded by repeating points; inverse: where each point sits in the padded order
    order, base = [], 0
    for n, m in zip(sizes, padded):
        p = base + torch.randperm(n, generator=g)
        order.append(torch.cat([p, p[:int(m) - n]]))
        base += n
    order = torch.cat(order)
    inverse = torch.empty(N, dtype=torch.long)
    inverse[order.flip(0)] = torch.arange(len(order)).flip(0)
    feat, target = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    cu_d = torch.as_tensor(cu).to(DEV)
    grads = []
    for attn in (lambda q, c, ms, s: _fa().flash_attn_varlen_qkvpacked_func(q, c, ms, softmax_scale=s),
                 lambda q, c, ms, s: _RoundedAttention.apply(q, cu, s)):
        torch.manual_seed(0)
        m = _SerializedAttentionLike(C, H, attn).to(DEV)
        loss = ((m(feat.to(DEV), order.to(DEV), inverse.to(DEV), cu_d, patch) - target.to(DEV)) ** 2).mean()
        loss.backward()
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        opt.step()
        grads.append({k: p.grad.detach().double().cpu() for k, p in m.named_parameters()})
        assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    # the rule of the operator test, propagated: both runs differ in dqkv by at most bar * (block maximum) per element, and the
    # parameter gradients are sums of such elements; normalise by the largest |gradient| of the parameter
    bar = R.bwd_bar(R.BWD_YARDSTICK_ULPS["short_h2_p48"] * R.ULP16)
    for k in grads[0]:
        err = float((grads[0][k] - grads[1][k]).abs().max() / grads[1][k].abs().max())
        print(f"[attention] module d{k}: normalised difference {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (k, err, bar)
