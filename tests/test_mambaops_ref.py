"""tests/mambaops_ref.py against torch's own F.conv1d / F.layer_norm in fp64 and against analytic answers, and what of
unipre3d_amd.causal_conv1d / unipre3d_amd.layernorm needs no device: the library's host-only queries, the header against the binding,
and the refusals that are decided before a kernel is launched."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import mambaops_ref as R
from conftest import ROOT


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("has_bias", [False, True])
def test_conv_restatement_is_torchs_padded_conv1d(width, has_bias):
    x, w, b, dout = R.conv_inputs(2, 5, 37, width, has_bias)
    torch_conv = lambda x, w, b: F.conv1d(F.pad(x, (width - 1, 0)), w[:, None, :], b, groups=5)
    (o1,), g1 = R.run_with_grads(lambda x, w, b: R.causal_conv1d(x, w, b), (x, w, b), (dout,))
    (o2,), g2 = R.run_with_grads(torch_conv, (x, w, b), (dout,))
    assert R.norm_err(o1, o2) < 1e-14
    for a, c in zip(g1, g2):
        assert (a is None) == (c is None) and (a is None or R.norm_err(a, c) < 1e-14)
    (s1,), _ = R.run_with_grads(lambda x, w, b: R.causal_conv1d(x, w, b, "silu"), (x, w, b), (dout,))
    assert R.norm_err(s1, F.silu(o2)) < 1e-14
    assert torch.equal(s1, R.causal_conv1d(x, w, b, "swish"))
    with pytest.raises(NotImplementedError, match="activation must be None, silu, or swish"):
        R.causal_conv1d(x, w, b, "relu")


def test_conv_one_hot_tap_is_a_shift():
    """weight[d, w] = 1 at one w: out[l] = x[l - (W-1) + w], zeros in front."""
    x, _, _, _ = R.conv_inputs(2, 4, 19, 4)
    for w in range(4):
        weight = torch.zeros(4, 4, dtype=torch.float64)
        weight[:, w] = 1.0
        out, shift = R.causal_conv1d(x, weight), 3 - w
        assert torch.equal(out[..., shift:], x[..., :19 - shift]) and float(out[..., :shift].abs().sum()) == 0.0


def test_conv_impulse_gives_reversed_weights():
    """x = 1 at step k: out[k + j] = weight[d, W-1-j]."""
    _, weight, _, _ = R.conv_inputs(1, 5, 8, 4)
    x = torch.zeros(1, 5, 12, dtype=torch.float64)
    x[:, :, 6] = 1.0
    out = R.causal_conv1d(x, weight)
    assert torch.equal(out[0, :, 6:10], weight.flip(-1)) and float(out[0, :, :6].abs().sum()) == 0.0 == float(out[0, :, 10:].abs().sum())


@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("has_residual", [False, True])
def test_norm_restatement_is_torchs_layer_norm(has_bias, has_residual):
    x, w, b, res, dy, dr = R.norm_inputs(7, 33, has_bias, has_residual)
    eps = 1e-5
    ours = lambda x, w, b, res: R.layer_norm(x, w, b, res, eps, prenorm=True)
    theirs = lambda x, w, b, res: (F.layer_norm(x if res is None else x + res, (33,), w, b, eps), x if res is None else x + res)
    o1, g1 = R.run_with_grads(ours, (x, w, b, res), (dy, dr))
    o2, g2 = R.run_with_grads(theirs, (x, w, b, res), (dy, dr))
    assert R.norm_err(o1[0], o2[0]) < 1e-13 and torch.equal(o1[1], o2[1])
    for a, c in zip(g1, g2):
        assert (a is None) == (c is None) and (a is None or R.norm_err(a, c) < 1e-13)
    rms = R.rms_norm(x, w, b, res, eps=eps)
    r = x if res is None else x + res
    want = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w
    assert R.norm_err(rms, want if b is None else want + b) < 1e-14


def test_norm_constant_row_gives_the_bias():
    _, w, b, _, _, _ = R.norm_inputs(3, 33)
    x = torch.tensor([1000.0, -3.25, 0.0], dtype=torch.float64)[:, None].expand(3, 33)
    assert torch.equal(R.layer_norm(x, w, b), b[None].expand(3, 33))


def test_block_prologue_chain_carries_the_residual():
    g = torch.Generator().manual_seed(3)
    hidden, mix = torch.randn(6, 16, generator=g, dtype=torch.float64), torch.randn(16, 16, generator=g, dtype=torch.float64) / 4
    w1, w2 = torch.ones(16, dtype=torch.float64), torch.full((16,), 0.5, dtype=torch.float64)
    h2, r2 = R.block_prologues(hidden, mix, w1, w2)
    h1 = torch.tanh(R.rms_norm(hidden, w1, None, eps=1e-5) @ mix)
    assert torch.equal(r2, h1 + hidden) and R.norm_err(h2, R.rms_norm(r2, w2, None, eps=1e-5)) < 1e-15


# ---- the library without a device ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cc():
    from unipre3d_amd import causal_conv1d
    causal_conv1d.load()
    return causal_conv1d


@pytest.fixture(scope="module")
def ln(cc):
    from unipre3d_amd import layernorm
    return layernorm


def test_host_queries(cc, ln):
    lib = cc.load()
    assert [cc.chunk_len(L) for L in (1, 64, 65, 128, 129, 192, 193, 256, 257, 4096)] == [64, 64, 128, 128, 192, 192, 256, 256, 256, 256]
    assert lib.u3d_cconv_bwd_scratch_bytes(2, 5) >= 2 * 5 * 5 * 4 and lib.u3d_cconv_bwd_scratch_bytes(2, 5) % 256 == 0
    assert lib.u3d_cconv_bwd_scratch_bytes(0, 5) == 0
    assert ln.max_n() >= 1024
    # the backward's row split: four rows per wave until 2048 waves are out, then longer runs
    assert [ln.bwd_waves(M) for M in (1, 4, 5, 37, 4128, 8192, 8193, 32768)] == [1, 1, 2, 10, 1032, 2048, 2048, 2048]
    for M, N in ((1, 1), (37, 384), (32768, 384)):
        assert lib.u3d_addnorm_bwd_scratch_bytes(M, N) >= 2 * ln.bwd_waves(M) * N * 4
    assert lib.u3d_addnorm_bwd_scratch_bytes(37, ln.max_n() + 1) == 0


_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)


def test_header_and_binding_agree(cc, ln):
    """include/unipre3d_mambaops.h against the modules' table and against what the loader set on the handle: the names, the parameter
    count, the return type and the class of every parameter."""
    hdr = open(os.path.join(ROOT, "include", "unipre3d_mambaops.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    declared = {}
    for ret, name, params in _DECLARATION.findall(hdr):
        types = []
        for q in (s.strip() for s in params.split(",")):
            if q in ("", "void"):
                continue
            types.append(q[:q.rindex("*") + 1].replace(" ", "") if "*" in q else " ".join(q.split()[:-1]))
        assert name not in declared
        declared[name] = (" ".join(ret.split()), types)
    assert len(declared) == 10 and set(declared) == set(cc.EXPORTS) and len(set(cc.EXPORTS)) == len(cc.EXPORTS)
    assert set(ln.EXPORTS) == {n for n in declared if n.startswith("u3d_addnorm_")}
    handle = cc.load()
    assert ln.load() is handle
    assert handle.u3d_mambaops_abi_version() == cc.ABI_VERSION == 1
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    launches = {"u3d_cconv_fwd", "u3d_cconv_bwd", "u3d_addnorm_fwd", "u3d_addnorm_bwd"}
    for name, (ret, params) in declared.items():
        fn = getattr(handle, name)
        assert fn.restype is scalars[ret], (name, ret)
        assert len(fn.argtypes) == len(params), name
        assert (params[-1:] == ["void*"]) == (name in launches), name          # the stream is the last argument of every launch
        for k, (c_type, bound) in enumerate(zip(params, fn.argtypes)):
            if c_type.endswith("*"):
                assert bound is ctypes.c_void_p, (name, k, c_type)
            else:
                assert bound is scalars[c_type], (name, k, c_type, bound)


def test_conv_refusals_without_a_device(cc):
    x, w, b = torch.randn(2, 6, 9), torch.randn(6, 4), torch.randn(6)
    f = cc.causal_conv1d_fn
    assert cc.causal_conv1d_update is None
    for act in ("relu", "gelu", True):
        with pytest.raises(NotImplementedError, match="activation must be None, silu, or swish"):
            f(x, w, b, act)
    for width in (1, 5):
        with pytest.raises(NotImplementedError, match="width"):
            f(x, torch.randn(6, width), b)
    for bad in ((x.half(), w, b), (x, w.double(), b), (x, w, b.bfloat16())):
        with pytest.raises(NotImplementedError, match="fp32 only"):
            f(*bad)
    for bad in ((x[0], w, b), (x, torch.randn(5, 4), b), (x, w, torch.randn(5)), (x, w.reshape(6, 1, 4), b), (x[:, :, :0], w, b)):
        with pytest.raises(ValueError):
            f(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, w, b, "silu")


def test_norm_refusals_without_a_device(ln):
    x, w, b = torch.randn(3, 5, 16), torch.randn(16), torch.randn(16)
    with pytest.raises(NotImplementedError, match="at most"):
        ln.layer_norm_fn(torch.randn(2, ln.max_n() + 1), torch.randn(ln.max_n() + 1), None)
    for bad in ((x.half(), w, b), (x, w.double(), b), (x, w, b, x.double())):
        with pytest.raises(NotImplementedError, match="fp32 only"):
            ln.layer_norm_fn(*bad)
    for bad in ((x, torch.randn(15), b), (x, w, torch.randn(1, 16)), (x, w, b, x[0]), (x[:0], w, b)):
        with pytest.raises(ValueError):
            ln.rms_norm_fn(*bad)
    for call in (lambda: ln.layer_norm_fn(x, w, b), lambda: ln.rms_norm_fn(x, w, None, residual=x, prenorm=True),
                 lambda: ln.RMSNorm(16)(x, residual=x, prenorm=True, residual_in_fp32=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    m = ln.RMSNorm(16)
    assert isinstance(m, torch.nn.Module) and m.eps == 1e-5 and m.bias is None and torch.equal(m.weight.detach(), torch.ones(16))
    assert [n for n, _ in m.named_parameters()] == ["weight"]
