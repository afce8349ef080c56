"""CPU checks of tests/attention_ref.py (the yardsticks of the GPU tests of unipre3d_amd.attention / unipre3d_amd.scatter) and of golden G12."""
import os

import numpy as np
import pytest
import torch

import attention_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_fp64_equals_sdpa_per_sequence():
    lens = (0, 1, 17, 1024, 5, 0, 48)
    qkv, dout, cu = R.make_inputs(lens, 3, 2, 1.0, 0)
    out, dqkv = R.attention_fp64(qkv, cu, 0.25, dout)
    x = qkv.double().requires_grad_(True)
    ref = torch.zeros_like(out)
    for a, b in zip(cu[:-1], cu[1:]):
        if b > a:
            q, k, v = (x[a:b, i].transpose(0, 1) for i in range(3))     # (H, L, D)
            ref[a:b] = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=0.25).transpose(0, 1)
    (dref,) = torch.autograd.grad(ref, x, dout.double())
    assert float((out - ref).abs().max()) <= 1e-12
    assert float((dqkv - dref).abs().max()) <= 1e-12
    assert not out[-3:].any() and not dqkv[-3:].any()


def test_g12_boundary_record():
    g = np.load(os.path.join(GOLDEN, "g12_ptv3_boundary.npz"), allow_pickle=False)
    sizes, patch = g["item_sizes"], int(g["patch_size"])
    assert sizes.tolist() == [17, 96, 130, 97] and patch == 48
    cu, padded = R.ptv3_padding(sizes, patch)
    assert g["attn_cu_seqlens"].dtype == np.int32 and np.array_equal(g["attn_cu_seqlens"], cu)
    assert cu[0] == 0 and cu[1] == 17, "the 17-point item is one 17-long sequence"
    assert np.diff(cu)[1:].tolist() == [48] * ((96 + 144 + 144) // 48)
    assert g["attn_qkv_shape"].tolist() == [int(padded.sum()), 3, 2, 16] and str(g["attn_qkv_dtype"]) == "torch.float16"
    assert int(g["attn_max_seqlen"]) == patch and float(g["attn_softmax_scale"]) == 16 ** -0.5
    ip = g["pool_indptr"]
    assert str(g["pool_indptr_dtype"]) == "torch.int64" and ip[0] == 0 and ip[-1] == sizes.sum() and np.all(np.diff(ip) >= 1)
    assert np.array_equal(ip, g["pool_indptr_coord"])
    assert str(g["pool_feat_reduce"]) == "max" and str(g["pool_coord_reduce"]) == "mean"
    assert g["pool_feat_src_shape"].tolist() == [int(sizes.sum()), 64] and g["pool_coord_src_shape"].tolist() == [int(sizes.sum()), 3]
    assert os.path.getsize(os.path.join(GOLDEN, "g12_ptv3_boundary.npz")) < 140 * 1024


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_segment_csr_ref(reduce):
    g = np.random.default_rng(3)
    src = g.normal(size=(60, 5)).astype(np.float32)
    indptr = np.array([0, 0, 7, 8, 8, 30, 60, 60], np.int64)
    out, arg = R.segment_csr_ref(src, indptr, reduce)
    lengths = torch.as_tensor(np.diff(indptr))
    ref = torch.segment_reduce(torch.as_tensor(src).double(), reduce, lengths=lengths, axis=0).numpy()
    ref[np.diff(indptr) == 0] = 0
    assert not out[[0, 3, 6]].any(), "empty segments give 0"
    if reduce in ("max", "min"):
        assert np.array_equal(out.astype(np.float64), ref)
        rows = np.where(arg >= 0, arg, 0)
        assert np.array_equal(np.take_along_axis(src, rows, 0)[arg >= 0], out[arg >= 0])
        assert np.all((arg >= indptr[:-1, None]) & (arg < indptr[1:, None]) | (arg == -1))
    else:
        assert np.allclose(out, ref, rtol=0, atol=2.0 ** -23 * 30 * np.abs(src).sum(0).max())
    tie = np.array([[2.0], [2.0], [1.0], [1.0]], np.float32)
    assert R.segment_csr_ref(tie, [0, 4], "max")[1].tolist() == [[0]] and R.segment_csr_ref(tie, [0, 4], "min")[1].tolist() == [[2]]


@pytest.mark.parametrize("name", list(R.CASES))
def test_backward_yardstick_constants(name):
    """BWD_YARDSTICK_ULPS is re-derived (attention_rounded against attention_fp64 on the case's inputs) and must cover the measured
    figure without being loose; the forward restatement stays inside one of the three units of the forward bar."""
    lens, tail, H, _, sc = R.CASES[name]
    qkv, dout, cu = R.make_inputs(lens, tail, H, sc, R.SEED)
    o64, d64 = R.attention_fp64(qkv, cu, R.SCALE, dout)
    o, d = R.attention_rounded(qkv, cu, R.SCALE, dout)
    measured = R.bwd_norm_err(d, d64, R.block_den(qkv, dout, d64, cu, R.SCALE)) / R.ULP16
    recorded = R.BWD_YARDSTICK_ULPS[name]
    print(f"[attention_ref] {name}: yardstick measured {measured:.3f} ulp, recorded {recorded}")
    assert measured <= recorded <= 1.3 * measured
    assert bool(((o.double() - o64).abs() <= R.fwd_bound(qkv, cu) / R.FWD_UNITS).all())
    assert R.bwd_bar(recorded * R.ULP16) == 2 * recorded * R.ULP16 + R.ULP16


# what each structured case must reach, on the fp64 scores of its fp16-valued inputs (attention_ref.structured_property)
STRUCTURED_REQUIRED = {
    "all_negative": lambda p, scale: p >= 8.0 / abs(scale),     # every real score <= -NEG: exp(-NEG |scale|) is below an fp16 ulp
    "all_positive": lambda p, scale: p >= 8.0 / abs(scale),
    "peak_last_key": lambda p, scale: p > 0,                     # the arg-max key of every row is len - 1
    "rising_max": lambda p, scale: p >= 4.0,                     # log2 units per 64-key step
    "uniform_q0": lambda p, scale: p == 0,                       # every row's scores are exactly equal
    "uniform_k_equal": lambda p, scale: p == 0,
    "one_hot": lambda p, scale: p >= 8.0,                        # every other key's weight is below an fp16 ulp
    "one_hot_p200": lambda p, scale: p >= 8.0,
    "v_large": lambda p, scale: 3e4 <= p <= 6e4,
    "subnormal": lambda p, scale: p > 0.5,                       # most values are fp16 subnormals
}


def test_structured_table():
    assert set(R.STRUCTURED) == set(R.STRUCTURED_YARDSTICK_ULPS)
    heads = {c[2] for c in R.STRUCTURED.values()}
    assert len(heads) >= 2 and any(h % 4 for h in heads)
    for name in ("scale_neg", "scale_zero", "scale_2", "dout_zero"):      # the mixed_h2 inputs
        assert R.STRUCTURED[name][:4] == R.CASES["mixed_h2"][:4]
    assert [R.STRUCTURED[n][4] for n in ("scale_neg", "scale_zero", "scale_2")] == [-0.25, 0.0, 2.0]
    assert R.STRUCTURED["all_negative"][0] == (1, 15, 17, 47, 49, 65, 130, 1009)
    assert R.STRUCTURED["peak_last_key"][0] == (17, 48, 64, 65, 129, 1009, 1024) and R.STRUCTURED["rising_max"][0] == (300, 1024)
    for name, (lens, tail, H, max_seqlen, scale) in R.STRUCTURED.items():
        qkv, dout, cu, ms, sc = R.make_structured(name)
        assert qkv.dtype == torch.float16 and dout.dtype == torch.float16 and qkv.shape == (sum(lens) + tail, 3, H, 16)
        assert ms == max_seqlen >= max(lens) and sc == scale and bool(torch.isfinite(qkv).all()) and bool(torch.isfinite(dout).all())
        assert torch.equal(qkv, R.make_structured(name)[0])
    assert not R.make_structured("dout_zero")[1].any()
    assert not R.make_structured("uniform_q0")[0][:-1, 0].any()


@pytest.mark.parametrize("name", list(R.STRUCTURED))
def test_structured_case(name):
    """The structure of the case holds on the fp64 scores; STRUCTURED_YARDSTICK_ULPS is re-derived exactly like BWD_YARDSTICK_ULPS and
    the forward restatement stays inside one of the three units of the forward bar."""
    qkv, dout, cu, _, scale = R.make_structured(name)
    prop = R.structured_property(name, qkv, cu, scale)
    o64, d64 = R.attention_fp64(qkv, cu, scale, dout)
    o, d = R.attention_rounded(qkv, cu, scale, dout)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(d).all()) and bool(torch.isfinite(d64).all())
    assert float(d64.abs().max()) < 65504 / 2, "the true gradient must sit well inside the fp16 range"
    measured = R.bwd_norm_err(d, d64, R.block_den(qkv, dout, d64, cu, scale)) / R.ULP16
    recorded = R.STRUCTURED_YARDSTICK_ULPS[name]
    unit = R.fwd_bound(qkv, cu) / R.FWD_UNITS
    units = float(((o.double() - o64).abs() / unit.clamp_min(1e-300)).max())
    print(f"[attention_ref] {name}: property {prop}, forward {units:.3f} unit, yardstick measured {measured:.3f} ulp, recorded {recorded}")
    if name in STRUCTURED_REQUIRED:
        assert prop is not None and STRUCTURED_REQUIRED[name](prop, scale), (name, prop)
    assert measured <= recorded <= 1.3 * measured
    assert bool(((o.double() - o64).abs() <= unit).all())
    if name == "dout_zero":
        assert not d64.any() and not d.any()
    if name == "scale_zero":
        assert not d64[:, :2].any() and not d[:, :2].any()
