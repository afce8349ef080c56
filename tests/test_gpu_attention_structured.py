"""unipre3d_amd.attention on the MI355X on structured inputs (attention_ref.STRUCTURED): all real scores strongly negative or positive,
the dominant key last, a maximum that rises in every 64-key step, exactly uniform and one-hot rows, softmax_scale of either sign and
0, the fp16 range ends, dO = 0; and the same ragged input under every launch shape that max_seqlen selects.  Bars and comparison are
test_gpu_attention.py's (_run / _compare: every element against the fp64 restatement); assertions are exact where the mathematics is."""
import numpy as np
import pytest
import torch

import attention_ref as R
from test_gpu_attention import _compare, _run

pytestmark = pytest.mark.gpu


def _seq_rows(cu):
    return [(int(a), int(b)) for a, b in zip(cu[:-1], cu[1:]) if b > a]


@pytest.mark.parametrize("name", list(R.STRUCTURED))
def test_structured_against_fp64(name):
    lens, tail, H, _, _ = R.STRUCTURED[name]
    qkv, dout, cu, max_seqlen, scale = R.make_structured(name)
    out, dqkv = _run(qkv, dout, cu, max_seqlen, scale)
    _compare(name, qkv, dout, cu, out, dqkv, R.STRUCTURED_YARDSTICK_ULPS[name] * R.ULP16, scale)
    out, dqkv = out.cpu(), dqkv.cpu()
    if tail:
        assert not out[-tail:].any() and not dqkv[-tail:].any(), "tail rows must be zero (output and gradient)"
    if name == "dout_zero":
        assert not dqkv.any(), "dO = 0: every gradient is exactly 0"
    if name == "uniform_q0":
        for a, b in _seq_rows(cu):
            assert bool((out[a:b] == out[a:a + 1]).all()), f"q = 0: rows {a}..{b} of one sequence must be the same fp16 vector"
    if name == "scale_zero":
        mean = torch.zeros_like(out, dtype=torch.float64)
        for a, b in _seq_rows(cu):
            mean[a:b] = qkv[a:b, 2].double().mean(0, keepdim=True).half().double()
        assert bool(((out.double() - mean).abs() <= R.fwd_bound(qkv, cu)).all()), "scale 0: out is the mean of v"
        assert not dqkv[:, :2].any(), "scale 0: dq and dk are exactly 0"
    if name == "v_large":
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
        assert float(out.abs().max()) <= float(qkv[:, 2].abs().max()), "out is a convex combination of v"


# ---- max_seqlen as the kernel selector ---------------------------------------------------------------------------------------
SWEEP_MAX_SEQLEN = (16, 17, 63, 64, 65, 256, 257, 512, 513, 1023, 1024)
SWEEP_H = 6          # two 4-head groups on the short path, the second half empty
SWEEP_YARDSTICK_CAP = max(R.BWD_YARDSTICK_ULPS.values())   # the restatement's own error on these Gaussian inputs must not exceed that of CASES


def _sweep_input():
    g = np.random.default_rng(16)
    lens = [0, 1, 16, 15] + [int(v) for v in g.integers(0, 17, size=68)]
    assert len(lens) >= 64 and max(lens) == 16 and 0 in lens and 1 in lens
    qkv, dout, cu = R.make_inputs(lens, 3, SWEEP_H, 1.0, 16)
    return qkv, dout, cu


def test_launch_shape_sweep():
    """One ragged input with lengths <= 16 under every launch shape: each run meets the fp64 bars; whether the runs are bit-identical
    is printed (an observation, not a requirement)."""
    qkv, dout, cu = _sweep_input()
    _, d = R.attention_rounded(qkv, cu, R.SCALE, dout)
    _, d64 = R.attention_fp64(qkv, cu, R.SCALE, dout)
    yard = R.bwd_norm_err(d, d64, R.block_den(qkv, dout, d64, cu, R.SCALE))
    assert yard <= SWEEP_YARDSTICK_CAP * R.ULP16
    results = {}
    for ms in SWEEP_MAX_SEQLEN:
        out, dqkv = _run(qkv, dout, cu, ms)
        _compare(f"sweep_max_seqlen_{ms}", qkv, dout, cu, out, dqkv, yard)
        assert not out[-3:].any() and not dqkv[-3:].any()
        results[ms] = (out.cpu(), dqkv.cpu())
    o0, d0 = results[SWEEP_MAX_SEQLEN[0]]
    same = {ms: bool(torch.equal(o, o0) and torch.equal(d, d0)) for ms, (o, d) in results.items()}
    print("[attention] launch-shape sweep: bit-identical to max_seqlen 16:", same)


@pytest.mark.parametrize("max_seqlen", [1, 65, 257, 513])
def test_longest_sequence_equals_max_seqlen(max_seqlen):
    lens = (max_seqlen, 0, 1, min(17, max_seqlen), max_seqlen, max(max_seqlen - 1, 1))
    qkv, dout, cu = R.make_inputs(lens, 2, 3, 1.0, 100 + max_seqlen)
    _, d = R.attention_rounded(qkv, cu, R.SCALE, dout)
    _, d64 = R.attention_fp64(qkv, cu, R.SCALE, dout)
    yard = R.bwd_norm_err(d, d64, R.block_den(qkv, dout, d64, cu, R.SCALE))
    assert yard <= SWEEP_YARDSTICK_CAP * R.ULP16
    out, dqkv = _run(qkv, dout, cu, max_seqlen)
    _compare(f"longest_equals_max_seqlen_{max_seqlen}", qkv, dout, cu, out, dqkv, yard)
    assert not out[-2:].any() and not dqkv[-2:].any()
