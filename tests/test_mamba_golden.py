"""The CPU restatements of the Mamba operators and mixers (tests/selective_scan_ref.py, tests/mambaops_ref.py, tests/mamba_mixer_ref.py)
against what the backbones' own code computed (tests/golden/g14_mamba.npz, recorded by make_g14_mamba.py): the restatements are what every
device test is judged by, so they have to mean what the backbones mean.

Rule for the fp32 records (scan, mixers, blocks, and the fp32 conv / norm records): the recorded tensor lies within
bar(yardstick) = max(4 x yardstick, 4 * 2^-23) of the restatement's fp64 run in norm_err, the yardstick being the restatement's own fp32 run.
Rule for the fp64 records (conv, norm): two fp64 evaluations of one formula agree to 1e-10 of the tensor maximum.
A semantic difference (tap order, the x_proj split, the group of a channel, where eps sits, the flipped axis) shows at 1e-2 or more.
Every figure is printed before it is asserted; U3D_MAMBA_GOLDEN_TOLERANCE_OUT=<file> collects them (profiles/mamba_golden/tolerance.json).
"""
import json
import os

import numpy as np
import pytest
import torch

import mamba_mixer_ref as X
import mambaops_ref as M
import selective_scan_ref as S

F64_BOUND = 1e-10
FIGURES = []


@pytest.fixture(scope="module")
def g14(golden):
    yield golden("g14_mamba.npz")
    path = os.environ.get("U3D_MAMBA_GOLDEN_TOLERANCE_OUT")
    if path and FIGURES:
        with open(path, "w") as f:
            json.dump({"unit": "max |recorded - restated f64| / max |restated f64| per tensor.  fp32 records: bar = max(4 x yardstick, "
                               "4 * 2^-23), yardstick = the fp32 run of the restatement.  fp64 records: bar = 1e-10",
                       "cases": FIGURES}, f, indent=1)


_t = X._t


def _check(case, name, recorded, want64, yardstick=None):
    """yardstick None: an fp64 record."""
    err = S.norm_err(recorded, want64)
    b = F64_BOUND if yardstick is None else S.bar(yardstick)
    FIGURES.append({"case": case, "tensor": name, "yardstick": yardstick, "bar": b, "reference": err})
    print(f"[mamba_golden] {case} {name}: yardstick {yardstick if yardstick is None else format(yardstick, '.3e')} bar {b:.3e} reference {err:.3e}")
    return [] if err <= b else [f"{case} {name}: {err:.3e} > {b:.3e}"]


# ---- 1. the scan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,tag,softplus,absent", X.SCAN_CASES, ids=[c[0] for c in X.SCAN_CASES])
def test_scan_restatement_is_the_reference(g14, case, tag, softplus, absent):
    t, dout = X.scan_inputs(g14, tag, softplus, absent)
    o64, g64, ys = S.yardstick_case(t, dout, delta_softplus=softplus)
    last64 = S.selective_scan(**t, delta_softplus=softplus, return_last_state=True)[1]
    last32 = S.selective_scan(**S.cast(t, torch.float32), delta_softplus=softplus, return_last_state=True)[1]
    bad = _check("scan_" + case, "out", _t(g14, f"scan_{case}_out"), o64, ys["out"])
    bad += _check("scan_" + case, "last_state", _t(g14, f"scan_{case}_last_state"), last64, S.norm_err(last32, last64))
    seen = 0
    for k in S.GRAD_NAMES:
        key = f"scan_{case}_d{k}"
        assert not (t[k] is None and key in g14.files)
        if key in g14.files:
            rec = _t(g14, key)
            assert rec.shape == t[k].shape
            bad += _check("scan_" + case, "d" + k, rec, g64[k], ys[k])
            seen += 1
    assert seen >= 2 and not bad, bad


def test_scan_inputs_tell_the_conventions_apart(g14):
    """On the recorded inputs, B <-> C, the other group of a channel and the bias added after the softplus each move out by > 1e-2."""
    t, _ = X.scan_inputs(g14, "4", True, ())
    want = S.selective_scan(**t, delta_softplus=True)
    assert S.norm_err(S.selective_scan(**{**t, "B": t["C"], "C": t["B"]}, delta_softplus=True), want) > 1e-2
    assert S.norm_err(S.selective_scan(**{**t, "B": t["B"].flip(1), "C": t["C"].flip(1)}, delta_softplus=True), want) > 1e-2
    interleaved = {**t, "B": t["B"].repeat(1, 4, 1, 1), "C": t["C"].repeat(1, 4, 1, 1)}          # channel d reads group d % G
    assert S.norm_err(S.selective_scan(**interleaved, delta_softplus=True), want) > 1e-2
    late = torch.nn.functional.softplus(t["delta"]) + t["delta_bias"][None, :, None]
    assert S.norm_err(S.selective_scan(**{**t, "delta": late, "delta_bias": None}), want) > 1e-2


# ---- 2. the conv -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_restatement_is_the_reference(g14, width):
    cases = [str(c) for c in g14["conv_cases"]]
    assert cases == ["none_b1", "none_b0", "silu_b1", "silu_b0"]
    x, w, b, dout = (_t(g14, k) for k in ("conv_x", f"conv_w{width}_weight", f"conv_w{width}_bias", f"conv_w{width}_dout"))
    assert x.shape == (2, 12, 19) and w.shape == (6, width)
    bad = []
    for i, case in enumerate(cases):
        act, has_b = (None if case.startswith("none") else "silu"), case.endswith("b1")
        tensors = (x[:, :6], w, b if has_b else None)
        (o64,), g64 = M.run_with_grads(lambda x, w, b: M.causal_conv1d(x, w, b, act), tensors, (dout,))
        (o32,), g32 = M.run_with_grads(lambda x, w, b: M.causal_conv1d(x, w, b, act), M.cast(tensors, torch.float32), (dout.float(),))
        name = f"conv_w{width}_{case}"
        for k, a64, a32 in (("out", o64, o32), ("dx", g64[0], g32[0]), ("dweight", g64[1], g32[1]), ("dbias", g64[2], g32[2])):
            rec32, rec64 = _t(g14, f"conv_w{width}_{k}")[i], _t(g14, f"conv_w{width}_{k}_f64")[i]
            if a64 is None:
                assert bool(torch.isnan(rec32).all()) and bool(torch.isnan(rec64).all())
                continue
            assert rec64.shape == a64.shape
            bad += _check(name, k + "_f64", rec64, a64) + _check(name, k, rec32, a64, S.norm_err(a32, a64))
    assert not bad, bad


def test_conv_inputs_tell_the_tap_order_apart(g14):
    x, w, b = _t(g14, "conv_x")[:, :6], _t(g14, "conv_w4_weight"), _t(g14, "conv_w4_bias")
    want = M.causal_conv1d(x, w, b, "silu")
    assert S.norm_err(M.causal_conv1d(x, w.flip(1), b, "silu"), want) > 1e-2


# ---- 3. add + norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x24", "3x384"])
def test_norm_restatement_is_the_reference(g14, shape):
    cases = [str(c) for c in g14["norm_cases"]]
    assert len(cases) == len(set(cases)) == 16
    eps = float(g14["eps"])
    x, w, b, res, dy, dr = (_t(g14, f"norm_{shape}_{k}") for k in ("x", "weight", "bias", "residual", "dy", "dr"))
    bad = []
    for i, case in enumerate(cases):
        kind, r, bb, p = case.split("_")
        rms, has_r, has_b, pre = kind == "rms", r == "r1", bb == "b1", p == "p1"
        tensors = (x, w, b if has_b else None, res if has_r else None)
        fn = lambda x, w, b, res: M.layer_norm(x, w, b, res, eps, pre, rms)
        o64, g64 = M.run_with_grads(fn, tensors, (dy, dr))
        o32, g32 = M.run_with_grads(fn, M.cast(tensors, torch.float32), (dy.float(), dr.float()))
        assert len(o64) == (2 if pre else 1)
        named = [("y", o64[0], o32[0]), ("r", o64[1] if pre else None, o32[1] if pre else None), ("dx", g64[0], g32[0]),
                 ("dweight", g64[1], g32[1]), ("dbias", g64[2], g32[2])]
        for k, a64, a32 in named:
            for suffix in ("", "_f64"):
                key = f"norm_{shape}_{k}{suffix}"
                if key not in g14.files:
                    assert shape == "3x384"                                           # the wide shape keeps the fp32 y alone
                    continue
                rec = _t(g14, key)[i]
                if a64 is None:
                    assert bool(torch.isnan(rec).all())
                    continue
                assert rec.shape == a64.shape
                bad += _check(f"norm_{shape}_{case}", k + suffix, rec, a64, S.norm_err(a32, a64) if not suffix else None)
        if has_r:
            assert torch.equal(g64[3], g64[0])                                        # the record asserts the same of the reference
    assert not bad, bad


def test_norm_inputs_tell_eps_and_the_variance_apart(g14):
    """eps = 1e-5 is invisible at O(1) rows, so the rows are scaled down until the mean square is of eps's size."""
    x, w = 3e-3 * _t(g14, "norm_5x24_x"), _t(g14, "norm_5x24_weight")
    eps = float(g14["eps"])
    for rms in (False, True):
        want = M.layer_norm(x, w, None, None, eps, False, rms)
        c = x if rms else x - x.mean(-1, keepdim=True)
        outside = c / (torch.sqrt((c * c).mean(-1, keepdim=True)) + eps) * w
        assert S.norm_err(outside, want) > 1e-2
    assert S.norm_err(M.layer_norm(x, w, None, None, eps, False, True), M.layer_norm(x, w, None, None, eps, False, False)) > 1e-2


# ---- 4. the mixers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,L", [("v4", 129), ("v2", 129), ("none", 129), ("slow", 129), ("v4", 257)])
def test_mixer_restatement_is_the_reference(g14, kind, L):
    w, ops = X.mix_weights(g14), X.restated_ops()
    hidden, cot = _t(g14, "mix_hidden")[:, :L], _t(g14, "mix_cot")[:, :L]
    tag = f"mix_{kind}" + ("_L257" if L == 257 else "")
    o64, g64 = X.mixer_run(ops, w, hidden, cot, kind)
    o32, g32 = X.mixer_run(ops, w, hidden, cot, kind, dtype=torch.float32)
    assert o64.shape == (2, L, 24)
    bad = _check(tag, "out", _t(g14, tag + "_out"), o64, S.norm_err(o32, o64))
    if tag + "_dhidden" in g14.files:
        bad += _check(tag, "dhidden", _t(g14, tag + "_dhidden"), g64["hidden"], S.norm_err(g32["hidden"], g64["hidden"]))
    for k in X.MIX_WEIGHTS:
        if kind in ("none", "slow") and (k.endswith("_b") or "_b." in k or k == "A_b_log"):
            assert g64[k] is None                                                     # the one-directional paths leave the second set alone
        if f"{tag}_g_{k}" in g14.files:
            bad += _check(tag, "d" + k, _t(g14, f"{tag}_g_{k}"), g64[k], S.norm_err(g32[k], g64[k]))
    assert not bad, bad


def test_mixer_records_tell_the_variants_apart(g14):
    """v4 against v2 on the same weights, and each with the other's axis, differ by > 1e-2, in the records and in the restatement."""
    assert S.norm_err(_t(g14, "mix_v4_out"), _t(g14, "mix_v2_out")) > 1e-2
    w, ops = X.mix_weights(g14), X.restated_ops()
    hidden, cot = _t(g14, "mix_hidden")[:, :129], _t(g14, "mix_cot")[:, :129]
    for kind in ("v4", "v2"):
        right, _ = X.mixer_run(ops, w, hidden, cot, kind)
        wrong, _ = X.mixer_run(ops, w, hidden, cot, kind, flip_axis=-3 - X.FLIP_AXIS[kind])
        assert S.norm_err(wrong, right) > 1e-2
        assert S.norm_err(_t(g14, f"mix_{kind}_out"), wrong) > 1e-2
    assert S.norm_err(_t(g14, "mix_none_out"), _t(g14, "mix_v2_out")) > 1e-2
    assert S.norm_err(_t(g14, "mix_slow_out"), _t(g14, "mix_none_out")) < 1e-5             # the slow path is the same function


# ---- 5. the blocks -----------------------------------------------------------------------------------------------------------------
def test_block_restatement_is_the_reference(g14):
    ops = X.restated_ops()
    o64, g64 = X.blocks_run(ops, g14)
    o32, g32 = X.blocks_run(ops, g14, dtype=torch.float32)
    bad = _check("block", "hidden", _t(g14, "block_hidden"), o64[0], S.norm_err(o32[0], o64[0]))
    bad += _check("block", "residual", _t(g14, "block_residual"), o64[1], S.norm_err(o32[1], o64[1]))
    bad += _check("block", "dhidden_in", _t(g14, "block_dhidden_in"), g64["hidden"], S.norm_err(g32["hidden"], g64["hidden"]))
    keys = [k for k in g14.files if k.startswith("block_g")]
    assert len(keys) == 18
    for key in keys:
        name = key[len("block_g"):].replace("_", ".", 1)                              # block_g1_mixer.D -> 1.mixer.D
        bad += _check("block", "d" + name, _t(g14, key), g64[name], S.norm_err(g32[name], g64[name]))
    assert not bad, bad
