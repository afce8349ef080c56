"""unipre3d_amd's Mamba operators on the MI355X on the inputs tests/golden/g14_mamba.npz records, and driven as the two backbones' mixers
and PCM's block drive them (tests/mamba_mixer_ref.py with the product's functions): against the fp64 restatement, which
tests/test_mamba_golden.py holds to the backbones' own recorded results.

Tolerance (selective_scan_ref's docstring): per tensor max |got - f64| / max |f64| <= max(4 x the fp32 restatement's own figure, 4 ulp).
Every figure is printed before it is asserted.
"""
import pytest
import torch

import mamba_mixer_ref as X
import mambaops_ref as M
import selective_scan_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
_t = X._t


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_mamba.npz")


@pytest.fixture(scope="module")
def ops():
    from unipre3d_amd import causal_conv1d, selective_scan
    selective_scan.load()
    causal_conv1d.load()
    return X.product_ops()


def _check(case, name, got, want64, yardstick):
    err, b = S.norm_err(got, want64), S.bar(yardstick)
    print(f"[mamba_golden_gpu] {case} {name}: yardstick {yardstick:.3e} bar {b:.3e} device {err:.3e}")
    return [] if err <= b else [f"{case} {name}: {err:.3e} > {b:.3e}"]


def _check_all(case, dev, f64, f32):
    """dev, f64, f32: ([outs], {name: grad or None}) of the device, the arbiter and the yardstick run."""
    bad = []
    assert len(dev[0]) == len(f64[0])
    for i, (a, b, c) in enumerate(zip(dev[0], f64[0], f32[0])):
        assert a.shape == b.shape
        bad += _check(case, f"out{i}", a, b, S.norm_err(c, b))
    for k, b in f64[1].items():
        assert (dev[1][k] is None) == (b is None), k
        if b is not None:
            assert dev[1][k].shape == b.shape, k
            bad += _check(case, "d" + k, dev[1][k], b, S.norm_err(f32[1][k], b))
    assert not bad, bad


# ---- the operators on the recorded inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,tag,softplus,absent", X.SCAN_CASES, ids=[c[0] for c in X.SCAN_CASES])
def test_scan_on_recorded_inputs(g14, ops, case, tag, softplus, absent):
    t, dout = X.scan_inputs(g14, tag, softplus, absent)
    o64, g64, ys = S.yardstick_case(t, dout, delta_softplus=softplus)
    last64 = S.selective_scan(**t, delta_softplus=softplus, return_last_state=True)[1]
    last32 = S.selective_scan(**S.cast(t, torch.float32), delta_softplus=softplus, return_last_state=True)[1]
    td = S.cast(t, torch.float32, DEV)
    out, grads = S.run_with_grads(ops.selective_scan_fn, td, dout.float().to(DEV), delta_softplus=softplus)
    bad = _check("scan_" + case, "out", out, o64, ys["out"])
    for k in S.GRAD_NAMES:
        assert (grads[k] is None) == (t[k] is None), k
        if t[k] is not None:
            assert grads[k].shape == t[k].shape, k
            bad += _check("scan_" + case, "d" + k, grads[k], g64[k], ys[k])
    _, last = ops.selective_scan_fn(**td, delta_softplus=softplus, return_last_state=True)
    bad += _check("scan_" + case, "last_state", last, last64, S.norm_err(last32, last64))
    assert not bad, bad


@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_on_recorded_inputs(g14, ops, width):
    """x is the first half of the recorded (2, 12, 19) tensor, read in place; the unused half gets a zero gradient."""
    xz, w, b, dout = (_t(g14, k) for k in ("conv_x", f"conv_w{width}_weight", f"conv_w{width}_bias", f"conv_w{width}_dout"))
    for case in (str(c) for c in g14["conv_cases"]):
        act, has_b = (None if case.startswith("none") else "silu"), case.endswith("b1")
        t = {"xz": xz, "weight": w, "bias": b} if has_b else {"xz": xz, "weight": w}
        run = lambda fn, t: X.run_with_grads(lambda q: fn(q["xz"].chunk(2, dim=1)[0], q["weight"], q.get("bias"), act), t, (dout,))
        f64 = run(M.causal_conv1d, t)
        f32 = run(M.causal_conv1d, {k: v.float() for k, v in t.items()})
        dev = run(ops.causal_conv1d_fn, {k: v.float().to(DEV) for k, v in t.items()})
        assert float(dev[1]["xz"][:, 6:].abs().max()) == 0.0
        _check_all(f"conv_w{width}_{case}", dev, f64, f32)


@pytest.mark.parametrize("shape", ["5x24", "3x384"])
def test_norm_on_recorded_inputs(g14, ops, shape):
    """layer_norm_fn for LayerNorm and rms_norm_fn for RMSNorm, each with its own argument order."""
    eps = float(g14["eps"])
    x, w, b, res, dy, dr = (_t(g14, f"norm_{shape}_{k}") for k in ("x", "weight", "bias", "residual", "dy", "dr"))
    for case in (str(c) for c in g14["norm_cases"]):
        kind, r, bb, p = case.split("_")
        rms, pre = kind == "rms", p == "p1"
        t = {"x": x, "weight": w}
        t.update({"bias": b} if bb == "b1" else {})
        t.update({"residual": res} if r == "r1" else {})
        ref = lambda q: M.layer_norm(q["x"], q["weight"], q.get("bias"), q.get("residual"), eps, pre, rms)
        if rms:
            dev_fn = lambda q: ops.rms_norm_fn(q["x"], q["weight"], q.get("bias"), residual=q.get("residual"), prenorm=pre,
                                               residual_in_fp32=True, eps=eps)
        else:
            dev_fn = lambda q: ops.layer_norm_fn(q["x"], q["weight"], q.get("bias"), residual=q.get("residual"), eps=eps, prenorm=pre,
                                                 residual_in_fp32=True)
        f64 = X.run_with_grads(ref, t, (dy, dr))
        f32 = X.run_with_grads(ref, {k: v.float() for k, v in t.items()}, (dy, dr))
        dev = X.run_with_grads(dev_fn, {k: v.float().to(DEV) for k, v in t.items()}, (dy, dr))
        assert len(dev[0]) == (2 if pre else 1)
        _check_all(f"norm_{shape}_{case}", dev, f64, f32)


# ---- the mixers and the blocks, called as the backbones call them ------------------------------------------------------------------
_MIXER_REFERENCES = {}


def _mixer_case(g, kind, L):
    """(weights, hidden, cot, the fp64 run, the fp32 run) of the restated mixer, computed once."""
    if (kind, L) not in _MIXER_REFERENCES:
        w, hidden, cot = X.mix_weights(g), _t(g, "mix_hidden")[:, :L], _t(g, "mix_cot")[:, :L]
        restated = X.restated_ops()
        _MIXER_REFERENCES[kind, L] = (w, hidden, cot, X.mixer_run(restated, w, hidden, cot, kind),
                                      X.mixer_run(restated, w, hidden, cot, kind, dtype=torch.float32))
    return _MIXER_REFERENCES[kind, L]


@pytest.mark.parametrize("kind,L", [("v4", 129), ("v2", 129), ("none", 129), ("slow", 129), ("v4", 257)])
def test_mixer_as_the_backbones_call_it(g14, ops, kind, L):
    w, hidden, cot, (o64, g64), (o32, g32) = _mixer_case(g14, kind, L)
    od, gd = X.mixer_run(ops, w, hidden, cot, kind, device=DEV, dtype=torch.float32)
    assert set(gd) == set(X.MIX_WEIGHTS) | {"hidden"}
    _check_all(f"mix_{kind}_L{L}", ([od], gd), ([o64], g64), ([o32], g32))


def test_mixer_variants_are_told_apart(g14, ops):
    """v4 and v2 on the same weights differ by > 1e-2 (fp64, CPU), so do each kind's right and wrong flip axis, and the device's output
    is as far from the wrong-axis answer: a test that could not see the flip could not pass."""
    outs = {}
    for kind in ("v4", "v2"):
        w, hidden, cot, (o64, _), _ = _mixer_case(g14, kind, 129)
        wrong, _ = X.mixer_run(X.restated_ops(), w, hidden, cot, kind, flip_axis=-3 - X.FLIP_AXIS[kind])
        assert S.norm_err(wrong, o64) > 1e-2
        od, _ = X.mixer_run(ops, w, hidden, cot, kind, device=DEV, dtype=torch.float32)
        assert S.norm_err(od, wrong) > 1e-2 and S.norm_err(od, o64) < 1e-4
        outs[kind] = o64
    assert S.norm_err(outs["v4"], outs["v2"]) > 1e-2


def test_blocks_as_pcm_chains_them(g14, ops):
    restated = X.restated_ops()
    f64, f32 = X.blocks_run(restated, g14), X.blocks_run(restated, g14, dtype=torch.float32)
    dev = X.blocks_run(ops, g14, device=DEV, dtype=torch.float32)
    assert dev[0][0].shape == dev[0][1].shape == (2, 37, 24)
    _check_all("block", dev, f64, f32)


def test_v4_mixer_two_runs_are_bit_identical(g14, ops):
    w, hidden, cot, _, _ = _mixer_case(g14, "v4", 257)
    a = X.mixer_run(ops, w, hidden, cot, "v4", device=DEV, dtype=torch.float32)
    b = X.mixer_run(ops, w, hidden, cot, "v4", device=DEV, dtype=torch.float32)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
