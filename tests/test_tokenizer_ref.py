"""The restatement of the group tokenizer (tests/tokenizer_ref.py) against the reference's own record (tests/golden/g24_tokenizer.npz,
recorded from the two `Encoder` classes of the reference on the CPU), the module's CPU path, its state_dict, the header against the
binding, and the `stat_reduce` hook on two ranks.  No GPU and no built library."""
import ctypes
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import tokenizer_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)


@pytest.fixture(scope="module")
def z():
    return np.load(TR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def w(z):
    return TR.weights(int(z["C"]))


def test_the_record_names_its_cases_and_the_recipe_reproduces_its_weights(z, w):
    assert tuple(str(n) for n in z["names"]) == TR.CASES and bool(z["classes_bit_identical"])
    assert float(z["eps"]) == TR.EPS and float(z["momentum"]) == TR.MOMENTUM and int(z["nbt0"]) == TR.NBT0
    np.testing.assert_allclose(TR.checksums(w), z["weight_checksums"], rtol=1e-12, atol=0)
    assert os.path.getsize(TR.GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(TR.GOLDEN), "g14_mamba.npz"))
    # nothing at its default: gamma != 1 (some negative), beta != 0, running mean != 0, running var != 1
    assert (w["g1"] < 0).any() and (w["g2"] < 0).any() and np.abs(w["be1"]).min() > 0 and (w["rv1"] > 0).all() and (w["rv2"] > 0).all()
    x = z["padded_x"]
    assert (x[:, :, x.shape[2] // 2:] == x[:, :, :1]).all()
    assert z["strided_x"].shape[1] == 3


@pytest.mark.parametrize("name", TR.CASES)
def test_restatement_fp64_against_every_recorded_quantity(z, w, name):
    x, dout, training = TR.golden_case(z, name)
    s = TR.forward(x, w, training=training)
    got = dict(TR.recorded(TR.backward(s, dout)), out=s["out"], **s["running"])
    ref = TR.record_of(z, name)
    for k in ("out", "x") + TR.PARAMS + TR.RUNNING:
        scale = float(np.abs(ref[TR.ZERO_IN_TRAINING[k]]).max()) if training and k in TR.ZERO_IN_TRAINING else None
        assert got[k].shape == ref[k].shape and TR.dist(got[k], ref[k], scale) < 1e-11, (k, TR.dist(got[k], ref[k], scale))
    assert s["nbt"] == int(z[f"{name}_nbt"]) == TR.NBT0 + int(training)
    if training:      # each of the three biases feeds only a BatchNorm: exact zeros up to rounding, on both sides
        for b, be in TR.ZERO_IN_TRAINING.items():
            assert np.abs(ref[b]).max() < 1e-10 * np.abs(ref[be]).max() and np.abs(got[b]).max() < 1e-10 * np.abs(ref[be]).max()


def test_fp32_restatement_in_the_kernels_order_sets_the_floors(z):
    with open(TR.TOLERANCE) as f:
        doc = json.load(f)
    rows = TR.floors(z)
    floors = {q: max(r[q] for r in rows.values()) for q in TR.QUANTITIES}
    print("floors", floors)
    assert set(doc["floors"]) == set(doc["bars"]) == set(TR.QUANTITIES)
    for q in TR.QUANTITIES:
        assert doc["bars"][q] == 2.0 * doc["floors"][q]
        # (f64 sums may differ in their last bit between numpy builds; that moves an fp32 result by an ulp at the most)
        assert 0.8 * doc["floors"][q] <= floors[q] <= 1.25 * doc["floors"][q], (q, floors[q], doc["floors"][q])
        assert 0 < floors[q] < 1e-5
    for row in doc["cases"]:
        for q in TR.QUANTITIES:
            assert row[f"{q}_yardstick"] == float(z[f"{row['case']}_yard_{q}"])


def test_module_keeps_the_reference_state_dict_and_layout(z):
    from unipre3d_amd.tokenizer import Encoder
    m = Encoder(int(z["C"]))
    assert list(m.state_dict().keys()) == [str(k) for k in z["state_keys"]]
    assert m.encoder_channel == int(z["C"])
    for seq in (m.first_conv, m.second_conv):
        assert [type(c) for c in seq] == [nn.Conv1d, nn.BatchNorm1d, nn.ReLU, nn.Conv1d]
    assert m.second_conv[3].out_channels == int(z["C"]) and m.second_conv[0].in_channels == 512


def test_convert_sync_batchnorm_keeps_keys_and_values(w):
    from unipre3d_amd.tokenizer import Encoder
    m = Encoder(40)
    m.load_state_dict(TR.state_dict(w), strict=True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    s = nn.SyncBatchNorm.convert_sync_batchnorm(m)
    assert isinstance(s.first_conv[1], nn.SyncBatchNorm) and isinstance(s.second_conv[1], nn.SyncBatchNorm)
    after = s.state_dict()
    assert list(after.keys()) == list(before.keys())
    for k in before:
        assert torch.equal(after[k], before[k]), k


@pytest.mark.parametrize("name", TR.CASES)
def test_module_cpu_path_equals_the_restatement(z, w, name):
    x, dout, training = TR.golden_case(z, name)
    m = TR.reference_module(int(z["C"]), w, torch.float64, training)
    out, grads, running, nbt = TR.reference_run(m, x, dout)
    s = TR.forward(x, w, training=training)
    ref = dict(TR.backward(s, dout), out=s["out"], **s["running"])
    d = TR.distances(dict(grads, out=out, **running), ref, training)
    assert max(d.values()) < 1e-11 and nbt == s["nbt"], d


def test_cumulative_average_momentum(w):
    """momentum=None: the factor is 1 / num_batches_tracked after the increment, as BatchNorm1d has it."""
    x = np.random.default_rng(5).uniform(-1, 1, (2, 2, 4, 3)).astype(np.float32)
    m = TR.reference_module(40, w, torch.float64, True)
    m.first_conv[1].momentum = m.second_conv[1].momentum = None
    _, _, running, nbt = TR.reference_run(m, x, np.ones((2, 2, 40), np.float32))
    s = TR.forward(x, w, training=True, momentum=None)
    assert nbt == s["nbt"] == TR.NBT0 + 1
    for k in TR.RUNNING:
        assert TR.dist(s["running"][k], running[k]) < 1e-12, k


# ---- the header and the binding ---------------------------------------------------------------------------------------------------
def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "unipre3d_tokenizer.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    out = {}
    for ret, name, params in _DECLARATION.findall(hdr):
        types = []
        for p in (q.strip() for q in params.split(",")):
            if p in ("", "void"):
                continue
            types.append(p[:p.rindex("*") + 1].replace(" ", "") if "*" in p else " ".join(p.split()[:-1]))
        assert name not in out, name
        out[name] = (" ".join(ret.split()), types)
    return out


def test_header_declares_exactly_the_exports_with_the_bound_types():
    tok = importlib.import_module("unipre3d_amd.tokenizer")
    declared = _declared_functions()
    assert set(declared) == set(tok.EXPORTS) and len(set(tok.EXPORTS)) == len(tok.EXPORTS) == 9
    ctype = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name, (ret, types) in declared.items():
        restype, argtypes = tok.SIGNATURES[name]
        assert restype is ctype[ret], name
        assert list(argtypes) == [ctypes.c_void_p if t.endswith("*") else ctype[t] for t in types], name
    hdr = open(os.path.join(ROOT, "include", "unipre3d_tokenizer.h")).read()
    for macro, value in (("U3D_TOK_ABI_VERSION", tok.ABI_VERSION), ("U3D_TOK_MAX_N", tok.MAX_N), ("U3D_TOK_MAX_CHANNELS", tok.MAX_CHANNELS),
                         ("U3D_TOK_FOLD1_FLOATS", tok.FOLD1_FLOATS), ("U3D_TOK_FOLD2_FLOATS", tok.FOLD2_FLOATS)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro


def test_tokenize_refuses_bad_arguments_before_touching_a_device(w):
    from unipre3d_amd import tokenizer
    params = [torch.from_numpy(w[k]) for k in TR.PARAMS]
    kw = dict(training=True, eps=1e-5, momentum=0.1)
    with pytest.raises(ValueError, match="more than 1 value"):
        tokenizer.tokenize(torch.zeros(1, 1, 1, 3), params, **kw)
    with pytest.raises(ValueError, match="n=257"):
        tokenizer.tokenize(torch.zeros(1, 1, 257, 3), params, **kw)
    with pytest.raises(ValueError, match="fp32 only"):
        tokenizer.tokenize(torch.zeros(1, 1, 4, 3, dtype=torch.float64), params, **kw)
    with pytest.raises(ValueError, match="running"):
        tokenizer.tokenize(torch.zeros(1, 1, 4, 3), params, training=False)
    with pytest.raises(RuntimeError, match="HIP device"):
        tokenizer.tokenize(torch.zeros(1, 1, 4, 3), params, **kw)


# ---- the hook on two ranks ----------------------------------------------------------------------------------------------------------
def two_rank_inputs():
    rng = np.random.default_rng(77)
    xa, xb = rng.uniform(-1, 1, (1, 3, 8, 3)).astype(np.float32), rng.uniform(-0.5, 1.5, (2, 3, 8, 3)).astype(np.float32)
    da, db = rng.uniform(-1, 1, (1, 3, 40)).astype(np.float32), rng.uniform(-1, 1, (2, 3, 40)).astype(np.float32)
    return xa, xb, da, db


def two_rank_restatement(w, dtype=np.float64):
    """[(state, grads) of rank A, of rank B], and the blocks each rank sent, in call order."""
    xa, xb, da, db = two_rank_inputs()

    def rank(x, dout):
        def fn(reduce):
            s = TR.forward(x, w, training=True, stat_reduce=reduce, dtype=dtype)
            return s, TR.backward(s, dout)
        return fn
    return TR.run_ranks([rank(xa, da), rank(xb, db)])


def test_two_ranks_with_the_hook_equal_one_process_on_the_joined_batch(w):
    xa, xb, da, db = two_rank_inputs()
    (ra, rb), sent = two_rank_restatement(w)
    assert [len(b) for b in sent[0]] == [len(b) for b in sent[1]] == [10, 1025, 1025, 257]
    m = TR.reference_module(40, w, torch.float64, True)
    out, grads, running, nbt = TR.reference_run(m, np.concatenate([xa, xb]), np.concatenate([da, db]))
    assert TR.dist(ra[0]["out"], out[:1]) < 1e-12 and TR.dist(rb[0]["out"], out[1:]) < 1e-12
    for k in TR.PARAMS:      # the ranks' gradients, summed, are autograd's on the joined batch
        scale = float(np.abs(grads[TR.ZERO_IN_TRAINING[k]]).max()) if k in TR.ZERO_IN_TRAINING else None
        assert TR.dist(ra[1][k] + rb[1][k], grads[k], scale) < 1e-11, k
    assert TR.dist(ra[1]["x"], grads["x"][:1]) < 1e-11 and TR.dist(rb[1]["x"], grads["x"][1:]) < 1e-11
    for k in TR.RUNNING:     # both ranks hold the joined batch's statistics
        assert TR.dist(ra[0]["running"][k], running[k]) < 1e-12 and TR.dist(rb[0]["running"][k], running[k]) < 1e-12, k
    # and without the hook rank A alone computes something else
    alone = TR.forward(xa, w, training=True)
    assert TR.dist(alone["out"], out[:1]) > 1e-3


@pytest.mark.parametrize("shape,training", [((1, 1, 2, 40), True), ((2, 2, 1, 40), True), ((1, 2, 3, 1), False)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_edge_shapes_have_their_own_cpu_measured_floor(shape, training):
    doc = TR.tolerance()
    assert set(doc["edge_cases"]) == {TR.edge_key(s, t) for s, t in TR.EDGE_MODES}
    row = doc["edge_cases"][TR.edge_key(shape, training)]
    floor = TR.edge_floor(shape, training)
    for q in TR.QUANTITIES:
        assert row["bars"][q] == 2.0 * max(row["floors"][q], doc["floors"][q])
        assert 0.8 * row["floors"][q] <= floor[q] <= 1.25 * row["floors"][q], (q, floor[q], row["floors"][q])


def test_relu_decisions_can_be_overridden_and_their_gap_is_measured(w):
    x, dout = TR.edge_inputs((2, 5, 24, 40))
    s = TR.forward(x, w, training=True)
    assert TR.mask_gap(s, s["mask1"], s["mask3"]) == 0.0
    r = int(s["arg4"][0, 0])                                                   # a row of group 0 that receives a gradient
    m3 = s["mask3"].copy()
    m3[r] = ~m3[r]
    t = TR.forward(x, w, training=True, mask3=m3)
    assert TR.mask_gap(s, s["mask1"], m3) == np.abs(s["pre3"][r]).max() / np.abs(s["pre3"]).max()
    assert np.array_equal(t["out"], s["out"])                                  # the forward does not depend on it
    g0, g1 = TR.backward(s, dout), TR.backward(t, dout)
    assert not np.array_equal(g0["W4"], g1["W4"]) or not np.array_equal(g0["x"], g1["x"]) or not np.array_equal(g0["W3"], g1["W3"])
