"""The pixel-sparse image branch without a GPU: the restatement (tests/image_fusion_ref.py) against golden G25 (the reference's
FeatureFusion on the reference's GroupNorm + 1x1 convolution, fp64), the closed-form backward against autograd, the wrong semantics held
at a distance, the tolerance record's arithmetic, and what of unipre3d_amd/image_fusion.py runs on the CPU: ImageConv's layout and dense
forward, and the error contract."""
import json
import os

import numpy as np
import pytest
import torch

import image_fusion_ref as IR
from conftest import ROOT

TOL = os.path.join(ROOT, "profiles", "image_fusion", "tolerance.json")


@pytest.fixture(scope="module")
def g25(golden):
    return golden("g25_image_fusion.npz")


@pytest.fixture(scope="module")
def restated(g25):
    """per case: the fp64 and the fp32 restatement of all five quantities, computed once"""
    out = {}
    for tag, cfg in IR.CASES.items():
        inp, sel = IR.case_inputs(tag), g25[f"{tag}_sel"]
        f64 = {"out": IR.forward(inp["map"], sel, inp, cfg["G"]), **IR.backward(inp["map"], sel, inp, cfg["G"], inp["cot"])}
        f32 = {"out": IR.forward32(inp["map"], sel, inp, cfg["G"]), **IR.backward32(inp["map"], sel, inp, cfg["G"], inp["cot"])}
        out[tag] = (inp, sel, f64, f32)
    return out


@pytest.mark.parametrize("tag", sorted(IR.CASES))
def test_inputs_are_the_recorded_ones(g25, tag):
    assert np.array_equal(IR.checksum(IR.case_inputs(tag)), g25[f"{tag}_checksum"])


@pytest.mark.parametrize("tag", sorted(IR.CASES))
def test_selection_of_the_record_is_the_projects(g25, tag):
    """sel of the record is what the scalar z-buffer restatement makes of the recorded camera points, and those are what the project's
    camera_points makes of the scene"""
    import fusion_ref
    from unipre3d_amd.fusion import FeatureFusion
    intr = g25[f"{tag}_intr"]
    cam = FeatureFusion.camera_points(torch.from_numpy(g25[f"{tag}_center"]), torch.from_numpy(g25[f"{tag}_c2w"])).numpy()
    assert np.array_equal(cam, g25[f"{tag}_cam"])
    _, sel, _ = fusion_ref.zbuffer_loop(cam, IR.case_inputs(tag)["map"], intr[0][0], intr[1][1], intr[0][2], intr[1][2])
    assert np.array_equal(sel, g25[f"{tag}_sel"])
    n_win = int((sel >= 0).sum())
    assert 0 < n_win < sel.size
    if tag == "nowin":
        assert not (sel[1] >= 0).any()


@pytest.mark.parametrize("tag", sorted(IR.CASES))
def test_restatement_equals_the_record(g25, restated, tag):
    """fp64 restatement against the reference's fp64 run: rounding of another order of summation only.  The const and offset cases
    amplify it (rstd up to 1000, a mean of 10 against a spread of 0.1), so the bound is 1e-11 and not 1e-14."""
    _, sel, f64, f32 = restated[tag]
    for q in IR.QUANTITIES:
        d = IR.distance(f64[q], g25[f"{tag}_{q}_f64"])
        print(tag, q, f"fp64 restatement {d:.2e}, fp32 restatement {IR.distance(f32[q], g25[f'{tag}_{q}_f64']):.2e}")
        assert d < 1e-11, (tag, q, d)
    lose = sel < 0
    assert not f32["out"][lose].any() and not np.signbit(f32["out"][lose]).any()


def test_tolerance_record_is_the_measured_floor(g25, restated):
    rec = json.load(open(TOL))
    floors = {q: max(IR.distance(restated[t][3][q], g25[f"{t}_{q}_f64"]) for t in IR.CASES) for q in IR.QUANTITIES}
    for q in IR.QUANTITIES:
        # (a maximum over rounding errors: another host's order of the f64 sums may move a rounded statistic, and the floor with it, a little)
        assert rec["floors"][q] == pytest.approx(floors[q], rel=0.05), q
        assert rec["bars"][q] == pytest.approx(2 * rec["floors"][q], rel=1e-12)
        assert 1e-8 < rec["bars"][q] < 1e-5, (q, rec["bars"][q])           # fp32 territory: a bar cannot have drifted to hide a wrong term
    assert [c["case"] for c in rec["cases"]] == list(IR.CASES)
    dims = [c for c in rec["cases"] if c["case"] == "dims"][0]
    for q in IR.QUANTITIES:                                              # two fp32 evaluations: the sparse bar + 2 x the dense path's own distance
        assert rec["dense32_against_sparse_bars"][q] == pytest.approx(rec["bars"][q] + 2 * dims[f"{q}_yardstick"], rel=1e-12)
        assert dims[f"{q}_yardstick"] == pytest.approx(IR.distance(g25[f"dims_{q}_f32"], g25[f"dims_{q}_f64"]), rel=1e-12)
    for name, e in rec["edge_cases"].items():
        for q in IR.QUANTITIES:
            assert e["bars"][q] == pytest.approx(2 * max(rec["floors"][q], e["floors"][q]), rel=1e-12), (name, q)


def test_backward_identity_against_autograd():
    """dW, dbias, dgamma, dbeta through S and s equal autograd's through the dense modules and the gather, in fp64"""
    rs = np.random.RandomState(7)
    B, N, Cin, G, Cout, H, W = 2, 9, 12, 3, 5, 4, 6
    x = rs.randn(B, Cin, H, W).astype(np.float32)
    p = {"gamma": rs.randn(Cin), "beta": rs.randn(Cin), "weight": rs.randn(Cout, Cin), "bias": rs.randn(Cout)}
    sel = rs.randint(-1, H * W, (B, N)).astype(np.int32)
    sel[0, 3] = sel[0, 2] = 5                                             # two rows on one pixel
    cot = rs.randn(B, N, Cout)
    conv = torch.nn.Sequential(torch.nn.GroupNorm(G, Cin, eps=IR.EPS), torch.nn.Conv2d(Cin, Cout, 1)).double()
    with torch.no_grad():
        for t, k in zip(conv.parameters(), ("gamma", "beta", "weight", "bias")):
            t.copy_(torch.from_numpy(p[k]).reshape(t.shape))
    dense = conv(torch.from_numpy(x).double()).reshape(B, Cout, H * W)
    mapped = torch.zeros(B, N, Cout, dtype=torch.float64)
    for b in range(B):
        for n in range(N):
            if sel[b, n] >= 0:
                mapped[b, n] = dense[b, :, int(sel[b, n])]
    grads = torch.autograd.grad((mapped * torch.from_numpy(cot)).sum(), list(conv.parameters()))
    got = IR.backward(x, sel, p, G, cot)
    assert IR.distance(IR.forward(x, sel, p, G), mapped.detach().numpy()) < 1e-13
    for t, k in zip(grads, ("dgamma", "dbeta", "dW", "dbias")):
        assert IR.distance(got[k], t.numpy().reshape(got[k].shape)) < 1e-13, k


@pytest.mark.parametrize("variant,tag", [("unbiased", "offset"), ("eps_outside", "const"), ("group_mod", "sq")])
def test_wrong_semantics_sit_far_from_the_record(g25, variant, tag):
    """The unbiased variance, eps outside the root and the channel's group taken as c % G each move some recorded quantity by 1e-2 or
    more: four orders of magnitude above the bars."""
    cfg, inp, sel = IR.CASES[tag], IR.case_inputs(tag), g25[f"{tag}_sel"]
    got = {"out": IR.forward(inp["map"], sel, inp, cfg["G"], variant=variant),
           **IR.backward(inp["map"], sel, inp, cfg["G"], inp["cot"], variant=variant)}
    d = {q: IR.distance(got[q], g25[f"{tag}_{q}_f64"]) for q in IR.QUANTITIES}
    print(variant, tag, d)
    assert max(d["out"], d["dW"], d["dgamma"]) >= 1e-2, d


def test_host_arithmetic_of_the_decomposition():
    assert IR.stats_chunks(128, 32, 128, 128) == 8 and IR.stats_chunks(12, 4, 5, 7) == 1 and IR.stats_chunks(128, 32, 46, 45) == 2
    assert IR.row_splits(64) == 1 and IR.row_splits(300) == 2 and IR.rows_per_split(300) == 160 and IR.row_splits(4096) == 16


# ---- product code on the CPU ------------------------------------------------------------------------------------------------------
def test_image_conv_has_the_reference_layout_and_dense_forward():
    from unipre3d_amd.image_fusion import ImageConv
    torch.manual_seed(3)
    ours = ImageConv(128, 384)
    theirs = torch.nn.Sequential(torch.nn.GroupNorm(32, 128, eps=1e-06), torch.nn.Conv2d(128, 384, kernel_size=1))   # gaussian_predictor.py:210-214
    assert isinstance(ours, torch.nn.Sequential) and ours[0].eps == 1e-6 and ours[0].num_groups == 32
    want = {k: tuple(v.shape) for k, v in theirs.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == want
    assert list(want) == ["0.weight", "0.bias", "1.weight", "1.bias"] and want["1.weight"] == (384, 128, 1, 1)
    holder = torch.nn.Module()
    holder.image_conv = ours
    assert list(holder.state_dict()) == ["image_conv.0.weight", "image_conv.0.bias", "image_conv.1.weight", "image_conv.1.bias"]
    ours.load_state_dict(theirs.state_dict())                            # a checkpoint loads unchanged
    x = torch.randn(2, 128, 6, 5)
    assert torch.equal(ours(x), theirs(x))
    small = ImageConv(12, 5, num_groups=3, eps=1e-5)
    assert small[0].num_groups == 3 and small[0].eps == 1e-5 and small[1].weight.shape == (5, 12, 1, 1)


def test_cpu_tensors_are_refused():
    from unipre3d_amd import image_fusion as IF
    conv = IF.ImageConv(8, 6, num_groups=2)
    x = torch.randn(2, 8, 4, 4)
    cam = torch.ones(2, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.deferred(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IF.sample_at_points(conv, x, cam, 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IF.group_stats(x, 2, 1e-6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # a dense tensor takes the inherited path, which has none either
        IF.FeatureFusion(torch.nn.Identity())(torch.zeros(2, 3, 0), torch.zeros(2, 3, 3), conv(x).detach(), torch.eye(4).repeat(2, 1, 1),
                                              np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]))
    with pytest.raises(ValueError):
        IF.group_stats(torch.randn(8, 4, 4), 2, 1e-6)
    assert issubclass(IF.FeatureFusion, __import__("unipre3d_amd.fusion", fromlist=["FeatureFusion"]).FeatureFusion)


def test_library_is_built_and_bound():
    """the header, the binding table and the built library name the same functions (no GPU: nothing is launched)"""
    import re
    from unipre3d_amd import image_fusion as IF
    hdr = open(os.path.join(ROOT, "include", "unipre3d_image_fusion.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(u3d_imgfus_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(IF.EXPORTS) and len(IF.EXPORTS) == 8
    lib = IF.load()
    assert lib.u3d_imgfus_abi_version() == IF.ABI_VERSION
    assert lib.u3d_imgfus_stats_chunks(128, 32, 128, 128) == IR.stats_chunks(128, 32, 128, 128) == 8
    assert lib.u3d_imgfus_stats_chunks(12, 5, 4, 4) == 0                  # Cin % G != 0
    for rows in (1, 64, 300, 4096, 10 ** 6):
        assert lib.u3d_imgfus_row_splits(rows) == IR.row_splits(rows)
    tok = __import__("unipre3d_amd.tokenizer", fromlist=["load"]).load()   # one split rule (csrc/u3d_mfma_tile.h) behind both exports
    for rows in (1, 255, 256, 257, 8192, 16384, 16385):
        assert lib.u3d_imgfus_row_splits(rows) == tok.u3d_tok_wgrad_splits(rows) == IR.row_splits(rows)
    assert lib.u3d_imgfus_stats_scratch_bytes(32, 128, 32, 128, 128) == 32 * 32 * 8 * 16
    assert lib.u3d_imgfus_backward_scratch_bytes(2, 128, 128, 384) < 1 << 20
    assert lib.u3d_imgfus_backward_scratch_bytes(2, 128, 128, 8193) == 0
    null = None
    assert lib.u3d_imgfus_stats(null, 1, 8, 2, 4, 4, 1e-6, null, null, null) == 1
    assert lib.u3d_imgfus_stats(null, 1, 8, 3, 4, 4, 1e-6, null, null, null) == 1
    assert lib.u3d_imgfus_rows_forward(*([null] * 7), 1, 1, 8, 2, 6, null, null) == 1
    assert lib.u3d_imgfus_rows_forward(*([null] * 7), 1, 1, 8, 2, 8193, null, null) == 2
    assert lib.u3d_imgfus_rows_backward(*([null] * 7), 1, 1, 8, 2, 6, *([null] * 6)) == 1


def test_a_missing_library_raises(tmp_path, monkeypatch):
    """no fallback: without libunipre3d_image_fusion.so the loader names the missing file"""
    from unipre3d_amd import _lib, image_fusion as IF
    IF.load()
    monkeypatch.setattr(_lib, "LIB_DIR", str(tmp_path))
    with pytest.raises(RuntimeError, match="no fallback") as e:
        IF.load()
    assert os.path.join(str(tmp_path), "libunipre3d_image_fusion.so") in str(e.value)
    monkeypatch.undo()
    assert IF.load().u3d_imgfus_abi_version() == IF.ABI_VERSION
