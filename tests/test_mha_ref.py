"""Dense attention without a GPU: the header against the module's binding table, the library's refusals, the three CPU restatements
(tests/mha_ref.py) against what the reference's own Attention.forward computed (tests/golden/g19_dense_attention.npz, made by
tests/golden/make_g19_dense_attention.py), the tolerance record, and the Attention module's surface."""
import ctypes
import importlib
import json
import os
import re

import numpy as np
import pytest

import mha_ref as MR
from conftest import ROOT

_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)
# the reference Attention(384, num_heads=6)'s state_dict (openpoints/models/backbone/transformer.py), recorded as keys and shapes
REFERENCE_STATE = {"qkv.weight": (1152, 384), "proj.weight": (384, 384), "proj.bias": (384,)}


@pytest.fixture(scope="module")
def golden():
    return np.load(MR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def kernel_order(golden):
    """{case: (out, lse, dqkv)} of the fp32 restatement in the kernel's order, computed once."""
    out = {}
    for c in MR.CASES:
        o, lse = MR.forward_kernel_f32(golden[f"{c}_qkv"])
        out[c] = (o, lse, MR.backward_kernel_f32(golden[f"{c}_qkv"], golden[f"{c}_dout"], out=o, lse=lse))
    return out


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "unipre3d_mha.h")).read()
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


def test_header_and_binding_agree():
    mha = importlib.import_module("unipre3d_amd.mha")
    declared = _declared_functions()
    assert set(declared) == set(mha.EXPORTS) == {"u3d_mha_abi_version", "u3d_mha_fwd", "u3d_mha_bwd"}
    assert len(set(mha.EXPORTS)) == len(mha.EXPORTS)
    assert declared["u3d_mha_abi_version"][1] == []
    assert declared["u3d_mha_fwd"][1] == ["constfloat*", "float*", "float*"] + ["int"] * 4 + ["float", "void*"]
    assert declared["u3d_mha_bwd"][1] == ["constfloat*"] * 4 + ["float*"] + ["int"] * 4 + ["float", "void*"]
    handle = mha.load()
    bound_as = {"int": ctypes.c_int, "float": ctypes.c_float}
    for name, (ret, params) in declared.items():
        fn = getattr(handle, name)
        assert ret == "int" and fn.restype is ctypes.c_int, name
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for c_type, bound in zip(params, fn.argtypes):
            assert bound is (ctypes.c_void_p if c_type.endswith("*") else bound_as[c_type]), (name, c_type, bound)
    hdr = open(os.path.join(ROOT, "include", "unipre3d_mha.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (U3D_MHA_\w+) (\d+)", hdr, re.M)}
    assert consts == {"U3D_MHA_ABI_VERSION": mha.ABI_VERSION, "U3D_MHA_MAX_SEQLEN": mha.MAX_SEQLEN, "U3D_MHA_HEAD_DIM": mha.HEAD_DIM}
    assert handle.u3d_mha_abi_version() == 1 and mha.MAX_SEQLEN == 1024 and mha.HEAD_DIM == 64


def test_library_carries_no_switches():
    from unipre3d_amd import mha
    blob = open(mha.LIB_PATH, "rb").read()
    assert b"U3D_" not in blob and b"getenv" not in blob


def test_refusals_return_before_any_launch():
    """Every argument check returns before anything touches a device: the pointers below are never dereferenced."""
    from unipre3d_amd import mha
    lib = mha.load()
    null, one, off = ctypes.c_void_p(0), ctypes.c_void_p(256), ctypes.c_void_p(260)
    s = 0.125
    fwd = lambda p=(one, one, one), B=1, N=17, H=2, D=64, sc=s: lib.u3d_mha_fwd(*p, B, N, H, D, sc, null)
    bwd = lambda p=(one,) * 5, B=1, N=17, H=2, D=64, sc=s: lib.u3d_mha_bwd(*p, B, N, H, D, sc, null)
    for call, n in ((fwd, 3), (bwd, 5)):
        for k in range(n):
            for bad in (null, off):                     # each pointer: null, and 4 bytes past a 16-byte boundary
                args = [one] * n
                args[k] = bad
                assert call(tuple(args)) == 1, (n, k)
        assert call(B=0) == 1 and call(N=0) == 1 and call(H=0) == 1 and call(B=-1) == 1
        assert call(sc=0.0) == 1 and call(sc=-0.125) == 1 and call(sc=float("nan")) == 1 and call(sc=float("inf")) == 1
        assert call(D=16) == 2 and call(D=128) == 2 and call(D=63) == 2
        assert call(N=1025) == 2
        assert call(B=2**31 - 1, H=2**15, N=1024) == 2  # more workgroups than a grid holds


def test_golden_layout(golden):
    keys = ("qkv", "dout", "out64", "dqkv64", "yard_out", "yard_dqkv")
    assert [str(n) for n in golden["names"]] == list(MR.CASES)
    assert sorted(golden.files) == sorted(["names"] + [f"{c}_{k}" for c in MR.CASES for k in keys])
    shapes = {"object": (1, 129, 1), "one": (2, 1, 2), "odd17": (2, 17, 2), "sharp17": (1, 17, 1), "huge9": (1, 9, 1)}
    for c, (B, N, H) in shapes.items():
        assert golden[f"{c}_qkv"].dtype == np.float32 and golden[f"{c}_qkv"].shape == (B, N, 3, H, 64)
        assert golden[f"{c}_dout"].dtype == np.float32 and golden[f"{c}_dout"].shape == (B, N, H, 64)
        assert golden[f"{c}_out64"].dtype == np.float64 and golden[f"{c}_out64"].shape == (B, N, H, 64)
        assert golden[f"{c}_dqkv64"].dtype == np.float64 and golden[f"{c}_dqkv64"].shape == (B, N, 3, H, 64)
        assert golden[f"{c}_yard_out"].shape == () and golden[f"{c}_yard_dqkv"].shape == ()
    # what the gains are for: a probability of about 1 in sharp17, scores of tens and more in huge9
    p = np.exp(MR.default_scale() * np.einsum("bnhd,bmhd->bhnm", *(golden["sharp17_qkv"][:, :, i].astype(np.float64) for i in (0, 1)))
               - MR.forward_f64(golden["sharp17_qkv"])[1][..., None])
    assert p.max() > 0.999
    s = MR.default_scale() * np.einsum("bnhd,bmhd->bhnm", *(golden["huge9_qkv"][:, :, i].astype(np.float64) for i in (0, 1)))
    assert np.abs(s).max() > 30
    assert golden["one_yard_out"] == 0 and golden["one_yard_dqkv"] == 0
    assert os.path.getsize(MR.GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_mamba.npz"))


@pytest.mark.parametrize("case", MR.CASES)
def test_fp64_restatement_is_the_references_fp64(golden, case):
    qkv, dout = golden[f"{case}_qkv"], golden[f"{case}_dout"]
    out, lse = MR.forward_f64(qkv)
    assert MR.dist(out, golden[f"{case}_out64"]) <= 1e-12
    assert MR.dist(MR.backward_f64(qkv, dout), golden[f"{case}_dqkv64"]) <= 1e-12
    assert lse.shape == (qkv.shape[0], qkv.shape[3], qkv.shape[1]) and np.isfinite(lse).all()


@pytest.mark.parametrize("case", MR.CASES)
def test_reference_form_reproduces_the_yardsticks(golden, case):
    out, dqkv = MR.reference_form(golden[f"{case}_qkv"], golden[f"{case}_dout"])
    assert out.dtype == np.float32 and dqkv.dtype == np.float32
    assert MR.dist(out, golden[f"{case}_out64"]) == pytest.approx(float(golden[f"{case}_yard_out"]), rel=1e-6, abs=1e-12)
    assert MR.dist(dqkv, golden[f"{case}_dqkv64"]) == pytest.approx(float(golden[f"{case}_yard_dqkv"]), rel=1e-6, abs=1e-12)
    o64, g64 = MR.reference_form(golden[f"{case}_qkv"], golden[f"{case}_dout"], dtype="float64")
    assert MR.dist(o64, golden[f"{case}_out64"]) <= 1e-12 and MR.dist(g64, golden[f"{case}_dqkv64"]) <= 1e-12


def test_tolerance_record_is_the_rule(golden, kernel_order):
    """The floors are the kernel-order restatement's largest distances, measured here; every bar is 2 x yardstick + floor."""
    tol = MR.tolerance()
    assert [r["case"] for r in tol["cases"]] == list(MR.CASES)
    floors = {"out": 0.0, "dqkv": 0.0}
    for r in tol["cases"]:
        c = r["case"]
        o, _, g = kernel_order[c]
        d_out, d_g = MR.dist(o, golden[f"{c}_out64"]), MR.dist(g, golden[f"{c}_dqkv64"])
        assert r["out_restatement_f32"] == pytest.approx(d_out, rel=1e-6, abs=1e-12)
        assert r["dqkv_restatement_f32"] == pytest.approx(d_g, rel=1e-6, abs=1e-12)
        assert r["out_yardstick"] == float(golden[f"{c}_yard_out"]) and r["dqkv_yardstick"] == float(golden[f"{c}_yard_dqkv"])
        floors["out"], floors["dqkv"] = max(floors["out"], d_out), max(floors["dqkv"], d_g)
    assert tol["floors"]["out"] == pytest.approx(floors["out"], rel=1e-6) and tol["floors"]["dqkv"] == pytest.approx(floors["dqkv"], rel=1e-6)
    for r in tol["cases"]:
        bo, bg = MR.case_bars(r["case"], tol)
        assert r["out_bar"] == pytest.approx(bo, rel=1e-12) and r["dqkv_bar"] == pytest.approx(bg, rel=1e-12)
        assert bo == 2 * r["out_yardstick"] + tol["floors"]["out"] and bg == 2 * r["dqkv_yardstick"] + tol["floors"]["dqkv"]
        assert "out_kernel_worst" in r and "dqkv_kernel_worst" in r
        for k in ("out", "dqkv"):            # a recorded kernel figure is within its bar
            assert r[f"{k}_kernel_worst"] is None or r[f"{k}_kernel_worst"] <= r[f"{k}_bar"]
    # fp32 arithmetic: no floor above a few hundred ulps, none below the rounding of one product
    assert 1e-8 < tol["floors"]["out"] < 1e-5 and 1e-8 < tol["floors"]["dqkv"] < 1e-5


def test_kernel_order_lse_and_blocks(golden, kernel_order):
    """The online softmax over key blocks gives the row log-sum-exp of the plain form, at one block and at three."""
    for c in MR.CASES:
        lse64 = MR.forward_f64(golden[f"{c}_qkv"])[1]
        assert np.abs(kernel_order[c][1] - lse64).max() <= 1e-6 * max(1.0, np.abs(lse64).max()), c
    assert golden["object_qkv"].shape[1] > 2 * MR.BLOCK


def test_analytic_backward_against_finite_differences():
    rng = np.random.default_rng(3)
    qkv, dout = rng.uniform(-1, 1, (1, 5, 3, 2, 64)), rng.uniform(-1, 1, (1, 5, 2, 64))
    g = MR.backward_f64(qkv, dout)
    for idx in ((0, 0, 0, 0, 0), (0, 4, 1, 1, 63), (0, 2, 2, 0, 17), (0, 3, 0, 1, 5), (0, 1, 1, 0, 40)):
        e = np.zeros_like(qkv)
        e[idx] = 1e-6
        fd = ((MR.forward_f64(qkv + e)[0] - MR.forward_f64(qkv - e)[0]) * dout).sum() / 2e-6
        assert fd == pytest.approx(g[idx], rel=1e-6, abs=1e-9), idx


def test_attention_module_surface():
    import torch
    from unipre3d_amd import mha
    a = mha.Attention(384, num_heads=6)
    assert set(a.state_dict()) == {"qkv.weight", "proj.weight", "proj.bias"}
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == REFERENCE_STATE
    assert set(mha.Attention(384, num_heads=6, qkv_bias=True).state_dict()) == {"qkv.weight", "qkv.bias", "proj.weight", "proj.bias"}
    assert a.num_heads == 6 and a.scale == 64 ** -0.5 and mha.Attention(128, 2, qk_scale=0.5).scale == 0.5
    assert isinstance(a.proj_drop, torch.nn.Dropout) and mha.Attention(64, 1, proj_drop=0.25).proj_drop.p == 0.25
    # a reference state_dict (keys and shapes as recorded above) loads, strictly
    gen = torch.Generator().manual_seed(0)
    state = {k: torch.randn(*s, generator=gen) for k, s in REFERENCE_STATE.items()}
    assert a.load_state_dict(state, strict=True).missing_keys == []
    assert torch.equal(a.qkv.weight, state["qkv.weight"]) and torch.equal(a.proj.bias, state["proj.bias"])
    with pytest.raises(NotImplementedError, match="attn_drop"):
        mha.Attention(384, 6, attn_drop=0.1)
    for dim, heads in ((384, 8), (384, 12), (128, 8), (100, 3)):
        with pytest.raises(NotImplementedError, match="64"):
            mha.Attention(dim, heads)
    mha.Attention(512)          # the default 8 heads of 64


def test_python_surface_refuses_cpu_tensors():
    import torch
    from unipre3d_amd import mha
    with pytest.raises(RuntimeError):
        mha.attention_qkvpacked(torch.zeros(1, 5, 3, 2, 64))
    with pytest.raises(RuntimeError):
        mha.Attention(128, 2)(torch.zeros(1, 5, 128))


def test_tolerance_file_is_json_with_every_case():
    with open(MR.TOLERANCE) as f:
        tol = json.load(f)
    assert set(tol) >= {"unit", "rule", "floors", "cases", "kernel_worst_source"} and set(tol["floors"]) == {"out", "dqkv"}
