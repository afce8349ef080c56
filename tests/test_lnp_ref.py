"""Local norm pooling without a GPU: the CPU restatements (tests/lnp_ref.py) against what the reference's own K_Norm + K_Pool and LNPBlock
computed (tests/golden/g20_lnp.npz, made by tests/golden/make_g20_lnp.py), the closed-form backward against autograd, the inverse lists,
the tolerance record, the header against the module's binding table, the library's refusals and the Python surface's argument checks."""
import ctypes
import importlib
import json
import os
import re

import numpy as np
import pytest

import lnp_ref as LR
from conftest import ROOT

_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)
SHAPES = {"object": (2, 128, 384, 4), "kg": (1, 5, 8, 5), "tiny": (2, 16, 8, 4), "k8": (1, 16, 12, 8), "sharp": (1, 16, 12, 4),
          "huge": (1, 16, 12, 4)}
BLOCK_KEYS = ("lga.affine_alpha_feat", "lga.affine_beta_feat", "mlp.share_mlp.weight", "mlp.share_mlp.bias", "pre_norm_ft.weight",
              "pre_norm_ft.bias")


@pytest.fixture(scope="module")
def golden():
    return np.load(LR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def kernel_order(golden):
    """{case: {quantity: fp32 array}} of the restatement in the kernels' order, cut to the recorded channels, computed once."""
    res = {}
    for c in LR.CASES:
        x, idx, alpha, beta, dout, cols = LR.golden_case(golden, c)
        saved = LR.forward_kernel_f32(x, idx, alpha, beta)
        grads = LR.backward_kernel_f32(x, idx, alpha, beta, dout, saved=saved)
        res[c] = LR.recorded(dict(zip(LR.QUANTITIES, (saved[0],) + grads)), cols)
    return res


def block_forms(z, dtype="float64"):
    """The whole LNPBlock around a given operator, in torch on the CPU: returns run(op) -> (y, dfeat, {key: grad}) where
    op(x (B,G,C), alpha, beta) -> (B,G,2C)."""
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype)

    def run(op):
        w = {k: torch.from_numpy(z[f"block_w_{k}"]).to(dt).requires_grad_(True) for k in BLOCK_KEYS}
        feat = torch.from_numpy(z["block_feat"]).to(dt).requires_grad_(True)
        pooled = op(feat[:, 1:, :], w["lga.affine_alpha_feat"], w["lga.affine_beta_feat"])
        n = F.layer_norm(pooled, (pooled.shape[-1],), w["pre_norm_ft.weight"], w["pre_norm_ft.bias"])
        y = torch.cat((feat[:, :1, :], F.silu(F.linear(n, w["mlp.share_mlp.weight"].squeeze(-1), w["mlp.share_mlp.bias"]))), dim=1)
        (y * torch.from_numpy(z["block_dy"]).to(dt)).sum().backward()
        return y.detach().numpy(), feat.grad.numpy(), {k: v.grad.numpy() for k, v in w.items()}
    return run


def test_golden_layout(golden):
    assert [str(n) for n in golden["names"]] == list(LR.CASES) == list(SHAPES)
    for c, (B, G, C, K) in SHAPES.items():
        x, idx, alpha, beta, dout, cols = LR.golden_case(golden, c)
        assert x.dtype == np.float32 and x.shape == (B, G, C) and dout.dtype == np.float32 and dout.shape == (B, G, 2 * C)
        assert idx.dtype == np.int32 and idx.shape == (B, G, K) and idx.min() >= 0 and idx.max() < G
        assert alpha.shape == beta.shape == (2 * C,) and golden[f"{c}_center"].shape == (B, G, 3)
        n = C if cols is None else len(cols)
        assert golden[f"{c}_out64"].dtype == np.float64 and golden[f"{c}_out64"].shape == (B, G, 2 * n)
        assert golden[f"{c}_dx64"].shape == (B, G, n) and golden[f"{c}_dalpha64"].shape == golden[f"{c}_dbeta64"].shape == (2 * C,)
        assert np.array_equal(idx[:, :, 0], np.broadcast_to(np.arange(G), (B, G)))       # a centre's nearest neighbour is itself
    assert (golden["object_cols"] % 8 == np.arange(48) % 8).all() and [f for f in golden.files if f.endswith("_cols")] == ["object_cols"]
    # what the gains are for
    p = lambda c: np.exp(LR._parts_f64(*LR.golden_case(golden, c)[:4], LR.EPS)[8] - LR.forward_f64(*LR.golden_case(golden, c)[:4])[1][:, :, None])
    assert p("sharp").max() > 0.999999
    v = LR._parts_f64(*LR.golden_case(golden, "huge")[:4], LR.EPS)[8]
    assert 150 < np.abs(v).max() < 700
    with np.errstate(over="ignore", invalid="ignore"):
        assert not np.isfinite(LR.reference_form(*LR.golden_case(golden, "huge")[:4])).all()      # the plain fp32 form overflows there
    assert os.path.getsize(LR.GOLDEN) < 1 << 20


@pytest.mark.parametrize("case", LR.CASES)
def test_fp64_restatement_is_the_references_fp64(golden, case):
    x, idx, alpha, beta, dout, cols = LR.golden_case(golden, case)
    got = LR.recorded(dict(zip(LR.QUANTITIES, (LR.forward_f64(x, idx, alpha, beta)[0],) + LR.backward_f64(x, idx, alpha, beta, dout))), cols)
    for q in LR.QUANTITIES:
        assert LR.dist(got[q], golden[f"{case}_{q}64"]) <= 1e-12, q


def test_fp64_restatement_is_the_references_whole_block(golden):
    import torch
    x_idx = golden["tiny_idx"]

    class Op(torch.autograd.Function):          # the restatement as an operator: forward_f64 and the closed-form backward_f64
        @staticmethod
        def forward(ctx, x, a, b):
            ctx.save_for_backward(x, a, b)
            return torch.from_numpy(LR.forward_f64(x.detach().numpy(), x_idx, a.detach().numpy(), b.detach().numpy())[0])

        @staticmethod
        def backward(ctx, g):
            x, a, b = ctx.saved_tensors
            dx, da, db = LR.backward_f64(x.detach().numpy(), x_idx, a.detach().numpy(), b.detach().numpy(), g.numpy())
            return torch.from_numpy(dx), torch.from_numpy(da).view_as(a), torch.from_numpy(db).view_as(b)

    y, dfeat, grads = block_forms(golden)(Op.apply)
    assert LR.dist(y, golden["block_y64"]) <= 1e-12 and LR.dist(dfeat, golden["block_dfeat64"]) <= 1e-12
    for k in BLOCK_KEYS:
        assert LR.dist(grads[k], golden[f"block_g64_{k}"]) <= 1e-12, k
        assert golden[f"block_yard_{k}"].shape == () and golden[f"block_yard_{k}"] < 1e-5
    assert np.array_equal(golden["block_y64"][:, 0], golden["block_feat"][:, 0])         # the cls token passes through


@pytest.mark.parametrize("shape", [(2, 9, 8, 3), (1, 33, 12, 32), (3, 7, 4, 2)])
def test_closed_form_backward_is_autograd_of_the_op_by_op_form(shape):
    B, G, C, K = shape
    rng = np.random.default_rng(sum(shape))
    x, dout = rng.standard_normal((B, G, C)), rng.standard_normal((B, G, 2 * C))
    alpha, beta = rng.uniform(0.5, 2.0, 2 * C) * rng.choice([-1, 1], 2 * C), rng.standard_normal(2 * C)
    idx = rng.integers(0, G, (B, G, K))
    out, (dx, da, db) = LR.reference_form(x, idx, alpha, beta, dout, dtype="float64")
    assert LR.dist(LR.forward_f64(x, idx, alpha, beta)[0], out) <= 1e-13
    for got, want in zip(LR.backward_f64(x, idx, alpha, beta, dout), (dx, da, db)):
        assert LR.dist(got, want) <= 1e-12
    so, sg = LR.reference_form(x, idx, alpha, beta, dout, dtype="float64", stable=True)          # the max-subtracted form is the same function
    assert LR.dist(so, out) <= 1e-13 and all(LR.dist(a, b) <= 1e-12 for a, b in zip(sg, (dx, da, db)))


def test_constant_rows_give_zero_std_and_finite_gradients():
    x = np.full((1, 6, 8), 0.75)
    idx = np.random.default_rng(0).integers(0, 6, (1, 6, 3))
    alpha, beta, dout = np.linspace(0.5, 2, 16), np.linspace(-1, 1, 16), np.random.default_rng(1).standard_normal((1, 6, 16))
    out, _, mu, s = LR.forward_f64(x, idx, alpha, beta)
    assert s == 0 and mu == 0 and np.isfinite(out).all() and np.allclose(out[0, :, :8], beta[:8])
    for g in LR.backward_f64(x, idx, alpha, beta, dout):
        assert np.isfinite(g).all()
    for g in LR.backward_kernel_f32(x, idx, alpha, beta, dout):
        assert np.isfinite(g).all()


def test_tolerance_record_is_the_rule(golden, kernel_order):
    """The floors are the kernel-order restatement's largest distances, measured here; every bar is 2 x yardstick + floor, and the
    restatement lies within the bars."""
    tol = LR.tolerance()
    assert [r["case"] for r in tol["cases"]] == list(LR.CASES) and set(tol["floors"]) == set(LR.QUANTITIES)
    floors = {q: 0.0 for q in LR.QUANTITIES}
    for r in tol["cases"]:
        c = r["case"]
        assert r["shape_BGCK"] == list(SHAPES[c])
        for q in LR.QUANTITIES:
            d = LR.dist(kernel_order[c][q], golden[f"{c}_{q}64"])
            assert r[f"{q}_restatement_f32"] == pytest.approx(d, rel=1e-6, abs=1e-12), (c, q)
            assert r[f"{q}_yardstick"] == float(golden[f"{c}_yard_{q}"])
            floors[q] = max(floors[q], d)
    for q in LR.QUANTITIES:
        assert tol["floors"][q] == pytest.approx(floors[q], rel=1e-6)
        assert 1e-8 < tol["floors"][q] < 1e-5          # fp32 arithmetic: below a few hundred ulps, above the rounding of one product
    for r in tol["cases"]:
        bars = LR.case_bars(r["case"], tol)
        for q in LR.QUANTITIES:
            assert r[f"{q}_bar"] == pytest.approx(bars[q], rel=1e-12) and bars[q] == 2 * r[f"{q}_yardstick"] + tol["floors"][q]
            assert r[f"{q}_restatement_f32"] <= bars[q]
            assert f"{q}_kernel_worst" in r and (r[f"{q}_kernel_worst"] is None or r[f"{q}_kernel_worst"] <= bars[q])
    with open(LR.TOLERANCE) as f:
        assert set(json.load(f)) >= {"unit", "rule", "floors", "cases", "kernel_worst_source"}


def test_kernel_order_saves_lse_and_stats(golden):
    for c in LR.CASES:
        x, idx, alpha, beta, _, _ = LR.golden_case(golden, c)
        _, lse, (mu, s, r, c0) = LR.forward_kernel_f32(x, idx, alpha, beta)
        _, lse64, mu64, s64 = LR.forward_f64(x, idx, alpha, beta)
        assert lse.dtype == np.float32 and np.abs(lse - lse64).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(lse64).max()), c
        assert abs(s - s64) <= 2.0 ** -23 * s64 and abs(mu - mu64) <= 2.0 ** -23 * s64 and r == np.float32(1) / np.float32(s + np.float32(1e-5))
        assert c0 == pytest.approx(float(r) ** 2 / ((x.size * idx.shape[2] - 1) * float(s)), rel=1e-6)


def _graphs():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1, 1, (2, 40, 3))
    d2 = ((pts[:, :, None] - pts[:, None]) ** 2).sum(-1)
    knn = np.argsort(d2, axis=-1, kind="stable")[:, :, :6]
    hub = np.zeros((2, 12, 4), np.int64)
    hub[:, :, 0] = 3                                        # row 3 is everyone's neighbour; rows 1, 2, 4.. are nobody's
    hub[:, :, 1:] = np.array([3, 0, 11])
    dup = rng.integers(0, 9, (1, 9, 5))
    dup[:, :, 1] = dup[:, :, 0]
    dup[:, :, 4] = dup[:, :, 2]
    out_of_range = rng.integers(0, 7, (1, 7, 3))
    out_of_range[0, 2, 1], out_of_range[0, 5, 0], out_of_range[0, 0, 2] = -1, 7, 2 ** 31 - 1
    return {"knn": knn, "hub": hub, "duplicates": dup, "out_of_range": out_of_range}


@pytest.mark.parametrize("graph", ["knn", "hub", "duplicates", "out_of_range"])
def test_inverse_lists_are_a_permutation_with_ascending_lists(graph):
    idx = _graphs()[graph]
    B, G, K = idx.shape
    ptr, ent = LR.inverse_lists(idx)
    assert ptr.dtype == np.int32 and ent.dtype == np.int32 and ptr.shape == (B, G + 1) and ent.shape == (B, G * K)
    sidx = LR.sanitize(idx)
    for b in range(B):
        assert ptr[b, 0] == 0 and ptr[b, G] == G * K and (np.diff(ptr[b]) >= 0).all()
        assert sorted(ent[b].tolist()) == list(range(G * K))                  # every (g, k) exactly once
        for j in range(G):
            lst = ent[b, ptr[b, j]:ptr[b, j + 1]]
            assert (np.diff(lst) > 0).all() and (sidx[b].reshape(-1)[lst] == j).all(), (b, j)
    if graph == "hub":
        assert ptr[0, 4] - ptr[0, 3] == 2 * 12 and ptr[0, 2] == ptr[0, 1] == ptr[0, 3]
    if graph == "out_of_range":
        assert sidx[0, 2, 1] == 2 and sidx[0, 5, 0] == 5 and sidx[0, 0, 2] == 0


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "unipre3d_lnp.h")).read()
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
    lnp = importlib.import_module("unipre3d_amd.lnp")
    declared = _declared_functions()
    assert set(declared) == set(lnp.EXPORTS) == {"u3d_lnp_abi_version", "u3d_lnp_scratch_bytes", "u3d_lnp_neighbours", "u3d_lnp_fwd",
                                                 "u3d_lnp_bwd"}
    assert len(set(lnp.EXPORTS)) == len(lnp.EXPORTS)
    assert declared["u3d_lnp_abi_version"] == ("int", []) and declared["u3d_lnp_scratch_bytes"] == ("size_t", ["int"] * 5)
    assert declared["u3d_lnp_neighbours"][1] == ["constint32_t*", "int32_t*", "int32_t*", "int", "int", "int", "void*"]
    assert declared["u3d_lnp_fwd"][1] == (["constfloat*", "long long", "constint32_t*", "constfloat*", "constfloat*", "float*", "float*",
                                           "float*", "void*"] + ["int"] * 4 + ["float", "void*"])
    assert declared["u3d_lnp_bwd"][1] == (["constfloat*", "long long"] + ["constint32_t*"] * 3 + ["constfloat*"] * 6 + ["float*"] * 3
                                          + ["void*"] + ["int"] * 4 + ["void*"])
    handle = lnp.load()
    bound_as = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
    for name, (ret, params) in declared.items():
        fn = getattr(handle, name)
        assert fn.restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[ret], name
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for c_type, bound in zip(params, fn.argtypes):
            assert bound is (ctypes.c_void_p if c_type.endswith("*") else bound_as[c_type]), (name, c_type, bound)
    hdr = open(os.path.join(ROOT, "include", "unipre3d_lnp.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (U3D_LNP_\w+) (\d+)", hdr, re.M)}
    assert consts == {"U3D_LNP_ABI_VERSION": lnp.ABI_VERSION, "U3D_LNP_MAX_GROUPS": lnp.MAX_GROUPS, "U3D_LNP_MAX_K": lnp.MAX_K,
                      "U3D_LNP_MAX_CHANNELS": lnp.MAX_CHANNELS}
    assert handle.u3d_lnp_abi_version() == 1 and (lnp.MAX_GROUPS, lnp.MAX_K, lnp.MAX_CHANNELS) == (1024, 32, 512)


def test_library_carries_no_switches():
    from unipre3d_amd import lnp
    blob = open(lnp.LIB_PATH, "rb").read()
    assert b"U3D_" not in blob and b"getenv" not in blob


def test_scratch_query_is_host_arithmetic():
    from unipre3d_amd import lnp
    q = lnp.load().u3d_lnp_scratch_bytes
    assert q(2, 128, 4, 384, 0) == 64 * 16 and q(32, 128, 8, 384, 0) == 256 * 16            # one pair of doubles per workgroup, at most 256
    assert q(2, 128, 4, 384, 1) == 32 * (16 + 16 * 384) and q(32, 128, 8, 384, 1) == 512 * (16 + 16 * 384)
    assert q(1, 1, 2, 4, 0) == 16 and q(1, 1, 2, 4, 1) == 16 + 64
    for bad in ((0, 8, 4, 8), (1, 0, 4, 8), (1, 1025, 4, 8), (1, 8, 1, 8), (1, 8, 33, 8), (1, 8, 4, 6), (1, 8, 4, 516), (1, 8, 4, 0),
                (2 ** 13, 1024, 4, 8)):
        assert q(*bad, 0) == 0 and q(*bad, 1) == 0, bad
    assert q(2 ** 12, 1024, 4, 8, 0) == 256 * 16


def test_refusals_return_before_any_launch():
    """Every argument check returns before anything touches a device: the pointers below are never dereferenced."""
    from unipre3d_amd import lnp
    lib = lnp.load()
    null, one, off = ctypes.c_void_p(0), ctypes.c_void_p(256), ctypes.c_void_p(260)
    nbr = lambda p=(one,) * 3, B=1, G=8, K=4: lib.u3d_lnp_neighbours(*p, B, G, K, null)
    fwd = lambda p=(one,) * 8, B=1, G=8, K=4, C=8, xs=64, eps=1e-5: lib.u3d_lnp_fwd(p[0], xs, *p[1:], B, G, K, C, eps, null)
    bwd = lambda p=(one,) * 14, B=1, G=8, K=4, C=8, xs=64: lib.u3d_lnp_bwd(p[0], xs, *p[1:], B, G, K, C, null)
    for call, n in ((nbr, 3), (fwd, 8), (bwd, 14)):
        for k in range(n):
            for bad in (null, off):                     # each pointer: null, and 4 bytes past a 16-byte boundary
                args = [one] * n
                args[k] = bad
                assert call(tuple(args)) == 1, (n, k)
        assert call(B=0) == 1 and call(G=0) == 1 and call(K=0) == 1 and call(B=-1) == 1
        assert call(G=1025) == 2 and call(K=1) == 2 and call(K=33) == 2
        assert call(B=2 ** 13, G=1024) == 2             # more rows than the library takes
    for call in (fwd, bwd):
        assert call(C=0) == 1 and call(C=6) == 2 and call(C=516) == 2
        assert call(xs=63) == 1 and call(xs=60) == 1 and call(xs=66) == 1 and call(xs=-64) == 1          # overlapping, or off 16 bytes
    assert fwd(eps=-1e-5) == 1 and fwd(eps=float("nan")) == 1 and fwd(eps=float("inf")) == 1


def test_module_surface_and_state_dict():
    import torch
    from unipre3d_amd import lnp
    blk = lnp.LNPBlock(lga_out_dim=768, k_group_size=4, alpha=100, beta=1000, mlp_in_dim=768, mlp_out_dim=384, num_group=128)
    # the reference LNPBlock's state_dict at these arguments, recorded as keys and shapes
    want = {"lga.affine_alpha_feat": (1, 1, 1, 768), "lga.affine_beta_feat": (1, 1, 1, 768), "mlp.share_mlp.weight": (384, 768, 1),
            "mlp.share_mlp.bias": (384,), "pre_norm_ft.weight": (768,), "pre_norm_ft.bias": (768,)}
    assert {k: tuple(v.shape) for k, v in blk.state_dict().items()} == want and set(want) == set(BLOCK_KEYS)
    assert torch.equal(blk.lga.affine_alpha_feat, torch.ones(1, 1, 1, 768)) and torch.equal(blk.lga.affine_beta_feat, torch.zeros(1, 1, 1, 768))
    gen = torch.Generator().manual_seed(0)
    state = {k: torch.randn(*s, generator=gen) for k, s in want.items()}
    assert blk.load_state_dict(state, strict=True).missing_keys == []
    assert isinstance(blk.act, torch.nn.SiLU) and isinstance(blk.pre_norm_ft, torch.nn.LayerNorm) and blk.num_group == 128
    import inspect
    assert list(inspect.signature(lnp.LNPBlock.forward).parameters) == ["self", "center", "feat", "neighbours"]
    assert list(inspect.signature(lnp.LNPBlock.__init__).parameters) == ["self", "lga_out_dim", "k_group_size", "alpha", "beta", "mlp_in_dim",
                                                                          "mlp_out_dim", "num_group", "act_layer", "drop_path", "norm_layer"]


def test_argument_errors_raise_without_touching_a_device():
    import torch
    from unipre3d_amd import lnp
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lnp.neighbours(torch.zeros(1, 8, 3), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lnp.neighbours_from_idx(torch.zeros(1, 8, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="expected"):
        lnp.neighbours(torch.zeros(8, 3), 4)
    with pytest.raises(ValueError, match="expected"):
        lnp.neighbours_from_idx(torch.zeros(8, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="empty"):
        lnp.neighbours_from_idx(torch.zeros(1, 0, 4, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="dtype"):
        lnp.neighbours_from_idx(torch.zeros(1, 8, 4))
    for k in (1, 33):
        with pytest.raises(NotImplementedError, match="K="):
            lnp.neighbours_from_idx(torch.zeros(1, 8, k, dtype=torch.int32))
        with pytest.raises(NotImplementedError, match="k="):
            lnp.neighbours(torch.zeros(1, 64, 3), k)
    with pytest.raises(NotImplementedError, match="1024"):
        lnp.neighbours_from_idx(torch.zeros(1, 1025, 4, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="1024"):
        lnp.neighbours(torch.zeros(1, 1025, 3), 4)
    # local_norm_pool: a hand-made Neighbours on the CPU shows that the device check comes first, and nothing else is reached
    nb = lnp.Neighbours(torch.zeros(1, 8, 4, dtype=torch.int32), torch.zeros(1, 9, dtype=torch.int32), torch.zeros(1, 32, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8), nb, torch.ones(16), torch.zeros(16))
    with pytest.raises(ValueError, match="nb"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8), None, torch.ones(16), torch.zeros(16))
    a16, b16 = torch.ones(16), torch.zeros(16)
    with pytest.raises(ValueError, match="expected"):
        lnp.local_norm_pool(torch.zeros(8, 8), nb, a16, b16)
    with pytest.raises(ValueError, match="built for"):
        lnp.local_norm_pool(torch.zeros(1, 9, 8), nb, a16, b16)
    with pytest.raises(ValueError, match="int32"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8), lnp.Neighbours(nb.idx, nb.ptr.long(), nb.ent), a16, b16)
    with pytest.raises(ValueError, match="int32"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8), lnp.Neighbours(nb.idx, nb.ptr, nb.ent[:, :16]), a16, b16)
    with pytest.raises(ValueError, match="2C"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8), nb, torch.ones(8), b16)
    with pytest.raises(ValueError, match="contiguous"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8).transpose(1, 2), nb, a16, b16)
    with pytest.raises(ValueError, match="contiguous"):
        lnp.local_norm_pool(torch.zeros(1, 8, 16)[:, :, :8], nb, a16, b16)
    with pytest.raises(ValueError, match="eps"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8), nb, a16, b16, eps=-1.0)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError, match="dtype"):
            lnp.local_norm_pool(torch.zeros(1, 8, 8, dtype=dtype), nb, a16, b16)
    with pytest.raises(NotImplementedError, match="dtype"):
        lnp.local_norm_pool(torch.zeros(1, 8, 8), nb, a16.double(), b16)
    for c in (6, 516):
        with pytest.raises(NotImplementedError, match="C="):
            lnp.local_norm_pool(torch.zeros(1, 8, c), nb, torch.ones(2 * c), torch.zeros(2 * c))
    blk = lnp.LNPBlock(16, 4, 100, 1000, 16, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk(torch.zeros(1, 8, 3), torch.zeros(1, 9, 8))
