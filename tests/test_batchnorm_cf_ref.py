"""The restatement of the channels-first fused BatchNorm (tests/batchnorm_cf_ref.py) against the reference's own modules recorded in fp64
(tests/golden/g27_pointmlp_blocks.npz), and the CPU surface of unipre3d_amd/batchnorm_cf.py: state_dict keys, bit-equality with the
unfused torch form on CPU tensors, the header against the binding table, every error.  No GPU."""
import copy
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import batchnorm_cf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tol():
    return json.load(open(R.TOLERANCE))


def test_the_record_is_complete():
    g = np.load(R.GOLDEN)
    assert list(map(str, g["modules"])) == ["pre_k24", "pre_k24_eval", "pcm_pre_k32", "pos", "cbr_l50", "res_groups", "cbr_gelu"]
    assert g["pre_k24_x"].shape == (2, 6, 24, 8) and g["pcm_pre_k32_x"].shape[:3] == (2, 5, 32) and g["pos_x"].shape == (2, 8, 40)
    assert g["cbr_l50_x"].shape == (2, 4, 50) and g["res_groups_x"].shape == (3, 8, 12) and str(g["cbr_gelu_act"]) == "gelu"
    assert "res_groups/net2.4" in map(str, g["cases"]) and not bool(g["pre_k24_eval_training"])
    pooled = [c for c in map(str, g["cases"]) if bool(g[c + "_pool"])]
    assert len(pooled) == 3
    for c in pooled:                                              # the margin the maker kept around every decision
        assert float(g[c + "_margin"]) >= 64 * float(g[c + "_dev"]) > 0
    assert os.path.getsize(R.GOLDEN) < 1 << 20


def test_restatement_against_the_recorded_norms():
    g, tol = np.load(R.GOLDEN), {c["case"]: c for c in _tol()["cases"]}
    assert sorted(tol) == sorted(map(str, g["cases"]))
    for c in map(str, g["cases"]):
        f64, f = R.norm_case(g, c, np.float64)
        f32, f_32 = R.norm_case(g, c, np.float32)
        if bool(g[c + "_pool"]):                                  # every recorded arg and mask, in fp64 and in fp32
            for ff in (f, f_32):
                assert np.array_equal(ff["arg"], g[c + "_arg"]) and np.array_equal(ff["mask"], g[c + "_mask"]), c
            assert np.allclose(f["y"], g[c + "_y"], rtol=0, atol=1e-12)
        for q in R.QUANTITIES:
            want = R.wanted(g, c, q)
            if want is None:
                assert f64[q] is None or q != "dresidual", (c, q)
                continue
            assert R.rel(f64[q], want) < 1e-12, (c, q, R.rel(f64[q], want))
            assert f32[q].dtype == np.float32 and R.rel(f32[q], want) <= tol[c][q + "_floor"] * (1 + 1e-9) < 1e-6, (c, q)
            assert tol[c][q + "_bar"] == 2 * tol[c][q + "_floor"]
        if bool(g[c + "_training"]):
            assert f["nbt"] == int(g[c + "_nbt1"]) == int(g[c + "_nbt0"]) + 1


def test_restated_modules_against_the_recorded_modules():
    g, tol = np.load(R.GOLDEN), {c["case"]: c for c in _tol()["module_cases"]}
    for m in map(str, g["modules"]):
        res64, tape = R.module_case(g, m, np.float64)
        res32, tape32 = R.module_case(g, m, np.float32)
        assert set(res64) == {k[len(m) + 1:] for k in g.files if k.startswith(m + "_") and k[len(m) + 1:len(m) + 3] in ("ou", "dx", "d_", "af")
                              and not k.startswith(m + "_eval")} - {"dout"}, m
        for k, v in res64.items():
            want = g[f"{m}_{k}"]
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(want)
            elif np.abs(want).max() < 1e-12:
                assert np.abs(v).max() < 1e-12 and np.abs(res32[k]).max() < 1e-4, (m, k)
            else:
                assert R.rel(v, want) < 1e-12, (m, k, R.rel(v, want))
                assert R.rel(res32[k], want) <= tol[m]["floors"][k] * (1 + 1e-9) < 2e-6, (m, k)
        for t in (tape, tape32):                                  # the pooled norm's decisions inside the module
            for bn, f in t.norms.items():
                if f["pool"]:
                    assert np.array_equal(f["arg"], g[f"{m}/{bn}_arg"]) and np.array_equal(f["mask"], g[f"{m}/{bn}_mask"]), (m, bn)


def test_decisions_override_the_restatement():
    rng = np.random.default_rng(5)
    x, dp = rng.standard_normal((4, 3, 6)), rng.standard_normal((4, 3))
    kw = dict(training=True, momentum=0.1, eps=1e-5, act="relu", pool=True)
    free = R.forward(x, None, None, **kw)
    arg = (free["arg"] + 1) % 6
    forced = R.forward(x, None, None, decisions=(arg, np.ones((4, 3), bool)), **kw)
    assert np.array_equal(forced["arg"], arg) and forced["mask"].all()
    assert np.array_equal(forced["pooled"], np.take_along_axis(free["y"], arg[:, :, None].astype(np.int64), 2)[:, :, 0])
    b = R.backward(forced, dp)
    assert (np.count_nonzero(b["dx"] - b["dx"].mean(2, keepdims=True), axis=2) > 0).all() and b["dresidual"] is None
    assert np.array_equal(R.from_groups(R.to_groups(dp[:4], 2), 2), dp[:4]) and R.to_groups(dp, 2).shape == (2, 3, 2)


def test_plan_restated_equals_the_library():
    from unipre3d_amd import batchnorm_cf
    for C in (1, 3, 4, 31, 32, 33, 128, 1024):
        for L in (1, 2, 3, 4, 5, 8, 16, 24, 32, 33, 64, 65, 100, 132, 256, 260, 1024, 2048):
            for aligned in (True, False):
                assert tuple(batchnorm_cf.plan(C, L, aligned)) == tuple(R.plan(C, L, aligned)), (C, L, aligned)
            assert batchnorm_cf.parts(1000, C, L) == R.parts(1000, C, L)
    assert tuple(batchnorm_cf.plan(128, 24))[:4] == (8, 32, 10, 4) and tuple(batchnorm_cf.plan(128, 32))[:4] == (8, 32, 8, 4)
    with pytest.raises(NotImplementedError):
        batchnorm_cf.plan(1025, 4)
    with pytest.raises(NotImplementedError):
        batchnorm_cf.parts(0, 4, 4)


def test_header_declarations_equal_the_binding_table():
    from unipre3d_amd import batchnorm_cf
    text = open(os.path.join(ROOT, "include", "unipre3d_batchnorm_cf.h")).read()
    body = text[text.index("#define U3D_BNCF_ABI_VERSION"):]
    decls = re.findall(r"^(?:int|long long) (u3d_bncf_\w+)\(([^;]*)\);", body, re.M | re.S)
    assert [n for n, _ in decls] == list(batchnorm_cf.EXPORTS)
    for name, args in decls:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(batchnorm_cf.SIGNATURES[name][1]), name
    assert int(re.search(r"#define U3D_BNCF_ABI_VERSION (\d+)", text).group(1)) == batchnorm_cf.ABI_VERSION
    assert int(re.search(r"#define U3D_BNCF_MAX_CHANNELS (\d+)", text).group(1)) == batchnorm_cf.MAX_CHANNELS
    assert "Non-finite inputs are outside the contract" in text


# ---- the module surface ---------------------------------------------------------------------------------------------------------------
def _fused_of(g, m):
    from unipre3d_amd import batchnorm_cf
    kind, sd = str(g[f"{m}_kind"]), {k: g[f"{m}_p_{k}"] for k in map(str, g[f"{m}_keys"])}
    act = str(g[f"{m}_act"])
    if kind == "ConvBNReLU1D":
        return batchnorm_cf.ConvBNReLU1D(4, 8, activation=act)
    if kind == "ConvBNReLURes1D":
        return batchnorm_cf.ConvBNReLURes1D(8, groups=2, res_expansion=0.5)
    if kind == "PosExtraction":
        return batchnorm_cf.PosExtraction(8, blocks=2)
    if "pcm" in m:
        return batchnorm_cf.PreExtraction(4, 8, blocks=1, bias=True, use_xyz=True, knn_grouper=False)
    assert "transfer.net.0.bias" not in sd
    return batchnorm_cf.PreExtraction(4, 8, blocks=2, bias=False, use_xyz=False)


def test_state_dict_keys_equal_the_recorded_lists():
    from unipre3d_amd import batchnorm_cf
    g = np.load(R.GOLDEN)
    for m in map(str, g["modules"]):
        mod = _fused_of(g, m)
        assert list(mod.state_dict()) == [str(k) for k in g[f"{m}_keys"]], m
        sd = {k: torch.from_numpy(g[f"{m}_p_{k}"]) for k in map(str, g[f"{m}_keys"])}
        mod.load_state_dict({k: v if k.endswith("num_batches_tracked") else v.float() for k, v in sd.items()})       # the record's shapes
    block = batchnorm_cf.ConvBNReLURes1D(8, groups=2, res_expansion=0.5)
    assert [type(c).__name__ for c in block.net2] == ["Conv1d", "BatchNormActCF", "Identity", "Conv1d", "BatchNormActCF"]
    assert [n for n, _ in block.named_children()] == ["act", "net1", "net2"] and isinstance(block.act, nn.Identity)
    assert [n for n, _ in batchnorm_cf.PreExtraction(4, 8).named_children()] == ["transfer", "operation"]
    assert isinstance(batchnorm_cf.ConvBNReLU1D(4, 8).net[2], nn.Identity) and isinstance(batchnorm_cf.ConvBNReLU1D(4, 8).net[0], nn.Conv1d)
    for kw in (dict(), dict(affine=False), dict(track_running_stats=False)):
        assert list(batchnorm_cf.BatchNormActCF(7, act="gelu", **kw).state_dict()) == list(nn.BatchNorm1d(7, **kw).state_dict())
    for bad in ("silu", "leakyrelu", "hardswish"):
        with pytest.raises(NotImplementedError):
            batchnorm_cf.ConvBNReLU1D(4, 8, activation=bad)
    with pytest.raises(NotImplementedError, match="gelu"):
        batchnorm_cf.ConvBNReLURes1D(8, activation="gelu")
    with pytest.raises(NotImplementedError, match="gelu"):
        batchnorm_cf.PosExtraction(8, activation="gelu")


def _step(module, x, dout):
    xi = x.clone().requires_grad_(True)
    out = module(xi)
    out.backward(dout)
    return [out.detach(), xi.grad] + [p.grad for p in module.parameters()] + list(module.buffers())


@pytest.mark.parametrize("name", ["pre_k24", "pre_k24_eval", "pcm_pre_k32", "pos", "cbr_l50", "res_groups", "cbr_gelu"])
def test_on_cpu_tensors_the_classes_and_fuse_pointmlp_blocks_give_the_unfused_bits(name):
    from unipre3d_amd import batchnorm_cf
    g = np.load(R.GOLDEN)
    plain = R.reference_module(g, name)
    holder = nn.Sequential(copy.deepcopy(plain))
    params, buffers = list(holder.parameters()), list(holder.buffers())
    assert batchnorm_cf.fuse_pointmlp_blocks(holder) == 1 and batchnorm_cf.fuse_pointmlp_blocks(holder) == 0
    assert type(holder[0]).__module__ == "unipre3d_amd.batchnorm_cf" and type(holder[0]).__name__ == str(g[name + "_kind"])
    assert all(a is b for a, b in zip(params, holder.parameters())) and all(a is b for a, b in zip(buffers, holder.buffers()))
    assert list(holder[0].state_dict()) == list(plain.state_dict()) and holder[0].training == plain.training
    assert not any(type(m) in (nn.BatchNorm1d, nn.ReLU, nn.GELU) for m in holder.modules())
    built = _fused_of(g, name)                                   # the class built by its own constructor, same state
    built.load_state_dict(plain.state_dict())
    built.train(plain.training)
    x, dout = torch.from_numpy(g[name + "_x"]).float(), torch.from_numpy(g[name + "_dout"]).float()
    want = _step(plain, x, dout)
    for module in (holder[0], built):
        got = _step(module, x, dout)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert R.rel(got[0].numpy(), g[name + "_out"]) < 2e-6


def test_from_norm_shares_state_and_carries_the_process_group_and_2d_inputs_go_to_batchnorm():
    from unipre3d_amd import batchnorm, batchnorm_cf
    sync = nn.SyncBatchNorm(4, eps=1e-3, momentum=0.01)
    sync.process_group = "group"
    new = batchnorm_cf.BatchNormActCF.from_norm(sync, "relu")
    assert isinstance(new, batchnorm_cf.BatchNormActCF) and new.sync and new.process_group == "group" and new.weight is sync.weight
    assert new.running_var is sync.running_var and new.num_batches_tracked is sync.num_batches_tracked and (new.eps, new.momentum) == (1e-3, 0.01)
    plain = nn.BatchNorm1d(4)
    new = batchnorm_cf.BatchNormActCF.from_norm(plain, "relu")
    assert not new.sync and list(new.state_dict()) == list(plain.state_dict())
    x = torch.randn(6, 4)
    a = new(x, torch.ones(6, 4))
    b = batchnorm.BatchNormAct.from_norm(nn.BatchNorm1d(4), "relu")(x, torch.ones(6, 4))
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="pool"):
        new(x, pool="max")
    # three dimensions: torch's own lines, pooled into (B / S, C, S)
    x3 = torch.randn(6, 4, 5)
    want = F.relu(F.batch_norm(x3, None, None, new.weight, new.bias, True, 0.1, 1e-5))
    assert torch.equal(new(x3), want)
    got = new(x3, pool="max", pool_groups=3)
    assert got.shape == (2, 4, 3) and torch.equal(got, want.max(2).values.reshape(2, 3, 4).permute(0, 2, 1))
    pooled, arg = batchnorm_cf.batch_norm_act_cf(x3, None, None, None, None, training=True, momentum=0.1, eps=1e-5, pool="max", return_arg=True)
    assert arg.dtype == torch.int32 and torch.equal(pooled, torch.gather(F.batch_norm(x3, None, None, None, None, True), 2, arg.long()[:, :, None])[:, :, 0])


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def _call(x, C=None, **kw):
    from unipre3d_amd import batchnorm_cf
    C = x.shape[1] if C is None else C
    args = dict(training=True, momentum=0.1, eps=1e-5)
    args.update(kw)
    rm, rv = args.pop("rm", torch.zeros(C)), args.pop("rv", torch.ones(C))
    return batchnorm_cf.batch_norm_act_cf(x, args.pop("weight", torch.ones(C)), args.pop("bias", torch.zeros(C)), rm, rv, args.pop("nbt", None), **args)


def test_errors():
    from unipre3d_amd import batchnorm, batchnorm_cf
    x = torch.randn(6, 4, 5)
    with pytest.raises(NotImplementedError, match="dtype"):
        _call(x.double())
    with pytest.raises(NotImplementedError, match="dtype"):
        _call(x, weight=torch.ones(4, dtype=torch.float16))
    with pytest.raises(NotImplementedError, match="1024"):
        _call(torch.randn(2, 1025, 2))
    with pytest.raises(NotImplementedError, match="gelu"):
        _call(x, act="gelu", residual=torch.randn(6, 4, 5))
    with pytest.raises(NotImplementedError, match="tanh"):
        _call(x, act="tanh")
    with pytest.raises(NotImplementedError):
        batchnorm_cf.BatchNormActCF(4, act="gelu_tanh")
    with pytest.raises(NotImplementedError, match="pool"):
        _call(x, pool="avg")
    with pytest.raises(ValueError, match="contiguous"):
        _call(torch.randn(6, 5, 4).transpose(1, 2))
    with pytest.raises(ValueError, match="expected"):
        _call(x, residual=torch.randn(6, 4, 6))
    with pytest.raises(ValueError, match="expected"):
        _call(x, weight=torch.ones(5))
    with pytest.raises(ValueError, match="expected"):
        _call(torch.randn(6, 4), C=4)
    with pytest.raises(ValueError, match="pool_groups"):
        _call(x, pool="max", pool_groups=4)
    with pytest.raises(ValueError, match="pool_groups"):
        _call(x, pool_groups=2)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        _call(torch.randn(1, 4, 1))
    with pytest.raises(ValueError, match="running"):
        _call(x, training=False, rm=None, rv=None)
    with pytest.raises(ValueError, match="num_batches_tracked"):
        _call(x, momentum=None)
    with pytest.raises(ValueError, match="expected"):            # the 2-D function still refuses three dimensions
        batchnorm.batch_norm_act(x, None, None, None, None, training=True, momentum=0.1, eps=1e-5)
    # a non-contiguous residual is copied, not refused
    r = torch.randn(6, 5, 4).transpose(1, 2)
    assert torch.equal(_call(x, act="relu", residual=r), _call(x, act="relu", residual=r.contiguous()))
    # B L == 1 is fine in eval mode; B == 0 or L == 0 gives an empty tensor and leaves the running statistics alone
    assert _call(torch.randn(1, 4, 1), training=False).shape == (1, 4, 1)
    rm, rv, nbt = torch.full((4,), 0.25), torch.full((4,), 2.0), torch.tensor(5)
    for shape, kw, want in (((0, 4, 5), {}, (0, 4, 5)), ((3, 4, 0), {}, (3, 4, 0)), ((0, 4, 5), dict(pool="max"), (0, 4)),
                            ((0, 4, 5), dict(pool="max", pool_groups=3), (0, 4, 3))):
        out = _call(torch.empty(shape), rm=rm, rv=rv, nbt=nbt, **kw)
        assert out.shape == want and torch.equal(rm, torch.full((4,), 0.25)) and torch.equal(rv, torch.full((4,), 2.0)) and int(nbt) == 5
    assert torch.equal(_call(x, act="relu"), F.relu(F.batch_norm(x, None, None, torch.ones(4), torch.zeros(4), True, 0.1, 1e-5)))
