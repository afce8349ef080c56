"""The fused BatchNorm + activation + residual on the CPU: the two restatements of tests/batchnorm_ref.py against torch's own
BatchNorm1d (+ ReLU / GELU / add) in fp64 and against the reference's record (tests/golden/g26_batchnorm.npz); the module surface of
unipre3d_amd/batchnorm.py (BatchNormAct, BasicBlock, fuse_norm_act: state_dict keys, shared Parameters, bit-identical CPU lines) and every
error it raises.  The kernels themselves: tests/test_gpu_batchnorm.py.

Bounds.  fp64 restatement against torch fp64: 1e-12 (a few hundred roundings of 1.1e-16 in the sums of at most 300 rows).  fp32
restatement against torch fp64: 1e-6, i.e. about 16 roundings of 2^-24 relative to the largest value -- it only has to show that the
fp32 order computes the same function; the sharp figure is the recorded floor of profiles/batchnorm/tolerance.json, which the g26 test
holds it to."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import batchnorm_ref as R

ACTS = ("none", "relu", "gelu")


def _torch_fp64(x, gamma, beta, rm, rv, nbt, training, momentum, eps, act, residual, dy):
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64))
    xt, gt, bt, rt = t(x).requires_grad_(True), t(gamma), t(beta), t(residual)
    for p in (gt, bt, rt):
        if p is not None:
            p.requires_grad_(True)
    rmt, rvt = t(rm), t(rv)
    n = nbt
    factor = 0.0 if momentum is None else momentum
    if training and rmt is not None:
        n = nbt + 1
        if momentum is None:
            factor = 1.0 / n
    z = F.batch_norm(xt, rmt, rvt, gt, bt, training, factor, eps)
    if rt is not None:
        z = z + rt
    y = F.relu(z) if act == "relu" else F.gelu(z) if act == "gelu" else z
    y.backward(t(dy))
    g = lambda p: None if p is None else p.grad.numpy()
    return dict(y=y.detach().numpy(), dx=g(xt), dgamma=g(gt), dbeta=g(bt), dresidual=g(rt), running_mean=None if rmt is None else rmt.numpy(),
                running_var=None if rvt is None else rvt.numpy(), nbt=n)


def _inputs(N, C, seed, residual):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-2, 2, C)).astype(np.float32)
    return dict(x=x, gamma=rng.uniform(0.5, 1.5, C).astype(np.float32) * np.where(np.arange(C) % 5 == 3, -1, 1).astype(np.float32),
                beta=rng.uniform(-0.5, 0.5, C).astype(np.float32), rm=rng.uniform(-0.5, 0.5, C).astype(np.float32),
                rv=rng.uniform(0.5, 1.5, C).astype(np.float32), dy=rng.standard_normal((N, C)).astype(np.float32),
                residual=rng.standard_normal((N, C)).astype(np.float32) if residual else None)


def _compare(got_f, got_b, want, bound):
    for k in ("y", "running_mean", "running_var"):
        if want[k] is not None:
            assert R.rel(got_f[k], want[k]) <= bound, k
    for k in ("dx", "dgamma", "dbeta", "dresidual"):
        if want[k] is not None:
            assert R.rel(got_b[k], want[k]) <= bound, k
    assert got_f["nbt"] == want["nbt"]


@pytest.mark.parametrize("act,residual", [("none", False), ("none", True), ("relu", False), ("relu", True), ("gelu", False)])
@pytest.mark.parametrize("training,momentum", [(True, 0.01), (True, 0.1), (True, None), (False, 0.01)])
@pytest.mark.parametrize("dtype,bound", [(np.float64, 1e-12), (np.float32, 1e-6)], ids=["fp64", "fp32"])
def test_restatements_against_torch_fp64(act, residual, training, momentum, dtype, bound):
    N, C = 300, 10                                             # two row chunks at C = 10 would need 410 rows: see the next test
    d = _inputs(N, C, 7, residual)
    want = _torch_fp64(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], 3, training, momentum, 1e-3, act, d["residual"], d["dy"])
    f = R.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], 3, training=training, momentum=momentum, eps=1e-3, act=act,
                  residual=d["residual"], dtype=dtype)
    _compare(f, R.backward(f, d["dy"]), want, bound)


@pytest.mark.parametrize("dtype,bound", [(np.float64, 1e-12), (np.float32, 1e-6)], ids=["fp64", "fp32"])
@pytest.mark.parametrize("N,C,wide", [(R.row_chunk(64) * 5 + 3, 64, None), (R.row_chunk(64) * 5 + 3, 64, False), (700, 3, None), (40, 260, None)])
def test_restatements_over_several_chunks_affine_false_and_no_running_stats(N, C, wide, dtype, bound):
    d = _inputs(N, C, 11, True)
    want = _torch_fp64(d["x"], None, None, None, None, None, True, 0.1, 1e-5, "relu", d["residual"], d["dy"])
    f = R.forward(d["x"], None, None, training=True, momentum=0.1, eps=1e-5, act="relu", residual=d["residual"], dtype=dtype, wide=wide)
    _compare(f, R.backward(f, d["dy"]), want, bound)
    assert f["running_mean"] is None and f["nbt"] is None


def test_stat_reduce_hook_two_halves_equal_the_full_batch():
    d = _inputs(200, 8, 13, False)
    full = R.forward(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], 3, training=True, momentum=0.1, eps=1e-3, act="relu")
    fb = R.backward(full, d["dy"])
    halves, blocks = [slice(0, 90), slice(90, 200)], {}

    def run(me, other):
        calls = []

        def hook(block):                                       # phase k of this half + phase k of the other half
            calls.append(block)
            return block + blocks[other][len(calls) - 1]
        f = R.forward(d["x"][me], d["gamma"], d["beta"], d["rm"], d["rv"], 3, training=True, momentum=0.1, eps=1e-3, act="relu", stat_reduce=hook)
        return f, R.backward(f, d["dy"][me])
    for i, h in enumerate(halves):                             # each half's own blocks first (a hook that adds nothing)
        rec = []
        f = R.forward(d["x"][h], d["gamma"], d["beta"], d["rm"], d["rv"], 3, training=True, momentum=0.1, eps=1e-3, act="relu",
                      stat_reduce=lambda b: (rec.append(b), b)[1])
        blocks[i] = rec
    # the backward block of a half depends on the reduced forward statistics: run forward with the hook, then record the backward block
    for i, h in enumerate(halves):
        f = R.forward(d["x"][h], d["gamma"], d["beta"], d["rm"], d["rv"], 3, training=True, momentum=0.1, eps=1e-3, act="relu",
                      stat_reduce=lambda b, i=i: b + blocks[1 - i][0])
        rec = []
        f["stat_reduce"] = lambda b: (rec.append(b), b)[1]
        R.backward(f, d["dy"][h])
        blocks[i].append(rec[0])
    (f0, b0), (f1, b1) = run(halves[0], 1), run(halves[1], 0)
    assert R.rel(np.concatenate([f0["y"], f1["y"]]), full["y"]) < 1e-12
    assert R.rel(np.concatenate([b0["dx"], b1["dx"]]), fb["dx"]) < 1e-12
    assert R.rel(b0["dgamma"] + b1["dgamma"], fb["dgamma"]) < 1e-12 and R.rel(b0["dbeta"] + b1["dbeta"], fb["dbeta"]) < 1e-12
    assert R.rel(f0["running_var"], full["running_var"]) < 1e-12 and R.rel(f1["running_mean"], full["running_mean"]) < 1e-12


def _golden_case(g, c, dtype):
    res = g[c + "_residual"] if c + "_residual" in g.files else None
    f = R.forward(g[c + "_x"], g[c + "_gamma"], g[c + "_beta"], g[c + "_rm0"], g[c + "_rv0"], int(g[c + "_nbt0"]),
                  training=bool(g[c + "_training"]), momentum=float(g["momentum"]), eps=float(g["eps"]), act=str(g[c + "_act"]),
                  residual=res, dtype=dtype)
    b = R.backward(f, g[c + "_dy"])
    got = dict(y=f["y"], dx=b["dx"], dgamma=b["dgamma"], dbeta=b["dbeta"], running_mean=f["running_mean"], running_var=f["running_var"])
    if c + "_dresidual" in g.files:
        got["dresidual"] = b["dresidual"]
    return got, f


WANT = {"y": "_y", "dx": "_dx", "dresidual": "_dresidual", "dgamma": "_dgamma", "dbeta": "_dbeta", "running_mean": "_rm1", "running_var": "_rv1"}


def test_restatements_against_the_record():
    g = np.load(R.GOLDEN)
    tol = {c["case"]: c for c in json.load(open(R.TOLERANCE))["cases"]}
    assert sorted(tol) == sorted(str(c) for c in g["cases"])
    for c in map(str, g["cases"]):
        got64, f64 = _golden_case(g, c, np.float64)
        got32, _ = _golden_case(g, c, np.float32)
        assert f64["nbt"] == int(g[c + "_nbt1"])
        for q, v in got64.items():
            assert R.rel(v, g[c + WANT[q]]) < 1e-12, (c, q)
        for q, v in got32.items():
            # the recorded floor IS this figure (tools/batchnorm_tolerance.py); 1e-9 of slack for another numpy's exp / erf
            assert R.rel(v, g[c + WANT[q]]) <= tol[c][q + "_floor"] + 1e-9, (c, q)
            assert tol[c][q + "_bar"] == 2 * tol[c][q + "_floor"]


# ---- the module surface ----------------------------------------------------------------------------------------------------------------
class PointSequential(nn.Module):
    """A container in the manner of pointcept's: named children, run in order (no nn.Sequential subclass)."""

    def add(self, module, name):
        self.add_module(name, module)

    def forward(self, x):
        for m in self._modules.values():
            x = m(x)
        return x


def test_state_dict_keys_equal_the_recorded_lists():
    from unipre3d_amd import batchnorm, sparseconv
    g = np.load(R.GOLDEN)
    norm_fn = lambda c: nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)
    assert list(batchnorm.BasicBlock(8, 8, norm_fn=norm_fn, indice_key="k").state_dict()) == [str(k) for k in g["block_same_keys"]]
    block = batchnorm.BasicBlock(6, 10, norm_fn=norm_fn, indice_key="k")
    assert list(block.state_dict()) == [str(k) for k in g["block_proj_keys"]]
    assert [n for n, _ in block.named_children()] == ["proj", "conv1", "bn1", "relu", "conv2", "bn2"]
    assert block.bn1.eps == 1e-3 and block.bn2.momentum == 0.01 and (block.bn1.act, block.bn2.act, block.proj[1].act) == ("relu", "relu", "none")
    sd = {n: torch.from_numpy(g["block_proj_p_" + n]) for n in map(str, g["block_proj_keys"])}
    block.load_state_dict({n: v if n.endswith("num_batches_tracked") else v.float() for n, v in sd.items()})     # the record's own shapes
    stem = sparseconv.SparseSequential(sparseconv.SubMConv3d(3, 12, kernel_size=5, padding=1, bias=False, indice_key="stem"), norm_fn(12), nn.ReLU())
    assert batchnorm.fuse_norm_act(stem) == 1 and list(stem.state_dict()) == [str(k) for k in g["stem_relu_keys"]]
    plain = nn.BatchNorm1d(7)
    for kw in (dict(), dict(affine=False), dict(track_running_stats=False)):
        assert list(batchnorm.BatchNormAct(7, act="gelu", **kw).state_dict()) == list(nn.BatchNorm1d(7, **kw).state_dict())
    assert list(batchnorm.BatchNormAct.from_norm(plain, "relu").state_dict()) == list(plain.state_dict())


def _models():
    torch.manual_seed(3)
    seq = nn.Sequential(nn.Linear(5, 8), nn.BatchNorm1d(8, eps=1e-3, momentum=0.01), nn.ReLU(), nn.Linear(8, 8), nn.BatchNorm1d(8), nn.GELU(),
                        nn.Linear(8, 6), nn.BatchNorm1d(6, affine=False), nn.Linear(6, 6), nn.BatchNorm1d(6, momentum=None),
                        nn.GELU(approximate="tanh"))
    ps = PointSequential()
    for name, m in (("lin", nn.Linear(5, 8)), ("norm", nn.BatchNorm1d(8, eps=1e-3, momentum=0.01)), ("act", nn.GELU())):
        ps.add(m, name)
    return seq, ps


@pytest.mark.parametrize("which,count", [(0, 3), (1, 1)], ids=["sequential", "pointsequential"])
@pytest.mark.parametrize("training", [True, False])
def test_fuse_norm_act_on_the_cpu_is_bit_identical_and_shares_the_parameters(which, count, training):
    from unipre3d_amd import batchnorm
    plain, fused = _models()[which], _models()[which]
    params, buffers, keys = list(fused.parameters()), list(fused.buffers()), list(fused.state_dict())
    assert batchnorm.fuse_norm_act(fused) == count
    assert all(a is b for a, b in zip(params, fused.parameters())) and all(a is b for a, b in zip(buffers, fused.buffers()))
    assert list(fused.state_dict()) == keys
    if which == 0:
        kinds = [type(m).__name__ for m in fused]
        assert kinds == ["Linear", "BatchNormAct", "Identity", "Linear", "BatchNormAct", "Identity", "Linear", "BatchNormAct", "Linear",
                         "BatchNorm1d", "GELU"]                                                    # the tanh GELU pair is left alone
        assert [fused[i].act for i in (1, 4, 7)] == ["relu", "gelu", "none"]
    else:
        assert type(fused.norm).__name__ == "BatchNormAct" and fused.norm.act == "gelu" and isinstance(fused.act, nn.Identity)
    x = torch.randn(9, 5, generator=torch.Generator().manual_seed(5))
    outs = []
    for m in (plain, fused):
        m.train(training)
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        (y * torch.arange(y.numel()).reshape(y.shape)).sum().backward()
        outs.append([y.detach(), xi.grad] + [p.grad for p in m.parameters()] + list(m.buffers()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert batchnorm.fuse_norm_act(fused) == 0                 # nothing left to replace


def test_fuse_norm_act_keeps_syncbatchnorm_settings_and_other_containers():
    from unipre3d_amd import batchnorm
    sync = nn.Sequential(nn.SyncBatchNorm(4, eps=1e-3, momentum=0.01), nn.ReLU())
    weight = sync[0].weight
    assert batchnorm.fuse_norm_act(sync) == 1
    assert sync[0].sync and sync[0].weight is weight and sync[0].eps == 1e-3 and sync[0].momentum == 0.01 and sync[0].act == "relu"

    class Pool(nn.Module):                                     # norm and act in two places, as PTv3's SerializedPooling keeps them
        def __init__(self):
            super().__init__()
            self.norm, self.act = PointSequential(), PointSequential()
            self.norm.add(nn.BatchNorm1d(4), "0")
            self.act.add(nn.GELU(), "0")
    pool = Pool()
    assert batchnorm.fuse_norm_act(pool) == 1 and pool.norm._modules["0"].act == "none" and isinstance(pool.act._modules["0"], nn.GELU)
    assert batchnorm.fuse_norm_act(Pool(), sequential_types=()) == 0


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def _call(x, C=None, **kw):
    from unipre3d_amd import batchnorm
    C = x.shape[1] if C is None else C
    args = dict(training=True, momentum=0.1, eps=1e-5)
    args.update(kw)
    rm, rv = args.pop("rm", torch.zeros(C)), args.pop("rv", torch.ones(C))
    return batchnorm.batch_norm_act(x, args.pop("weight", torch.ones(C)), args.pop("bias", torch.zeros(C)), rm, rv, args.pop("nbt", None), **args)


def test_errors():
    from unipre3d_amd import batchnorm
    x = torch.randn(6, 4)
    with pytest.raises(NotImplementedError, match="dtype"):
        _call(x.double())
    with pytest.raises(NotImplementedError, match="dtype"):
        _call(x, weight=torch.ones(4, dtype=torch.float16))
    with pytest.raises(NotImplementedError, match="1024"):
        _call(torch.randn(2, 1025))
    with pytest.raises(NotImplementedError, match="gelu"):
        _call(x, act="gelu", residual=torch.randn(6, 4))
    with pytest.raises(NotImplementedError, match="tanh"):
        _call(x, act="tanh")
    with pytest.raises(NotImplementedError):
        batchnorm.BatchNormAct(4, act="gelu_tanh")
    with pytest.raises(ValueError, match="contiguous"):
        _call(torch.randn(4, 6).t())
    with pytest.raises(ValueError, match="contiguous"):
        _call(x, residual=torch.randn(4, 6).t())
    with pytest.raises(ValueError, match="expected"):
        _call(x, residual=torch.randn(6, 5))
    with pytest.raises(ValueError, match="expected"):
        _call(x, weight=torch.ones(5))
    with pytest.raises(ValueError, match="expected"):
        _call(torch.randn(2, 4, 3), C=4)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        _call(torch.randn(1, 4))
    with pytest.raises(ValueError, match="running"):
        _call(x, training=False, rm=None, rv=None)
    with pytest.raises(ValueError, match="num_batches_tracked"):
        _call(x, momentum=None)
    # N == 1 is fine in eval mode; N == 0 gives an empty tensor and leaves the running statistics alone
    assert _call(torch.randn(1, 4), training=False).shape == (1, 4)
    rm, rv, nbt = torch.full((4,), 0.25), torch.full((4,), 2.0), torch.tensor(5)
    out = _call(torch.empty(0, 4), rm=rm, rv=rv, nbt=nbt)
    assert out.shape == (0, 4) and torch.equal(rm, torch.full((4,), 0.25)) and torch.equal(rv, torch.full((4,), 2.0)) and int(nbt) == 5
    assert torch.equal(_call(x, act="relu"), F.relu(F.batch_norm(x, None, None, torch.ones(4), torch.zeros(4), True, 0.1, 1e-5)))
