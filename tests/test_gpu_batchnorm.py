"""libunipre3d_batchnorm.so through unipre3d_amd.batchnorm on the device, against the reference's fp64 record
(tests/golden/g26_batchnorm.npz) and the fp64 restatement (tests/batchnorm_ref.py).

The rule (profiles/batchnorm/tolerance.json): unit max|x - fp64| / max|fp64| per quantity; bar = 2 x floor, the floor being the fp32
restatement's distance from the fp64 values.  A recorded case takes its own recorded bars.  A generated case takes the floor of the fp32
restatement on that very input (computed here on the CPU), not less than the largest recorded floor of the quantity.  Module tests
(BasicBlock, a fused SparseSequential) run the op-by-op form with torch's own batch_norm on the device next to the fused one and hold
the fused one to 2 x the op-by-op form's distance from fp64 + the recorded floor of y, the rule of the module cases of
profiles/feature_propagation/tolerance.json.  Every figure is printed before it is asserted."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import batchnorm_ref as R
import spconv_ref

pytestmark = pytest.mark.gpu

CONFIGS = [("none", False), ("none", True), ("relu", False), ("relu", True), ("gelu", False)]
WANT = {"y": "_y", "dx": "_dx", "dresidual": "_dresidual", "dgamma": "_dgamma", "dbeta": "_dbeta", "running_mean": "_rm1", "running_var": "_rv1"}


def _tol():
    return json.load(open(R.TOLERANCE))


def _device(d, *, training=True, momentum=0.1, eps=1e-3, act="none", res_grad=True, stat_reduce=None, offset=False, affine=True, track=True):
    """One forward + backward of batch_norm_act on the device -> numpy results (and the autograd node's saved tensors' shapes)."""
    from unipre3d_amd import batchnorm

    def place(a, grad=False):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if offset and t.dim() == 2:                            # the same rows 4 bytes off a 16-byte boundary
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
            buf[1:].copy_(t.flatten())
            t = buf[1:].view(t.shape)
            assert t.data_ptr() % 16 == 4
        return t.requires_grad_(True) if grad else t
    x, res = place(d["x"], True), place(d.get("residual"), res_grad)
    gamma, beta = (place(d["gamma"], True), place(d["beta"], True)) if affine else (None, None)
    rm, rv = (place(d["rm"]), place(d["rv"])) if track or not training else (None, None)
    nbt = torch.tensor(int(d.get("nbt", 3)), device="cuda") if track and training else None
    y = batchnorm.batch_norm_act(x, gamma, beta, rm, rv, nbt, training=training, momentum=momentum, eps=eps, act=act, residual=res,
                                 stat_reduce=stat_reduce)
    saved = [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None]
    y.backward(place(d["dy"]))
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    return dict(y=n(y), dx=n(x.grad), dresidual=None if res is None else n(res.grad), dgamma=None if gamma is None else n(gamma.grad),
                dbeta=None if beta is None else n(beta.grad), running_mean=n(rm), running_var=n(rv), nbt=None if nbt is None else int(nbt),
                saved=saved)


def _restate(d, dtype, *, training=True, momentum=0.1, eps=1e-3, act="none", wide=None, affine=True, track=True, stat_reduce=None):
    keep = track or not training
    f = R.forward(d["x"], d["gamma"] if affine else None, d["beta"] if affine else None, d["rm"] if keep else None, d["rv"] if keep else None,
                  int(d.get("nbt", 3)) if track and training else None, training=training, momentum=momentum, eps=eps, act=act,
                  residual=d.get("residual"), dtype=dtype, wide=wide, stat_reduce=stat_reduce)
    b = R.backward(f, d["dy"])
    out = dict(y=f["y"], dx=b["dx"], dresidual=b["dresidual"] if d.get("residual") is not None else None,
               dgamma=b["dgamma"] if affine else None, dbeta=b["dbeta"] if affine else None, running_mean=f["running_mean"],
               running_var=f["running_var"], nbt=f["nbt"])
    return out


def _inputs(N, C, seed, residual):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-2, 2, C)).astype(np.float32)
    return dict(x=x, gamma=rng.uniform(0.5, 1.5, C).astype(np.float32) * np.where(np.arange(C) % 5 == 3, -1, 1).astype(np.float32),
                beta=rng.uniform(-0.5, 0.5, C).astype(np.float32), rm=rng.uniform(-0.5, 0.5, C).astype(np.float32),
                rv=rng.uniform(0.5, 1.5, C).astype(np.float32), dy=rng.standard_normal((N, C)).astype(np.float32),
                residual=rng.standard_normal((N, C)).astype(np.float32) if residual else None)


def _hold(label, got, d, floors, skip=(), **kw):
    """The device's results against the fp64 restatement under 2 x max(recorded floor, this input's fp32-restatement floor)."""
    wide = False if kw.pop("offset", False) else None
    want, f32 = _restate(d, np.float64, wide=wide, **kw), _restate(d, np.float32, wide=wide, **kw)
    for q in R.QUANTITIES:
        if want[q] is None or q in skip:
            assert got[q] is None, (label, q)
            continue
        assert got[q] is not None and np.isfinite(got[q]).all(), (label, q)
        err, bar = R.rel(got[q], want[q]), 2 * max(floors[q], R.rel(f32[q], want[q]))
        print(f"{label} {q}: kernel {err:.3e} bar {bar:.3e}")
        assert err <= bar, (label, q, err, bar)
    assert got["nbt"] == want["nbt"], label


def test_golden_cases():
    g, tol = np.load(R.GOLDEN), {c["case"]: c for c in _tol()["cases"]}
    figures = {}
    for c in map(str, g["cases"]):
        d = dict(x=g[c + "_x"].astype(np.float32), gamma=g[c + "_gamma"].astype(np.float32), beta=g[c + "_beta"].astype(np.float32),
                 rm=g[c + "_rm0"].astype(np.float32), rv=g[c + "_rv0"].astype(np.float32), dy=g[c + "_dy"].astype(np.float32),
                 nbt=int(g[c + "_nbt0"]), residual=g[c + "_residual"].astype(np.float32) if c + "_residual" in g.files else None)
        training = bool(g[c + "_training"])
        got = _device(d, training=training, momentum=float(g["momentum"]), eps=float(g["eps"]), act=str(g[c + "_act"]))
        figures[c] = {}
        for q in R.QUANTITIES:
            if c + WANT[q] not in g.files:
                continue
            err = R.rel(got[q], g[c + WANT[q]])
            figures[c][q] = float(f"{err:.4g}")
            print(f"{c} {q}: kernel {err:.3e} floor {tol[c][q + '_floor']:.3e} bar {tol[c][q + '_bar']:.3e}")
        assert got["nbt"] == (int(g[c + "_nbt1"]) if training else None)          # (eval mode is given no count to advance)
    if os.environ.get("U3D_BN_FIGURES"):
        with open(os.environ["U3D_BN_FIGURES"], "w") as fh:
            json.dump(figures, fh)
    for c, row in figures.items():
        for q, err in row.items():
            assert err <= tol[c][q + "_bar"], (c, q, err, tol[c][q + "_bar"])


@pytest.mark.parametrize("C", [1, 3, 4, 32, 96, 100, 256, 1024])
def test_every_dispatch_class_at_its_smallest_shape(C):
    floors = _tol()["floors"]
    k = [1, 3, 4, 32, 96, 100, 256, 1024].index(C)
    for j, N in enumerate((2, 63, 64, 65)):
        act, residual = CONFIGS[(k + j) % 5]
        kw = dict(training=(k + j) % 4 != 3, momentum=(0.01, 0.1, None)[(k + j) % 3], act=act, affine=(k + 2 * j) % 5 != 4)
        d = _inputs(N, C, 100 * C + N, residual)
        got = _device(d, **kw)
        _hold(f"C={C} N={N} {act} res={residual} {kw}", got, d, floors, **kw)


@pytest.mark.parametrize("C,offset", [(4, False), (32, False), (100, False), (1024, False), (32, True), (256, True)])
def test_row_chunk_edges_and_the_scalar_path_of_an_offset_view(C, offset):
    from unipre3d_amd import batchnorm
    floors, ch = _tol()["floors"], batchnorm.row_chunk(C)
    assert ch == R.row_chunk(C) == batchnorm.load().u3d_bn_row_chunk(C)
    for j, N in enumerate((ch - 1, ch, ch + 1, 3 * ch + 5)):
        configs = CONFIGS if N > 3 * ch and C in (32, 100) else [CONFIGS[(j + C) % 5]]
        for act, residual in configs:
            d = _inputs(N, C, 7 * C + N, residual)
            kw = dict(act=act, momentum=0.01)
            _hold(f"C={C} N={N} offset={offset} {act} res={residual}", _device(d, offset=offset, **kw), d, floors, offset=offset, **kw)


def test_residual_without_grad_eval_without_parameter_grads_and_what_is_saved():
    from unipre3d_amd import batchnorm
    N, C = 300, 32
    d = _inputs(N, C, 5, True)
    floors = _tol()["floors"]
    for act in ("relu", "none"):
        got = _device(d, act=act, res_grad=False)
        assert got["dresidual"] is None
        _hold(f"no residual grad {act}", got, d, floors, skip=("dresidual",), act=act)
        assert got["saved"].count((N, C)) == (2 if act == "relu" else 1), got["saved"]       # x, and y for the ReLU mask only
    got = _device(dict(d, residual=None), act="gelu")
    assert got["saved"].count((N, C)) == 1
    # no running statistics: batch statistics in both modes, nothing to update; affine=False
    got = _device(d, act="relu", track=False, affine=False)
    _hold("no running stats, affine=False", got, d, floors, act="relu", track=False, affine=False)
    # eval mode with a frozen norm: only x asks for a gradient, so no reduce pass runs and dx = g * scale
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    t = lambda k: torch.from_numpy(d[k]).cuda()
    y = batchnorm.batch_norm_act(x, t("gamma"), t("beta"), t("rm"), t("rv"), None, training=False, momentum=0.1, eps=1e-3, act="relu",
                                 residual=t("residual"))
    y.backward(t("dy"))
    want = _restate(d, np.float64, training=False, act="relu")
    f32 = _restate(d, np.float32, training=False, act="relu")
    for q, v in (("y", y.detach()), ("dx", x.grad)):
        err, bar = R.rel(v.cpu().numpy(), want[q]), 2 * max(floors[q], R.rel(f32[q], want[q]))
        print(f"frozen eval {q}: kernel {err:.3e} bar {bar:.3e}")
        assert err <= bar


def test_structured_inputs():
    """A per-channel mean of 1000 with unit spread (sum x^2 - mean^2 would lose everything in fp32), one constant channel (var = 0) and a
    channel whose ReLU mask is all-off."""
    N, C = 700, 12
    floors = _tol()["floors"]
    d = _inputs(N, C, 9, True)
    rng = np.random.default_rng(10)
    d["x"] = (1000.0 + rng.standard_normal((N, C))).astype(np.float32)
    d["x"][:, 5] = 3.25                                        # constant channel
    d["beta"][7], d["gamma"][7] = -50.0, 0.5                   # pre-activation far below zero in every row
    d["residual"][:, 7] = np.abs(d["residual"][:, 7])
    for act, residual in (("relu", True), ("gelu", False), ("none", False)):
        dd = dict(d, residual=d["residual"] if residual else None)
        got = _device(dd, act=act, eps=1e-3, momentum=0.01)
        _hold(f"structured {act}", got, dd, floors, act=act, eps=1e-3, momentum=0.01)
        if act == "none":
            assert np.all(got["y"][:, 5] == d["beta"][5])                                         # x - mean is an exact zero there
        if act == "relu":
            assert np.all(got["y"][:, 7] == 0) and np.all(got["dx"][:, 7] == 0) and got["dgamma"][7] == 0 and got["dbeta"][7] == 0
            assert np.all(got["dresidual"][:, 7] == 0)


def test_thousands_of_chunks_against_torch_fp64():
    """The BasicBlock tail at (350000, 32): 2735 row chunks, six steps of the partial sum.  Against torch's own lines in fp64 on the CPU
    under the recorded bars (2 x the largest recorded floor): with f64 sums no quantity's error grows with N."""
    from unipre3d_amd import batchnorm
    N, C = 350000, 32
    bars = {q: 2 * v for q, v in _tol()["floors"].items()}
    g = torch.Generator().manual_seed(N + C)
    x0, r0, dy0 = torch.randn(N, C, generator=g) * 1.5 + 0.3, torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    w0, b0 = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5

    def run(dev, dt):
        x, r, w, b = (t.to(dev, dt).requires_grad_(True) for t in (x0, r0, w0, b0))
        rm, rv = torch.zeros(C, device=dev, dtype=dt), torch.ones(C, device=dev, dtype=dt)
        if dev == "cuda":
            y = batchnorm.batch_norm_act(x, w, b, rm, rv, None, training=True, momentum=0.01, eps=1e-3, act="relu", residual=r)
        else:
            y = F.relu(F.batch_norm(x, rm, rv, w, b, True, 0.01, 1e-3) + r)
        grads = torch.autograd.grad(y, (x, w, b, r), dy0.to(dev, dt))
        return [t.detach().double().cpu().numpy() for t in (y,) + grads + (rm, rv)]
    want = run("cpu", torch.float64)
    for q, a, b in zip(("y", "dx", "dgamma", "dbeta", "dresidual", "running_mean", "running_var"), run("cuda", torch.float32), want):
        err = R.rel(a, b)
        print(f"(350000, 32) tail {q}: kernel {err:.3e} bar {bars[q]:.3e}")
        assert err <= bars[q], q


def test_two_runs_are_bit_identical():
    d = _inputs(3 * R.row_chunk(96) + 17, 96, 21, True)
    a, b = _device(d, act="relu"), _device(d, act="relu")
    for q in R.QUANTITIES:
        assert a[q].tobytes() == b[q].tobytes(), q
    d = _inputs(5000, 3, 22, False)
    a, b = _device(d, act="gelu", momentum=None), _device(d, act="gelu", momentum=None)
    for q in ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
        assert a[q].tobytes() == b[q].tobytes(), q


def test_graph_capture_replays_the_training_step():
    from unipre3d_amd import batchnorm
    N, C = 2 * R.row_chunk(32) + 9, 32
    d = _inputs(N, C, 31, True)
    t = lambda k: torch.from_numpy(d[k]).cuda()

    def fresh():
        return dict(x=t("x").requires_grad_(True), res=t("residual").requires_grad_(True), gamma=t("gamma").requires_grad_(True),
                    beta=t("beta").requires_grad_(True), rm=t("rm"), rv=t("rv"), nbt=torch.tensor(3, device="cuda"), dy=t("dy"))

    def step(s):
        y = batchnorm.batch_norm_act(s["x"], s["gamma"], s["beta"], s["rm"], s["rv"], s["nbt"], training=True, momentum=None, eps=1e-3,
                                     act="relu", residual=s["res"])
        return (y,) + torch.autograd.grad(y, (s["x"], s["gamma"], s["beta"], s["res"]), s["dy"])
    e = fresh()
    eager = [step(e) for _ in range(3)][-1]
    torch.cuda.synchronize()
    s = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s)                                                # warm-up on a side stream (it moves the buffers: put them back)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s["rm"].copy_(t("rm")), s["rv"].copy_(t("rv")), s["nbt"].fill_(3)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(s)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
    assert torch.equal(s["rm"], e["rm"]) and torch.equal(s["rv"], e["rv"]) and int(s["nbt"]) == int(e["nbt"]) == 6
    # the buffers really moved three times, by the cumulative average whose factor is computed on the device (1e-6: three fp32 roundings)
    rm, rv, nbt = d["rm"], d["rv"], 3
    for _ in range(3):
        f = R.forward(d["x"], d["gamma"], d["beta"], rm, rv, nbt, training=True, momentum=None, eps=1e-3, act="relu", residual=d["residual"])
        rm, rv, nbt = f["running_mean"], f["running_var"], f["nbt"]
    assert R.rel(e["rm"].cpu().numpy(), rm) < 1e-6 and R.rel(e["rv"].cpu().numpy(), rv) < 1e-6 and R.rel(d["rm"], rm) > 1e-2


class _Hook:
    """stat_reduce for one of two halves: call k adds adds[k] (None: nothing) and records what it was given."""

    def __init__(self, adds):
        self.adds, self.seen = adds, []

    def __call__(self, block):
        k = len(self.seen)
        self.seen.append(block.clone())
        return block if self.adds[k] is None else block + self.adds[k]


def test_stat_reduce_two_halves_equal_the_full_batch():
    N, C = 2 * R.row_chunk(32) + 40, 32
    d = _inputs(N, C, 41, True)
    bars = {q: 2 * v for q, v in _tol()["floors"].items()}
    full = _device(d, act="relu")
    cut = R.row_chunk(32) + 11
    halves = [slice(0, cut), slice(cut, N)]
    part = lambda h: dict(d, x=d["x"][h], dy=d["dy"][h], residual=d["residual"][h])
    fwd = [_Hook([None, None]) for _ in halves]
    for h, hook in zip(halves, fwd):
        _device(part(h), act="relu", stat_reduce=hook)
    bwd = [_Hook([fwd[1 - i].seen[0], None]) for i in range(2)]
    for h, hook in zip(halves, bwd):
        _device(part(h), act="relu", stat_reduce=hook)
    got = [_device(part(h), act="relu", stat_reduce=_Hook([fwd[1 - i].seen[0], bwd[1 - i].seen[1]])) for i, h in enumerate(halves)]
    both = dict(y=np.concatenate([g["y"] for g in got]), dx=np.concatenate([g["dx"] for g in got]),
                dresidual=np.concatenate([g["dresidual"] for g in got]), dgamma=got[0]["dgamma"] + got[1]["dgamma"],
                dbeta=got[0]["dbeta"] + got[1]["dbeta"], running_mean=got[0]["running_mean"], running_var=got[1]["running_var"])
    for q, v in both.items():
        err = R.rel(v, full[q])
        print(f"two halves {q}: {err:.3e} bar {bars[q]:.3e}")
        assert err <= bars[q], q
    assert fwd[0].seen[0][0].item() == cut and bwd[1].seen[1][0].item() == N - cut             # each block starts with this half's row count


# ---- modules -------------------------------------------------------------------------------------------------------------------------------
def _bn_lines(bn, f, act=None, residual=None):
    """torch's own lines for one BatchNorm1d (+ add + ReLU) on the device, with the module's parameters and buffers."""
    if bn.training:
        bn.num_batches_tracked.add_(1)
    z = F.batch_norm(f, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)
    if residual is not None:
        z = z + residual
    return F.relu(z) if act == "relu" else F.gelu(z) if act == "gelu" else z


def _reference_block_forward(block, x):
    """spconv_unet_v1m1_base.py:87-104, op by op, with the block's own sparseconv modules."""
    residual = x
    out = block.conv1(x)
    out = out.replace_feature(_bn_lines(block.bn1, out.features))
    out = out.replace_feature(F.relu(out.features))
    out = block.conv2(out)
    out = out.replace_feature(_bn_lines(block.bn2, out.features))
    if len(block.proj) == 2:
        r = block.proj[0](residual)
        r = r.replace_feature(_bn_lines(block.proj[1], r.features))
    else:
        r = residual
    out = out.replace_feature(out.features + r.features)
    return out.replace_feature(F.relu(out.features))


def _module_step(g, name, module, forward):
    from unipre3d_amd import sparseconv
    sd = {k: torch.from_numpy(g[f"{name}_p_{k}"]) for k in map(str, g[f"{name}_keys"])}
    module.load_state_dict({k: v if k.endswith("num_batches_tracked") else v.float() for k, v in sd.items()})
    module.cuda().train(bool(g[f"{name}_training"]))
    module.zero_grad()
    x = torch.from_numpy(g[f"{name}_x"]).float().cuda().requires_grad_(True)
    st = sparseconv.SparseConvTensor(x, torch.from_numpy(g[f"{name}_indices"]).cuda(), list(g[f"{name}_spatial_shape"]), int(g[f"{name}_batch_size"]))
    out = forward(module, st)
    out.features.backward(torch.from_numpy(g[f"{name}_dout"]).float().cuda())
    torch.cuda.synchronize()
    res = {"out": out.features.detach(), "dx": x.grad}
    res.update({"d_" + k: p.grad for k, p in module.named_parameters()})
    res.update({"after_" + k: b for k, b in module.named_buffers() if b.is_floating_point()})
    return {k: R.rel(v.cpu().numpy(), g[f"{name}_{k}"]) for k, v in res.items()}, {k: int(b) for k, b in module.named_buffers() if not b.is_floating_point()}


def _hold_module(label, fused, plain, floor):
    for k, err in fused.items():
        print(f"{label} {k}: fused {err:.3e} op-by-op {plain[k]:.3e} bar {2 * plain[k] + floor:.3e}")
    for k, err in fused.items():
        assert err <= 2 * plain[k] + floor, (label, k, err, plain[k])


@pytest.mark.parametrize("name,cin,cout", [("block_same", 8, 8), ("block_proj", 6, 10)])
def test_basic_block_against_the_reference_forward_op_by_op(name, cin, cout):
    from unipre3d_amd import batchnorm
    g = np.load(R.GOLDEN)
    norm_fn = lambda c: nn.BatchNorm1d(c, eps=float(g["eps"]), momentum=float(g["momentum"]))
    block = batchnorm.BasicBlock(cin, cout, norm_fn=norm_fn, indice_key="k")
    plain, counts_p = _module_step(g, name, block, _reference_block_forward)
    fused, counts_f = _module_step(g, name, block, lambda m, st: m(st))
    assert counts_p == counts_f and all(v == 4 for v in counts_f.values())
    _hold_module(name, fused, plain, _tol()["floors"]["y"])


def test_fused_sparse_sequential_against_the_unfused_one():
    from unipre3d_amd import batchnorm, sparseconv
    rng = np.random.default_rng(51)
    n, cin, cout, shape, batch = 200, 6, 32, (7, 7, 7), 2
    cells = np.sort(rng.choice(batch * 343, size=n, replace=False))
    idx = np.stack(np.unravel_index(cells, (batch,) + shape), 1).astype(np.int32)
    x = (rng.standard_normal((n, cin)) + np.linspace(-1, 1, cin)).astype(np.float32)
    dout = rng.standard_normal((n, cout)).astype(np.float32)
    torch.manual_seed(52)
    stem = sparseconv.SparseSequential(sparseconv.SubMConv3d(cin, cout, kernel_size=5, padding=1, bias=False, indice_key="stem"),
                                       nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01), nn.ReLU())
    with torch.no_grad():
        stem[1].weight.uniform_(0.5, 1.5), stem[1].bias.uniform_(-0.3, 0.3), stem[1].running_mean.uniform_(-0.3, 0.3)
    state = {k: v.clone() for k, v in stem.state_dict().items()}
    # fp64 on the CPU: tests/spconv_ref.subm, then torch's BatchNorm1d and ReLU
    w64 = state["0.weight"].double().requires_grad_(True)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    bn64 = nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01).double()
    bn64.load_state_dict({k[2:]: (v if v.dtype == torch.int64 else v.double()) for k, v in state.items() if k.startswith("1.")})
    y64 = F.relu(bn64(spconv_ref.subm(x64, w64, None, spconv_ref.subm_table(idx, shape, 5))))
    y64.backward(torch.from_numpy(dout).double())
    want = {"out": y64.detach(), "dx": x64.grad, "d_0.weight": w64.grad, "d_1.weight": bn64.weight.grad, "d_1.bias": bn64.bias.grad,
            "after_1.running_mean": bn64.running_mean, "after_1.running_var": bn64.running_var}

    def run(module):
        module.load_state_dict(state)
        module.cuda().train()
        module.zero_grad()
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        out = module(sparseconv.SparseConvTensor(xt, torch.from_numpy(idx).cuda(), list(shape), batch))
        out.features.backward(torch.from_numpy(dout).cuda())
        torch.cuda.synchronize()
        res = {"out": out.features.detach(), "dx": xt.grad}
        res.update({"d_" + k: p.grad for k, p in module.named_parameters()})
        res.update({"after_" + k: b for k, b in module.named_buffers() if b.is_floating_point()})
        assert int(module[1].num_batches_tracked) == 1
        return {k: R.rel(v.cpu().numpy(), want[k].numpy()) for k, v in res.items()}
    plain = run(stem)
    assert batchnorm.fuse_norm_act(stem) == 1 and isinstance(stem[2], nn.Identity)
    _hold_module("stem", run(stem), plain, _tol()["floors"]["y"])
