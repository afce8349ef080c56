"""libunipre3d_batchnorm_cf.so through unipre3d_amd.batchnorm_cf on the device, against the reference's fp64 record
(tests/golden/g27_pointmlp_blocks.npz) and the fp64 restatement (tests/batchnorm_cf_ref.py).

The rule (profiles/batchnorm_cf/tolerance.json): unit max|x - fp64| / max|fp64| per quantity; bar = 2 x floor, the floor being the fp32
restatement's distance from the fp64 values.  A recorded case takes its own recorded bars, and its arg and mask must equal the record
everywhere.  A generated case takes the floor of the fp32 restatement on that very input (computed here on the CPU), not less than the
largest recorded floor of the quantity; a generated pooled case is held to the fp64 restatement under the device's own arg and mask,
and that choice must itself be admissible: the fp64 y at the device's arg lies within the y bar of the fp64 row maximum, and the mask
differs from fp64's only where |fp64 y| is within that bar of zero.  Module tests run the op-by-op form with torch's own layers on the
device next to the fused one and hold the fused one to 2 x the op-by-op form's distance from fp64 + the recorded floor of y.  Every
figure is printed before it is asserted."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import batchnorm_cf_ref as R

pytestmark = pytest.mark.gpu

CONFIGS = [("none", False), ("none", True), ("relu", False), ("relu", True), ("gelu", False)]
# 16: the groups of 4 x 4 and 16 x 1 floats; 132: 64 lanes of 4 floats in one sweep; 65 and 260: just over the reach of 64 lanes
LENGTHS = [1, 2, 3, 4, 5, 8, 16, 24, 32, 33, 64, 100, 132, 65, 260]


def _tol():
    return json.load(open(R.TOLERANCE))


def offset(t):
    """The same values 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.flatten())
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _device(d, *, training=True, momentum=0.1, eps=1e-5, act="none", pool=False, groups=1, res_grad=True, stat_reduce=None, off=False,
            affine=True, track=True):
    """One forward + backward of batch_norm_act_cf on the device -> numpy results (pooled and arg as (B, C)) and the saved shapes."""
    from unipre3d_amd import batchnorm_cf

    def place(a, grad=False):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if off and t.dim() == 3:
            t = offset(t)
        return t.requires_grad_(True) if grad else t
    x, res = place(d["x"], True), place(d.get("residual"), res_grad)
    gamma, beta = (place(d["gamma"], True), place(d["beta"], True)) if affine else (None, None)
    rm, rv = (place(d["rm"]), place(d["rv"])) if track or not training else (None, None)
    nbt = torch.tensor(int(d.get("nbt", 3)), device="cuda") if track and training else None
    out = batchnorm_cf.batch_norm_act_cf(x, gamma, beta, rm, rv, nbt, training=training, momentum=momentum, eps=eps, act=act, residual=res,
                                         pool="max" if pool else None, pool_groups=groups, stat_reduce=stat_reduce, return_arg=pool)
    y, arg = out if pool else (out, None)
    saved = [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None]
    dy = d["dy"] if not pool else R.to_groups(d["dpooled"], groups)
    y.backward(place(dy))
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    y, arg = n(y), n(arg)
    if pool:
        assert y.shape == arg.shape == ((x.shape[0], x.shape[1]) if groups == 1 else (x.shape[0] // groups, x.shape[1], groups))
        y, arg = R.from_groups(y, groups), R.from_groups(arg, groups)
    return dict(y=y, arg=arg, dx=n(x.grad), dresidual=None if res is None or not res_grad else n(res.grad),
                dgamma=None if gamma is None else n(gamma.grad), dbeta=None if beta is None else n(beta.grad), running_mean=n(rm),
                running_var=n(rv), nbt=None if nbt is None else int(nbt), saved=saved)


def _restate(d, dtype, *, training=True, momentum=0.1, eps=1e-5, act="none", pool=False, decisions=None, wide=None, affine=True, track=True,
             stat_reduce=None):
    keep = track or not training
    f = R.forward(d["x"], d["gamma"] if affine else None, d["beta"] if affine else None, d["rm"] if keep else None, d["rv"] if keep else None,
                  int(d.get("nbt", 3)) if track and training else None, training=training, momentum=momentum, eps=eps, act=act,
                  residual=d.get("residual"), pool=pool, decisions=decisions, dtype=dtype, wide=wide, stat_reduce=stat_reduce)
    b = R.backward(f, d["dpooled"] if pool else d["dy"])
    return dict(y=f["pooled"] if pool else f["y"], dense=f["y"], dx=b["dx"], dresidual=b["dresidual"], dgamma=b["dgamma"] if affine else None,
                dbeta=b["dbeta"] if affine else None, running_mean=f["running_mean"], running_var=f["running_var"], nbt=f["nbt"])


def _inputs(B, C, L, seed, residual):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x = (rng.standard_normal((B, C, L)) * rng.uniform(0.5, 2.0, (1, C, 1)) + rng.uniform(-2, 2, (1, C, 1))).astype(np.float32)
    return dict(x=x, gamma=rng.uniform(0.5, 1.5, C).astype(np.float32) * np.where(np.arange(C) % 5 == 3, -1, 1).astype(np.float32),
                beta=rng.uniform(-0.5, 0.5, C).astype(np.float32), rm=rng.uniform(-0.5, 0.5, C).astype(np.float32),
                rv=rng.uniform(0.5, 1.5, C).astype(np.float32), dy=f(B, C, L), dpooled=f(B, C), residual=f(B, C, L) if residual else None)


def _hold(label, got, d, floors, skip=(), off=False, **kw):
    """The device's results against the fp64 restatement under 2 x max(recorded floor, this input's fp32-restatement floor); a pooled
    case under the device's own arg and mask, after holding those to the fp64 evaluation's."""
    kw.pop("groups", None), kw.pop("res_grad", None)
    wide = False if off else None
    pool, dec = kw.get("pool", False), None
    if pool:
        free = _restate(d, np.float64, wide=wide, **kw)
        f32 = _restate(d, np.float32, wide=wide, **kw)
        ybar = 2 * max(floors["y"], R.rel(f32["y"], free["y"])) * float(np.abs(free["y"]).max())
        B, C, L = d["x"].shape
        assert got["arg"].dtype == np.int32 and got["arg"].min() >= 0 and got["arg"].max() < L, label
        at = np.take_along_axis(free["dense"], got["arg"][:, :, None].astype(np.int64), 2)[:, :, 0]
        gap = float((free["y"] - at).max())
        print(f"{label} arg: fp64 y at the device's arg is at most {gap:.3e} under the row maximum, bar {ybar:.3e}")
        assert gap <= ybar, (label, gap, ybar)
        mask = got["y"] > 0
        if kw.get("act") == "relu":
            wrong = (mask != (free["y"] > 0)) & (np.abs(at) > ybar)
            assert not wrong.any(), (label, int(wrong.sum()))
        dec = (got["arg"], mask)
    want, f32 = _restate(d, np.float64, wide=wide, decisions=dec, **kw), _restate(d, np.float32, wide=wide, decisions=dec, **kw)
    for q in R.QUANTITIES:
        if want[q] is None or q in skip:
            assert got[q] is None, (label, q)
            continue
        assert got[q] is not None and np.isfinite(got[q]).all(), (label, q)
        err, bar = R.rel(got[q], want[q]), 2 * max(floors[q], R.rel(f32[q], want[q]))
        print(f"{label} {q}: kernel {err:.3e} bar {bar:.3e}")
        assert err <= bar, (label, q, err, bar)
    assert got["nbt"] == want["nbt"], label


def test_golden_norm_cases():
    g, tol = np.load(R.GOLDEN), {c["case"]: c for c in _tol()["cases"]}
    figures = {}
    for c in map(str, g["cases"]):
        f32 = lambda k: g[c + k].astype(np.float32)
        pool, r = bool(g[c + "_pool"]), R.residual_of(g, c)
        d = dict(x=f32("_x"), gamma=f32("_gamma"), beta=f32("_beta"), rm=f32("_rm0"), rv=f32("_rv0"), dy=f32("_dy"), nbt=int(g[c + "_nbt0"]),
                 residual=None if r is None else r.astype(np.float32), dpooled=f32("_dpooled") if pool else None)
        training = bool(g[c + "_training"])
        got = _device(d, training=training, momentum=float(g["momentum"]), eps=float(g["eps"]), act=str(g[c + "_act"]), pool=pool)
        figures[c] = {}
        for q in R.QUANTITIES:
            want = R.wanted(g, c, q)
            if want is None:
                continue
            err = R.rel(got[q], want)
            figures[c][q] = float(f"{err:.4g}")
            print(f"{c} {q}: kernel {err:.3e} floor {tol[c][q + '_floor']:.3e} bar {tol[c][q + '_bar']:.3e}")
        if pool:
            same = np.array_equal(got["arg"], g[c + "_arg"]) and np.array_equal(got["y"] > 0, g[c + "_mask"])
            print(f"{c}: arg and mask equal to the record: {same}")
            assert same, c
        assert got["nbt"] == (int(g[c + "_nbt1"]) if training else None)          # (eval mode is given no count to advance)
    if os.environ.get("U3D_BNCF_FIGURES"):
        with open(os.environ["U3D_BNCF_FIGURES"], "w") as fh:
            json.dump(figures, fh)
    for c, row in figures.items():
        for q, err in row.items():
            assert err <= tol[c][q + "_bar"], (c, q, err, tol[c][q + "_bar"])


# ---- modules ------------------------------------------------------------------------------------------------------------------------
def _zero_bars(g, name):
    """The gradient of a Conv1d bias in front of a norm is a sum of B L terms (the norm's dx) that is zero in exact arithmetic, so it has
    no relative unit.  What fp32 leaves of it is bounded by the summation error, n u sum|terms| with n = B L and u = 2^-24 (the terms'
    own rounding errors, a few u each, are inside that bound for n >= 8): per such bias the largest bound over its channels, from the
    fp64 restatement of the module."""
    _, tape = R.module_case(g, name, np.float64)
    bars = {}
    for conv, dx in tape.norm_dx.items():
        n = dx.shape[0] * dx.shape[2]
        bars["d_" + conv + ".bias"] = float(n * 2.0 ** -24 * np.abs(dx).sum((0, 2)).max())
    return bars


def _module_step(module, x, dout, want, zero_bars=None):
    module = module.cuda()
    module.zero_grad()
    xt = torch.from_numpy(x).float().cuda().requires_grad_(True)
    out = module(xt)
    out.backward(torch.from_numpy(dout).float().cuda())
    torch.cuda.synchronize()
    res = {"out": out.detach(), "dx": xt.grad}
    res.update({"d_" + k: p.grad for k, p in module.named_parameters()})
    res.update({"after_" + k: b for k, b in module.named_buffers() if b.is_floating_point()})
    zero = {k for k in res if np.abs(want[k]).max() < 1e-12}                     # a Conv1d bias in front of a norm: no gradient
    for k in sorted(zero):
        got = float(res[k].abs().max())
        print(f"{k}: zero in the record, largest absolute value {got:.3e}, summation bound {zero_bars[k]:.3e}")
        assert got <= zero_bars[k], (k, got, zero_bars[k])
    err = {k: R.rel(v.cpu().numpy(), want[k]) for k, v in res.items() if k not in zero}
    return err, {k: int(b) for k, b in module.named_buffers() if not b.is_floating_point()}, out.detach().cpu().numpy()


def _hold_module(label, fused, plain, floor):
    for k, err in fused.items():
        print(f"{label} {k}: fused {err:.3e} op-by-op {plain[k]:.3e} bar {2 * plain[k] + floor:.3e}")
    for k, err in fused.items():
        assert err <= 2 * plain[k] + floor, (label, k, err, plain[k])


@pytest.mark.parametrize("name", ["pre_k24", "pre_k24_eval", "pcm_pre_k32", "pos", "cbr_l50", "res_groups", "cbr_gelu"])
def test_golden_module_cases_fused_against_op_by_op(name):
    from unipre3d_amd import batchnorm_cf
    g = np.load(R.GOLDEN)
    assert name in map(str, g["modules"])
    want = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_") and not k.startswith(name + "_eval")}
    plain_module = R.reference_module(g, name)
    holder = torch.nn.Sequential(copy.deepcopy(plain_module))
    assert batchnorm_cf.fuse_pointmlp_blocks(holder) == 1 and type(holder[0]).__module__ == batchnorm_cf.__name__
    assert list(holder[0].state_dict().keys()) == list(map(str, g[name + "_keys"]))
    bars = _zero_bars(g, name)
    plain, counts_p, _ = _module_step(plain_module, g[name + "_x"], g[name + "_dout"], want, bars)
    fused, counts_f, out = _module_step(holder[0], g[name + "_x"], g[name + "_dout"], want, bars)
    assert counts_p == counts_f and all(v == (4 if bool(g[name + "_training"]) else 3) for v in counts_f.values())
    _hold_module(name, fused, plain, _tol()["floors"]["y"])
    if str(g[name + "_act"]) == "relu":
        assert np.array_equal(out > 0, g[name + "_out"] > 0), name               # every mask decision of the module's output
    if str(g[name + "_kind"]) == "PreExtraction":
        assert out.shape == g[name + "_out"].shape


def test_fuse_pointmlp_blocks_on_a_small_stack():
    """A PointMLP-like stage (PreExtraction over K = 24 neighbours, then PosExtraction) of the restated reference classes: fused against
    unfused on the device, both against the unfused stack in fp64 on the CPU."""
    from unipre3d_amd import batchnorm_cf
    cls = R.reference_classes()
    torch.manual_seed(61)
    stack = torch.nn.Sequential(cls["PreExtraction"](14, 24, blocks=2, bias=False), cls["PosExtraction"](24, blocks=1, bias=False))
    with torch.no_grad():
        for m in stack.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.3, 0.3), m.running_mean.uniform_(-0.3, 0.3)
    rng = np.random.default_rng(62)
    x, dout = rng.standard_normal((2, 9, 24, 14)), rng.standard_normal((2, 24, 9))
    ref = copy.deepcopy(stack).double()
    x64 = torch.from_numpy(x).requires_grad_(True)
    out64 = ref(x64)
    out64.backward(torch.from_numpy(dout))
    want = {"out": out64.detach().numpy(), "dx": x64.grad.numpy()}
    want.update({"d_" + k: p.grad.numpy() for k, p in ref.named_parameters()})
    want.update({"after_" + k: b.numpy() for k, b in ref.named_buffers() if b.is_floating_point()})
    fused_stack = copy.deepcopy(stack)
    assert batchnorm_cf.fuse_pointmlp_blocks(fused_stack) == 2
    assert list(fused_stack.state_dict().keys()) == list(stack.state_dict().keys())
    assert not any(type(m) is torch.nn.BatchNorm1d for m in fused_stack.modules())
    plain, _, _ = _module_step(stack, x, dout, want)
    fused, _, out = _module_step(fused_stack, x, dout, want)
    _hold_module("stack", fused, plain, _tol()["floors"]["y"])
    assert out.shape == (2, 24, 9)


# ---- every dispatch class ------------------------------------------------------------------------------------------------------------
def test_the_plan_is_the_restated_one_and_every_class_is_reached():
    from unipre3d_amd import batchnorm_cf
    seen = set()
    for L in LENGTHS:
        for aligned in (True, False):
            for C in (1, 3, 40, 1024):
                p = batchnorm_cf.plan(C, L, aligned)
                assert tuple(p) == tuple(R.plan(C, L, aligned)), (C, L, aligned)
                assert batchnorm_cf.parts(2 * p.batch_chunk + 1, C, L) == 3
                seen.add((p.lanes_per_row, p.vec, p.sweeps > 1))
    groups = {1, 2, 4, 8, 16, 32, 64}
    assert {s[0] for s in seen if s[1] == 1} == groups and {s[0] for s in seen if s[1] == 4} == groups
    assert {s for s in seen if s[2]} == {(64, 1, True), (64, 4, True)} and (64, 1, False) in seen and (64, 4, False) in seen


@pytest.mark.parametrize("off", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
def test_every_dispatch_class_at_its_smallest_shapes(L, off):
    from unipre3d_amd import batchnorm_cf
    floors = _tol()["floors"]
    k = LENGTHS.index(L)
    rows = 256 // batchnorm_cf.plan(1024, L, not off).lanes_per_row              # the channel tile of a wide tensor
    for j, C in enumerate((1, 3, rows, rows + 1)):
        p = batchnorm_cf.plan(C, L, not off)
        assert p.vec == (4 if L % 4 == 0 and not off else 1) and p.channel_tile == min(C, rows)
        B = (1, p.batch_chunk, p.batch_chunk + 1, 2 * p.batch_chunk + 1)[(j + k) % 4]
        act, residual = CONFIGS[(k + j) % 5]
        training = not (B * L < 2 or (k + j) % 7 == 6)
        kw = dict(training=training, momentum=(0.01, 0.1, None)[(k + j) % 3], act=act, pool=(k + j) % 2 == 1)
        d = _inputs(B, C, L, 1000 * L + 10 * C + B, residual)
        got = _device(d, off=off, **kw)
        _hold(f"L={L} C={C} B={B} off={off} {act} res={residual} {kw} {tuple(p)}", got, d, floors, off=off, **kw)


@pytest.mark.parametrize("act,residual", CONFIGS)
@pytest.mark.parametrize("pool", [False, True])
def test_every_combination_of_act_residual_and_pool(act, residual, pool):
    from unipre3d_amd import batchnorm_cf
    C, L = 40, 24
    B = 2 * batchnorm_cf.plan(C, L).batch_chunk + 1
    floors = _tol()["floors"]
    d = _inputs(B, C, L, 77, residual)
    for training in (True, False):
        kw = dict(act=act, pool=pool, training=training)
        _hold(f"{act} res={residual} pool={pool} training={training}", _device(d, **kw), d, floors, **kw)


@pytest.mark.parametrize("rows", [1, 3])
def test_pool_groups_write_the_channels_first_result(rows):
    C, L, S = 5, 24, 7
    floors = _tol()["floors"]
    d = _inputs(rows * S, C, L, 80 + rows, True)
    kw = dict(act="relu", pool=True, groups=S)
    _hold(f"pool_groups={S} rows={rows}", _device(d, **kw), d, floors, **kw)       # (_device checks the (rows, C, S) shape)


def test_affine_false_momentum_none_and_no_running_statistics():
    floors = _tol()["floors"]
    d = _inputs(9, 12, 33, 90, True)
    for kw in (dict(affine=False), dict(momentum=None), dict(track=False), dict(track=False, affine=False, pool=True)):
        kw = dict(act="relu", **kw)
        _hold(f"{kw}", _device(d, **kw), d, floors, **kw)


def test_residual_without_grad_and_what_the_pooled_node_keeps():
    B, C, L = 50, 16, 24
    floors = _tol()["floors"]
    d = _inputs(B, C, L, 95, True)
    got = _device(d, act="relu", res_grad=False)
    _hold("no residual grad", got, d, floors, skip=("dresidual",), act="relu")
    assert got["saved"].count((B, C, L)) == 2                                     # x, and y for the ReLU mask
    for act in ("relu", "none"):
        got = _device(d, act=act, pool=True)
        assert got["saved"].count((B, C, L)) == 1, got["saved"]                   # x alone: neither y nor the residual
        assert all(s in ((B, C, L), (B, C), (C,)) for s in got["saved"]), got["saved"]
    got = _device(dict(d, residual=None), act="gelu", pool=True)
    assert got["saved"].count((B, C, L)) == 1


def test_two_runs_are_bit_identical():
    from unipre3d_amd import batchnorm_cf
    C, L = 40, 24
    d = _inputs(3 * batchnorm_cf.plan(C, L).batch_chunk + 2, C, L, 21, True)
    for pool in (False, True):
        a, b = _device(d, act="relu", pool=pool), _device(d, act="relu", pool=pool)
        for q in R.QUANTITIES:
            assert a[q].tobytes() == b[q].tobytes(), q
    d = _inputs(700, 3, 5, 22, False)
    a, b = _device(d, act="gelu", momentum=None), _device(d, act="gelu", momentum=None)
    for q in ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
        assert a[q].tobytes() == b[q].tobytes(), q


@pytest.mark.parametrize("pool", [False, True])
def test_graph_capture_replays_the_training_step(pool):
    from unipre3d_amd import batchnorm_cf
    C, L = 32, 24
    B = 2 * batchnorm_cf.plan(C, L).batch_chunk + 3
    d = _inputs(B, C, L, 31, True)
    t = lambda k: torch.from_numpy(d[k]).cuda()

    def fresh():
        return dict(x=t("x").requires_grad_(True), res=t("residual").requires_grad_(True), gamma=t("gamma").requires_grad_(True),
                    beta=t("beta").requires_grad_(True), rm=t("rm"), rv=t("rv"), nbt=torch.tensor(3, device="cuda"),
                    dy=t("dpooled" if pool else "dy"))

    def step(s):
        y = batchnorm_cf.batch_norm_act_cf(s["x"], s["gamma"], s["beta"], s["rm"], s["rv"], s["nbt"], training=True, momentum=None, eps=1e-5,
                                           act="relu", residual=s["res"], pool="max" if pool else None)
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


class _Hook:
    """stat_reduce for one of two halves: call k adds adds[k] (None: nothing) and records what it was given."""

    def __init__(self, adds):
        self.adds, self.seen = adds, []

    def __call__(self, block):
        k = len(self.seen)
        self.seen.append(block.clone())
        return block if self.adds[k] is None else block + self.adds[k]


@pytest.mark.parametrize("pool", [False, True])
def test_stat_reduce_two_halves_equal_the_full_batch(pool):
    from unipre3d_amd import batchnorm_cf
    C, L = 32, 24
    bc = batchnorm_cf.plan(C, L).batch_chunk
    B, cut = 2 * bc + 5, bc + 2
    d = _inputs(B, C, L, 41, True)
    bars = {q: 2 * v for q, v in _tol()["floors"].items()}
    kw = dict(act="relu", pool=pool)
    full = _device(d, **kw)
    halves = [slice(0, cut), slice(cut, B)]
    part = lambda h: {k: (v[h] if v is not None and v.shape[:1] == (B,) else v) for k, v in d.items()}
    fwd = [_Hook([None, None]) for _ in halves]
    for h, hook in zip(halves, fwd):
        _device(part(h), stat_reduce=hook, **kw)
    bwd = [_Hook([fwd[1 - i].seen[0], None]) for i in range(2)]
    for h, hook in zip(halves, bwd):
        _device(part(h), stat_reduce=hook, **kw)
    got = [_device(part(h), stat_reduce=_Hook([fwd[1 - i].seen[0], bwd[1 - i].seen[1]]), **kw) for i, h in enumerate(halves)]
    both = dict(y=np.concatenate([g["y"] for g in got]), dx=np.concatenate([g["dx"] for g in got]),
                dresidual=np.concatenate([g["dresidual"] for g in got]), dgamma=got[0]["dgamma"] + got[1]["dgamma"],
                dbeta=got[0]["dbeta"] + got[1]["dbeta"], running_mean=got[0]["running_mean"], running_var=got[1]["running_var"])
    for q, v in both.items():
        err = R.rel(v, full[q])
        print(f"two halves pool={pool} {q}: {err:.3e} bar {bars[q]:.3e}")
        assert err <= bars[q], q
    assert fwd[0].seen[0][0].item() == cut * L and bwd[1].seen[1][0].item() == (B - cut) * L     # each block starts with this half's count
    if pool:
        assert np.array_equal(np.concatenate([g["arg"] for g in got]), full["arg"])
