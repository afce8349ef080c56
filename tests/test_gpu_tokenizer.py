"""unipre3d_amd/tokenizer.py on the device: the golden record of the reference's own `Encoder` (tests/golden/g24_tokenizer.npz), the module
against the record, SyncBatchNorm children without a process group, the `stat_reduce` hook with an injected reducer, graph capture,
reproducibility, the kernels' edge shapes against the fp64 restatement, and the refusals.

The rule (profiles/tokenizer/tolerance.json, tests/tokenizer_ref.py): bar = 2 x floor per quantity, in max|x - fp64| / max|fp64|, the
floor being the CPU-measured distance of the fp32 restatement in the kernels' order from the fp64 record.  Gradients are compared with
the fp64 restatement evaluated under the device's own max and ReLU decisions (both discontinuous); the decisions are checked on their
own: arg2 is exactly the lowest row attaining the maximum of the device's stored f2 and g is that value bitwise, the fp64 f4 at the
device's arg4 lies within the `out` bar of the fp64 maximum, no pick is a row whose coordinates bit-duplicate an earlier row of its
group, and where a ReLU decision (recomputed from the kept folds, x and y3) differs from the fp64 arithmetic's, the fp64 pre-activation
lies within the `out` bar of zero.  A shape without a recorded case has its own CPU-measured floor in the same file (`edge_cases`, the
fp32 restatement on the test's seeded inputs): bar = 2 x max(floor of the golden cases, floor of the shape).

Edge shapes (B, G, n, C) and the constants of csrc/u3d_tokenizer.hip they come from:
  (1, 1, 2, 40)        one group, the smallest batch BatchNorm accepts; a 64-row tile with two live rows
  (2, 5, 24, 40)       240 rows: a ragged last 64-row tile, groups straddling tiles, a ragged 64-column tile (C = 40)
  (1, 3, 33, 384)      odd n (the dh3m kernel's 8 row phases own 5 or 4 rows), the reference's C; C > 256: two rounds of staging dout
  (2, 2, 1, 40)        n = 1, where max is the identity
  (1, 2, 256, 16)      the largest n: the whole 256 x 32 LDS slab of the dh3m kernel, exactly one 512-row statistics split
  (2, 5, 30, 40)       300 rows: u3d_tok_wgrad_splits(300) = 2 splits of 160 rows, the last one ragged (140 = 4 x 32 + 12)
  (1, 2, 3, 1)         C = 1       (1, 2, 4, 1024)  the largest C (16 column tiles, four rounds of staging dout)
  (1, 9, 64, 72)       576 rows: two statistics splits of 288 rows, C one 64-column tile and a ragged one
  (4, 128, 32, 384)    workload-shaped: 16384 rows, 512 groups (8 group splits of dW4), 64 weight-gradient and 32 statistics splits;
                       in training mode only (the eval path differs in the folds alone, which the other shapes cover)
The list itself, the inputs and the floors live in tests/tokenizer_ref.py (EDGES, edge_inputs, edge_floor)."""
import numpy as np
import pytest
import torch
from torch import nn

import tokenizer_ref as TR

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def golden():
    return np.load(TR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def bars():
    return TR.tolerance()["bars"]


def _params(w):
    return [torch.from_numpy(w[k]).cuda().requires_grad_(True) for k in TR.PARAMS]


def _running(w, nbt=TR.NBT0):
    r = {k: torch.from_numpy(w[k]).cuda() for k in TR.RUNNING}
    n1, n2 = torch.tensor(nbt, device="cuda"), torch.tensor(nbt, device="cuda")
    return r, (r["rm1"], r["rv1"], n1, r["rm2"], r["rv2"], n2)


def _device_x(x):
    """The numpy array (possibly a transposed view) on the device with the same logical strides."""
    base = x.base if x.base is not None and not x.flags["C_CONTIGUOUS"] else None
    if base is None:
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    assert base.shape == (x.shape[0], 3, x.shape[1], x.shape[2])       # the transformer's (B, 3, G, n) permuted to (B, G, n, 3)
    t = torch.from_numpy(np.ascontiguousarray(base)).cuda().permute(0, 2, 3, 1)
    assert not t.is_contiguous()
    return t


def _kept(saved):
    """What the autograd function keeps, by name (its save_for_backward order)."""
    return {k: saved[i].cpu().numpy() for k, i in (("fold1", 7), ("fold2", 8), ("f2", 9), ("y3", 10), ("g", 11), ("arg2", 12), ("arg4", 13))}


def _run(x, dout, w, training, stat_reduce=None, momentum=TR.MOMENTUM):
    """{name: host array} of tokenize(): out, the twelve gradients, x, the running statistics, nbt, and the saved f2, g, arg2, arg4."""
    from unipre3d_amd import tokenizer
    params = _params(w)
    rdict, running = _running(w)
    xt = _device_x(x).requires_grad_(True)
    out = tokenizer.tokenize(xt, params, training=training, eps=TR.EPS, momentum=momentum, running=running, stat_reduce=stat_reduce)
    saved = out.grad_fn.saved_tensors
    out.backward(torch.from_numpy(np.ascontiguousarray(dout)).cuda())
    torch.cuda.synchronize()
    got = {k: p.grad.cpu().numpy().reshape(w[k].shape) for k, p in zip(TR.PARAMS, params)}
    got.update(out=out.detach().cpu().numpy(), x=xt.grad.cpu().numpy(), nbt=(int(running[2]), int(running[5])),
               **_kept(saved))
    got.update({k: v.cpu().numpy() for k, v in rdict.items()})
    return got


def _check_picks(got, s64, x, bar_out):
    B, G, n, _ = x.shape
    M = B * G
    f2 = got["f2"].reshape(M, n, TR.C2)
    assert np.array_equal(got["arg2"], np.argmax(f2, axis=1)), "arg2 is not the lowest row attaining the maximum of the stored f2"
    assert np.array_equal(got["g"].view(np.int32), np.max(f2, axis=1).view(np.int32)), "g is not that maximum bitwise"
    C = got["arg4"].shape[1]
    assert got["arg4"].min() >= 0 and got["arg4"].max() < n
    f4 = s64["f4"].reshape(M, n, C)
    at_pick = np.take_along_axis(f4, got["arg4"][:, None, :].astype(np.int64), 1)[:, 0]
    gap = float(np.max(f4.max(axis=1) - at_pick) / np.abs(s64["out"]).max())
    assert gap <= bar_out, f"the fp64 f4 at the device's arg4 lies {gap:.3g} below the fp64 maximum"
    xb = np.ascontiguousarray(x).reshape(M, n, 3).view(np.int32)
    dup = np.zeros((M, n), bool)                  # rows whose coordinates bit-duplicate an earlier row of the group
    for i in range(1, n):
        dup[:, i] = (xb[:, :i] == xb[:, i:i + 1]).all(axis=2).any(axis=1)
    for arg in (got["arg2"], got["arg4"]):
        assert not np.take_along_axis(dup, arg.astype(np.int64), 1).any(), "a pick is a bit-duplicate of an earlier row"
    return gap


def _compare(got, x, dout, w, training, bars, out_ref=None):
    """Worst figures per quantity; gradients against the fp64 restatement under the device's own picks."""
    fwd = lambda **kw: TR.forward(x, w, training=training, **kw)
    mask1, mask3 = TR.kernel_masks(x, got["fold1"], got["fold2"], got["y3"])
    s64 = fwd(arg2=got["arg2"], arg4=got["arg4"], mask1=mask1, mask3=mask3)
    free = fwd()
    ref = dict(TR.backward(s64, dout), out=free["out"] if out_ref is None else out_ref, **free["running"])
    mine = {k: got[k] for k in ("out", "x") + TR.PARAMS + TR.RUNNING}
    d = TR.distances(mine, ref, training)
    per = {k: TR.dist(mine[k], ref[k], float(np.abs(ref[TR.ZERO_IN_TRAINING[k]]).max()) if training and k in TR.ZERO_IN_TRAINING else None)
           for k in TR.PARAMS}
    print("  per parameter:", " ".join(f"{k} {v:.1e}" for k, v in per.items()))
    d["arg4_gap"] = _check_picks(got, free, x, bars["out"])
    d["relu_gap"] = TR.mask_gap(free, mask1, mask3)
    assert d["relu_gap"] <= bars["out"], f"a ReLU decision differs where the fp64 pre-activation is {d['relu_gap']:.3g} of the largest"
    return d, ref


def _assert_bars(d, bars, what):
    print(what, " ".join(f"{q} {d[q]:.3e}" for q in d))
    for q in TR.QUANTITIES:
        assert d[q] <= bars[q], f"{what}: {q} {d[q]:.3e} above the bar {bars[q]:.3e}"


@pytest.mark.parametrize("case", TR.CASES)
def test_golden_cases(golden, bars, case):
    x, dout, training = TR.golden_case(golden, case)
    w = TR.weights(int(golden["C"]))
    got = _run(x, dout, w, training)
    assert got["out"].shape == dout.shape and got["x"].shape == x.shape
    d, ref = _compare(got, x, dout, w, training, bars, out_ref=golden[f"{case}_out64"])
    _assert_bars(d, bars, f"golden {case}:")
    assert got["nbt"] == (int(golden[f"{case}_nbt"]),) * 2
    # where the device decided as the reference's fp64 run did, its gradients are held to the record itself
    s = TR.forward(x, w, training=training)
    if np.array_equal(s["arg2"], got["arg2"]) and np.array_equal(s["arg4"], got["arg4"]):
        rec = TR.record_of(golden, case)
        mine = dict(TR.recorded({k: got[k] for k in TR.PARAMS}), out=got["out"], x=got["x"], **{k: got[k] for k in TR.RUNNING})
        _assert_bars(TR.distances(mine, rec, training), bars, f"golden {case} against the record:")
    if not training:
        for k in TR.RUNNING:
            assert np.array_equal(got[k], w[k]), k


def _module(C, w, training, sync=False):
    from unipre3d_amd.tokenizer import Encoder
    m = Encoder(C)
    m.load_state_dict(TR.state_dict(w), strict=True)
    if sync:
        m = nn.SyncBatchNorm.convert_sync_batchnorm(m)
    return m.cuda().train(training)


def _module_run(m, x, dout):
    xt = _device_x(x).requires_grad_(True)
    m.zero_grad()
    out = m(xt)
    saved = [t.clone() for t in out.grad_fn.saved_tensors]
    out.backward(torch.from_numpy(np.ascontiguousarray(dout)).cuda())
    torch.cuda.synchronize()
    inv = {v: k for k, v in TR.STATE_KEYS.items()}
    got = {inv[k]: p.grad.cpu().numpy().reshape(p.shape[:2] if p.dim() == 3 else p.shape) for k, p in m.named_parameters()}
    sd = m.state_dict()
    got.update(out=out.detach().cpu().numpy(), x=xt.grad.cpu().numpy(), **{k: sd[TR.STATE_KEYS[k]].cpu().numpy() for k in TR.RUNNING})
    got["nbt"] = (int(sd["first_conv.1.num_batches_tracked"]), int(sd["second_conv.1.num_batches_tracked"]))
    got.update(_kept(saved))
    return got


@pytest.mark.parametrize("case", TR.CASES)
def test_module_against_the_record(golden, bars, case):
    x, dout, training = TR.golden_case(golden, case)
    C = int(golden["C"])
    w = TR.weights(C)
    got = _module_run(_module(C, w, training), x, dout)
    d, _ = _compare(got, x, dout, w, training, bars, out_ref=golden[f"{case}_out64"])
    _assert_bars(d, bars, f"module {case}:")
    assert got["nbt"] == (int(golden[f"{case}_nbt"]),) * 2
    # the functional form on the same inputs gives the same bits
    fn = _run(x, dout, w, training)
    for k in ("out", "x") + TR.PARAMS + TR.RUNNING:
        assert np.array_equal(got[k], fn[k]), k


def test_sync_batchnorm_children_without_a_process_group_behave_as_plain(golden):
    x, dout, _ = TR.golden_case(golden, "train")
    C = int(golden["C"])
    w = TR.weights(C)
    assert not (torch.distributed.is_available() and torch.distributed.is_initialized())
    plain, sync = _module_run(_module(C, w, True), x, dout), _module_run(_module(C, w, True, sync=True), x, dout)
    for k in ("out", "x", "nbt") + TR.PARAMS + TR.RUNNING:
        assert np.array_equal(plain[k], sync[k]), k


def test_injected_reducer_rank_a_of_two(bars):
    """Device rank A, fed rank B's sums as the restatement's rank B sent them, against the restatement's rank A."""
    from test_tokenizer_ref import two_rank_inputs, two_rank_restatement
    w = TR.weights(40)
    xa, xb, da, db = two_rank_inputs()
    _, sent = two_rank_restatement(w)
    calls = []

    def reduce(block):
        other = sent[1][len(calls)]
        calls.append(block.shape[0])
        return block + torch.from_numpy(other).to(block.device)

    got = _run(xa, da, w, True, stat_reduce=reduce)
    assert calls == [10, 1025, 1025, 257]

    def ref_fn(**kw):
        it = iter(sent[1])
        return TR.forward(xa, w, training=True, stat_reduce=lambda b: b + next(it), **kw)

    mask1, mask3 = TR.kernel_masks(xa, got["fold1"], got["fold2"], got["y3"])
    s64 = ref_fn(arg2=got["arg2"], arg4=got["arg4"], mask1=mask1, mask3=mask3)
    it = iter(sent[1][2:])                                   # backward's two blocks follow forward's two
    s64["stat_reduce"] = lambda b: b + next(it)
    free = ref_fn()
    ref = dict(TR.backward(s64, da), out=free["out"], **free["running"])
    # (under a reducer the three biases' gradients are not zero on one rank, only over the ranks: each is held on its own scale)
    d = TR.distances({k: got[k] for k in ("out", "x") + TR.PARAMS + TR.RUNNING}, ref, False)
    _assert_bars(d, bars, "rank A of two:")
    _check_picks(got, free, xa, bars["out"])
    assert TR.mask_gap(free, mask1, mask3) <= bars["out"]
    alone = TR.forward(xa, w, training=True)
    assert TR.dist(got["out"], alone["out"]) > 1e-3          # the reducer did change the statistics


def test_two_runs_are_bitwise_equal():
    w = TR.weights(72)
    x, dout = TR.edge_inputs((1, 9, 64, 72))
    a, b = _run(x, dout, w, True), _run(x, dout, w, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_graph_capture_and_replay_equal_eager_bitwise():
    from unipre3d_amd import tokenizer
    w = TR.weights(40)
    x, dout = TR.edge_inputs((2, 5, 24, 40))
    params = _params(w)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    dt = torch.from_numpy(dout).cuda()

    def step():
        out = tokenizer.tokenize(xt, params, training=True, eps=TR.EPS, momentum=TR.MOMENTUM)
        return (out,) + torch.autograd.grad(out, [xt] + params, dt)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eager, captured)):
        assert torch.equal(a, b), i


@pytest.mark.parametrize("shape,training", TR.EDGE_MODES, ids=[TR.edge_key(s, t) for s, t in TR.EDGE_MODES])
def test_edge_shapes(shape, training):
    w = TR.weights(shape[3])
    x, dout = TR.edge_inputs(shape)
    bars = TR.tolerance()["edge_cases"][TR.edge_key(shape, training)]["bars"]
    got = _run(x, dout, w, training)
    d, _ = _compare(got, x, dout, w, training, bars)
    _assert_bars(d, bars, f"{TR.edge_key(shape, training)}:")
    assert got["nbt"] == (TR.NBT0 + int(training),) * 2


def test_the_split_shape_has_two_weight_gradient_splits_and_a_ragged_last_one():
    from unipre3d_amd import tokenizer
    lib = tokenizer.load()
    rows = 2 * 5 * 30
    assert lib.u3d_tok_wgrad_splits(rows) == TR.wgrad_splits(rows) == 2
    assert rows % TR.wgrad_rows_per_split(rows) % 32 != 0
    assert lib.u3d_tok_wgrad_splits(4 * 128 * 32) == TR.wgrad_splits(4 * 128 * 32) == 64


def test_cumulative_average_and_untracked_statistics(bars):
    w = TR.weights(40)
    x, dout = TR.edge_inputs((2, 5, 24, 40))
    got = _run(x, dout, w, True, momentum=None)
    s = TR.forward(x, w, training=True, momentum=None)
    for k in TR.RUNNING:
        assert TR.dist(got[k], s["running"][k]) <= bars["running"], k
    assert got["nbt"] == (TR.NBT0 + 1,) * 2
    from unipre3d_amd import tokenizer
    out = tokenizer.tokenize(torch.from_numpy(x).cuda(), _params(w), training=True, running=None)
    assert np.array_equal(out.detach().cpu().numpy(), got["out"])


def test_refusals():
    from unipre3d_amd import tokenizer
    w = TR.weights(40)
    params = [p.detach() for p in _params(w)]
    kw = dict(training=True, eps=1e-5, momentum=0.1)
    with pytest.raises(ValueError, match="more than 1 value"):
        tokenizer.tokenize(torch.zeros(1, 1, 1, 3, device="cuda"), params, **kw)
    with pytest.raises(ValueError, match="n=257"):
        tokenizer.tokenize(torch.zeros(1, 1, 257, 3, device="cuda"), params, **kw)
    with pytest.raises(ValueError, match="fp32 only"):
        tokenizer.tokenize(torch.zeros(1, 1, 4, 3, device="cuda", dtype=torch.float16), params, **kw)
    with pytest.raises(ValueError, match="fp32 only"):
        tokenizer.tokenize(torch.zeros(1, 1, 4, 3, device="cuda", dtype=torch.float64), params, **kw)
    # one point in eval mode is fine, as it is for BatchNorm1d
    _, running = _running(w)
    out = tokenizer.tokenize(torch.zeros(1, 1, 1, 3, device="cuda"), params, training=False, running=running)
    assert out.shape == (1, 1, 40) and torch.isfinite(out).all()
