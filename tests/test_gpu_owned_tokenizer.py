"""libunipre3d_tokenizer.so writes every element it owns and nothing else: its six compute entry points called directly in the order of
a training (or eval) step, with every pointer inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the
module's own wrapper on ordinary tensors, bit for bit (tests/test_gpu_tokenizer.py holds the wrapper to the reference's fp64 record).

  entry point       owned outputs (none pre-zeroed: they hold the poison before the call)
  u3d_tok_moments   sums1 (10 f64), and every byte of its scratch
  u3d_tok_fwd_a     fold1 (1280), f2 (rows,256), g and arg2 (M,256), y3 (rows,512), sums2 (1025 f64), running_mean1 / running_var1 /
                    num_batches_tracked1 (updated in place), scratch
  u3d_tok_fwd_b     fold2 (2048), out and arg4 (M,C), the second BatchNorm's running statistics, scratch
  u3d_tok_bwd_1     dW4 (C,512), db4 (C), dh3m (rows,512), sums3 (1025 f64), scratch
  u3d_tok_bwd_2     dgamma2, dbeta2, dW3 (512,512), db3, dW2 (256,128), db2, df2 (rows,256), dh1m (rows,128), sums1b (257 f64), scratch
  u3d_tok_bwd_3     dgamma1, dbeta1, dW1 (128,3), db1, dx (rows,3), scratch
  u3d_tok_abi_version, u3d_tok_wgrad_splits, u3d_tok_scratch_bytes   host only: called here for their values

Cases (B, G, n, C): (2, 5, 30, 40) training, contiguous x: 300 rows, two weight-gradient splits with a ragged last one, ragged row and
column tiles; (1, 3, 33, 72) training, x read through the strides of the transformer's permuted (B, 3, G, n) tensor; (2, 2, 1, 40) eval
mode (no statistics pass: sums are null pointers and the scratch of u3d_tok_fwd_a is smaller).
A pointer 4 (f64: 8) bytes past a 16-byte boundary: the call returns 1 and not one byte of the arena changes."""
import numpy as np
import pytest
import torch

import tokenizer_ref as TR
from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

CASES = [((2, 5, 30, 40), True, False), ((1, 3, 33, 72), True, True), ((2, 2, 1, 40), False, False)]


def _inputs(shape, permuted):
    B, G, n, C = shape
    rng = np.random.default_rng(B * 100 + n)
    x = rng.uniform(-1, 1, (B, G, n, 3)).astype(np.float32)
    if n >= 4:
        x[:, :, n - n // 4:] = x[:, :, :1]
    stored = np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))) if permuted else x
    return x, stored, rng.uniform(-1, 1, (B, G, C)).astype(np.float32), TR.weights(C)


def _wrapper(stored, permuted, dout, w, training):
    from unipre3d_amd import tokenizer
    params = [torch.from_numpy(w[k]).cuda().requires_grad_(True) for k in TR.PARAMS]
    r = [torch.from_numpy(w[k]).cuda() for k in TR.RUNNING]
    nbt = [torch.tensor(TR.NBT0, device="cuda"), torch.tensor(TR.NBT0, device="cuda")]
    xt = torch.from_numpy(stored).cuda()
    xt = (xt.permute(0, 2, 3, 1) if permuted else xt).requires_grad_(True)
    out = tokenizer.tokenize(xt, params, training=training, eps=TR.EPS, momentum=TR.MOMENTUM, running=(r[0], r[1], nbt[0], r[2], r[3], nbt[1]))
    saved = [t.clone() for t in out.grad_fn.saved_tensors]
    out.backward(torch.from_numpy(dout).cuda())
    torch.cuda.synchronize()
    want = {"fold1": saved[7], "fold2": saved[8], "f2": saved[9], "y3": saved[10], "g": saved[11], "arg2": saved[12], "arg4": saved[13],
            "out": out.detach().reshape(-1, out.shape[-1]), "dx": xt.grad.reshape(-1, 3), "rm1": r[0], "rv1": r[1], "rm2": r[2], "rv2": r[3],
            "nbt1": nbt[0].reshape(1), "nbt2": nbt[1].reshape(1)}
    want.update({"d" + k: p.grad.reshape(w[k].shape) for k, p in zip(TR.PARAMS, params)})
    return want


def _strides(shape, permuted):
    B, G, n, _ = shape
    return (3 * G * n, n, 1, G * n) if permuted else (G * n * 3, n * 3, 3, 1)


@pytest.mark.parametrize("shape,training,permuted", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tokenizer_writes_what_it_owns(shape, training, permuted):
    from unipre3d_amd import _lib, tokenizer
    lib = tokenizer.load()
    B, G, n, C = shape
    M, rows = B * G, B * G * n
    _, stored, dout_cpu, w = _inputs(shape, permuted)
    want = _wrapper(stored, permuted, dout_cpu, w, training)
    assert lib.u3d_tok_abi_version() == tokenizer.ABI_VERSION
    assert lib.u3d_tok_wgrad_splits(rows) == TR.wgrad_splits(rows) and lib.u3d_tok_wgrad_splits(0) == 0
    sizes = [lib.u3d_tok_scratch_bytes(M, n, C if ph in (2, 3) else 1, ph, int(training)) for ph in range(6)]
    assert all(s > 0 and s % 16 == 0 for s in sizes), sizes
    assert lib.u3d_tok_scratch_bytes(M, 257, C, 2, 1) == 0 and lib.u3d_tok_scratch_bytes(M, n, 1025, 2, 1) == 0
    assert sizes[2] == rows * C * 4                               # f4 passes through scratch and is not kept
    if training:
        assert sizes[1] > lib.u3d_tok_scratch_bytes(M, n, 1, 1, 0)
    s0, s1, s2, s3 = _strides(shape, permuted)
    P = _lib.ptr
    f32, f64, i32 = torch.float32, torch.float64, torch.int32

    def case_fn(arena):
        st = _lib.stream_ptr(arena.buf.device)
        x = arena.inp(torch.from_numpy(stored), name="x")
        xa = [P(x), s0, s1, s2, s3, B, G, n]
        p = {k: arena.inp(torch.from_numpy(w[k]), name=k) for k in TR.PARAMS}
        run = {}
        for k in TR.RUNNING:                                      # updated in place: owned outputs that start from the module's buffers
            run[k] = arena.out(w[k].shape, f32, name=k)
            run[k].copy_(torch.from_numpy(w[k]))
        nbt = [arena.out((1,), torch.int64, name=f"nbt{i}") for i in (1, 2)]
        for t in nbt:
            t.fill_(TR.NBT0)
        sc = [arena.scratch(s, name=f"scratch{ph}") for ph, s in enumerate(sizes)]
        outs = []
        sums1 = sums2 = None
        if training:
            sums1, sums2 = arena.out((10,), f64, name="sums1"), arena.out((1025,), f64, name="sums2")
            assert lib.u3d_tok_moments(*xa, P(sums1), P(sc[0]), st) == 0
            outs += [sums1, sums2, sc[0]]
        fold1, fold2 = arena.out((1280,), f32, name="fold1"), arena.out((2048,), f32, name="fold2")
        f2, y3 = arena.out((rows, 256), f32, name="f2"), arena.out((rows, 512), f32, name="y3")
        g, arg2 = arena.out((M, 256), f32, name="g"), arena.out((M, 256), i32, name="arg2")
        assert lib.u3d_tok_fwd_a(*xa, P(p["W1"]), P(p["b1"]), P(p["g1"]), P(p["be1"]), P(p["W2"]), P(p["b2"]), P(p["W3"]), P(p["b3"]),
                                 P(sums1), P(run["rm1"]), P(run["rv1"]), P(nbt[0]) if training else None, TR.EPS, TR.MOMENTUM, P(fold1),
                                 P(f2), P(g), P(arg2), P(y3), P(sums2), P(sc[1]), st) == 0
        out, arg4 = arena.out((M, C), f32, name="out"), arena.out((M, C), i32, name="arg4")
        assert lib.u3d_tok_fwd_b(P(y3), M, n, C, P(p["g2"]), P(p["be2"]), P(p["W4"]), P(p["b4"]), P(sums2), P(run["rm2"]), P(run["rv2"]),
                                 P(nbt[1]) if training else None, TR.EPS, TR.MOMENTUM, P(fold2), P(out), P(arg4), P(sc[2]), st) == 0
        dout = arena.inp(torch.from_numpy(dout_cpu), name="dout")
        dW4, db4 = arena.out((C, 512), f32, name="dW4"), arena.out((C,), f32, name="db4")
        dh3m, sums3 = arena.out((rows, 512), f32, name="dh3m"), arena.out((1025,), f64, name="sums3")
        assert lib.u3d_tok_bwd_1(P(dout), P(y3), P(arg4), P(fold2), P(p["W4"]), M, n, C, P(dW4), P(db4), P(dh3m), P(sums3), P(sc[3]), st) == 0
        dg2, dbe2 = arena.out((512,), f32, name="dg2"), arena.out((512,), f32, name="dbe2")
        dW3, db3 = arena.out((512, 512), f32, name="dW3"), arena.out((512,), f32, name="db3")
        dW2, db2 = arena.out((256, 128), f32, name="dW2"), arena.out((256,), f32, name="db2")
        df2, dh1m = arena.out((rows, 256), f32, name="df2"), arena.out((rows, 128), f32, name="dh1m")
        sums1b = arena.out((257,), f64, name="sums1b")
        assert lib.u3d_tok_bwd_2(*xa, P(dh3m), P(y3), P(f2), P(g), P(arg2), P(fold1), P(fold2), P(p["g2"]), P(sums2), P(sums2),
                                 P(sums3), P(sums3), int(training), P(p["W2"]), P(p["W3"]), P(dg2), P(dbe2), P(dW3), P(db3), P(dW2), P(db2), P(df2), P(dh1m),
                                 P(sums1b), P(sc[4]), st) == 0
        dg1, dbe1 = arena.out((128,), f32, name="dg1"), arena.out((128,), f32, name="dbe1")
        dW1, db1, dx = arena.out((128, 3), f32, name="dW1"), arena.out((128,), f32, name="db1"), arena.out((rows, 3), f32, name="dx")
        assert lib.u3d_tok_bwd_3(*xa, P(dh1m), P(fold1), P(p["g1"]), P(sums1), P(sums1), P(sums1b), P(sums1b), int(training), P(p["W1"]), P(dg1), P(dbe1),
                                 P(dW1), P(db1), P(dx), P(sc[5]), st) == 0
        named = [fold1, fold2, f2, y3, g, arg2, out, arg4, dx, run["rm1"], run["rv1"], run["rm2"], run["rv2"], nbt[0], nbt[1],
                 dW1, db1, dg1, dbe1, dW2, db2, dW3, db3, dg2, dbe2, dW4, db4]
        if not training:
            arena.own(sc[0], 0)                                   # eval mode: no moments pass, its scratch stays untouched
        return named + [dh3m, sums3, df2, dh1m, sums1b] + sc[1:] + outs

    run_a, _ = run_twice(case_fn, "cuda", capacity=160 << 20)
    names = ("fold1", "fold2", "f2", "y3", "g", "arg2", "out", "arg4", "dx", "rm1", "rv1", "rm2", "rv2", "nbt1", "nbt2",
             "dW1", "db1", "dg1", "dbe1", "dW2", "db2", "dW3", "db3", "dg2", "dbe2", "dW4", "db4")
    for got, name in zip(run_a, names):
        if got.is_floating_point():
            assert torch.isfinite(got).all(), name                # the poison (NaN / 1.5e16) is gone everywhere
        assert same_bits(got, want[name].detach().cpu().reshape(got.shape)), name
    for got in run_a[len(names):len(names) + 5]:
        assert torch.isfinite(got).all()


@pytest.mark.parametrize("which", ["sums1", "f2", "out", "dW4", "df2", "dW1"])
def test_tokenizer_refuses_a_pointer_off_16_bytes_and_writes_nothing(which):
    from unipre3d_amd import _lib, tokenizer
    lib = tokenizer.load()
    shape = (2, 5, 30, 40)
    B, G, n, C = shape
    M, rows = B * G, B * G * n
    _, stored, dout_cpu, w = _inputs(shape, False)
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    arena = Arena("cuda", 0x5A, 64 << 20)
    P = _lib.ptr
    st = _lib.stream_ptr(arena.buf.device)
    x = arena.inp(torch.from_numpy(stored), name="x")
    xa = [P(x), G * n * 3, n * 3, 3, 1, B, G, n]
    p = {k: arena.inp(torch.from_numpy(w[k]), name=k) for k in TR.PARAMS}
    dout = arena.inp(torch.from_numpy(dout_cpu), name="dout")
    spec = {"sums1": ((12,), f64), "sums2": ((1025,), f64), "sums3": ((1025,), f64), "sums1b": ((257,), f64), "fold1": ((1280,), f32),
            "fold2": ((2048,), f32), "f2": ((rows, 256), f32), "y3": ((rows, 512), f32), "g": ((M, 256), f32), "arg2": ((M, 256), i32),
            "out": ((M, C), f32), "arg4": ((M, C), i32), "dW4": ((C, 512), f32), "db4": ((C,), f32), "dh3m": ((rows, 512), f32),
            "dg2": ((512,), f32), "dbe2": ((512,), f32), "dW3": ((512, 512), f32), "db3": ((512,), f32), "dW2": ((256, 128), f32),
            "db2": ((256,), f32), "df2": ((rows, 256), f32), "dh1m": ((rows, 128), f32), "dg1": ((128,), f32), "dbe1": ((128,), f32),
            "dW1": ((128, 3), f32), "db1": ((128,), f32), "dx": ((rows, 3), f32)}
    # owned=0: nothing of these may be written by a refused call (their bytes are never looked at by one either)
    off = 8 if spec[which][1] == f64 else 4                       # (a placement moves by whole elements)
    b = {k: arena.out(s, dt, off if k == which else 0, owned=0, name=k) for k, (s, dt) in spec.items()}
    sc = arena.out((max(lib.u3d_tok_scratch_bytes(M, n, C if ph in (2, 3) else 1, ph, 1) for ph in range(6)),), torch.uint8, owned=0,
                   name="scratch")
    assert b[which].data_ptr() % 16 == off
    q = {k: P(v) for k, v in b.items()}
    calls = {
        "sums1": lambda: lib.u3d_tok_moments(*xa, q["sums1"], P(sc), st),
        "f2": lambda: lib.u3d_tok_fwd_a(*xa, P(p["W1"]), P(p["b1"]), P(p["g1"]), P(p["be1"]), P(p["W2"]), P(p["b2"]), P(p["W3"]), P(p["b3"]),
                                        q["sums1"], None, None, None, TR.EPS, TR.MOMENTUM, q["fold1"], q["f2"], q["g"], q["arg2"], q["y3"],
                                        q["sums2"], P(sc), st),
        "out": lambda: lib.u3d_tok_fwd_b(q["y3"], M, n, C, P(p["g2"]), P(p["be2"]), P(p["W4"]), P(p["b4"]), q["sums2"], None, None, None,
                                         TR.EPS, TR.MOMENTUM, q["fold2"], q["out"], q["arg4"], P(sc), st),
        "dW4": lambda: lib.u3d_tok_bwd_1(P(dout), q["y3"], q["arg4"], q["fold2"], P(p["W4"]), M, n, C, q["dW4"], q["db4"], q["dh3m"],
                                         q["sums3"], P(sc), st),
        "df2": lambda: lib.u3d_tok_bwd_2(*xa, q["dh3m"], q["y3"], q["f2"], q["g"], q["arg2"], q["fold1"], q["fold2"], P(p["g2"]),
                                         q["sums2"], q["sums2"], q["sums3"], q["sums3"], 1, P(p["W2"]), P(p["W3"]), q["dg2"], q["dbe2"], q["dW3"], q["db3"],
                                         q["dW2"], q["db2"], q["df2"], q["dh1m"], q["sums1b"], P(sc), st),
        "dW1": lambda: lib.u3d_tok_bwd_3(*xa, q["dh1m"], q["fold1"], P(p["g1"]), q["sums1"], q["sums1"], q["sums1b"], q["sums1b"], 1, P(p["W1"]), q["dg1"],
                                         q["dbe1"], q["dW1"], q["db1"], q["dx"], P(sc), st),
    }
    code = calls[which]()
    torch.cuda.synchronize()
    assert code == 1
    arena.check_guards()
    # a shape the library does not take is refused with 2, n = 0 with 1, before anything is launched
    assert lib.u3d_tok_moments(P(x), 1, 1, 1, 1, 1, 1, 257, q["sums2"], P(sc), st) == 2
    assert lib.u3d_tok_moments(P(x), 1, 1, 1, 1, 1, 1, 0, q["sums2"], P(sc), st) == 1
    torch.cuda.synchronize()
    arena.check_guards()
