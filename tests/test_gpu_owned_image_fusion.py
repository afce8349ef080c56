"""libunipre3d_image_fusion.so writes every element it owns and nothing else: its three compute entry points called directly, with every
pointer inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors, bit
for bit (tests/test_gpu_image_fusion.py holds the wrapper to the reference's fp64 record).

  entry point                 owned outputs (none pre-zeroed: they hold the poison before the call)
  u3d_imgfus_stats            stats (B, G, 2), and every byte of its scratch (u3d_imgfus_stats_scratch_bytes)
  u3d_imgfus_rows_forward     out (B N, Cout), the zero rows of the losers included
  u3d_imgfus_rows_backward    dW (Cout, Cin), dbias (Cout), dgamma, dbeta (Cin); scratch of u3d_imgfus_backward_scratch_bytes
  u3d_imgfus_abi_version, u3d_imgfus_stats_chunks, u3d_imgfus_row_splits and the two size functions are host only: called for their values

Cases (tests/image_fusion_ref.py::EDGE_SHAPES): two_splits (300 rows: two row splits with a ragged last one, ragged row, column and
reduction tiles, losers among the rows), split_group (a group cut into two chunks whose last is ragged and misaligned, B = 1) and none_win
(every output row is a zero row the kernel itself writes).
A pointer 4 bytes past a 16-byte boundary: the call returns 1 and not one byte of the arena changes."""
import numpy as np
import pytest
import torch

import image_fusion_ref as IR
from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

CASES = ["two_splits", "split_group", "none_win"]
PARAMS = ("gamma", "beta", "weight", "bias")


def _wrapper(inp, cam, G):
    from unipre3d_amd.image_fusion import ImageConv, sample_at_points
    Cout, Cin = inp["weight"].shape
    conv = ImageConv(Cin, Cout, num_groups=G, eps=IR.EPS).cuda()
    with torch.no_grad():
        for t, k in zip(conv.parameters(), PARAMS):
            t.copy_(torch.from_numpy(inp[k]).reshape(t.shape))
    out, sel = sample_at_points(conv, torch.from_numpy(inp["map"]).cuda(), torch.from_numpy(cam).cuda(), 1.0, 1.0, 0.0, 0.0)
    rows, _, stats = (t.clone() for t in out.grad_fn.saved_tensors[:3])
    dgamma, dbeta, dW, dbias = torch.autograd.grad(out, list(conv.parameters()), torch.from_numpy(inp["cot"]).cuda())
    torch.cuda.synchronize()
    return {"rows": rows.cpu(), "sel": sel.cpu(), "stats": stats.cpu(), "out": out.detach().reshape(-1, Cout).cpu(),
            "dW": dW.reshape(Cout, Cin).cpu(), "dbias": dbias.cpu(), "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu()}


@pytest.mark.parametrize("name", CASES)
def test_image_fusion_writes_what_it_owns(name):
    from unipre3d_amd import _lib, image_fusion
    lib = image_fusion.load()
    B, N, Cin, G, Cout, H, W, _ = IR.EDGE_SHAPES[name]
    inp, cam, sel_ref = IR.edge_inputs(name)
    want = _wrapper(inp, cam, G)
    assert np.array_equal(want["sel"].numpy(), sel_ref)
    assert lib.u3d_imgfus_abi_version() == image_fusion.ABI_VERSION
    assert lib.u3d_imgfus_stats_chunks(Cin, G, H, W) == IR.stats_chunks(Cin, G, H, W)
    assert lib.u3d_imgfus_row_splits(B * N) == IR.row_splits(B * N)
    s_stats, s_bwd = lib.u3d_imgfus_stats_scratch_bytes(B, Cin, G, H, W), lib.u3d_imgfus_backward_scratch_bytes(B, N, Cin, Cout)
    assert s_stats == B * G * IR.stats_chunks(Cin, G, H, W) * 16 and s_bwd > 0 and s_bwd % 16 == 0
    P, f32 = _lib.ptr, torch.float32

    def case_fn(arena):
        st = _lib.stream_ptr(arena.buf.device)
        xmap = arena.inp(torch.from_numpy(inp["map"]), name="map")
        p = {k: arena.inp(torch.from_numpy(inp[k]), name=k) for k in PARAMS}
        rows, sel = arena.inp(want["rows"], name="rows"), arena.inp(want["sel"], name="sel")
        cot = arena.inp(torch.from_numpy(inp["cot"]), name="cot")
        sc0, sc1 = arena.scratch(s_stats, name="stats_scratch"), arena.scratch(s_bwd, name="backward_scratch")
        stats = arena.out((B, G, 2), f32, name="stats")
        assert lib.u3d_imgfus_stats(P(xmap), B, Cin, G, H, W, IR.EPS, P(stats), P(sc0), st) == 0
        out = arena.out((B * N, Cout), f32, name="out")
        assert lib.u3d_imgfus_rows_forward(P(rows), P(sel), P(stats), P(p["gamma"]), P(p["beta"]), P(p["weight"]), P(p["bias"]), B, N, Cin, G,
                                           Cout, P(out), st) == 0
        dW, dbias = arena.out((Cout, Cin), f32, name="dW"), arena.out((Cout,), f32, name="dbias")
        dgamma, dbeta = arena.out((Cin,), f32, name="dgamma"), arena.out((Cin,), f32, name="dbeta")
        assert lib.u3d_imgfus_rows_backward(P(cot), P(rows), P(sel), P(stats), P(p["gamma"]), P(p["beta"]), P(p["weight"]), B, N, Cin, G, Cout,
                                            P(dW), P(dbias), P(dgamma), P(dbeta), P(sc1), st) == 0
        return [stats, out, dW, dbias, dgamma, dbeta, sc0]

    run_a, _ = run_twice(case_fn, "cuda")
    for got, key in zip(run_a, ("stats", "out", "dW", "dbias", "dgamma", "dbeta")):
        assert torch.isfinite(got).all(), key                          # the poison (NaN / 1.5e16) is gone everywhere
        assert same_bits(got, want[key].reshape(got.shape)), key


@pytest.mark.parametrize("which", ["stats", "out", "dW", "dbeta"])
def test_image_fusion_refuses_a_pointer_off_16_bytes_and_writes_nothing(which):
    from unipre3d_amd import _lib, image_fusion
    lib = image_fusion.load()
    B, N, Cin, G, Cout, H, W, _ = IR.EDGE_SHAPES["two_splits"]
    inp, _, sel = IR.edge_inputs("two_splits")
    arena = Arena("cuda", 0x5A)
    P, f32 = _lib.ptr, torch.float32
    st = _lib.stream_ptr(arena.buf.device)
    xmap = arena.inp(torch.from_numpy(inp["map"]), name="map")
    p = {k: arena.inp(torch.from_numpy(inp[k]), name=k) for k in PARAMS}
    rows = arena.inp(torch.from_numpy(IR.gather(inp["map"], sel)), name="rows")
    selt, cot = arena.inp(torch.from_numpy(sel), name="sel"), arena.inp(torch.from_numpy(inp["cot"]), name="cot")
    spec = {"stats": (B, G, 2), "out": (B * N, Cout), "dW": (Cout, Cin), "dbias": (Cout,), "dgamma": (Cin,), "dbeta": (Cin,)}
    # owned=0: nothing of these may be written by a refused call
    b = {k: arena.out(s, f32, 4 if k == which else 0, owned=0, name=k) for k, s in spec.items()}
    sc = arena.out((max(lib.u3d_imgfus_stats_scratch_bytes(B, Cin, G, H, W), lib.u3d_imgfus_backward_scratch_bytes(B, N, Cin, Cout)),),
                   torch.uint8, owned=0, name="scratch")
    assert b[which].data_ptr() % 16 == 4
    q = {k: P(v) for k, v in b.items()}
    fwd = lambda: lib.u3d_imgfus_rows_forward(P(rows), P(selt), q["stats"], P(p["gamma"]), P(p["beta"]), P(p["weight"]), P(p["bias"]), B, N, Cin,
                                              G, Cout, q["out"], st)
    bwd = lambda: lib.u3d_imgfus_rows_backward(P(cot), P(rows), P(selt), q["stats"], P(p["gamma"]), P(p["beta"]), P(p["weight"]), B, N, Cin, G,
                                               Cout, q["dW"], q["dbias"], q["dgamma"], q["dbeta"], P(sc), st)
    calls = {"stats": lambda: lib.u3d_imgfus_stats(P(xmap), B, Cin, G, H, W, IR.EPS, q["stats"], P(sc), st), "out": fwd, "dW": bwd, "dbeta": bwd}
    code = calls[which]()
    torch.cuda.synchronize()
    assert code == 1
    arena.check_guards()
    # a shape the library does not take is refused with 2, a group count that does not divide the channels with 1, before any launch
    assert lib.u3d_imgfus_rows_forward(P(rows), P(selt), q["stats"], P(p["gamma"]), P(p["beta"]), P(p["weight"]), P(p["bias"]), B, N, Cin, G,
                                       8193, q["out"], st) == 2
    assert lib.u3d_imgfus_stats(P(xmap), B, Cin, 5, H, W, IR.EPS, q["stats"], P(sc), st) == 1
    torch.cuda.synchronize()
    arena.check_guards()
