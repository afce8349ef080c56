"""libunipre3d_feature_propagation.so writes every element it owns and nothing else: its four compute entry points called directly, with
every pointer inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors,
bit for bit (tests/test_gpu_feature_propagation.py holds the wrapper to the reference's fp64 record), and tests/feature_propagation_ref.py's
inverse lists.

  cases (B, N, S, D1, D2)
  (1, 16384, 8192, 4, 4)   the largest N: 49152 entries for u3d_feature_propagation_lists, 128 workgroups of the search
  (1, 7, 5, 3, 5)          workgroups with idle lanes everywhere, channel tiles that end early, one index out of range
  (1, 8, 4, 4, 2048)       the largest D2
  (2, 40, 1, 3, 5)         S = 1
  (1, 9, 6, 0, 5)          no points1: a null pointer with D1 = 0
  Outputs: idx, weight (B,N,3), ptr (B,S+1), ent (B,3N), out (B,D1+D2,N), dpoints2 (B,D2,S) and the lists' scratch, whose every byte
  u3d_feature_propagation_scratch_bytes counts is written; none pre-zeroed: they hold the poison before the call.  (The scratch keeps the
  entries in the order the atomic cursors dropped them, so it is held to its value range and to the cursors' final values, not to its bits.)
  A pointer 4 bytes past a 16-byte boundary: the call returns 1 and not one byte of the arena changes."""
import numpy as np
import pytest
import torch

import feature_propagation_ref as FR
from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

CASES = [(1, 16384, 8192, 4, 4), (1, 7, 5, 3, 5), (1, 8, 4, 4, 2048), (2, 40, 1, 3, 5), (1, 9, 6, 0, 5)]


def _inputs(B, N, S, D1, D2, seed):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a)
    return (t(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)), t(rng.uniform(-1, 1, (B, S, 3)).astype(np.float32)),
            t(rng.uniform(-1, 1, (B, D1, N)).astype(np.float32)) if D1 else None, t(rng.uniform(-1, 1, (B, D2, S)).astype(np.float32)),
            t(rng.uniform(-1, 1, (B, D1 + D2, N)).astype(np.float32)))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_feature_propagation_writes_what_it_owns(case):
    from unipre3d_amd import _lib, feature_propagation as fp
    lib = fp.load()
    B, N, S, D1, D2 = case
    xyz1_cpu, xyz2_cpu, p1_cpu, p2_cpu, dout_cpu = _inputs(*case, seed=N + D2)

    # the wrapper on ordinary tensors; the forward and backward entry points get an idx with one entry out of range
    idx_w, weight_w = fp.neighbours(xyz1_cpu.cuda(), xyz2_cpu.cuda())
    over = idx_w.clone()
    over[0, N // 2, 1] = -1
    a1, a2 = (None if p1_cpu is None else p1_cpu.cuda().requires_grad_(True)), p2_cpu.cuda().requires_grad_(True)
    out_w = fp.propagate(xyz1_cpu.cuda(), xyz2_cpu.cuda(), a1, a2, neighbours=(over, weight_w))
    (g2_w,) = torch.autograd.grad(out_w, (a2,), dout_cpu.cuda())
    over_cpu, weight_cpu = over.cpu(), weight_w.cpu()
    lists_ref = [torch.from_numpy(x) for x in FR.inverse_lists(over_cpu.numpy(), S)]
    nbytes = lib.u3d_feature_propagation_scratch_bytes(B, N, S)
    assert nbytes == 4 * B * (S + 1 + 3 * N)

    def case_fn(arena):
        xyz1, xyz2 = arena.inp(xyz1_cpu, name="xyz1"), arena.inp(xyz2_cpu, name="xyz2")
        st = _lib.stream_ptr(xyz1.device)
        idx, weight = arena.out((B, N, 3), torch.int32, name="idx"), arena.out((B, N, 3), torch.float32, name="weight")
        assert lib.u3d_feature_propagation_search(_lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(idx), _lib.ptr(weight), B, N, S, st) == 0
        # the other three on inputs of their own, so that each is checked on its own
        idx_in, w_in = arena.inp(over_cpu, name="idx_in"), arena.inp(weight_cpu, name="weight_in")
        ptr, ent = arena.out((B, S + 1), torch.int32, name="ptr"), arena.out((B, 3 * N), torch.int32, name="ent")
        sl = arena.out((nbytes,), torch.uint8, name="scratch_lists")
        assert lib.u3d_feature_propagation_lists(_lib.ptr(idx_in), _lib.ptr(ptr), _lib.ptr(ent), _lib.ptr(sl), B, N, S, st) == 0
        p1 = None if p1_cpu is None else arena.inp(p1_cpu, name="points1")
        p2, dout = arena.inp(p2_cpu, name="points2"), arena.inp(dout_cpu, name="dout")
        o = arena.out((B, D1 + D2, N), torch.float32, name="out")
        assert lib.u3d_feature_propagation_fwd(_lib.ptr(idx_in), _lib.ptr(w_in), _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(o), B, N, S, D1, D2,
                                               st) == 0
        p_in, e_in = arena.inp(lists_ref[0], name="ptr_in"), arena.inp(lists_ref[1], name="ent_in")
        dp2 = arena.out((B, D2, S), torch.float32, name="dpoints2")
        assert lib.u3d_feature_propagation_bwd(_lib.ptr(p_in), _lib.ptr(e_in), _lib.ptr(w_in), _lib.ptr(dout), _lib.ptr(dp2), B, N, S, D1,
                                               D2, st) == 0
        return [idx, weight, ptr, ent, o, dp2, sl]

    # scratch_lists (position 6) holds the entries as the atomic cursors dropped them: the one buffer whose order may differ between two
    # calls.  Every word of it is written all the same: none keeps a poison (-1 or 1515870810), each is a cursor or an entry.
    run, other = run_twice(case_fn, "cuda", deterministic=range(6), capacity=64 << 20)
    for r in (run, other):
        words = r[6].view(torch.int32)
        assert words.numel() == B * (S + 1 + 3 * N) and int(words.min()) >= 0 and int(words.max()) <= 3 * N, "scratch_lists"
        cur = words[:B * (S + 1)].view(B, S + 1)
        assert torch.equal(cur[:, :S], lists_ref[0][:, 1:]) and bool((cur[:, S] == 3 * N).all())      # each cursor ends at the next list's start
        tmp = words[B * (S + 1):].view(B, 3 * N)
        assert torch.equal(torch.sort(tmp, dim=1)[0], torch.arange(3 * N, dtype=torch.int32).expand(B, -1))
    want = [idx_w, weight_w, lists_ref[0], lists_ref[1], out_w.detach(), g2_w]
    for got, exp, name in zip(run[:6], want, ("idx", "weight", "ptr", "ent", "out", "dpoints2")):
        if got.is_floating_point():
            assert torch.isfinite(got).all(), name            # the poison (NaN / 1.5e16) is gone everywhere
        assert same_bits(got, exp), name


@pytest.mark.parametrize("which", ["xyz1", "xyz2", "idx", "weight", "ptr", "ent", "scratch", "points1", "points2", "out", "dout", "dpoints2"])
def test_feature_propagation_refuses_a_pointer_off_16_bytes_and_writes_nothing(which):
    from unipre3d_amd import _lib, feature_propagation as fp
    lib = fp.load()
    B, N, S, D1, D2 = CASES[1]
    xyz1_cpu, xyz2_cpu, p1_cpu, p2_cpu, dout_cpu = _inputs(B, N, S, D1, D2, seed=3)
    arena = Arena("cuda", 0x5A)
    off = lambda name: 4 if name == which else 0
    t = {"xyz1": arena.inp(xyz1_cpu, off("xyz1"), name="xyz1"), "xyz2": arena.inp(xyz2_cpu, off("xyz2"), name="xyz2"),
         "points1": arena.inp(p1_cpu, off("points1"), name="points1"), "points2": arena.inp(p2_cpu, off("points2"), name="points2"),
         "dout": arena.inp(dout_cpu, off("dout"), name="dout")}
    # owned=0: nothing of these may be written by a refused call (idx, weight, ptr and ent are inputs of some entry points and outputs of
    # others; a refused call looks at none of their bytes)
    for name, shape, dtype in (("idx", (B, N, 3), torch.int32), ("weight", (B, N, 3), torch.float32), ("ptr", (B, S + 1), torch.int32),
                               ("ent", (B, 3 * N), torch.int32), ("out", (B, D1 + D2, N), torch.float32),
                               ("dpoints2", (B, D2, S), torch.float32),
                               ("scratch", (lib.u3d_feature_propagation_scratch_bytes(B, N, S),), torch.uint8)):
        t[name] = arena.out(shape, dtype, off(name), owned=0, name=name)
    assert t[which].data_ptr() % 16 == 4
    p = {k: _lib.ptr(v) for k, v in t.items()}
    st = _lib.stream_ptr(t["out"].device)
    codes = {}
    if which in ("xyz1", "xyz2", "idx", "weight"):
        codes["search"] = lib.u3d_feature_propagation_search(p["xyz1"], p["xyz2"], p["idx"], p["weight"], B, N, S, st)
    if which in ("idx", "ptr", "ent", "scratch"):
        codes["lists"] = lib.u3d_feature_propagation_lists(p["idx"], p["ptr"], p["ent"], p["scratch"], B, N, S, st)
    if which in ("idx", "weight", "points1", "points2", "out"):
        codes["fwd"] = lib.u3d_feature_propagation_fwd(p["idx"], p["weight"], p["points1"], p["points2"], p["out"], B, N, S, D1, D2, st)
    if which in ("ptr", "ent", "weight", "dout", "dpoints2"):
        codes["bwd"] = lib.u3d_feature_propagation_bwd(p["ptr"], p["ent"], p["weight"], p["dout"], p["dpoints2"], B, N, S, D1, D2, st)
    torch.cuda.synchronize()
    assert codes and set(codes.values()) == {1}, codes
    arena.check_guards()


def test_feature_propagation_refuses_sizes_out_of_scope():
    from unipre3d_amd import _lib, feature_propagation as fp
    lib = fp.load()
    arena = Arena("cuda", 0x5A)
    buf = arena.out((4096,), torch.float32, owned=0, name="buf")
    p, st = _lib.ptr(buf), _lib.stream_ptr(buf.device)
    assert lib.u3d_feature_propagation_search(p, p, p, p, 1, 4, 2, st) == 2                  # S = 2
    assert lib.u3d_feature_propagation_search(p, p, p, p, 1, 16385, 4, st) == 2
    assert lib.u3d_feature_propagation_lists(p, p, p, p, 1, 4, 16385, st) == 2
    assert lib.u3d_feature_propagation_lists(p, p, p, p, 0, 4, 4, st) == 1
    assert lib.u3d_feature_propagation_fwd(p, p, p, p, p, 1, 4, 4, 2049, 4, st) == 2
    assert lib.u3d_feature_propagation_fwd(p, p, p, p, p, 1, 4, 4, 0, 0, st) == 1
    assert lib.u3d_feature_propagation_fwd(p, p, None, p, p, 1, 4, 4, 1, 4, st) == 1         # D1 > 0 needs points1
    assert lib.u3d_feature_propagation_bwd(p, p, p, p, p, 1, 4, 4, 4, 2049, st) == 2
    assert lib.u3d_feature_propagation_bwd(p, p, p, p, p, 4096, 4096, 4, 4, 4, st) == 2      # B N = 2^24
    assert lib.u3d_feature_propagation_scratch_bytes(1, 4, 2) == 0 and lib.u3d_feature_propagation_scratch_bytes(1, 4, 3) == 4 * (4 + 12)
    torch.cuda.synchronize()
    arena.check_guards()
