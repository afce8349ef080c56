"""libunipre3d_local_grouper.so writes every element it owns and nothing else: its three compute entry points called directly, with every
pointer inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors, bit
for bit (tests/test_gpu_local_grouper.py holds the wrapper to the reference's fp64 record), and tests/local_grouper_ref.py's inverse lists.

  entry point              cases (B, N, S, D, K), each with its mode, use_xyz, input layout and output layout
  u3d_local_grouper_lists  (1, 16384, 8192, 4, 2): the most rows; center, xyz, rows contiguous, channels first
  u3d_local_grouper_fwd    (1, 7, 5, 260, 3): a lane's fifth channel, workgroups with idle waves; anchor, xyz, transposed, channels last
  u3d_local_grouper_bwd    (1, 7, 5, 260, 3) again with no normalisation: no parameters, statistics or forward scratch
                           (1, 40, 33, 512, 32): the largest D; center, xyz, transposed, channels first
                           (2, 514, 514, 4, 2): S == N with no fps, points read through a batch stride of (N + 1) D; anchor, no xyz
                           Outputs: ptr, fptr (B,N+1), ent (B,S K), fent (B,S), out, new_xyz (B,S,3), mean (B,S,D+A), stats (B,4), dpoints,
                           dalpha and dbeta (D+A), and the scratch of each pass, whose every byte u3d_local_grouper_scratch_bytes counts is
                           written; none pre-zeroed: they hold the poison before the call.  (The lists' scratch keeps the entries in the
                           order the atomic cursors dropped them, so it is held to its value range, not to its bits.)
                           A pointer 4 bytes past a 16-byte boundary: the call returns 1 and not one byte of the arena changes.
"""
import numpy as np
import pytest
import torch

import local_grouper_ref as GR
from guarded import Arena, run_twice, same_bits

pytestmark = pytest.mark.gpu

# (B, N, S, D, K, mode, use_xyz, transposed, channels_first, padded batch stride)
CASES = [(1, 16384, 8192, 4, 2, "center", True, False, True, False), (1, 7, 5, 260, 3, "anchor", True, True, False, False),
         (1, 7, 5, 260, 3, None, True, True, False, False), (1, 40, 33, 512, 32, "center", True, True, True, False),
         (2, 514, 514, 4, 2, "anchor", False, False, True, True)]
MODES = {None: 0, "center": 1, "anchor": 2}
EPS = 1e-5


def _inputs(B, N, S, D, K, use_xyz, seed):
    rng = np.random.default_rng(seed)
    Cn = D + (3 if use_xyz else 0)
    fps = None if S == N else np.stack([rng.permutation(N)[:S] for _ in range(B)]).astype(np.int32)
    idx = rng.integers(0, N, (B, S, K)).astype(np.int32)
    idx[:, :, 0] = np.arange(S) if fps is None else fps
    idx[0, S // 2, 1] = -1                                   # one index out of range: never dereferenced
    if fps is not None:
        fps[0, 1] = fps[0, 0]                                # a duplicate anchor
    t = lambda a: torch.from_numpy(a)
    return (t(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)), t(rng.uniform(-1, 1, (B, N + 1, D)).astype(np.float32)),
            None if fps is None else t(fps), t(idx), t(rng.uniform(0.5, 1.5, Cn).astype(np.float32)),
            t(rng.uniform(-0.5, 0.5, Cn).astype(np.float32)), t(rng.uniform(-1, 1, (B, S, K, D + Cn)).astype(np.float32)))


def _layout(full_cpu, transposed, padded):
    """(host tensor to place, offset of element (0, 0, 0) in floats, (batch, point, channel) strides) of the (B, N, D) points: rows 1 .. N
    of `full` (B, N + 1, D) when padded, else a copy of them, as rows or as (B, D, N)."""
    B, N1, D = full_cpu.shape
    N = N1 - 1
    if padded:
        return full_cpu, D, (N1 * D, D, 1)
    p = full_cpu[:, 1:, :]
    return (p.permute(0, 2, 1).contiguous(), 0, (N * D, 1, N)) if transposed else (p.contiguous(), 0, (N * D, D, 1))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:5])) + f"_{c[5]}")
def test_local_grouper_writes_what_it_owns(case):
    from unipre3d_amd import _lib, local_grouper as lg
    lib = lg.load()
    B, N, S, D, K, mode, use_xyz, transposed, cf, padded = case
    nm, ux = MODES[mode], int(use_xyz)
    Cn, C = D + 3 * ux, 2 * D + 3 * ux
    xyz_cpu, full_cpu, fps_cpu, idx_cpu, alpha_cpu, beta_cpu, dout_cpu = _inputs(B, N, S, D, K, use_xyz, N + D)
    placed_cpu, first, (sb, sp, sc) = _layout(full_cpu, transposed, padded)
    dout_placed = dout_cpu.permute(0, 1, 3, 2).contiguous() if cf else dout_cpu

    # the wrapper on ordinary tensors
    leaf = placed_cpu.cuda().requires_grad_(True)
    pts = leaf[:, 1:, :] if padded else (leaf.permute(0, 2, 1) if transposed else leaf)
    a = b = None
    if mode is not None:
        a, b = alpha_cpu.cuda().requires_grad_(True), beta_cpu.cuda().requires_grad_(True)
    fps_dev = None if fps_cpu is None else fps_cpu.cuda()
    out, new_xyz, stats = lg._LocalGroup.apply(xyz_cpu.cuda(), pts, a, b, fps_dev, idx_cpu.cuda(), nm, use_xyz, EPS, cf)
    mean = out.grad_fn.saved_tensors[3] if mode is not None else None
    out.backward(dout_placed.cuda())
    grad = leaf.grad[:, 1:, :].contiguous() if padded else leaf.grad
    if padded:
        assert not leaf.grad[:, 0].any()
    lists_ref = [torch.from_numpy(x) for x in GR.inverse_lists(None if fps_cpu is None else fps_cpu.numpy(), idx_cpu.numpy(), N)]
    nbytes = [lib.u3d_local_grouper_scratch_bytes(B, N, S, K, D, ux, nm, p) for p in (0, 1, 2)]
    assert nbytes[1] > 0 and nbytes[2] > 0 and (nbytes[0] > 0) == (mode is not None)

    def case_fn(arena):
        xyz, pl, idx, dout = arena.inp(xyz_cpu, name="xyz"), arena.inp(placed_cpu, name="points"), arena.inp(idx_cpu, name="idx"), \
            arena.inp(dout_placed, name="dout")
        fps = None if fps_cpu is None else arena.inp(fps_cpu, name="fps")
        al = be = None
        if mode is not None:
            al, be = arena.inp(alpha_cpu, name="alpha"), arena.inp(beta_cpu, name="beta")
        st = _lib.stream_ptr(xyz.device)
        p_ptr = pl.data_ptr() + 4 * first
        ptr, fptr = arena.out((B, N + 1), torch.int32, name="ptr"), arena.out((B, N + 1), torch.int32, name="fptr")
        ent, fent = arena.out((B, S * K), torch.int32, name="ent"), arena.out((B, S), torch.int32, name="fent")
        sl = arena.out((nbytes[2],), torch.uint8, name="scratch_lists")
        assert lib.u3d_local_grouper_lists(_lib.ptr(fps), _lib.ptr(idx), _lib.ptr(ptr), _lib.ptr(ent), _lib.ptr(fptr), _lib.ptr(fent),
                                           _lib.ptr(sl), B, N, S, K, st) == 0
        o = arena.out(tuple(dout_placed.shape), torch.float32, name="out")
        nx = arena.out((B, S, 3), torch.float32, name="new_xyz")
        owned = [ptr, ent, fptr, fent, o, nx]
        mn = sx = sf = None
        if mode is not None:
            mn, sx = arena.out((B, S, Cn), torch.float32, name="mean"), arena.out((B, 4), torch.float32, name="stats")
            sf = arena.out((nbytes[0],), torch.uint8, name="scratch_fwd")
        assert lib.u3d_local_grouper_fwd(_lib.ptr(xyz), p_ptr, sb, sp, sc, _lib.ptr(fps), _lib.ptr(idx), _lib.ptr(al), _lib.ptr(be),
                                         _lib.ptr(o), _lib.ptr(nx), _lib.ptr(mn), _lib.ptr(sx), _lib.ptr(sf), B, N, S, K, D, ux, nm,
                                         int(cf), EPS, st) == 0
        # the backward on inputs of its own, so that it is checked on its own
        p_in, e_in, fp_in, fe_in = (arena.inp(t, name=n) for t, n in zip(lists_ref, ("ptr_in", "ent_in", "fptr_in", "fent_in")))
        m_in = s_in = None
        if mode is not None:
            m_in, s_in = arena.inp(mean.cpu(), name="mean_in"), arena.inp(stats.cpu(), name="stats_in")
        gshape, (gb, gp, gc) = ((B, D, N), (N * D, 1, N)) if transposed else ((B, N, D), (N * D, D, 1))
        dp = arena.out(gshape, torch.float32, name="dpoints")
        da = db = None
        if mode is not None:
            da, db = arena.out((Cn,), torch.float32, name="dalpha"), arena.out((Cn,), torch.float32, name="dbeta")
        sbw = arena.out((nbytes[1],), torch.uint8, name="scratch_bwd")
        assert lib.u3d_local_grouper_bwd(_lib.ptr(xyz), p_ptr, sb, sp, sc, _lib.ptr(fps), _lib.ptr(idx), _lib.ptr(p_in), _lib.ptr(e_in),
                                         _lib.ptr(fp_in), _lib.ptr(fe_in), _lib.ptr(al), _lib.ptr(m_in), _lib.ptr(s_in), _lib.ptr(dout),
                                         _lib.ptr(dp), gb, gp, gc, _lib.ptr(da), _lib.ptr(db), _lib.ptr(sbw), B, N, S, K, D, ux, nm, int(cf),
                                         st) == 0
        owned += [dp, sl, sbw]
        if mode is not None:
            owned += [mn, sx, da, db, sf]
        return owned

    # scratch_lists (position 7) holds the lists' entries as the atomic cursors dropped them: the one buffer whose order may differ between
    # two calls.  Every word of it is written all the same: none keeps a poison (-1 or 1515870810), each is a cursor or an entry.
    count = 13 if mode is not None else 9
    run, other = run_twice(case_fn, "cuda", deterministic=[i for i in range(count) if i != 7], capacity=64 << 20)
    for r in (run, other):
        words = r[7].view(torch.int32)
        assert words.numel() == B * (N + S * K + S) and int(words.min()) >= 0 and int(words.max()) <= S * K, "scratch_lists"
        assert torch.equal(words[:B * N].view(B, N), lists_ref[2][:, 1:])          # the cursors end at the next list's start
    want = lists_ref[:2] + lists_ref[2:] + [out.detach(), new_xyz, grad]
    names = ["ptr", "ent", "fptr", "fent", "out", "new_xyz", "dpoints"]
    for got, exp, name in zip(run[:7], want, names):
        if got.is_floating_point():
            assert torch.isfinite(got).all(), name            # the poison (NaN / 1.5e16) is gone everywhere
        assert same_bits(got, exp), name
    if mode is not None:
        for got, exp, name in zip(run[9:13], (mean, stats, a.grad, b.grad), ("mean", "stats", "dalpha", "dbeta")):
            assert torch.isfinite(got).all() and same_bits(got, exp), name


@pytest.mark.parametrize("which", ["xyz", "points", "fps", "idx", "ptr", "ent", "fptr", "fent", "alpha", "beta", "out", "new_xyz", "mean",
                                   "stats", "dout", "dpoints", "dalpha", "dbeta", "scratch"])
def test_local_grouper_refuses_a_pointer_off_16_bytes_and_writes_nothing(which):
    from unipre3d_amd import _lib, local_grouper as lg
    lib = lg.load()
    B, N, S, D, K = CASES[1][:5]
    Cn, C = D + 3, 2 * D + 3
    xyz_cpu, full_cpu, fps_cpu, idx_cpu, alpha_cpu, beta_cpu, dout_cpu = _inputs(B, N, S, D, K, True, 3)
    arena = Arena("cuda", 0x5A)
    off = lambda name: 4 if name == which else 0
    t = {"xyz": arena.inp(xyz_cpu, off("xyz"), name="xyz"), "points": arena.inp(full_cpu[:, 1:, :], off("points"), name="points"),
         "fps": arena.inp(fps_cpu, off("fps"), name="fps"), "idx": arena.inp(idx_cpu, off("idx"), name="idx"),
         "alpha": arena.inp(alpha_cpu, off("alpha"), name="alpha"), "beta": arena.inp(beta_cpu, off("beta"), name="beta"),
         "dout": arena.inp(dout_cpu, off("dout"), name="dout")}
    # owned=0: nothing of these outputs may be written by a refused call
    for name, shape, dtype in (("ptr", (B, N + 1), torch.int32), ("ent", (B, S * K), torch.int32), ("fptr", (B, N + 1), torch.int32),
                               ("fent", (B, S), torch.int32), ("out", (B, S, K, C), torch.float32), ("new_xyz", (B, S, 3), torch.float32),
                               ("mean", (B, S, Cn), torch.float32), ("stats", (B, 4), torch.float32), ("dpoints", (B, N, D), torch.float32),
                               ("dalpha", (Cn,), torch.float32), ("dbeta", (Cn,), torch.float32),
                               ("scratch", (max(lib.u3d_local_grouper_scratch_bytes(B, N, S, K, D, 1, 2, p) for p in (0, 1, 2)),), torch.uint8)):
        t[name] = arena.out(shape, dtype, off(name), owned=0, name=name)
    assert t[which].data_ptr() % 16 == 4
    p = {k: _lib.ptr(v) for k, v in t.items()}
    st = _lib.stream_ptr(t["out"].device)
    codes = {}
    if which in ("fps", "idx", "ptr", "ent", "fptr", "fent", "scratch"):
        codes["lists"] = lib.u3d_local_grouper_lists(p["fps"], p["idx"], p["ptr"], p["ent"], p["fptr"], p["fent"], p["scratch"], B, N, S, K, st)
    if which in ("xyz", "points", "fps", "idx", "alpha", "beta", "out", "new_xyz", "mean", "stats", "scratch"):
        codes["fwd"] = lib.u3d_local_grouper_fwd(p["xyz"], p["points"], N * D, D, 1, p["fps"], p["idx"], p["alpha"], p["beta"], p["out"],
                                                 p["new_xyz"], p["mean"], p["stats"], p["scratch"], B, N, S, K, D, 1, 2, 0, EPS, st)
    if which not in ("beta", "out", "new_xyz"):
        # (the backward reads mean, stats and the lists: the same placements serve, their bytes are never looked at by a refused call)
        codes["bwd"] = lib.u3d_local_grouper_bwd(p["xyz"], p["points"], N * D, D, 1, p["fps"], p["idx"], p["ptr"], p["ent"], p["fptr"],
                                                 p["fent"], p["alpha"], p["mean"], p["stats"], p["dout"], p["dpoints"], N * D, D, 1,
                                                 p["dalpha"], p["dbeta"], p["scratch"], B, N, S, K, D, 1, 2, 0, st)
    torch.cuda.synchronize()
    assert codes and set(codes.values()) == {1}, codes
    arena.check_guards()
