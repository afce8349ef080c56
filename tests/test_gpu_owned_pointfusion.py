"""libunipre3d_pointfusion.so writes every element it owns and nothing else: its entry points called directly, with every pointer inside
a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrappers on ordinary tensors, bit for bit
(tests/test_gpu_pointfusion.py holds the wrappers to the numpy restatement).

The outputs of compact / pick / inverse are sized for n_max = P rows, of which the library owns the first n (points that passed the
filters) or M (voxels); both are read from `meta` between the calls, as the wrapper does, must agree across the two runs, and the rows
beyond them must keep the poison -- as must the rows of coord_out beyond n that voxelize is handed but may not use.

  entry point                       cases
  u3d_pointfusion_minmax            50 points, one set (the box of the pipeline below)
  u3d_pointfusion_compact           P = 4097 pixels (two scan tiles, the second with one pixel) of which 1300 survive: the others have
  u3d_pointfusion_voxelize          w == 0 or lie outside the box; and P = 1.  voxelize takes n from meta[0] (n = -1), pick runs in
  u3d_pointfusion_pick              test mode, part 1, with src_map.  meta (4 words), voxel_offsets (2) and the scratch are whole
  u3d_pointfusion_inverse           placements.  And a ragged batch of four sets of (300, 0, 1, 700) points through set_offsets, with
                                    GridSample's own origin (origin 1, the (S, 6) minmax rows as min_coord) and the seeded train pick.
  u3d_pointfusion_gather_forward    (V, C, H, W, M) = (2, 7, 9, 11, 37), and M = 0 (forward: nothing to write, out NULL; backward: every
  u3d_pointfusion_gather_backward   element of grad_feat and of the pixel_map scratch is still written)
"""
import numpy as np
import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

GRID = 0.05


def _scene(P, keep):
    rng = np.random.default_rng(P)
    init = rng.uniform(0.0, 1.0, (50, 3)).astype(np.float32)
    lo, hi = init.min(0), init.max(0)
    uc = np.zeros((P, 4), np.float32)
    uc[:, :3] = rng.uniform(lo + 0.01, hi - 0.01, (P, 3)).astype(np.float32)
    uc[:, 3] = 1.0
    drop = rng.permutation(P)[:P - keep]
    uc[drop[::2], 3] = 0.0                       # invalid pixels ...
    uc[drop[1::2], :3] += 10.0                   # ... and valid ones outside the box
    return torch.from_numpy(init), torch.from_numpy(uc)


@pytest.mark.parametrize("P, keep, shape", [(4097, 1300, (1, 17, 241)), (1, 1, (1, 1, 1))])
def test_fusion_pipeline_writes_what_it_owns(P, keep, shape):
    from unipre3d_amd import _lib, pointfusion as pf
    lib = pf.load()
    init_cpu, uc_cpu = _scene(P, keep)
    nbytes = int(lib.u3d_pointfusion_scratch_bytes(P, 1))
    counts = []

    def case(arena):
        p, st = _lib.ptr, _lib.stream_ptr(torch.device("cuda:0"))
        init, uc = arena.inp(init_cpu, name="init_coord"), arena.inp(uc_cpu, name="uc4")
        box = arena.out((1, 6), torch.float32, name="minmax")
        assert lib.u3d_pointfusion_minmax(len(init_cpu), 1, None, p(init), p(box), st) == 0
        scratch = arena.out((nbytes,), torch.uint8, name="scratch")
        meta = arena.out((4,), torch.int32, name="meta")
        coord = arena.out((P, 3), torch.float32, name="coord_out")
        src_of_point = arena.out((P,), torch.int32, name="src_out")
        voxel_offsets = arena.out((2,), torch.int32, name="voxel_offsets")
        assert scratch.data_ptr() % 256 == 0
        assert lib.u3d_pointfusion_compact(P, p(uc), p(box), p(coord), p(src_of_point), p(meta), p(scratch), st) == 0
        assert lib.u3d_pointfusion_voxelize(P, -1, 1, None, p(coord), p(box), 6, 0, GRID, p(meta), p(voxel_offsets), p(scratch), st) == 0
        n, M, max_count, _ = meta.tolist()
        counts.append((n, M, max_count))
        assert n == keep and 1 <= M <= n
        index = arena.out((P,), torch.int64, owned=M, name="out_index")
        out_coord = arena.out((P, 3), torch.float32, owned=M, name="out_coord")
        grid = arena.out((P, 3), torch.int64, owned=M, name="out_grid")
        src = arena.out((P,), torch.int32, owned=M, name="out_src")
        inverse = arena.out((P,), torch.int64, owned=n, name="inverse")
        assert lib.u3d_pointfusion_pick(M, P, 1, None, p(voxel_offsets), p(coord), p(box), 6, 0, GRID, 1, 1, None, 0, p(src_of_point),
                                        p(index), p(out_coord), p(grid), p(src), p(scratch), st) == 0
        assert lib.u3d_pointfusion_inverse(n, P, 1, None, p(voxel_offsets), p(inverse), p(scratch), st) == 0
        return [box, meta, voxel_offsets, arena.own(coord, n), arena.own(src_of_point, n), index[:M], out_coord[:M], grid[:M], src[:M],
                inverse[:n]]

    run, _ = run_twice(case, "cuda")
    assert counts[0] == counts[1]
    n, M, max_count = counts[0]
    box, meta, voxel_offsets, coord, src_of_point, index, out_coord, grid, src, inverse = run

    kept = ((uc_cpu[:, 3] != 0) & (uc_cpu[:, :3] >= init_cpu.min(0).values).all(1) & (uc_cpu[:, :3] <= init_cpu.max(0).values).all(1))
    assert int(kept.sum()) == keep
    assert same_bits(box, torch.cat([init_cpu.min(0).values, init_cpu.max(0).values]).reshape(1, 6))
    assert same_bits(coord, uc_cpu[kept, :3]) and same_bits(src_of_point, torch.nonzero(kept).flatten().int())
    assert meta.tolist() == [n, M, max_count, 0] and voxel_offsets.tolist() == [0, M]

    V, H, W = shape
    feat = torch.zeros(V, 1, H, W, device="cuda")
    fused = pf.fuse_pixels(feat, uc_cpu.cuda().reshape(1, P, 4), init_cpu.cuda(), GRID, mode="test", part=1)
    assert fused["n"] == n
    assert same_bits(out_coord, fused["coord"]) and same_bits(grid, fused["grid_coord"]) and same_bits(src, fused["src_pixel"])
    sample = pf.grid_sample(coord.cuda(), GRID, min_coord=init_cpu.min(0).values, mode="test", part=1, return_inverse=True)
    assert sample["max_count"] == max_count
    assert same_bits(index, sample["index"]) and same_bits(inverse, sample["inverse"]) and same_bits(out_coord, sample["coord"])


def test_ragged_grid_sample_writes_what_it_owns():
    from unipre3d_amd import _lib, pointfusion as pf
    lib = pf.load()
    sizes = (300, 0, 1, 700)
    S, N = len(sizes), sum(sizes)
    rng = np.random.default_rng(S)
    coord_cpu = torch.from_numpy(rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32))
    offsets_cpu = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    nbytes = int(lib.u3d_pointfusion_scratch_bytes(N, S))
    seed = pf._seed(torch.Generator().manual_seed(7))
    counts = []

    def case(arena):
        p, st = _lib.ptr, _lib.stream_ptr(torch.device("cuda:0"))
        coord, offsets = arena.inp(coord_cpu, name="coord"), arena.inp(offsets_cpu, name="set_offsets")
        mins = arena.out((S, 6), torch.float32, name="minmax")
        assert lib.u3d_pointfusion_minmax(N, S, p(offsets), p(coord), p(mins), st) == 0
        scratch = arena.out((nbytes,), torch.uint8, name="scratch")
        meta, voxel_offsets = arena.out((4,), torch.int32, name="meta"), arena.out((S + 1,), torch.int32, name="voxel_offsets")
        assert lib.u3d_pointfusion_voxelize(N, N, S, p(offsets), p(coord), p(mins), 6, 1, GRID, p(meta), p(voxel_offsets), p(scratch), st) == 0
        n, M, max_count, _ = meta.tolist()
        counts.append((n, M, max_count))
        assert n == N and S - 1 <= M <= N
        index = arena.out((N,), torch.int64, owned=M, name="out_index")
        out_coord = arena.out((N, 3), torch.float32, owned=M, name="out_coord")
        grid = arena.out((N, 3), torch.int64, owned=M, name="out_grid")
        inverse = arena.out((N,), torch.int64, name="inverse")
        assert lib.u3d_pointfusion_pick(M, N, S, p(offsets), p(voxel_offsets), p(coord), p(mins), 6, 1, GRID, 0, 0, None, seed, None,
                                        p(index), p(out_coord), p(grid), None, p(scratch), st) == 0
        assert lib.u3d_pointfusion_inverse(N, N, S, p(offsets), p(voxel_offsets), p(inverse), p(scratch), st) == 0
        return [mins, meta, voxel_offsets, index[:M], out_coord[:M], grid[:M], inverse]

    run, _ = run_twice(case, "cuda")
    assert counts[0] == counts[1]
    mins, meta, voxel_offsets, index, out_coord, grid, inverse = run
    for s_, (a, e) in enumerate(zip(offsets_cpu[:-1].tolist(), offsets_cpu[1:].tolist())):
        if e > a:
            assert same_bits(mins[s_], torch.cat([coord_cpu[a:e].min(0).values, coord_cpu[a:e].max(0).values]))
    want = pf.grid_sample(coord_cpu.cuda(), GRID, None, "train", sizes=sizes, generator=torch.Generator().manual_seed(7), return_inverse=True)
    assert meta.tolist() == [N, counts[0][1], want["max_count"], 0]
    assert same_bits((voxel_offsets[1:] - voxel_offsets[:-1]).long(), want["voxel_sizes"]) and voxel_offsets[0].item() == 0
    assert same_bits(index, want["index"]) and same_bits(out_coord, want["coord"]) and same_bits(grid, want["grid_coord"])
    assert same_bits(inverse, want["inverse"])


@pytest.mark.parametrize("M", [37, 0])
def test_pixel_gather_writes_what_it_owns(M):
    from unipre3d_amd import _lib, pointfusion as pf
    lib = pf.load()
    V, C, H, W = 2, 7, 9, 11
    rng = np.random.default_rng(M)
    feat_cpu = torch.from_numpy(rng.standard_normal((V, C, H, W)).astype(np.float32))
    src_cpu = torch.from_numpy(rng.permutation(V * H * W)[:M].astype(np.int32))          # every pixel at most once
    g_cpu = torch.from_numpy(rng.standard_normal((M, C)).astype(np.float32))

    def case(arena):
        p, st = _lib.ptr, _lib.stream_ptr(torch.device("cuda:0"))
        feat = arena.inp(feat_cpu, name="feat")
        src = arena.inp(src_cpu, name="src") if M else None
        g = arena.inp(g_cpu, name="grad_out") if M else None
        out = arena.out((M, C), torch.float32, name="out") if M else None
        pixel_map = arena.out((V * H * W,), torch.int32, name="pixel_map")
        grad_feat = arena.out((V, C, H, W), torch.float32, name="grad_feat")
        assert lib.u3d_pointfusion_gather_forward(M, C, H * W, p(feat), p(src), p(out), st) == 0
        assert lib.u3d_pointfusion_gather_backward(V, C, H * W, M, p(g), p(src), p(pixel_map), p(grad_feat), st) == 0
        return [grad_feat, pixel_map] + ([out] if M else [])

    run, _ = run_twice(case, "cuda")
    want_map = torch.full((V * H * W,), -1, dtype=torch.int32)
    want_map[src_cpu.long()] = torch.arange(M, dtype=torch.int32)
    assert same_bits(run[1], want_map)
    if M:
        f = feat_cpu.cuda().requires_grad_(True)
        out = pf.pixel_gather(f, src_cpu.cuda())
        out.backward(g_cpu.cuda())
        assert same_bits(run[2], out.detach()) and same_bits(run[0], f.grad)
    else:
        assert same_bits(run[0], torch.zeros(V, C, H, W))
