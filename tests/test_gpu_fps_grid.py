"""Furthest point sampling over a grid of workgroups (csrc/u3d_fps_grid.h): the dense entry point against the C oracle and against
u3d_furthest_point_sampling itself, the offset-batched one against tests/fps_ref.py.  Every comparison is exact integer equality;
shapes derive from P = u3d_fps_grid_points_per_workgroup(); the status word reads 0 after every case."""
import numpy as np
import pytest
import torch

import fps_ref
from oracle import pointops as po
from test_pointops_oracle import _cloud

pytestmark = pytest.mark.gpu
MODES = ("fma_llvm", "fma_chain", "none")


def _set_mode(mode):
    from unipre3d_amd import pointops
    po.set_contraction(mode)
    pointops.set_contraction(mode)


@pytest.fixture
def default_mode():
    _set_mode("fma_llvm")
    yield
    _set_mode("fma_llvm")


@pytest.fixture(params=MODES)
def mode(request):
    _set_mode(request.param)
    yield request.param
    _set_mode("fma_llvm")


def _P():
    from unipre3d_amd import pointops
    return int(pointops.load().u3d_fps_grid_points_per_workgroup())


def _workspace(b):
    from unipre3d_amd import pointops
    return torch.full((int(pointops.load().u3d_fps_grid_workspace_bytes(b)),), 0xAB, dtype=torch.uint8, device="cuda")   # the library clears it


def _status(ws):
    return int(ws[:4].view(torch.int32).item())


def _grid(xyz, m, stream=None, ws=None):
    """u3d_furthest_point_sampling_grid on (B,N,3) -> ((B,m) int32 tensor, workspace)."""
    from unipre3d_amd import _lib, pointops
    B, N, _ = xyz.shape
    ws = _workspace(B) if ws is None else ws
    out = torch.full((B, m), -7, dtype=torch.int32, device="cuda")
    rc = pointops.load().u3d_furthest_point_sampling_grid(B, N, m, _lib.ptr(xyz), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(xyz.device))
    assert rc == 0
    return out, ws


def _parent(xyz, m):
    """u3d_furthest_point_sampling, the one-workgroup-per-cloud path."""
    from unipre3d_amd import _lib, pointops
    B, N, _ = xyz.shape
    temp = torch.empty(B, N, dtype=torch.float32, device="cuda")
    out = torch.empty(B, m, dtype=torch.int32, device="cuda")
    assert pointops.load().u3d_furthest_point_sampling(B, N, m, _lib.ptr(xyz), _lib.ptr(temp), _lib.ptr(out), _lib.stream_ptr(xyz.device)) == 0
    return out


def _inputs(N, seed):
    """A random cloud, and a scaled integer lattice in shuffled order: its many equal distances fall on both sides of every slice
    boundary, so the winner of a tie and its runner-up usually sit in different workgroups."""
    return {"random": _cloud(1, N, seed=seed), "lattice": _cloud(1, N, seed=seed + 1, grid=True)}


@pytest.mark.parametrize("which", ["random", "lattice"])
@pytest.mark.parametrize("n_of_P", [lambda P: P + 1, lambda P: 2 * P, lambda P: 3 * P - 1], ids=["P+1", "2P", "3P-1"])
def test_dense_one_cloud(n_of_P, which, mode):
    N, M = n_of_P(_P()), 64
    xyz = _inputs(N, N)[which]
    want = po.furthest_point_sampling(xyz, M)
    dev = torch.from_numpy(xyz).cuda()
    got, ws = _grid(dev, M)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_parent(dev, M).cpu().numpy(), want)
    assert _status(ws) == 0


def test_dense_three_clouds_meet_independently(mode):
    N, M = 2 * _P() + 5, 48
    xyz = np.concatenate([_cloud(1, N, seed=3), _cloud(1, N, seed=4, grid=True), _cloud(1, N, seed=5) * 0.01])
    got, ws = _grid(torch.from_numpy(xyz).cuda(), M)
    assert np.array_equal(got.cpu().numpy(), po.furthest_point_sampling(xyz, M))
    assert _status(ws) == 0


@pytest.fixture(scope="module")
def many_meetings():
    """n = 5 P, m = 2000: every slot is recycled ~670 times.  'clustered': slices 1 and 3 are tight clumps near the origin that almost
    never hold the furthest point after the first few selections -- their workgroups arrive early and wait (uneven load)."""
    P = _P()
    N, M = 5 * P, 2000
    rng = np.random.RandomState(11)
    even = rng.randn(1, N, 3).astype(np.float32)
    clustered = even.copy()
    for s in (1, 3):
        clustered[0, s * P:(s + 1) * P] = (rng.randn(P, 3) * 1e-3).astype(np.float32)
    po.set_contraction("fma_llvm")
    return {k: (v, po.furthest_point_sampling(v, M)) for k, v in (("even", even), ("clustered", clustered))}


@pytest.mark.parametrize("which", ["even", "clustered"])
def test_many_meetings_recycle_the_slots(many_meetings, which, default_mode):
    xyz, want = many_meetings[which]
    got, ws = _grid(torch.from_numpy(xyz).cuda(), want.shape[1])
    assert np.array_equal(got.cpu().numpy(), want)
    if which == "clustered":
        P = _P()
        late = want[0, 200:]                                   # a clump is ~4e-3 across, far below the spacing of 2000 samples: it wins at most once or twice
        assert np.sum(((late >= P) & (late < 2 * P)) | ((late >= 3 * P) & (late < 4 * P))) <= 4    # ... so the load IS uneven
    assert _status(ws) == 0


def _ragged_cloud(sizes, seed):
    """Lattice rows (ties) in the small segments and in half of each large one, random rows elsewhere."""
    rng = np.random.RandomState(seed)
    parts = []
    for s in sizes:
        lat = (rng.randint(0, 12, (s, 3)) * 0.125).astype(np.float32)
        rnd = rng.randn(s, 3).astype(np.float32)
        parts.append(np.where((np.arange(s) % 2 == 0)[:, None] | (s < 1000), lat, rnd))
    return np.concatenate(parts).astype(np.float32)


def _offsets(sizes):
    return np.cumsum(np.asarray(sizes, dtype=np.int64)).astype(np.int32)


def test_ragged_mixed_segments(mode):
    """One-slice and multi-slice segments, a zero request, more selections than points, an all-points request."""
    from unipre3d_amd import offset_ops, pointops
    P = _P()
    sizes, req = [1, P + 1, 0, 700, 3 * P, 5], [1, 50, 0, 700, 90, 9]
    xyz = _ragged_cloud(sizes, 21)
    off, noff = _offsets(sizes), _offsets(req)
    want = fps_ref.furthestsampling_lex(xyz, off, noff, mode)
    got = offset_ops.furthestsampling(torch.from_numpy(xyz).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(noff).cuda())
    assert got.dtype == torch.int32 and got.shape == (sum(req),)
    assert np.array_equal(got.cpu().numpy(), want)
    assert pointops.grid_status(got.device) == 0


def test_ragged_without_sync(mode):
    """The same batch without its empty segment, int64 offsets, m passed: nothing reads the offsets on the host."""
    from unipre3d_amd import offset_ops, pointops
    P = _P()
    sizes, req = [1, P + 1, 700, 3 * P, 5], [1, 50, 700, 90, 9]
    xyz = _ragged_cloud(sizes, 22)
    off, noff = _offsets(sizes), _offsets(req)
    want = fps_ref.furthestsampling_lex(xyz, off, noff, mode)
    got = offset_ops.furthestsampling(torch.from_numpy(xyz).cuda(), torch.from_numpy(off).cuda().long(), torch.from_numpy(noff).cuda().long(),
                                      m=sum(req))
    assert np.array_equal(got.cpu().numpy(), want)
    assert pointops.grid_status(got.device) == 0


def test_ragged_empty_segment_asked_for_rows(default_mode):
    from unipre3d_amd import offset_ops, pointops
    sizes, req = [40, 0, 9], [5, 3, 4]
    xyz = _ragged_cloud(sizes, 23)
    off, noff = _offsets(sizes), _offsets(req)
    got = offset_ops.furthestsampling(torch.from_numpy(xyz).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(noff).cuda()).cpu().numpy()
    assert got[5:8].tolist() == [-1, -1, -1]
    assert np.array_equal(got, fps_ref.furthestsampling_ref(xyz, off, noff, "fma_llvm"))
    assert pointops.grid_status(torch.device("cuda", torch.cuda.current_device())) == 0


def test_ragged_entry_point_is_the_dense_one_with_offsets(default_mode):
    """u3d_offset_furthest_sampling on equal segments = the dense form plus the segment starts (one kernel, one flag)."""
    from unipre3d_amd import _lib, pointops
    P = _P()
    B, N, M = 2, P + 77, 40
    xyz = np.concatenate([_cloud(1, N, seed=8, grid=True), _cloud(1, N, seed=9)])
    dev = torch.from_numpy(xyz).cuda()
    off = torch.tensor([N, 2 * N], dtype=torch.int32, device="cuda")
    noff = torch.tensor([M, 2 * M], dtype=torch.int32, device="cuda")
    ws = _workspace(B)
    out = torch.full((B * M,), -7, dtype=torch.int32, device="cuda")
    assert pointops.load().u3d_offset_furthest_sampling(B, B * N, B * M, _lib.ptr(dev), _lib.ptr(off), _lib.ptr(noff), _lib.ptr(ws), _lib.ptr(out),
                                                        _lib.stream_ptr(dev.device)) == 0
    want = po.furthest_point_sampling(xyz, M) + np.arange(B, dtype=np.int32)[:, None] * N
    assert np.array_equal(out.cpu().numpy().reshape(B, M), want)
    assert _status(ws) == 0


def test_loader_stand_in(default_mode):
    """The scene-level loader's call: one cloud of 100 000 points through pointops.furthest_point_sample."""
    from unipre3d_amd import pointops
    xyz = _cloud(1, 100000, seed=31)
    got = pointops.furthest_point_sample(torch.from_numpy(xyz).cuda(), 512)
    assert np.array_equal(got.cpu().numpy(), po.furthest_point_sampling(xyz, 512))
    assert pointops.grid_status(got.device) == 0


def test_two_calls_in_flight(default_mode):
    """Two dense calls on two streams with separate workspaces: the library chains the grids, both results are sound."""
    P = _P()
    N, M = 3 * P, 300
    a, b = _cloud(1, N, seed=41), _cloud(1, N, seed=42, grid=True)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    wa, wb = _workspace(1), _workspace(1)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ga, _ = _grid(da, M, ws=wa)
    with torch.cuda.stream(s2):
        gb, _ = _grid(db, M, ws=wb)
    torch.cuda.synchronize()
    assert np.array_equal(ga.cpu().numpy(), po.furthest_point_sampling(a, M))
    assert np.array_equal(gb.cpu().numpy(), po.furthest_point_sampling(b, M))
    assert _status(wa) == 0 and _status(wb) == 0


def test_capacity_status_and_fallback(default_mode):
    """Beyond (256 - b) P rows the entry point returns 2 and launches nothing; furthest_point_sample then takes the one-workgroup path."""
    from unipre3d_amd import _lib, pointops
    P = _P()
    N = 255 * P + 1
    xyz = torch.from_numpy(_cloud(1, N, seed=51)).cuda()
    ws = _workspace(1)
    out = torch.full((1, 2), -7, dtype=torch.int32, device="cuda")
    lib = pointops.load()
    assert lib.u3d_furthest_point_sampling_grid(1, N, 2, _lib.ptr(xyz), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(xyz.device)) == 2
    assert out.cpu().tolist() == [[-7, -7]] and int(ws[0].item()) == 0xAB                  # nothing ran
    assert lib.u3d_furthest_point_sampling_grid(1, N - 1, 0, _lib.ptr(xyz), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(xyz.device)) == 0
    assert lib.u3d_furthest_point_sampling_grid(1, 16, 2, None, _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(xyz.device)) == 1
    got = pointops.furthest_point_sample(xyz, 2).cpu().numpy()
    assert np.array_equal(got, po.furthest_point_sampling(xyz.cpu().numpy(), 2))
