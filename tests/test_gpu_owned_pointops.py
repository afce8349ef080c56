"""libunipre3d_pointops.so writes every element it owns and nothing else: its eleven launching entry points called directly, with every
pointer inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrappers on ordinary tensors,
bit for bit (tests/test_gpu_pointops*.py and test_gpu_fps_grid.py hold the wrappers to their references), plus tests/fps_ref.py for the
offset form and tests/pointops_grad_ref.py for the three accumulating gradients.

Constants that decide a class are read from unipre3d_amd/csrc/u3d_pointops.hip (GP_CH, IL_CB, NN_TILE) or asked of the library (P =
u3d_fps_grid_points_per_workgroup); the class of a case is asserted through the library's host-arithmetic queries before the case runs.

  entry point                       cases (class query asserted)
  u3d_furthest_point_sampling       b = 2, m = 4 (m = 3 at n = 3); one n per kernel the host code selects: 3, 128 (wave kernel, two points per
                                    lane), 129 (four per lane), 257 (eight per lane), 513, 1025, 2049, 4097 (the four multi-wave classes),
                                    5462 (the first n whose staging takes the opt-in beyond 64 KB of LDS), 8193 (fps_kernel_large).  `temp` as
                                    the wrapper passes it: NULL up to 8192; at 8193 an owned (B, N) output, checked for its guards and for
                                    independence from the poison (the header calls it unused scratch; the large kernel writes all of it).
                                    n = 8193 with temp = NULL: returns 1, the arena is untouched.
  u3d_furthest_point_sampling_grid  b = 2, n = P + 1 (two slices per cloud), m = 4; the workspace a guarded scratch of exactly
                                    u3d_fps_grid_workspace_bytes(b), left out of the comparison, its first word 0 after the call; idx = the
                                    one-workgroup entry point's.
  u3d_offset_furthest_sampling      segments of (5, 0, P + 3) rows asked for (2, 1, 4) selections; idx two rows longer than new_offset[-1], of
                                    which only the first new_offset[-1] are owned (the tail keeps the poison); the empty segment's row is -1;
                                    = offset_ops.furthestsampling = fps_ref.furthestsampling_lex.
  u3d_ball_query                    b = 2, n = 70, m = 37, nsample 1 and 16; query 5 of cloud 0 has no support point within the radius: its
                                    row is written as zeros.
  u3d_group_points                  b = 2, n = 23, c = 1 and GP_CH + 1, three forms (u3d_group_points_form): vector (npoints * nsample = 36,
  u3d_gather_points (nsample = 1)   idx and out on 16 bytes: 1), scalar because the total is 27 (0), scalar because `out` sits 4 bytes past a
                                    16-byte boundary at a total of 36 (0; no torch allocation is ever so placed).
  u3d_three_nn                      b = 2, n = 37; m = 70; m = 2 (the unfilled slot is +inf with index 0); m = 0 with known = NULL (all three);
                                    m = NN_TILE + 1 (the second tile of known points holds one point, a query's nearest: m = 70 alone stays
                                    inside one tile).
  u3d_three_interpolate             n = 37, c = 1 and IL_CB + 1, both forms of u3d_three_interpolate_form: m = 70 (1: rows staged in LDS) and
                                    m = 2049 (0: global gather).
  u3d_group_points_grad (+)         every rows-per-workgroup class u3d_group_points_grad_rows / u3d_three_interpolate_grad_rows answer: 1, 2, 4, 8,
  u3d_gather_points_grad (+)        16 at n resp. m = 24 and c = 37 or 3073 (never a multiple of the class: the last workgroup has fewer rows),
  u3d_three_interpolate_grad (+)    and 0 (the global-atomic kernel) at a row of 16385 floats.  (+): they accumulate, so grad_points is
                                    prefilled inside the case with integers from -3 .. 3 and prefill + gradient is expected.  Cotangents are
                                    integers and weights multiples of 1/8 (as in tests/pointops_grad_ref.py): every partial sum is exact in any
                                    order, so the outputs are deterministic despite the atomics and equal the fp64 reference exactly.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import fps_ref
import pointops_grad_ref as GR
from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

SOURCE = (Path(__file__).resolve().parent.parent / "unipre3d_amd" / "csrc" / "u3d_pointops.hip").read_text()


def _const(name):
    return int(re.search(rf"constexpr int (?:\w+ = \d+, )*{name} = (\d+)", SOURCE).group(1))


GP_CH, IL_CB, NN_TILE = _const("GP_CH"), _const("IL_CB"), _const("NN_TILE")
FPS_N = (3, 128, 129, 257, 513, 1025, 2049, 4097, 5462, 8193)
# (b, c, row length) per rows-per-workgroup class
GRAD_SHAPES = {1: (2, 37, 24), 2: (1, 3073, 24), 4: (3, 3073, 24), 8: (7, 3073, 24), 16: (15, 3073, 24), 0: (1, 3, 16385)}


def _lib():
    from unipre3d_amd import pointops
    return pointops.load()


def _cloud(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def _p(view):
    from unipre3d_amd import _lib as L
    return L.ptr(view)


def _stream():
    from unipre3d_amd import _lib as L
    return L.stream_ptr(torch.device("cuda:0"))


# ---- furthest point sampling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FPS_N)
def test_furthest_point_sampling_writes_what_it_owns(n):
    from unipre3d_amd import pointops
    lib, b, m = _lib(), 2, min(4, n)
    xyz = _cloud(np.random.default_rng(n), b, n, 3)
    with_temp = n > 8192

    def case(arena):
        x = arena.inp(xyz, name="points")
        temp = arena.out((b, n), torch.float32, name="temp") if with_temp else None
        idx = arena.out((b, m), torch.int32, name="idx")
        assert lib.u3d_furthest_point_sampling(b, n, m, _p(x), _p(temp), _p(idx), _stream()) == 0
        return [idx] + ([temp] if with_temp else [])

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], pointops.furthest_point_sample(xyz.cuda(), m))
    assert (run[0][:, 0] == 0).all() and int(run[0].min()) >= 0 and int(run[0].max()) < n


def test_furthest_point_sampling_large_without_temp_is_refused_before_any_launch():
    lib, b, n, m = _lib(), 2, 8193, 4
    xyz = _cloud(np.random.default_rng(1), b, n, 3)

    def case(arena):
        x = arena.inp(xyz, name="points")
        idx = arena.out((b, m), torch.int32, owned=0, name="idx")
        assert lib.u3d_furthest_point_sampling(b, n, m, _p(x), None, _p(idx), _stream()) == 1
        return []

    run_twice(case, "cuda")


def test_furthest_point_sampling_grid_writes_what_it_owns():
    from unipre3d_amd import pointops
    lib, b, m = _lib(), 2, 4
    P = int(lib.u3d_fps_grid_points_per_workgroup())
    n = P + 1
    assert -(-n // P) == 2
    xyz = _cloud(np.random.default_rng(7), b, n, 3)
    ws_bytes = int(lib.u3d_fps_grid_workspace_bytes(b))
    assert ws_bytes >= 4

    def case(arena):
        x = arena.inp(xyz, name="points")
        ws = arena.scratch(ws_bytes, name="workspace")
        idx = arena.out((b, m), torch.int32, name="idx")
        assert lib.u3d_furthest_point_sampling_grid(b, n, m, _p(x), _p(ws), _p(idx), _stream()) == 0
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "the status word"
        return [idx]

    run, _ = run_twice(case, "cuda")
    dev = xyz.cuda()
    want = torch.empty(b, m, dtype=torch.int32, device="cuda")
    assert n <= 8192 and lib.u3d_furthest_point_sampling(b, n, m, _p(dev), None, _p(want), _stream()) == 0
    assert same_bits(run[0], want) and same_bits(run[0], pointops.furthest_point_sample(dev, m))


def test_offset_furthest_sampling_writes_what_it_owns():
    from unipre3d_amd import offset_ops, pointops
    lib = _lib()
    P = int(lib.u3d_fps_grid_points_per_workgroup())
    rows, asked, extra = (5, 0, P + 3), (2, 1, 4), 2
    offset, new_offset = np.cumsum(rows).astype(np.int32), np.cumsum(asked).astype(np.int32)
    b, n, m_own = len(rows), int(offset[-1]), int(new_offset[-1])
    m = m_own + extra
    xyz = _cloud(np.random.default_rng(9), n, 3)
    ws_bytes = int(lib.u3d_fps_grid_workspace_bytes(b))

    def case(arena):
        x, off, noff = (arena.inp(t, name=nm) for t, nm in ((xyz, "xyz"), (torch.from_numpy(offset), "offset"), (torch.from_numpy(new_offset), "new_offset")))
        ws = arena.scratch(ws_bytes, name="workspace")
        idx = arena.out((m,), torch.int32, name="idx")
        owned = arena.own(idx, m_own)
        assert lib.u3d_offset_furthest_sampling(b, n, m, _p(x), _p(off), _p(noff), _p(ws), _p(idx), _stream()) == 0
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "the status word"
        return [owned]

    run, _ = run_twice(case, "cuda")
    got = run[0]
    want = offset_ops.furthestsampling(xyz.cuda(), torch.from_numpy(offset).cuda(), torch.from_numpy(new_offset).cuda(), m=m)
    assert (want[m_own:] == -1).all() and same_bits(got, want[:m_own])
    mode = {v: k for k, v in pointops.CONTRACTIONS.items()}[int(lib.u3d_pointops_get_contraction())]
    ref = fps_ref.furthestsampling_lex(xyz.numpy(), offset, new_offset, mode, m=m_own)
    assert np.array_equal(got.numpy(), ref)
    assert got[2] == -1 and got[0] == 0 and got[3] == 5 and (got[3:] >= 5).all() and (got[3:] < n).all()


# ---- ball query ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [1, 16])
def test_ball_query_writes_what_it_owns(nsample):
    from unipre3d_amd import pointops
    lib, b, n, m, radius = _lib(), 2, 70, 37, 0.7
    rng = np.random.default_rng(70)
    xyz = torch.from_numpy(rng.uniform(-1, 1, (b, n, 3)).astype(np.float32))
    new_xyz = torch.from_numpy(rng.uniform(-1, 1, (b, m, 3)).astype(np.float32))
    new_xyz[0, 5] = torch.tensor([10.0, 10.0, 10.0])             # no support point within the radius
    d2 = ((new_xyz.double()[:, :, None] - xyz.double()[:, None]) ** 2).sum(-1)
    hits = (d2 < radius ** 2 * (1 - 1e-6)).sum(-1)
    assert hits[0, 5] == 0 and (d2[0, 5] > 100).all() and int(hits.max()) > 1 and (nsample == 1 or int((hits > 0).sum()) > b * m // 2)

    def case(arena):
        q, x = arena.inp(new_xyz, name="new_xyz"), arena.inp(xyz, name="xyz")
        idx = arena.out((b, m, nsample), torch.int32, name="idx")
        assert lib.u3d_ball_query(b, n, m, radius, nsample, _p(q), _p(x), _p(idx), _stream()) == 0
        return [idx]

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], pointops.ball_query(radius, nsample, xyz.cuda(), new_xyz.cuda()))
    assert (run[0][0, 5] == 0).all() and int(run[0].min()) >= 0 and int(run[0].max()) < n


# ---- group / gather ----------------------------------------------------------------------------------------------------------------------------
FORMS = {"vector": (36, 0, 1), "scalar_total": (27, 0, 0), "scalar_misaligned_out": (36, 4, 0)}   # total, misalign of out, form


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c", [1, GP_CH + 1])
@pytest.mark.parametrize("op", ["group", "gather"])
def test_group_and_gather_points_write_what_they_own(op, c, form):
    from unipre3d_amd import pointops
    lib, b, n = _lib(), 2, 23
    total, misalign, want_form = FORMS[form]
    npoints, nsample = (total // (4 if total % 4 == 0 else 3), 4 if total % 4 == 0 else 3) if op == "group" else (total, 1)
    assert npoints * nsample == total
    rng = np.random.default_rng(c * 100 + total)
    points = _cloud(rng, b, c, n)
    index = torch.from_numpy(rng.integers(0, n, (b, npoints, nsample) if op == "group" else (b, npoints)).astype(np.int32))
    index.view(b, -1)[:, 0], index.view(b, -1)[:, -1] = n - 1, 0

    def case(arena):
        p, i = arena.inp(points, name="points"), arena.inp(index, name="idx")
        out = arena.out((b, c, npoints, nsample) if op == "group" else (b, c, npoints), torch.float32, misalign=misalign, name="out")
        assert out.data_ptr() % 16 == misalign and i.data_ptr() % 16 == 0
        assert lib.u3d_group_points_form(npoints, nsample, _p(i), _p(out)) == want_form
        if op == "group":
            assert lib.u3d_group_points(b, c, n, npoints, nsample, _p(p), _p(i), _p(out), _stream()) == 0
        else:
            assert lib.u3d_gather_points(b, c, n, npoints, _p(p), _p(i), _p(out), _stream()) == 0
        return [out]

    run, _ = run_twice(case, "cuda")
    wrapper = pointops.grouping_operation if op == "group" else pointops.gather_operation
    assert same_bits(run[0], wrapper(points.cuda(), index.cuda()))


# ---- three_nn / three_interpolate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [70, 2, 0, NN_TILE + 1])
def test_three_nn_writes_what_it_owns(m):
    from unipre3d_amd import pointops
    lib, b, n = _lib(), 2, 37
    rng = np.random.default_rng(300 + m)
    unknown, known = _cloud(rng, b, n, 3), _cloud(rng, b, m, 3)
    if m > NN_TILE:
        known[0, NN_TILE] = unknown[0, 0]                         # the lone point of the second tile is someone's nearest neighbour

    def case(arena):
        u = arena.inp(unknown, name="unknown")
        k = arena.inp(known, name="known") if m else None
        dist2 = arena.out((b, n, 3), torch.float32, name="dist2")
        idx = arena.out((b, n, 3), torch.int32, name="idx")
        assert lib.u3d_three_nn(b, n, m, _p(u), _p(k), _p(dist2), _p(idx), _stream()) == 0
        return [dist2, idx]

    run, _ = run_twice(case, "cuda")
    want_d, want_i = pointops.three_nn(unknown.cuda(), known.cuda())
    assert same_bits(run[1], want_i) and same_bits(torch.sqrt(run[0].cuda()), want_d)
    filled = min(m, 3)
    assert torch.isfinite(run[0][:, :, :filled]).all() and (run[0][:, :, :filled] >= 0).all()
    assert (run[0][:, :, filled:] == float("inf")).all() and (run[1][:, :, filled:] == 0).all()
    if m > NN_TILE:
        assert run[1][0, 0, 0] == NN_TILE and run[0][0, 0, 0] == 0


@pytest.mark.parametrize("m, form", [(70, 1), (2049, 0)])
@pytest.mark.parametrize("c", [1, IL_CB + 1])
def test_three_interpolate_writes_what_it_owns(c, m, form):
    from unipre3d_amd import pointops
    lib, b, n = _lib(), 2, 37
    assert lib.u3d_three_interpolate_form(c, m) == form
    rng = np.random.default_rng(c * 10000 + m)
    points = _cloud(rng, b, c, m)
    index = torch.from_numpy(rng.integers(0, m, (b, n, 3)).astype(np.int32))
    index[:, 0], index[:, -1] = m - 1, 0
    weight = torch.from_numpy(rng.uniform(0, 1, (b, n, 3)).astype(np.float32))

    def case(arena):
        p, i, w = arena.inp(points, name="points"), arena.inp(index, name="idx"), arena.inp(weight, name="weight")
        out = arena.out((b, c, n), torch.float32, name="out")
        assert lib.u3d_three_interpolate(b, c, m, n, _p(p), _p(i), _p(w), _p(out), _stream()) == 0
        return [out]

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], pointops.three_interpolate(points.cuda(), index.cuda(), weight.cuda()))


# ---- the accumulating gradients ------------------------------------------------------------------------------------------------------------------
def _ints(rng, lo, hi, *shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float32))


def _exact(ref64, prefill):
    want = ref64 + prefill.numpy().astype(np.float64)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.abs(want).max() < 2 ** 24
    return torch.from_numpy(want.astype(np.float32))


@pytest.mark.parametrize("op", ["group", "gather"])
@pytest.mark.parametrize("rows", list(GRAD_SHAPES))
def test_group_and_gather_points_grad_write_what_they_own(rows, op):
    from unipre3d_amd import pointops
    lib = _lib()
    b, c, n = GRAD_SHAPES[rows]
    assert lib.u3d_group_points_grad_rows(b, c, n) == rows and (rows == 0 or c % rows != 0 or rows == 1)
    assert (n > 16384) == (rows == 0)
    npoints, nsample = (5, 3) if op == "group" else (15, 1)
    rng = np.random.default_rng(rows * 10 + len(op))
    index = torch.from_numpy(rng.integers(0, n, (b, npoints, nsample) if op == "group" else (b, npoints)).astype(np.int32))
    index.view(b, -1)[:, 0], index.view(b, -1)[:, 1], index.view(b, -1)[:, 2:5] = n - 1, 0, 7      # both ends of a row, and a run of three
    go = _ints(rng, -8, 8, *((b, c, npoints, nsample) if op == "group" else (b, c, npoints)))
    prefill = _ints(rng, -3, 3, b, c, n)

    def case(arena):
        g, i = arena.inp(go, name="grad_out"), arena.inp(index, name="idx")
        gp = arena.out((b, c, n), torch.float32, name="grad_points")
        gp.copy_(prefill)
        if op == "group":
            assert lib.u3d_group_points_grad(b, c, n, npoints, nsample, _p(g), _p(i), _p(gp), _stream()) == 0
        else:
            assert lib.u3d_gather_points_grad(b, c, n, npoints, _p(g), _p(i), _p(gp), _stream()) == 0
        return [gp]

    run, _ = run_twice(case, "cuda")
    want = _exact(GR.group_grad_fp64(go.numpy(), index.numpy(), n, with_mag=False)[0], prefill)
    assert same_bits(run[0], want)
    pts = torch.zeros(b, c, n, device="cuda", requires_grad=True)
    (pointops.grouping_operation if op == "group" else pointops.gather_operation)(pts, index.cuda()).backward(go.cuda())
    assert same_bits(run[0], pts.grad.cpu() + prefill)


@pytest.mark.parametrize("rows", list(GRAD_SHAPES))
def test_three_interpolate_grad_writes_what_it_owns(rows):
    from unipre3d_amd import pointops
    lib = _lib()
    b, c, m = GRAD_SHAPES[rows]
    n = 9
    assert lib.u3d_three_interpolate_grad_rows(b, c, m) == rows and (rows == 0 or c % rows != 0 or rows == 1)
    rng = np.random.default_rng(rows * 10 + 3)
    index = torch.from_numpy(rng.integers(0, m, (b, n, 3)).astype(np.int32))
    index[:, 0, 0], index[:, 0, 1], index[:, 1] = m - 1, 0, 7                                         # both ends of a row, and one destination three times
    go = _ints(rng, -8, 8, b, c, n)
    weight = _ints(rng, 0, 8, b, n, 3) / 8
    prefill = _ints(rng, -3, 3, b, c, m)

    def case(arena):
        g, i, w = arena.inp(go, name="grad_out"), arena.inp(index, name="idx"), arena.inp(weight, name="weight")
        gp = arena.out((b, c, m), torch.float32, name="grad_points")
        gp.copy_(prefill)
        assert lib.u3d_three_interpolate_grad(b, c, n, m, _p(g), _p(i), _p(w), _p(gp), _stream()) == 0
        return [gp]

    run, _ = run_twice(case, "cuda")
    want = _exact(GR.interp_grad_fp64(go.numpy(), index.numpy(), weight.numpy(), m, with_mag=False)[0], prefill)
    assert same_bits(run[0], want)
    pts = torch.zeros(b, c, m, device="cuda", requires_grad=True)
    pointops.three_interpolate(pts, index.cuda(), weight.cuda()).backward(go.cuda())
    assert same_bits(run[0], pts.grad.cpu() + prefill)
