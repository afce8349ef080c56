"""The local grouper without a GPU: the CPU restatements (tests/local_grouper_ref.py) against what the reference's own two LocalGrouper classes
computed (tests/golden/g21_local_grouper.npz, made by tests/golden/make_g21_local_grouper.py), the closed-form backward against autograd,
the inverse lists, the tolerance record, the header against the module's binding table, the library's refusals and the Python surface."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import local_grouper_ref as GR
from conftest import ROOT

_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)
# name: (module, B, N, S, D, K, mode, use_xyz, k_stride)
CASES = {f"{m}_{'xyz' if u else 'noxyz'}": ("pointmlp", 2, 16, 8, 8, 4, m, u, 1) for m in ("none", "center", "anchor") for u in (True, False)}
CASES.update({"pcm_stride": ("pcm", 1, 64, 32, 12, 24, "center", False, 2), "pcm_full": ("pcm", 1, 12, 12, 4, 3, "center", True, 1),
              "scales": ("pointmlp", 3, 32, 16, 8, 4, "center", True, 1), "stage1": ("pointmlp", 2, 256, 128, 64, 32, "anchor", True, 1)})


@pytest.fixture(scope="module")
def golden():
    return np.load(GR.GOLDEN, allow_pickle=False)


def _args(c):
    return c["xyz"], c["points"], c["fps"], GR.used_idx(c), c["alpha"], c["beta"]


def test_golden_layout(golden):
    assert [str(n) for n in golden["names"]] == list(CASES)
    for name, (module, B, N, S, D, K, mode, use_xyz, ks) in CASES.items():
        c = GR.golden_case(golden, name)
        Cn = D + (3 if use_xyz else 0)
        assert (c["module"], c["mode"] or "none", c["use_xyz"], c["k_stride"], c["sample_ratio"]) == (module, mode, use_xyz, ks, N // S)
        assert c["xyz"].dtype == c["points"].dtype == c["dout"].dtype == np.float32
        assert c["xyz"].shape == (B, N, 3) and c["points"].shape == (B, N, D) and c["dout"].shape == (B, S, K // ks, D + Cn)
        assert c["idx"].dtype == np.int32 and c["idx"].shape == (B, S, K) and c["idx"].min() >= 0 and c["idx"].max() < N
        assert (c["fps"] is None) == (S == N)
        if c["fps"] is not None:
            assert c["fps"].dtype == np.int32 and c["fps"].shape == (B, S) and c["fps"].min() >= 0 and c["fps"].max() < N
            if module == "pcm":
                assert (np.diff(c["fps"], axis=1) > 0).all()                      # PCM sorts its anchors
        # an anchor is among its own neighbours, and no neighbour is named twice
        anchors = GR.sanitize(c["fps"], c["idx"], N)[0]
        assert (c["idx"] == anchors[:, :, None]).sum(-1).min() == 1 and (np.diff(np.sort(c["idx"], -1), axis=-1) > 0).all()
        assert (c["alpha"] is None) == (c["beta"] is None) == (mode == "none")
        if mode != "none":
            assert c["alpha"].shape == c["beta"].shape == golden[f"{name}_dalpha64"].shape == golden[f"{name}_dbeta64"].shape == (Cn,)
        assert (c["points_res"] is not None) == (module == "pcm") and (c["cut"] is not None) == (name == "stage1")
        if c["cut"] is None:
            assert golden[f"{name}_out64"].dtype == np.float64 and golden[f"{name}_out64"].shape == c["dout"].shape
            assert golden[f"{name}_dpoints64"].shape == (B, N, D)
        else:
            rows, cols, dcols = c["cut"]
            assert golden[f"{name}_out64"].shape == (B, len(rows), K, len(cols)) and golden[f"{name}_dpoints64"].shape == (B, N, len(dcols))
            assert (dcols % 8 == np.arange(8)).all() and set(cols) == set(dcols) | {D, D + 1, D + 2} | set(D + 3 + dcols)
    # the three clouds of `scales` differ in scale by 10 and 100
    p = golden["scales_points"]
    assert 5 < np.abs(p[1]).max() / np.abs(p[0]).max() < 20 and 50 < np.abs(p[2]).max() / np.abs(p[0]).max() < 200
    assert os.path.getsize(GR.GOLDEN) <= 614965                                  # no larger than g20_lnp.npz


@pytest.mark.parametrize("case", list(CASES))
def test_fp64_restatement_is_the_references_fp64(golden, case):
    c = GR.golden_case(golden, case)
    qs = GR.quantities(c["mode"])
    fwd = GR.forward_f64(*_args(c), c["mode"], c["use_xyz"])
    got = GR.recorded(dict(zip(qs, (fwd[0],) + GR.backward_f64(*_args(c), c["dout"], c["mode"], c["use_xyz"]))), c["cut"])
    for q in qs:
        assert GR.dist(got[q], golden[f"{case}_{q}64"]) <= 1e-12, q
    assert np.array_equal(fwd[1], golden[f"{case}_new_xyz64"])
    if c["points_res"] is not None:
        fps = GR.sanitize(c["fps"], c["idx"], c["xyz"].shape[1])[0]
        assert np.array_equal(GR._take(c["points_res"].astype(np.float64), fps), golden[f"{case}_res64"])


def test_a_whole_tensor_std_would_miss_the_scales_record(golden):
    """What the `scales` case is for: with one std over the whole tensor, the restatement is far from the record."""
    c = GR.golden_case(golden, "scales")
    src, fps, idx, g, d, (n, mu, s) = GR._parts_f64(c["xyz"], c["points"], c["fps"], GR.used_idx(c), c["mode"], c["use_xyz"])
    assert s[1] / s[0] > 5 and s[2] / s[1] > 5
    whole = c["alpha"] * d / (d.std(ddof=1) + GR.EPS) + c["beta"]
    assert GR.dist(whole, golden["scales_out64"][..., :d.shape[3]]) > 0.1


@pytest.mark.parametrize("shape", [(2, 9, 5, 8, 3, "center", True), (1, 33, 33, 12, 32, "anchor", False), (3, 7, 2, 4, 2, "anchor", True),
                                   (2, 6, 6, 4, 2, None, True)])
def test_closed_form_backward_is_autograd_of_the_op_by_op_form(shape):
    B, N, S, D, K, mode, use_xyz = shape
    rng = np.random.default_rng(sum(shape[:5]))
    Cn = D + (3 if use_xyz else 0)
    xyz, points, dout = rng.standard_normal((B, N, 3)), rng.standard_normal((B, N, D)), rng.standard_normal((B, S, K, D + Cn))
    alpha, beta = rng.uniform(0.5, 2.0, Cn) * rng.choice([-1, 1], Cn), rng.standard_normal(Cn)
    fps = rng.integers(0, N, (B, S)) if S < N else None          # (with duplicates)
    idx = rng.integers(0, N, (B, S, K))
    out, grads = GR.reference_form(xyz, points, fps, idx, alpha, beta, mode, use_xyz, dout, dtype="float64")
    assert GR.dist(GR.forward_f64(xyz, points, fps, idx, alpha, beta, mode, use_xyz)[0], out) <= 1e-13
    for got, want in zip(GR.backward_f64(xyz, points, fps, idx, alpha, beta, dout, mode, use_xyz), grads):
        assert (got is None) == (want is None)
        if got is not None:
            assert GR.dist(got, want) <= 1e-12


def _graphs():
    rng = np.random.default_rng(7)
    hub = np.full((2, 6, 4), 3)                                   # every entry names point 3: one list of S K entries, all others empty
    dup = np.array([[0, 5, 5, 2, 9, 5], [1, 1, 1, 1, 1, 1]])     # duplicates among the anchors
    bad = rng.integers(0, 10, (2, 6, 4))
    bad[0, 2, 1], bad[1, 5, 0], bad[0, 0, 2] = -1, 10, 2 ** 31 - 1
    bad_fps = dup.copy()
    bad_fps[0, 4] = 10
    return {"random": (rng.integers(0, 10, (2, 6, 4)), rng.integers(0, 10, (2, 6)), 10), "hub": (hub, dup, 10), "duplicate_fps": (bad, dup, 10),
            "out_of_range": (bad, bad_fps, 10), "identity": (rng.integers(0, 6, (2, 6, 4)), None, 6)}


@pytest.mark.parametrize("graph", ["random", "hub", "duplicate_fps", "out_of_range", "identity", "golden"])
def test_inverse_lists_invert_idx_and_fps(golden, graph):
    if graph == "golden":
        c = GR.golden_case(golden, "pcm_stride")
        idx, fps, N = GR.used_idx(c), c["fps"], c["xyz"].shape[1]
    else:
        idx, fps, N = _graphs()[graph]
    sfps, sidx = GR.sanitize(fps, idx, N)
    assert sidx.min() >= 0 and sidx.max() < N and sfps.min() >= 0 and sfps.max() < N
    ptr, ent, fptr, fent = GR.inverse_lists(fps, idx, N)
    B, S, K = sidx.shape
    assert all(a.dtype == np.int32 for a in (ptr, ent, fptr, fent))
    for p, e, table in ((ptr, ent, sidx.reshape(B, -1)), (fptr, fent, sfps)):
        n = table.shape[1]
        assert p.shape == (B, N + 1) and e.shape == (B, n)
        for b in range(B):
            assert p[b, 0] == 0 and p[b, N] == n and (np.diff(p[b]) >= 0).all()
            assert sorted(e[b].tolist()) == list(range(n))                     # every entry exactly once
            for j in range(N):
                lst = e[b, p[b, j]:p[b, j + 1]]
                assert (np.diff(lst) > 0).all() and (table[b][lst] == j).all(), (b, j)
    if graph == "hub":
        assert ptr[0, 4] - ptr[0, 3] == S * K and ptr[0, 3] == 0 and fptr[0, 6] - fptr[0, 5] == 3 and fptr[1, 2] - fptr[1, 1] == S
    if graph == "out_of_range":
        assert sidx[0, 2, 1] == sfps[0, 2] == 5 and sfps[0, 4] == 4 and sidx[1, 5, 0] == 1 and sidx[0, 0, 2] == 0
    if graph == "identity":
        assert np.array_equal(fent, np.broadcast_to(np.arange(S), (B, S))) and np.array_equal(fptr[0], np.arange(N + 1))


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_restatement_lies_within_the_floors_on_file(golden, case):
    tol = GR.tolerance()
    c = GR.golden_case(golden, case)
    qs = GR.quantities(c["mode"])
    out, stats = GR.forward_kernel_f32(*_args(c), c["mode"], c["use_xyz"])
    got = GR.recorded(dict(zip(qs, (out,) + GR.backward_kernel_f32(*_args(c), c["dout"], c["mode"], c["use_xyz"]))), c["cut"])
    row = {r["case"]: r for r in tol["cases"]}[case]
    for q in qs:
        d = GR.dist(got[q], golden[f"{case}_{q}64"])
        assert got[q].dtype == np.float32 and d <= tol["floors"][q], q
        assert d == pytest.approx(row[f"{q}_restatement_f32"], rel=1e-6, abs=1e-12)
    if c["mode"] is not None:
        _, _, mu64, s64 = GR.forward_f64(*_args(c), c["mode"], c["use_xyz"])
        assert stats.shape == (c["xyz"].shape[0], 4) and np.abs(stats[:, 1] - s64).max() <= 2.0 ** -23 * s64.max()
        assert np.abs(stats[:, 0] - mu64).max() <= 2.0 ** -23 * s64.max()


def test_tolerance_record_follows_its_rule(golden):
    tol = GR.tolerance()
    assert [r["case"] for r in tol["cases"]] == list(CASES) and set(tol["floors"]) == set(GR.QUANTITIES)
    for r in tol["cases"]:
        mode = CASES[r["case"]][6]
        for q in GR.QUANTITIES:
            if q not in GR.quantities(None if mode == "none" else mode):
                assert r[f"{q}_yardstick"] is None and r[f"{q}_bar"] is None
                continue
            assert r[f"{q}_yardstick"] == float(golden[f"{r['case']}_yard_{q}"])
            assert r[f"{q}_bar"] == pytest.approx(2 * r[f"{q}_yardstick"] + tol["floors"][q], rel=1e-12)
            assert r[f"{q}_restatement_f32"] <= tol["floors"][q] < 1e-5 and r[f"{q}_yardstick"] < 1e-5
            assert GR.case_bars(r["case"], tol)[q] == r[f"{q}_bar"]
            worst = r[f"{q}_kernel_worst"]
            assert worst is None or worst <= r[f"{q}_bar"], (r["case"], q)
    for q in GR.QUANTITIES:
        assert tol["floors"][q] == max(r[f"{q}_restatement_f32"] for r in tol["cases"] if r[f"{q}_restatement_f32"] is not None)


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "unipre3d_local_grouper.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    out = {}
    for ret, name, params in _DECLARATION.findall(hdr):
        types = []
        for p in (q.strip() for q in params.split(",")):
            if p in ("", "void"):
                continue
            types.append(p[:p.rindex("*") + 1].replace(" ", "") if "*" in p else " ".join(p.split()[:-1]))
        assert name not in out, name
        out[name] = (" ".join(ret.split()), types)
    return out


def test_header_and_binding_agree():
    lg = importlib.import_module("unipre3d_amd.local_grouper")
    declared = _declared_functions()
    assert set(declared) == set(lg.EXPORTS) == {"u3d_local_grouper_abi_version", "u3d_local_grouper_scratch_bytes", "u3d_local_grouper_lists",
                                                "u3d_local_grouper_fwd", "u3d_local_grouper_bwd"}
    assert len(set(lg.EXPORTS)) == len(lg.EXPORTS)
    assert declared["u3d_local_grouper_scratch_bytes"] == ("size_t", ["int"] * 8)
    assert declared["u3d_local_grouper_lists"][1] == ["constint32_t*"] * 2 + ["int32_t*"] * 4 + ["void*"] + ["int"] * 4 + ["void*"]
    handle = lg.load()
    bound_as = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
    for name, (ret, params) in declared.items():
        fn = getattr(handle, name)
        assert fn.restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[ret], name
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for c_type, bound in zip(params, fn.argtypes):
            assert bound is (ctypes.c_void_p if c_type.endswith("*") else bound_as[c_type]), (name, c_type, bound)
    hdr = open(os.path.join(ROOT, "include", "unipre3d_local_grouper.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (U3D_LOCAL_GROUPER_\w+) (\d+)", hdr, re.M)}
    assert consts == {"U3D_LOCAL_GROUPER_ABI_VERSION": lg.ABI_VERSION, "U3D_LOCAL_GROUPER_MAX_POINTS": lg.MAX_POINTS,
                      "U3D_LOCAL_GROUPER_MAX_K": lg.MAX_K, "U3D_LOCAL_GROUPER_MAX_CHANNELS": lg.MAX_CHANNELS}
    assert handle.u3d_local_grouper_abi_version() == 1 and (lg.MAX_POINTS, lg.MAX_K, lg.MAX_CHANNELS) == (16384, 64, 512)


def test_scratch_query_is_host_arithmetic():
    from unipre3d_amd import local_grouper as lg
    q = lg.load().u3d_local_grouper_scratch_bytes
    # forward: one pair of doubles per workgroup, at most 128 per batch element; nothing without a normalisation
    assert q(2, 256, 128, 32, 64, 1, 2, 0) == 2 * 32 * 16 and q(3, 16384, 8192, 2, 4, 1, 1, 0) == 3 * 128 * 16 and q(2, 16, 8, 4, 8, 1, 0, 0) == 0
    # backward: per workgroup (at most 32 per batch element) a pair of doubles and 2 (D + A) floats; sum_k gy, sum_k d, sum_k ga per row
    assert q(2, 256, 128, 32, 64, 1, 2, 1) == 2 * 16 * (16 + 8 * 67) + 2 * 128 * 4 * (2 * 67 + 64)
    assert q(1, 16384, 8192, 2, 4, 0, 1, 1) == 32 * (16 + 8 * 4) + 8192 * 4 * 12 and q(2, 16, 8, 4, 8, 1, 0, 1) == 2 * 8 * 8 * 4
    # lists: a cursor per point, an entry per (s, k) and per s
    assert q(2, 256, 128, 32, 64, 1, 2, 2) == 4 * 2 * (256 + 128 * 32 + 128)
    for bad in ((0, 8, 8, 4, 8), (1, 0, 0, 4, 8), (1, 8, 9, 4, 8), (1, 16385, 8, 4, 8), (1, 8, 8, 1, 8), (1, 8, 8, 65, 8), (1, 8, 8, 4, 6),
                (1, 8, 8, 4, 516), (1, 8, 8, 4, 0), (2 ** 10, 16384, 256, 64, 8), (2 ** 10, 16384, 1, 2, 8)):
        assert all(q(*bad, 1, 1, p) == 0 for p in (0, 1, 2)), bad
    assert q(1, 8, 8, 4, 8, 2, 1, 1) == 0 and q(1, 8, 8, 4, 8, 1, 3, 1) == 0 and q(1, 8, 8, 4, 8, 1, 1, 3) == 0


def test_refusals_return_before_any_launch():
    """Every argument check returns before anything touches a device: the pointers below are never dereferenced."""
    from unipre3d_amd import local_grouper as lg
    lib = lg.load()
    null, one, off = ctypes.c_void_p(0), ctypes.c_void_p(256), ctypes.c_void_p(260)

    def lists(p=(one,) * 7, B=1, N=8, S=8, K=4, **_):
        return lib.u3d_local_grouper_lists(*p, B, N, S, K, null)

    def fwd(p=(one,) * 11, B=1, N=8, S=8, K=4, D=8, st=(64, 8, 1), xyz=1, mode=1, cf=1, eps=1e-5, **_):
        return lib.u3d_local_grouper_fwd(p[0], p[1], *st, *p[2:], B, N, S, K, D, xyz, mode, cf, eps, null)

    def bwd(p=(one,) * 16, B=1, N=8, S=8, K=4, D=8, st=(64, 8, 1), gst=(64, 1, 8), xyz=1, mode=1, cf=1, **_):
        return lib.u3d_local_grouper_bwd(p[0], p[1], *st, *p[2:13], *gst, *p[13:], B, N, S, K, D, xyz, mode, cf, null)

    for call, n, fps_at in ((lists, 7, 0), (fwd, 11, 2), (bwd, 16, 2)):
        for k in range(n):
            for bad in (null, off):                     # each pointer: null, and 4 bytes past a 16-byte boundary
                if k == fps_at and bad is null:
                    continue                            # (a null fps is the identity)
                args = [one] * n
                args[k] = bad
                assert call(tuple(args)) == 1, (n, k)
        assert call(B=0) == 1 and call(N=0, S=0) == 1 and call(K=0) == 1 and call(B=-1) == 1
        assert call(N=16385, S=8) == 2 and call(S=9) == 2 and call(K=1) == 2 and call(K=65) == 2
        assert call(B=2 ** 12, N=4096, S=4096, st=(4096 * 8, 8, 1), gst=(4096 * 8, 8, 1)) == 2          # more rows than the library takes
        args = [one] * n
        args[fps_at] = null
        assert call(tuple(args), S=4) == 1                                        # the identity needs S == N
    for call in (fwd, bwd):
        assert call(D=0) == 1 and call(D=6, st=(48, 6, 1), gst=(48, 6, 1)) == 2 and call(D=516, st=(8 * 516, 516, 1), gst=(8 * 516, 516, 1)) == 2
        for st in ((63, 8, 1), (64, 8, 2), (64, 4, 1), (64, 1, 4), (-64, 8, 1), (64, 2, 8)):
            assert call(st=st) == 1, st
        assert call(xyz=2) == 1 and call(mode=3) == 1 and call(mode=-1) == 1 and call(cf=2) == 1
    assert bwd(gst=(64, 8, 2)) == 1 and bwd(gst=(60, 8, 1)) == 1
    assert fwd(eps=-1e-5) == 1 and fwd(eps=float("nan")) == 1 and fwd(eps=float("inf")) == 1


def test_module_surface_and_state_dict():
    import torch
    from unipre3d_amd import local_grouper as lg
    for cls, extra in ((lg.LocalGrouper, {}), (lg.PCMLocalGrouper, {"k_stride": 2})):
        for use_xyz, n in ((True, 67), (False, 64)):
            m = cls(64, 2, 24, use_xyz=use_xyz, normalize="anchor", **extra)
            assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {"affine_alpha": (1, 1, 1, n), "affine_beta": (1, 1, 1, n)}
            assert torch.equal(m.affine_alpha, torch.ones(1, 1, 1, n)) and torch.equal(m.affine_beta, torch.zeros(1, 1, 1, n))
            assert (m.sample_ratio, m.kneighbors, m.use_xyz, m.normalize, m.channels_first) == (2, 24, use_xyz, "anchor", True)
        assert cls(64, 2, 24, normalize=None, **extra).state_dict() == {} and cls(64, 2, 24, normalize="Center").normalize == "center"
        assert cls(64, 2, 24, normalize="batch").normalize is None
    assert list(inspect.signature(lg.LocalGrouper.__init__).parameters) == ["self", "channel", "sample_ratio", "kneighbors", "use_xyz",
                                                                            "normalize", "kwargs"]
    assert list(inspect.signature(lg.PCMLocalGrouper.__init__).parameters) == ["self", "channel", "sample_ratio", "kneighbors", "use_xyz",
                                                                               "normalize", "k_stride", "kwargs"]
    assert inspect.signature(lg.PCMLocalGrouper.__init__).parameters["kneighbors"].default == 12
    assert list(inspect.signature(lg.LocalGrouper.forward).parameters) == ["self", "xyz", "points", "fps_idx", "idx"]
    assert list(inspect.signature(lg.PCMLocalGrouper.forward).parameters) == ["self", "xyz", "points", "points_res", "fps_idx", "idx"]
    assert list(inspect.signature(lg.local_group).parameters) == ["xyz", "points", "fps_idx", "idx", "alpha", "beta", "normalize", "use_xyz",
                                                                  "eps", "channels_first"]
    assert inspect.signature(lg.local_group).parameters["channels_first"].default is True


def test_argument_errors_raise_without_touching_a_device():
    import torch
    from unipre3d_amd import local_grouper as lg
    xyz, pts, fps, idx = torch.zeros(1, 16, 3), torch.zeros(1, 16, 8), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8, 4, dtype=torch.int32)
    a, b = torch.ones(11), torch.zeros(11)
    call = lambda *args, **kw: lg.local_group(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(xyz, pts, fps, idx, a, b, "center", True)
    with pytest.raises(NotImplementedError, match="xyz.requires_grad"):
        call(xyz.clone().requires_grad_(True), pts, fps, idx, a, b, "center", True)
    with pytest.raises(ValueError, match="normalize"):
        call(xyz, pts, fps, idx, a, b, "batch", True)
    with pytest.raises(ValueError, match="expected"):
        call(xyz[0], pts, fps, idx, a, b, "center", True)
    with pytest.raises(ValueError, match="expected"):
        call(xyz, pts[:, :8], fps, idx, a, b, "center", True)
    with pytest.raises(ValueError, match="identity"):
        call(xyz, pts, None, idx, a, b, "center", True)
    with pytest.raises(ValueError, match="D \\+ A"):
        call(xyz, pts, fps, idx, a[:8], b[:8], "center", True)
    with pytest.raises(ValueError, match="eps"):
        call(xyz, pts, fps, idx, a, b, "center", True, eps=-1.0)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError, match="dtype"):
            call(xyz, pts.to(dtype), fps, idx, a, b, "center", True)
    with pytest.raises(NotImplementedError, match="dtype"):
        call(xyz, pts, fps, idx.float(), a, b, "center", True)
    # out of scope: N, S > N, K, D, B S K
    with pytest.raises(NotImplementedError, match="N="):
        call(torch.zeros(1, 16385, 3), torch.zeros(1, 16385, 8), fps, idx, a, b, "center", True)
    with pytest.raises(NotImplementedError, match="N="):
        call(xyz, pts, torch.zeros(1, 17, dtype=torch.int32), torch.zeros(1, 17, 4, dtype=torch.int32), a, b, "center", True)
    for k in (1, 65):
        with pytest.raises(NotImplementedError, match="K="):
            call(xyz, pts, fps, torch.zeros(1, 8, k, dtype=torch.int32), a, b, "center", True)
    for d in (6, 516):
        with pytest.raises(NotImplementedError, match="D="):
            call(xyz, torch.zeros(1, 16, d), fps, idx, torch.ones(d + 3), torch.zeros(d + 3), "center", True)
    with pytest.raises(NotImplementedError, match="2\\^24"):
        call(xyz.expand(2 ** 20, 16, 3), pts.expand(2 ** 20, 16, 8), fps.expand(2 ** 20, 8), idx.expand(2 ** 20, 8, 4), a, b, "center", True)
    m = lg.LocalGrouper(8, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(xyz, pts, fps, idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lg.PCMLocalGrouper(8, 1, 4)(xyz, pts, None, None, torch.zeros(1, 16, 4, dtype=torch.int32))
