"""tests/feature_propagation_ref.py against the record of the reference's own two PointNetFeaturePropagation classes
(tests/golden/g22_feature_propagation.npz), and what unipre3d_amd/feature_propagation.py decides before it reaches the device: the
restatement within the floors of profiles/feature_propagation/tolerance.json, its fp64 variant, the tie rule, the inverse lists against a
brute-force construction, S = 2, k != 3, and both modules' state_dict keys and shapes."""
import numpy as np
import pytest
import torch

import feature_propagation_ref as FR
from unipre3d_amd import feature_propagation as fp


@pytest.fixture(scope="module")
def golden():
    return np.load(FR.GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def tol():
    return FR.tolerance()


def _names(key):
    return [str(n) for n in np.load(FR.GOLDEN, allow_pickle=False)[key]]


def _d1(c):
    return 0 if c["points1"] is None else c["points1"].shape[1]


def _ref64(golden, case, q):
    return golden[f"{case}_out64" if q == "out" else f"{case}_{q}_64"]


@pytest.mark.parametrize("case", _names("names"))
def test_restatement_selects_the_recorded_indices_and_lies_within_the_floors(golden, tol, case):
    c = FR.golden_case(golden, case)
    got = FR.restatement(c["xyz1"], c["xyz2"], c["points1"], c["points2"], c["dout"], FR.f32)
    assert got["out"].dtype == np.float32 and got["dpoints2"].dtype == np.float32 and got["weight"].dtype == np.float32
    assert np.array_equal(got["idx"], c["idx64"])
    cut = FR.recorded(got, c["cut"], _d1(c))
    row = next(r for r in tol["cases"] if r["case"] == case)
    for q in FR.QUANTITIES:
        d = FR.dist(cut[q], _ref64(golden, case, q))
        assert d <= tol["floors"][q] and abs(d - row[f"{q}_restatement_f32"]) <= 1e-12, (q, d)
    assert (got["weight"] >= 0).all() and np.abs(got["weight"].sum(-1) - 1).max() <= 3 * 2.0 ** -24
    if _d1(c):
        assert np.array_equal(got["out"][:, :_d1(c)], c["points1"])


def test_tolerance_file_states_twice_the_floor(tol):
    assert set(tol["floors"]) == set(FR.QUANTITIES)
    for q in FR.QUANTITIES:
        assert tol["floors"][q] == max(r[f"{q}_restatement_f32"] for r in tol["cases"])
        assert tol["bars"][q] == 2.0 * tol["floors"][q] == FR.bars(tol)[q]
        assert 0 < tol["floors"][q] < 8 * 2.0 ** -24            # a few roundings of fp32
    for r in tol["module_cases"]:
        for q in FR.MODULE_QUANTITIES:
            assert r[f"{q}_bar"] == 2.0 * r[f"{q}_yardstick"] + r[f"{q}_floor"]


@pytest.mark.parametrize("case", _names("names"))
def test_fp64_restatement_is_the_record(golden, case):
    """The fp64 variant differs from the reference's fp64 run in the form of the distance alone: at most the matmul form's f64 rounding
    of |a|^2 + |b|^2 - 2ab (a few 2^-53 |a|^2, 1e-11 at scale 100) against the 1e-8 in the denominator, on a weight of about 1."""
    c = FR.golden_case(golden, case)
    got = FR.restatement(c["xyz1"], c["xyz2"], c["points1"], c["points2"], c["dout"], FR.f64)
    assert np.array_equal(got["idx"], c["idx64"])
    cut = FR.recorded(got, c["cut"], _d1(c))
    for q in FR.QUANTITIES:
        assert FR.dist(cut[q], _ref64(golden, case, q)) <= 1e-9, q


def test_s1_repeats_the_single_support_point(golden):
    c = FR.golden_case(golden, "s1")
    out, idx, w = FR.forward(c["xyz1"], c["xyz2"], c["points1"], c["points2"], FR.f32)
    assert not idx.any() and np.array_equal(w, np.broadcast_to(np.array([1, 0, 0], np.float32), w.shape))
    assert np.array_equal(out[:, 8:], np.broadcast_to(c["points2"], out[:, 8:].shape))
    d2 = FR.backward(idx, w, c["dout"], 8, 1, FR.f32)
    assert np.array_equal(d2, c["dout"][:, 8:].astype(np.float64).sum(-1, keepdims=True).astype(np.float32))


def test_equal_distances_go_to_the_lower_index():
    rng = np.random.default_rng(5)
    xyz1 = rng.uniform(-1, 1, (1, 9, 3)).astype(np.float32)
    base = rng.uniform(-1, 1, (1, 4, 3)).astype(np.float32)
    xyz2 = np.concatenate([base, base[:, ::-1]], axis=1)              # support point s and 7 - s coincide
    for dt in (FR.f32, FR.f64):
        idx, w = FR.search(xyz1, xyz2, dt)
        assert (idx[:, :, 0] < 4).all() and np.array_equal(idx[:, :, 1], 7 - idx[:, :, 0]) and (idx[:, :, 2] < 4).all()
        assert np.array_equal(w[:, :, 0], w[:, :, 1])
    # a query on a support point: distance 0 twice, then the lower index again
    idx, w = FR.search(base[:, :1], xyz2, FR.f32)
    assert idx[0, 0, 0] == 0 and idx[0, 0, 1] == 7 and w[0, 0, 0] == w[0, 0, 1] and abs(float(w[0, 0, :2].sum()) - 1) < 1e-6


def test_inverse_lists_against_a_brute_force_construction():
    rng = np.random.default_rng(6)
    B, N, S = 3, 37, 11
    idx = rng.integers(0, S, (B, N, 3)).astype(np.int32)
    idx[1] = 4                                                        # one list holds every entry
    for (b, n, j), v in {(0, 3, 1): -1, (0, 20, 0): S, (2, 36, 2): 2 ** 31 - 1, (2, 0, 0): -2 ** 31}.items():
        idx[b, n, j] = v
    ptr, ent = FR.inverse_lists(idx, S)
    bptr, bent = FR.brute_force_lists(idx, S)
    assert np.array_equal(ptr, bptr) and np.array_equal(ent, bent) and ptr.dtype == ent.dtype == np.int32
    assert ptr[0, S] == 3 * N - 2 and ptr[1, S] == 3 * N and ptr[2, S] == 3 * N - 2 and (ptr[:, 0] == 0).all()
    assert np.array_equal(ent[0, ptr[0, S]:], [3 * 3 + 1, 3 * 20]) and np.array_equal(ent[1], np.arange(3 * N))
    for b in range(B):
        assert sorted(ent[b]) == list(range(3 * N))
        for s in range(S):
            li = ent[b, ptr[b, s]:ptr[b, s + 1]]
            assert (np.diff(li) > 0).all() and (idx[b].reshape(-1)[li] == s).all()
    # an out-of-range entry contributes nothing and receives no gradient
    w = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
    p2, dout = rng.uniform(-1, 1, (B, 5, S)).astype(np.float32), rng.uniform(-1, 1, (B, 5, N)).astype(np.float32)
    out = FR.forward(None, np.zeros((B, S, 3), np.float32), None, p2, FR.f64, neighbours=(idx, w))[0]
    w0 = w.copy()
    w0[(idx < 0) | (idx >= S)] = 0
    assert np.array_equal(out, FR.forward(None, np.zeros((B, S, 3), np.float32), None, p2, FR.f64, neighbours=(np.clip(idx, 0, S - 1), w0))[0])
    assert np.array_equal(FR.backward(idx, w, dout, 0, S, FR.f64), FR.backward(np.clip(idx, 0, S - 1), w0, dout, 0, S, FR.f64))


def test_two_support_points_raise():
    with pytest.raises(ValueError, match="S = 2"):
        FR.search(np.zeros((1, 4, 3), np.float32), np.zeros((1, 2, 3), np.float32))
    xyz1, xyz2 = torch.zeros(1, 4, 3), torch.zeros(1, 2, 3)
    with pytest.raises(ValueError, match="S = 2"):
        fp.neighbours(xyz1, xyz2)
    with pytest.raises(ValueError, match="S = 2"):
        fp.propagate(xyz1, xyz2, None, torch.zeros(1, 4, 2))
    with pytest.raises(ValueError, match="S = 2"):
        fp.PointNetFeaturePropagation(4, 4)(xyz1, xyz2, None, torch.zeros(1, 4, 2))


def test_checks_made_before_the_device():
    xyz1, xyz2, p2 = torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="k=2"):
        fp.PCMPointNetFeaturePropagation(4, 4)(xyz1, xyz2, None, p2, k=2)
    with pytest.raises(NotImplementedError, match="requires_grad"):
        fp.propagate(xyz1.clone().requires_grad_(True), xyz2, None, p2)
    with pytest.raises(NotImplementedError, match="requires_grad"):
        fp.propagate(xyz1, xyz2.clone().requires_grad_(True), None, p2)
    with pytest.raises(RuntimeError, match="HIP device"):
        fp.propagate(xyz1, xyz2, None, p2)                            # CPU tensors: there is no fallback
    with pytest.raises(NotImplementedError, match="N="):
        fp.neighbours(torch.zeros(1, fp.MAX_POINTS + 1, 3), xyz2)
    with pytest.raises(NotImplementedError, match="D1="):
        fp.propagate(xyz1, xyz2, None, torch.zeros(1, fp.MAX_CHANNELS + 1, 3))
    with pytest.raises(ValueError, match="points2"):
        fp.propagate(xyz1, xyz2, None, torch.zeros(1, 4, 5))
    with pytest.raises(ValueError, match="points1"):
        fp.propagate(xyz1, xyz2, torch.zeros(1, 4, 5), p2)
    assert fp.EXPORTS == tuple(fp.SIGNATURES) and all(n.startswith("u3d_feature_propagation_") for n in fp.EXPORTS)


def _module(kind, blocks, **kw):
    return (fp.PointNetFeaturePropagation if kind == "pointmlp" else fp.PCMPointNetFeaturePropagation)(24, 16, blocks=blocks, **kw)


@pytest.mark.parametrize("case", _names("module_names"))
def test_modules_have_the_recorded_state_dict(golden, case):
    m = _module(str(golden[f"{case}_kind"]), int(golden[f"{case}_blocks"]))
    names = [str(k) for k in golden[f"{case}_sd_names"]]
    sd = m.state_dict()
    assert list(sd) == names and "fuse.net.0.weight" in names
    assert ("extraction.operation.0.net1.0.weight" in names) == (int(golden[f"{case}_blocks"]) > 0)
    for i, k in enumerate(names):
        assert tuple(sd[k].shape) == golden[f"{case}_sd_{i}"].shape, k
    m.load_state_dict({k: torch.from_numpy(golden[f"{case}_sd_{i}"]) for i, k in enumerate(names)}, strict=True)
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in golden[f"{case}_param_names"]]


def test_module_constructors():
    m = fp.PointNetFeaturePropagation(24, 16, has_MLP=False)
    assert not m.state_dict() and m.has_MLP is False
    g = fp.PointNetFeaturePropagation(24, 16, blocks=2, groups=2, res_expansion=0.5, bias=False, activation="gelu")
    keys = list(g.state_dict())
    assert "extraction.operation.1.net2.3.weight" in keys and "extraction.operation.1.net2.4.running_var" in keys
    assert "fuse.net.0.bias" not in keys and g.extraction.operation[0].net1[0].weight.shape == (8, 8, 1)
    assert isinstance(g.extraction.operation[0].act, torch.nn.GELU) and isinstance(g.fuse.act, torch.nn.ReLU)
    assert isinstance(fp.PCMPointNetFeaturePropagation(24, 16, blocks=0).extraction, torch.nn.Identity)
    with pytest.raises(TypeError):
        fp.PCMPointNetFeaturePropagation(24, 16, has_MLP=False)


@pytest.mark.parametrize("case", _names("module_names"))
def test_modules_on_the_restatement_lie_within_the_bars(golden, tol, case):
    """The project's torch layers under the recorded weights, fed by the fp32 restatement on the CPU, against the reference's fp64 run."""
    d = FR.module_dists(golden, case, FR.module_run(golden, case, FR.ref_propagate))
    bars = FR.module_bars(case, tol)
    for q in FR.MODULE_QUANTITIES:
        assert d[q] <= bars[q], (q, d[q], bars[q])
