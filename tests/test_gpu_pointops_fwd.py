"""The FORWARD kernels of the point operators at every dispatch class: group / gather (vector and scalar kernel), three_interpolate (LDS and
global-gather kernel, both staging copies of the LDS one) and three_nn (tile edges of the known cloud, the four lanes of a query's quad), against
the plain fp64 references of tests/pointops_fwd_ref.py.

The library says which kernel a shape launches (u3d_group_points_form, u3d_three_interpolate_form: host arithmetic), so the shape lists are
checked for coverage without a GPU, and the references are held to oracle/pointops_oracle.c bit for bit on the CPU before any GPU test trusts
them.  Inputs are exact (integers, eighths, quarters: pointops_fwd_ref's header), so the bar is EQUALITY with fp64 in all three contraction
modes; group / gather do not depend on the mode and run once."""
import functools

import numpy as np
import pytest

import pointops_fwd_ref as R
from oracle import pointops as po

gpu = pytest.mark.gpu
MODES = ("fma_llvm", "fma_chain", "none")
GP_CH, IC_CH, IL_CB, IL_WG = 8, 8, 4, 1024          # csrc/u3d_pointops.hip: channels per block of the three kernels; points per LDS-form workgroup
ALIGNED = 1 << 20                                   # a 16-byte aligned address that is never dereferenced

# (name, (b, c, n, npoint, nsample), options, form): total = npoint * nsample outputs per (cloud, channel); a vector-kernel thread owns 4 of
# them, a workgroup 1024; form 1 = vector kernel.  idx_offset / points_offset: the tensor is a contiguous view that many ELEMENTS into a buffer.
GROUP_CASES = [
    ("total_4", (2, 9, 50, 1, 4), {}, 1),                              # one live thread; channel blocks 8 + 1
    ("total_1024", (2, 8, 50, 256, 4), {}, 1),                         # exactly one workgroup; exactly one channel block
    ("total_1028", (2, 17, 50, 257, 4), {}, 1),                        # one thread into a second chunk; channel blocks 8 + 8 + 1
    ("one_source_point", (1, 1, 1, 3, 4), {}, 1),
    ("total_255", (2, 9, 50, 51, 5), {}, 0),                           # total % 4 != 0
    ("gather_257", (2, 3, 50, 257, 1), {"gather": True}, 0),           # a second workgroup of one thread
    ("idx_at_4_bytes", (2, 9, 50, 64, 4), {"idx_offset": 1}, 0),       # total % 4 == 0 but no int4 load possible
    ("idx_at_16_bytes", (2, 9, 50, 64, 4), {"idx_offset": 4}, 1),
    ("points_at_4_bytes", (2, 9, 50, 64, 4), {"points_offset": 1}, 1),  # the gathers are scalar: any source alignment
    ("int64_idx", (2, 9, 50, 64, 4), {"int64": True}, 1),
]
# (name, (b, c, m, n), element offset of `features` in its buffer, form): form 1 = LDS kernel (0 < m <= 2048).  Its workgroup stages the
# nc = min(4, c - c0) rows of channel block c0 of cloud bi, `nc * m` floats from byte `base + (bi * c + c0) * m * 4`, with a float4 copy when
# that address is on 16 bytes AND nc * m % 4 == 0, else dword by dword (_staging below):
#   2x5x6    cloud 0: block 0 float4 (24 floats at 0), block 1 (one row, 6 floats) dword; cloud 1: base 120 % 16 = 8: 24 floats, unaligned -> dword
#   2x4x2048 float4 throughout;  2x3x3: 9 floats -> dword;  1x1x1: dword;  2x8x64 at element 1: every base % 16 = 4 -> dword, lengths 256
INTERP_CASES = [
    ("lds_2x5x6_300", (2, 5, 6, 300), 0, 1),
    ("lds_2x4x2048_1025", (2, 4, 2048, 1025), 0, 1),                   # at the threshold; a second workgroup with ONE live point
    ("lds_2x3x3_1024", (2, 3, 3, 1024), 0, 1),                         # exactly one workgroup; only a 3-row tail block
    ("lds_1x1x1_1", (1, 1, 1, 1), 0, 1),
    ("lds_2x8x64_257_view", (2, 8, 64, 257), 1, 1),
    ("global_2x9x2049_257", (2, 9, 2049, 257), 0, 0),                  # a one-channel tail of IC_CH; a second workgroup of one point
    ("global_1x8x2049_256", (1, 8, 2049, 256), 0, 0),
    ("global_1x16x4096_1023", (1, 16, 4096, 1023), 0, 0),
]
NN_SIZES = [(n, 70) for n in (1, 63, 64, 65, 130)] + [(65, m) for m in (0, 1, 2, 3, 4, 5, 2047, 2048, 2049, 4096, 4097)]   # (n, m), b = 2


def _ids(cases):
    return [c[0] for c in cases]


def _forms():
    from unipre3d_amd import pointops
    lib = pointops.load()
    return lib.u3d_group_points_form, lib.u3d_three_interpolate_form


def _staging(b, c, m, base=0):
    """[(cloud, first channel, rows, base address % 16, length % 4, copy)] of every workgroup row of the LDS form"""
    out = []
    for bi in range(b):
        for c0 in range(0, c, IL_CB):
            nc = min(IL_CB, c - c0)
            a, l = (base + (bi * c + c0) * m * 4) % 16, nc * m % 4
            out.append((bi, c0, nc, a, l, "float4" if a == 0 and l == 0 else "dword"))
    return out


@pytest.fixture(params=MODES)
def contraction(request):
    """the HIP kernels and the oracle are switched together (test_gpu_pointops.py's fixture, asked for by the tests that contain a three-term sum)"""
    from unipre3d_amd import pointops
    po.set_contraction(request.param)
    pointops.set_contraction(request.param)
    yield request.param
    po.set_contraction("fma_llvm")
    pointops.set_contraction("fma_llvm")


# ---- shared inputs and references (computed once) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _group_inputs(name):
    (b, c, n, npoint, nsample) = next(s for k, s, _, _ in GROUP_CASES if k == name)
    pts = R.special_features(b, c, n, seed=c + npoint)
    sets = R.group_index_sets(b, n, npoint, nsample, seed=n + npoint)
    return pts, {k: (idx, np.ascontiguousarray(R.group(pts, idx))) for k, idx in sets.items()}


@functools.lru_cache(maxsize=None)
def _interp_exact(name):
    (b, c, m, n) = next(s for k, s, _, _ in INTERP_CASES if k == name)
    feats = R.exact_features(b, c, m)
    return feats, {k: (idx, w, R.three_interpolate_fp64(feats, idx, w)[0]) for k, (idx, w) in R.interp_index_sets(b, m, n, seed=m + n).items()}


@functools.lru_cache(maxsize=None)
def _interp_gauss(name):
    (b, c, m, n) = next(s for k, s, _, _ in INTERP_CASES if k == name)
    feats, idx, w = R.gauss_interp_inputs(b, c, m, n, seed=c + m)
    return (feats, idx, w) + R.three_interpolate_fp64(feats, idx, w)


@functools.lru_cache(maxsize=None)
def _interp_gauss_oracle(name, mode):
    feats, idx, w, _, _ = _interp_gauss(name)
    before = po._load().po_get_contraction()                                            # (a caller under the mode fixture keeps its mode)
    po.set_contraction(mode)
    try:
        return po.three_interpolate(feats, idx, w)
    finally:
        po.set_contraction(before)


@functools.lru_cache(maxsize=None)
def _nn_sized(n, m):
    unk, kn = R.exact_coords(2, n, seed=n + 3 * m), R.exact_coords(2, m, seed=7 * n + m + 1)
    return (unk, kn) + R.three_nn_lex(unk, kn)


@functools.lru_cache(maxsize=None)
def _nn_constructions():
    """{name: (unknown, known, d2 fp64, idx)}, every construction's claim asserted on the reference first"""
    out = {}
    unk, kn, want = R.twins_over_tile_edge()
    d2, idx = R.three_nn_lex(unk, kn)
    assert kn.shape[1] == 2 * R.NN_TILE + 4
    for b in range(2):
        assert tuple(idx[b, 0]) == want[0] and tuple(d2[b, 0]) == (0.0, 0.0, 0.5)
        assert tuple(idx[b, 1, :2]) == want[1] and tuple(d2[b, 1, :2]) == (0.0, 0.0) and d2[b, 1, 2] > 0
        assert tuple(idx[b, 2]) == want[2] and tuple(d2[b, 2]) == (0.25, 0.25, 0.25)
        assert np.count_nonzero(((kn[b] - unk[b, 2]) ** 2).sum(-1) == 0.25) == 4       # 2049 is the fourth at that distance, and loses
    out["twins_over_tile_edge"] = (unk, kn, d2, idx)
    for m in (7, 2):
        unk, kn, want, filled = R.all_known_identical(m)
        d2, idx = R.three_nn_lex(unk, kn)
        assert (idx == np.array(want, np.int32)).all() and np.isfinite(d2[..., :filled]).all() and np.isinf(d2[..., filled:]).all()
        assert (d2[..., :filled] == d2[..., :1]).all()
        if m == 7:
            assert len({k % R.NN_SPLIT for k in want}) == 3                             # three different lanes of the quad
        out[f"all_known_identical_{m}"] = (unk, kn, d2, idx)
    unk, kn, want = R.last_three_nearest()
    d2, idx = R.three_nn_lex(unk, kn)
    assert kn.shape[1] - R.NN_TILE == 3 and (idx == np.array(want, np.int32)).all() and (d2[..., 2] < 1).all()
    assert (((unk[:, :, None, :] - kn[:, None, :R.NN_TILE, :]) ** 2).sum(-1) >= 1).all()
    out["last_three_nearest"] = (unk, kn, d2, idx)
    unk, kn, want = R.nearest_in_every_sublane()
    d2, idx = R.three_nn_lex(unk, kn)
    assert [k % R.NN_SPLIT for k in want] == [0, 1, 2, 3] and (idx[:, :, 0] == np.array(want, np.int32)).all()
    assert (d2[..., 0] == 0).all() and (d2[..., 1] > 0).all()
    out["nearest_in_every_sublane"] = (unk, kn, d2, idx)
    for m in (2, 4):
        unk, kn, far = R.far_known_point(m)
        d2, idx = R.three_nn_lex(unk, kn)
        with np.errstate(over="ignore"):
            assert np.isinf(((unk[:, :, None, :] - kn[:, None, far:far + 1, :]) ** 2).sum(-1).astype(np.float32)).all()
        assert (((unk[:, :, None, :].astype(np.float64) - kn[:, None, far:far + 1, :]) ** 2).sum(-1) < 1e40).all()   # a finite double: only fp32 overflows
        if m == 2:
            assert not idx.any() and np.isfinite(d2[..., 0]).all() and np.isinf(d2[..., 1:]).all()
        else:
            assert np.isfinite(d2).all() and not (idx == far).any() and all(sorted(t) == [0, 2, 3] for t in idx.reshape(-1, 3).tolist())
        out[f"far_known_point_{m}"] = (unk, kn, d2, idx)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {at}: got {got[at]:#010x}, want {want[at]:#010x}")


def _equals_fp64(got, ref, what):
    """a fp32 result against the fp64 reference of exact inputs: the same number, element for element"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bad = got.astype(np.float64) != ref
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {at}: got {got[at]!r}, want {ref[at]!r}")


# ---- a. coverage: no GPU ----------------------------------------------------------------------------------------------------------------------
def test_group_cases_reach_both_kernels_and_every_tail():
    """Fails when an edit of the case list, or of the launch's choice, loses a class: both kernels, one live thread, one full workgroup, one
    thread beyond it, a channel tail and none, and the alignment branch with a total that would otherwise vectorise."""
    form, _ = _forms()
    got = {}
    for name, (b, c, n, npoint, nsample), opt, want in GROUP_CASES:
        idx_at = ALIGNED + 4 * opt.get("idx_offset", 0)
        got[name] = form(npoint, nsample, idx_at, ALIGNED)
        assert got[name] == want, (name, got[name])
    vec = [s for name, s, _, _ in GROUP_CASES if got[name] == 1]
    sca = [(s, o) for name, s, o, _ in GROUP_CASES if got[name] == 0]
    assert {p * k for _, _, _, p, k in vec} >= {4, 1024, 1028}
    assert {c % GP_CH for _, c, _, _, _ in vec} >= {0, 1} and any(c > 2 * GP_CH for _, c, _, _, _ in vec) and any(c < GP_CH for _, c, _, _, _ in vec)
    assert any((p * k) % 4 != 0 for (_, _, _, p, k), _ in sca) and any(o.get("gather") and p > 256 for (_, _, _, p, k), o in sca)
    assert any((p * k) % 4 == 0 and o.get("idx_offset") == 1 for (_, _, _, p, k), o in sca)
    # the thresholds themselves
    for total in (4, 1024, 1028):
        assert form(total // 4, 4, ALIGNED, ALIGNED) == 1 and form(total, 1, ALIGNED, ALIGNED) == 1
        assert form(total // 4, 4, ALIGNED + 4, ALIGNED) == 0                            # idx 4 bytes into its allocation
        assert form(total // 4, 4, ALIGNED, ALIGNED + 8) == 0 and form(total // 4, 4, ALIGNED + 16, ALIGNED + 32) == 1
    assert form(51, 5, ALIGNED, ALIGNED) == 0 and form(255, 1, ALIGNED, ALIGNED) == 0 and form(0, 4, ALIGNED, ALIGNED) == 0
    assert form(65535 * 256, 4, ALIGNED, ALIGNED) == 1 and form(65535 * 256 + 1, 4, ALIGNED, ALIGNED) == 0   # the grid cap: 65535 chunks in y


def test_interp_cases_reach_both_kernels_and_both_staging_copies():
    """Fails when the case list or the launch's choice loses the threshold, a workgroup edge, a channel tail or one of the staging copies."""
    _, form = _forms()
    assert form(4, 2048) == 1 and form(4, 2049) == 0 and form(4, 0) == 0 and form(4, 1) == 1 and form(1, 2048) == 1
    got = {name: form(s[1], s[2]) for name, s, _, _ in INTERP_CASES}
    assert got == {name: want for name, _, _, want in INTERP_CASES}
    lds = [(s, off) for name, s, off, _ in INTERP_CASES if got[name] == 1]
    glo = [s for name, s, _, _ in INTERP_CASES if got[name] == 0]
    assert any(m == 2048 for (_, _, m, _), _ in lds) and any(m == 2049 for _, _, m, _ in glo)
    assert any(n == IL_WG + 1 for (_, _, _, n), _ in lds) and any(n == IL_WG for (_, _, _, n), _ in lds) and any(n == 1 for (_, _, _, n), _ in lds)
    assert {c % IL_CB for (_, c, _, _), _ in lds} >= {0, 1, 3} and any(c < IL_CB for (_, c, _, _), _ in lds)
    assert {c % IC_CH for _, c, _, _ in glo} >= {0, 1} and any(c > IC_CH for _, c, _, _ in glo)
    assert any(n == 257 for _, _, _, n in glo) and any(n == 256 for _, _, _, n in glo) and any(n % 256 == 255 for _, _, _, n in glo)
    rows = [r for (b, c, m, n), off in lds for r in _staging(b, c, m, base=4 * off)]
    assert {r[-1] for r in rows} == {"float4", "dword"}
    assert any(a != 0 and l == 0 for _, _, _, a, l, _ in rows), "length a multiple of 4, base unaligned"
    assert any(a == 0 and l != 0 for _, _, _, a, l, _ in rows) and any(nc == 1 for _, _, nc, _, _, _ in rows)
    assert [r[-1] for r in _staging(2, 5, 6)] == ["float4", "dword", "dword", "dword"] and _staging(2, 5, 6)[2][3:5] == (8, 0)
    assert {r[-1] for r in _staging(2, 4, 2048)} == {"float4"} and {r[-1] for r in _staging(2, 8, 64, base=4)} == {"dword"}
    # every set names m - 1 in every staged row ("last"), and the random sets do somewhere
    for name, (b, c, m, n), _, _ in INTERP_CASES:
        sets = _interp_exact(name)[1]
        assert (sets["last"][0] == m - 1).all() and not sets["first"][0].any() and (sets["same"][0] == sets["same"][0][:, :, :1]).all()
        assert (sets["zero_weight"][1][:, :, 1] == 0).all() and (sets["zero_weight"][1][:, :, 0] > 0).all()
        assert all(0 <= s[0].min() and s[0].max() < m for s in sets.values())


def test_three_nn_sizes_straddle_every_edge():
    """Fails when an edit of NN_SIZES loses a side of an LDS tile edge, of the 64-query workgroup edge, a count below three or a residue of
    the four-lane split."""
    ms = sorted({m for _, m in NN_SIZES})
    assert set(ms) >= {0, 1, 2, 3, 4, 5, R.NN_TILE - 1, R.NN_TILE, R.NN_TILE + 1, 2 * R.NN_TILE, 2 * R.NN_TILE + 1}
    assert {n for n, _ in NN_SIZES} >= {1, 63, 64, 65, 130}                              # 64 queries per workgroup
    assert {m % R.NN_SPLIT for m in ms} == {0, 1, 2, 3}


# ---- the inputs tell clouds, channels and points apart; the constructions hold what they claim --------------------------------------------------
def test_structured_inputs_tell_clouds_channels_and_points_apart():
    """A kernel that read another cloud, another channel or a neighbouring point would change the reference's answer: swapping two clouds,
    swapping two channels and rotating idx by one each do."""
    b, c, m, n = 2, 5, 6, 300
    feats, sets = _interp_exact("lds_2x5x6_300")
    idx, w, ref = sets["random"]
    assert feats.min() >= -8 and feats.max() <= 8 and np.array_equal(feats, np.round(feats)) and np.array_equal(w * 8, np.round(w * 8))
    assert w.min() >= 0 and w.max() <= 1
    swapped = feats.copy(); swapped[:, [0, 1]] = feats[:, [1, 0]]
    for other in (R.three_interpolate_fp64(feats[::-1], idx, w)[0], R.three_interpolate_fp64(swapped, idx, w)[0],
                  R.three_interpolate_fp64(feats, (idx + 1) % m, w)[0]):
        assert (other != ref)[:, :2].mean() > 0.5                                        # (channels 0 and 1: the swapped pair)
    for name, (b, c, m, n), _, _ in INTERP_CASES:                                        # every case: neighbouring blocks and clouds differ
        f = _interp_exact(name)[0]
        assert all((f[:, k] != f[:, k - 1]).any() for k in range(1, c)) and (b == 1 or (f[0] != f[1]).any())
        assert all((f[:, k] != f[:, k - IL_CB]).any() for k in range(IL_CB, c)) and all((f[:, k] != f[:, k - IC_CH]).any() for k in range(IC_CH, c))
    pts, gsets = _group_inputs("total_1028")
    idx, ref = gsets["random"]
    swapped = pts.copy(); swapped[:, [0, 1]] = pts[:, [1, 0]]
    for other in (R.group(pts[::-1], idx), R.group(swapped, idx), R.group(pts, (idx + 1) % 50)):
        assert (_bits(other) != _bits(ref))[:, :2].mean() > 0.5
    for n, m in ((65, 70), (65, 4097)):
        unk, kn, d2, idx = _nn_sized(n, m)
        assert np.array_equal(unk * 4, np.round(unk * 4)) and np.abs(kn).max() <= 2 and np.abs(unk).max() <= 2
        d2s, idxs = R.three_nn_lex(unk, kn[::-1])
        assert (idxs != idx).mean() > 0.5
    unk, kn, d2, idx = _nn_sized(65, 4097)
    assert (d2[..., 0] == d2[..., 1]).any(), "the quarter lattice repeats sites: exact ties"


def test_group_features_carry_every_special_where_an_index_reads_it():
    """-0.0, denormals, +-Inf and NaNs of two payloads are in the rows AND in the expected outputs: a kernel that recomputed a value (x * 1,
    x + 0, a flush to zero, a canonical NaN) instead of copying it would differ in one of them."""
    for name, (b, c, n, npoint, nsample), _, _ in GROUP_CASES:
        pts, sets = _group_inputs(name)
        present = set(_bits(pts).reshape(-1).tolist())
        if n >= len(R.SPECIALS):
            assert present >= set(R.SPECIALS.tolist()), name
            read = set().union(*(set(_bits(ref).reshape(-1).tolist()) for _, ref in sets.values()))
            assert read >= set(R.SPECIALS.tolist()), name
            if npoint * nsample >= 64:
                assert set(_bits(sets["random"][1]).reshape(-1).tolist()) >= set(R.SPECIALS.tolist()), name
        else:
            assert present & set(R.SPECIALS.tolist()), name
        idx = sets["padded"][0]
        assert (idx[:, :, -1] == idx[:, :, 0]).mean() > (0.3 if nsample > 1 else 0.99) and (sets["last"][0] == n - 1).all()
    assert np.isnan(R.SPECIALS.view(np.float32)[-2:]).all() and R.SPECIALS[-2] & 0x3FFFFF != R.SPECIALS[-1] & 0x3FFFFF


def test_three_nn_constructions_hold_what_they_claim():
    """the claims are asserted where the constructions are built (shared with the GPU tests); swapping the clouds changes the answer"""
    cons = _nn_constructions()
    assert set(cons) == {"twins_over_tile_edge", "all_known_identical_7", "all_known_identical_2", "last_three_nearest", "nearest_in_every_sublane",
                         "far_known_point_2", "far_known_point_4"}
    unk, kn, d2, idx = cons["twins_over_tile_edge"]
    d2s, idxs = R.three_nn_lex(unk, kn[::-1])
    assert (idxs[:, 3:] != idx[:, 3:]).any() and np.array_equal(idxs[:, :3, :2], idx[:, :3, :2])


# ---- b. the references against the oracle: no GPU ----------------------------------------------------------------------------------------------
def test_group_reference_equals_oracle_bit_for_bit():
    """tests/pointops_fwd_ref.py and oracle/pointops_oracle.c are two independent statements of the copy; a wrong stride or a value that went
    through arithmetic in either shows here"""
    for name, (b, c, n, npoint, nsample), opt, _ in GROUP_CASES:
        pts, sets = _group_inputs(name)
        for k, (idx, ref) in sets.items():
            _same_bits(po.group_points(pts, idx), ref, f"{name} {k}")
            if opt.get("gather"):
                _same_bits(po.gather_points(pts, idx[:, :, 0]), R.gather(pts, idx[:, :, 0]), f"{name} {k} (gather)")
                _same_bits(R.gather(pts, idx[:, :, 0]), ref[..., 0], f"{name} {k} (gather is group)")


def test_interp_reference_equals_oracle_in_every_mode():
    """on the exact inputs the fp64 sum IS the fp32 result of every contraction: the oracle's three modes all equal it, element for element"""
    try:
        for mode in MODES:
            po.set_contraction(mode)
            for name, _, _, _ in INTERP_CASES:
                feats, sets = _interp_exact(name)
                for k, (idx, w, ref) in sets.items():
                    _equals_fp64(po.three_interpolate(feats, idx, w), ref, f"{name} {k} {mode}")
    finally:
        po.set_contraction("fma_llvm")


def test_three_nn_reference_equals_oracle_in_every_mode():
    """the lexicographic definition against the oracle's scan, on every size and every construction, in every mode: indices equal, squared
    distances equal as numbers (+inf for the unfilled slots)"""
    cases = [(f"n={n} m={m}", _nn_sized(n, m)) for n, m in NN_SIZES] + list(_nn_constructions().items())
    try:
        for mode in MODES:
            po.set_contraction(mode)
            for name, (unk, kn, d2, idx) in cases:
                od2, oidx = po.three_nn(unk, kn)
                assert np.array_equal(oidx, idx), (name, mode)
                _equals_fp64(od2, d2, f"{name} {mode}")
    finally:
        po.set_contraction("fma_llvm")


def test_oracle_modes_differ_on_the_gaussian_inputs():
    """the mode fixture of the Gaussian test is not vacuous: each pair of contraction modes differs in some output bit on these inputs"""
    for name in ("lds_2x5x6_300", "global_2x9x2049_257"):
        o = {mode: _bits(_interp_gauss_oracle(name, mode)) for mode in MODES}
        for a, b in (("fma_llvm", "fma_chain"), ("fma_llvm", "none"), ("fma_chain", "none")):
            assert (o[a] != o[b]).any(), (name, a, b)


def test_empty_calls_return_zero_without_a_device():
    """b = 0, c = 0, npoint = 0, n = 0: nothing to do is success, decided before any pointer is looked at"""
    import ctypes
    from unipre3d_amd import pointops
    lib, null = pointops.load(), ctypes.c_void_p(0)
    for (b, c, npoint) in ((0, 3, 2), (2, 0, 2), (2, 3, 0)):
        assert lib.u3d_group_points(b, c, 5, npoint, 4, null, null, null, null) == 0
        assert lib.u3d_gather_points(b, c, 5, npoint, null, null, null, null) == 0
    for (b, c, n) in ((0, 3, 2), (2, 0, 2), (2, 3, 0)):
        assert lib.u3d_three_interpolate(b, c, 5, n, null, null, null, null, null) == 0
    for (b, n) in ((0, 2), (2, 0)):
        assert lib.u3d_three_nn(b, n, 5, null, null, null, null, null) == 0


# ---- GPU helpers --------------------------------------------------------------------------------------------------------------------------------
def _view_at(a, offset):
    """the array on the device as a contiguous view `offset` ELEMENTS into a larger buffer (offset 0: a tensor of its own)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if offset == 0:
        return t.cuda()
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * t.element_size()) % 16
    return v


# ---- c. group / gather ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", GROUP_CASES, ids=_ids(GROUP_CASES))
def test_group_gather_copy_the_bits(case):
    """out[b, c, p, s] carries the BITS of points[b, c, idx[b, p, s]] (uint32 compare: -0.0, denormals, Inf, NaN payloads), for random indices,
    all 0, all n - 1 and ball-query padding, in the kernel the case claims.  Fails on a wrong chunk / channel-block / cloud offset, on a tail
    thread or channel that is skipped or runs over, on an int4 load from an address that is not on 16 bytes, on any arithmetic on the value."""
    from unipre3d_amd import pointops
    name, (b, c, n, npoint, nsample), opt, want_form = case
    form, _ = _forms()
    pts, sets = _group_inputs(name)
    pts_t = _view_at(pts, opt.get("points_offset", 0))
    for k, (idx, ref) in sets.items():
        ix = idx[:, :, 0] if opt.get("gather") else idx
        idx_t = _view_at(ix.astype(np.int64) if opt.get("int64") else ix, opt.get("idx_offset", 0))
        if opt.get("idx_offset") == 1:
            assert idx_t.data_ptr() % 16 == 4
        out = (pointops.gather_operation if opt.get("gather") else pointops.grouping_operation)(pts_t, idx_t)
        seen = ALIGNED if opt.get("int64") else idx_t.data_ptr()                        # (int64 indices reach the kernel as a fresh int32 tensor)
        assert form(npoint, nsample, seen, out.data_ptr()) == want_form, (name, k)
        _same_bits(out.cpu().numpy(), ref[..., 0] if opt.get("gather") else ref, f"{name} {k}")


# ---- d. three_interpolate -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", INTERP_CASES, ids=_ids(INTERP_CASES))
def test_three_interpolate_exact(case, contraction):
    """Integer features, weights in eighths: the output EQUALS the fp64 sum in every contraction mode, for random triples, i0 == i1 == i2, every
    index m - 1 (the last element of every staged row), every index 0, and a weight of exactly 0.  Fails on a wrong channel-block or cloud
    offset, a wrong `nc` clamp, a padded channel or a clamped dead point leaking into a store, a staging copy that misses its tail or reads
    float4 from an unaligned row."""
    from unipre3d_amd import pointops
    name, (b, c, m, n), off, want_form = case
    assert _forms()[1](c, m) == want_form
    feats, sets = _interp_exact(name)
    f_t = _view_at(feats, off)
    assert f_t.data_ptr() % 16 == 4 * off
    for k, (idx, w, ref) in sets.items():
        out = pointops.three_interpolate(f_t, _view_at(idx, 0), _view_at(w, 0))
        _equals_fp64(out.cpu().numpy(), ref, f"{name} {k} {contraction}")


@gpu
@pytest.mark.parametrize("case", INTERP_CASES, ids=_ids(INTERP_CASES))
def test_three_interpolate_gaussian(case, contraction, capsys):
    """Gaussian features, uniform weights.  (1) bit-equal to the oracle in the current mode (the modes differ on these inputs:
    test_oracle_modes_differ_on_the_gaussian_inputs), which fails on the wrong product left unfused.  (2) Independently of the oracle,
    |got - fp64| <= 6 * 2^-24 * mag, mag = sum_k |w_k p_k|: three rounded products and two rounded additions, each at most 2^-24 of a partial sum
    that does not exceed mag, and one unit for second-order terms -- derived, not measured."""
    from unipre3d_amd import pointops
    name, (b, c, m, n), off, _ = case
    feats, idx, w, ref, mag = _interp_gauss(name)
    out = pointops.three_interpolate(_view_at(feats, off), _view_at(idx, 0), _view_at(w, 0)).cpu().numpy()
    ratio = float((np.abs(out.astype(np.float64) - ref) / (2.0 ** -24 * mag)).max())
    with capsys.disabled():
        print(f"\n[pointops fwd] three_interpolate {name} {contraction}: worst |got - fp64| / (2^-24 mag) = {ratio:.3f} (bound 6)")
    _same_bits(out, _interp_gauss_oracle(name, contraction), f"{name} {contraction} against the oracle")
    assert (mag > 0).all() and ratio <= 6.0, ratio


# ---- e. three_nn --------------------------------------------------------------------------------------------------------------------------------
def _check_three_nn(unk, kn, d2, idx, what):
    import torch
    from unipre3d_amd import pointops
    dist, got = pointops.three_nn(torch.from_numpy(unk).cuda(), torch.from_numpy(kn).cuda())
    assert got.dtype == torch.int32 and dist.dtype == torch.float32
    got, dist = got.cpu().numpy(), dist.cpu().numpy()
    bad = (got != idx).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} queries differ, first {tuple(np.argwhere(bad)[0])}: got {got[bad][0]}, want {idx[bad][0]}"
    f32 = d2.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), d2)
    assert np.array_equal(dist, np.sqrt(f32)), what                                      # the wrapper returns L2 distances


@gpu
@pytest.mark.parametrize("n,m", NN_SIZES, ids=[f"n{n}_m{m}" for n, m in NN_SIZES])
def test_three_nn_sizes_exact(n, m, contraction):
    """Quarter-lattice clouds (two different ones: the batch offset matters), full of exact ties: indices equal the lexicographic definition,
    distances the root of the exact squared distance.  Fails on a tile whose tail is scanned too far or not at all (m = 2047 .. 2049, 4096,
    4097), on a query tail of the 64-query workgroup (n = 63 .. 65), on unfilled slots that are not (+inf, 0) (m < 3), on a tie to the higher index."""
    unk, kn, d2, idx = _nn_sized(n, m)
    _check_three_nn(unk, kn, d2, idx, f"three_nn n={n} m={m} {contraction}")


@gpu
@pytest.mark.parametrize("name", ["twins_over_tile_edge", "all_known_identical_7", "all_known_identical_2", "last_three_nearest",
                                  "nearest_in_every_sublane", "far_known_point_2", "far_known_point_4"])
def test_three_nn_constructions(name, contraction):
    """Ties placed on purpose: twins in two LDS tiles and at both ends of the cloud, four points at one distance around the tile edge, ties held
    by three different lanes of the quad (the merge must order by index), winners in a 3-point last tile, the nearest point in each of the
    four lanes, and a point whose fp32 squared distance is +inf (never inserted: the slot stays (+inf, 0))."""
    unk, kn, d2, idx = _nn_constructions()[name]
    _check_three_nn(unk, kn, d2, idx, f"three_nn {name} {contraction}")


# ---- f. empties ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_empty_shapes_through_the_wrappers():
    """b = 0, c = 0, npoint = 0, n = 0: tensors of the right shape, no error (the library returns 0 and launches nothing)"""
    import torch
    from unipre3d_amd import pointops
    dev = "cuda"
    f = lambda *s: torch.zeros(*s, device=dev)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    for (b, c, npoint) in ((0, 3, 2), (2, 0, 2), (2, 3, 0)):
        assert pointops.grouping_operation(f(b, c, 5), i(b, npoint, 4)).shape == (b, c, npoint, 4)
        assert pointops.gather_operation(f(b, c, 5), i(b, npoint)).shape == (b, c, npoint)
    for (b, c, n) in ((0, 3, 2), (2, 0, 2), (2, 3, 0)):
        out = pointops.three_interpolate(f(b, c, 5), i(b, n, 3), f(b, n, 3))
        assert out.shape == (b, c, n) and out.dtype == torch.float32
    for (b, n) in ((0, 2), (2, 0)):
        dist, idx = pointops.three_nn(f(b, n, 3), f(b, 5, 3))
        assert dist.shape == (b, n, 3) and idx.shape == (b, n, 3) and idx.dtype == torch.int32
    torch.cuda.synchronize()
