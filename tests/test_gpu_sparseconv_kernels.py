"""The contraction kernels of u3d_sparseconv.hip (gemm_mfma / gemm_valu, wgrad_mfma / wgrad_valu<>, split_sum / split_sum_wave, colsum,
dupsum) called through sparseconv._gemm / _wgrad / _colsum / _dupsum on hand-made tables -- no map kernel involved -- at every tile and
split class, against the plain int64 / fp64 references of tests/spconv_kernel_ref.py.

Exact cases: A, W, G and bias hold integers from -4 .. 4 in fp32.  Every product and every partial sum stays below 2^24 (the largest GEMM
sum is 27 * 65 * 16 + 4, the largest row sum 129 025 * 4, the largest weight-gradient sum 32 257 * 16), so any summation order, with or
without fma and through the MFMA chains, gives the integer result exactly and the comparison is bit for bit.

The class boundaries come from the header's U3D_SPCONV_* macros and the split counts from the library's two partial_floats queries
(host arithmetic), so the shape lists are checked for coverage without a GPU."""
import numpy as np
import pytest
import torch

import spconv_kernel_ref as KR
from test_gpu_sparseconv import TOL_W, TOL_X

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
MACROS = KR.header_macros()
SMALL_C, TILE, KSTEP, WAVE_SUM = MACROS["SMALL_C"], MACROS["TILE"], MACROS["KSTEP"], MACROS["WAVE_SUM_SPLITS"]

# ---- shape lists ---------------------------------------------------------------------------------------------------------------------------------
GEMM_ROWS = [1, 63, 64, 65, 129]
GEMM_CHANNELS = [(8, 8), (8, 9), (9, 8), (9, 9), (32, 64), (33, 65), (64, 63), (65, 128)]
GEMM_TAPS = [1, 8, 27]
# every channel pair at every row count; the tap count rotates so that each pair and each row count meets K = 1, 8 and 27
GEMM_SHAPES = [(R, GEMM_TAPS[(i + j) % 3], ci, co) for i, (ci, co) in enumerate(GEMM_CHANNELS) for j, R in enumerate(GEMM_ROWS)]
LIST_SHAPES = [(R, K, ci, co) for (ci, co) in [(8, 9), (9, 9), (33, 65), (65, 128)] for R, K in [(1, 8), (65, 27), (129, 8)]]
MASK_SHAPES = [(65, 8, 8, 8), (129, 27, 9, 9), (129, 8, 33, 65)]
CONTAIN_SHAPES = [(129, 8, 8, 9), (129, 8, 33, 65)]
WGRAD_SHAPES = [(1, 27, 16, 16), (31, 8, 9, 9), (32, 8, 9, 9), (33, 8, 9, 9), (33, 8, 33, 65), (257, 27, 65, 9), (300, 8, 8, 16), (300, 8, 9, 16),
                (513, 27, 6, 6), (16128, 27, 16, 16), (16129, 27, 16, 16), (16385, 1, 16, 16), (19201, 27, 16, 16), (32256, 8, 3, 16),
                (32257, 8, 3, 16), (32257, 8, 16, 6)]
COLSUM_SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (2048, 64), (2049, 65), (129024, 16), (129025, 16)]
# Gaussian data, one shape per kernel class
VALUE_GEMM = [("table", 300, 27, 6, 37), ("table", 300, 27, 33, 65), ("list", 300, 8, 65, 128)]
VALUE_WGRAD = [(513, 27, 6, 6), (32257, 8, 3, 16), (32257, 8, 16, 6), (257, 27, 65, 9), (19201, 27, 16, 16)]
VALUE_COLSUM = [(2049, 65), (129025, 16)]


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _load():
    from unipre3d_amd import sparseconv
    return sparseconv.load()


def gemm_class(Cin, Cout):
    return "valu" if Cin <= SMALL_C or Cout <= SMALL_C else "mfma"


def wgrad_class(Cin, Cout):
    if Cin <= SMALL_C:
        return "valu_both" if Cout <= SMALL_C else "valu_cin"
    return "valu_cout" if Cout <= SMALL_C else "mfma"


def wgrad_splits(R, K, Cin, Cout):
    """(splits launched, rows per split, splits that own a row)"""
    splits = _load().u3d_spconv_wgrad_partial_floats(R, K, Cin, Cout) // (K * Cin * Cout)
    rps = -(-(-(-R // splits)) // KSTEP) * KSTEP
    return splits, rps, -(-R // rps)


def colsum_splits(R, C):
    return _load().u3d_spconv_colsum_partial_floats(R, C) // C


# ---- a. coverage: no GPU ------------------------------------------------------------------------------------------------------------------------
def test_shape_lists_reach_every_tile_and_split_class():
    """a retune of a threshold (header macro or split rule) fails here instead of silently moving a shape out of its class"""
    S = SMALL_C
    assert {(S, S), (S, S + 1), (S + 1, S), (S + 1, S + 1)} <= set(GEMM_CHANNELS)
    assert [gemm_class(*c) for c in [(S, S), (S, S + 1), (S + 1, S), (S + 1, S + 1)]] == ["valu", "valu", "valu", "mfma"]
    mf = [c for c in GEMM_CHANNELS if gemm_class(*c) == "mfma"]
    assert any(co == TILE + 1 for _, co in mf), "a second column tile holding one column"
    assert any(co == TILE - 1 for _, co in mf) and any(co == 2 * TILE for _, co in mf) and any(co == TILE for _, co in mf)
    assert any(ci == KSTEP + 1 for ci, _ in mf) and any(ci == 2 * KSTEP + 1 for ci, _ in mf) and any(ci == KSTEP for ci, _ in mf)
    assert {1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1} <= set(GEMM_ROWS)
    for c in GEMM_CHANNELS:   # every pair at every row count and at K = 1, 8, 27
        assert {R for R, K, ci, co in GEMM_SHAPES if (ci, co) == c} == set(GEMM_ROWS)
        assert {K for R, K, ci, co in GEMM_SHAPES if (ci, co) == c} == set(GEMM_TAPS)
    for shapes in (LIST_SHAPES, MASK_SHAPES, CONTAIN_SHAPES):
        assert {gemm_class(ci, co) for _, _, ci, co in shapes} == {"valu", "mfma"}
    assert any(R > TILE and gemm_class(ci, co) == "mfma" for R, _, ci, co in LIST_SHAPES)
    assert {gemm_class(ci, co) for _, _, _, ci, co in VALUE_GEMM} == {"valu", "mfma"} and {m for m, *_ in VALUE_GEMM} == {"table", "list"}

    # weight gradient: kernel classes, then split counts per class
    info = {s: (wgrad_class(s[2], s[3]),) + wgrad_splits(*s) for s in WGRAD_SHAPES}
    assert {v[0] for v in info.values()} == {"valu_cin", "valu_cout", "valu_both", "mfma"}, info
    assert wgrad_class(S, S + 8) == "valu_cin" and wgrad_class(S + 1, S + 8) == "mfma" and (300, 8, S, 16) in info and (300, 8, S + 1, 16) in info
    by = lambda cls: {s: v for s, v in info.items() if v[0] == cls}
    n = lambda d: sorted({v[1] for v in d.values()})
    mfma = by("mfma")
    assert n(mfma)[0] == 1 and any(1 < x < WAVE_SUM - 1 for x in n(mfma)), n(mfma)
    assert info[(16128, 27, 16, 16)][1] == WAVE_SUM - 1 and info[(16129, 27, 16, 16)][1] == WAVE_SUM       # 63 | 64: thread sum | wave sum
    assert any(x > max(WAVE_SUM, 64) for x in n(mfma)), "a lane of the wave sum adds two partials"
    assert info[(16385, 1, 16, 16)][1] == 65 and info[(19201, 27, 16, 16)][1:] == (75, 288, 67), info       # eight trailing splits own no row
    assert any(v[3] < v[1] for v in mfma.values()), "a shape with empty trailing splits"
    assert any(s[0] < KSTEP for s in mfma) and {KSTEP - 1, KSTEP, KSTEP + 1} <= {s[0] for s in mfma}         # a split shorter than one step
    assert any(s[2] > TILE for s in mfma) and any(s[3] > TILE for s in mfma)                               # a second tile of Cin, of Cout
    assert info[(32256, 8, 3, 16)][1] == WAVE_SUM - 1 and info[(32257, 8, 3, 16)][1] == WAVE_SUM             # the VALU kernels at 63 | 64
    assert info[(32257, 8, 16, 6)][:2] == ("valu_cout", WAVE_SUM)
    assert any(1 < v[1] < WAVE_SUM - 1 for v in by("valu_both").values()) and any(v[1] == 1 for v in by("valu_cin").values())
    assert {wgrad_class(s[2], s[3]) for s in VALUE_WGRAD} == {"valu_cin", "valu_cout", "valu_both", "mfma"} and set(VALUE_WGRAD) <= set(info)
    assert any(info[s][1] >= WAVE_SUM for s in VALUE_WGRAD) and any(info[s][1] < WAVE_SUM for s in VALUE_WGRAD)

    # bias gradient
    cs = {s: colsum_splits(*s) for s in COLSUM_SHAPES}
    assert cs[(2048, 64)] == 1 and cs[(2049, 65)] == 2 and cs[(129024, 16)] == WAVE_SUM - 1 and cs[(129025, 16)] == WAVE_SUM, cs
    assert {C for _, C in COLSUM_SHAPES} >= {1, 63, 64, 65}                                                   # one and two 64-column workgroups
    assert sorted(colsum_splits(*s) for s in VALUE_COLSUM) == [2, WAVE_SUM]


def test_exact_data_stays_below_two_to_the_24():
    """the claim of the module docstring, for the shapes of the lists"""
    big = 2 ** 24
    assert all(K * ci * 16 + 4 < big for _, K, ci, _ in GEMM_SHAPES + LIST_SHAPES + MASK_SHAPES + CONTAIN_SHAPES)
    assert all(R * 16 < big for R, *_ in WGRAD_SHAPES) and all(R * 4 < big for R, _ in COLSUM_SHAPES)
    assert max(R * C for R, C in COLSUM_SHAPES) * 4 <= 8.3e6 and max(R * K for R, K, _, _ in WGRAD_SHAPES) * 4 <= 8.3e6   # bytes of the largest buffers


# ---- helpers of the GPU tests ---------------------------------------------------------------------------------------------------------------------
def _ints(g, *shape):
    return torch.as_tensor(g.integers(-4, 5, size=shape)).float()


def _d(a, dt=None):
    if a is None:
        return None
    return torch.as_tensor(a).to(DEV, dt) if dt is not None else torch.as_tensor(a).to(DEV)


def _exact(ref):
    f = ref.float()
    assert torch.equal(f.double(), ref), "the integer-valued reference must be representable in fp32"
    return f


def _same(got, want, what):
    """bit-for-bit equality (NaN equals NaN), with the first mismatch in the message"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    if bool(bad.any()):
        at = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: got {got[at].item()!r}, want {want[at].item()!r}")


def _gemm(R, K, A, W, bias, table, list_row=None, mask=None, out_rows=None):
    from unipre3d_amd import sparseconv as sp
    return sp._gemm(R, K, _d(A), _d(W), _d(bias), _d(table, torch.int32), _d(list_row, torch.int32), _d(mask, torch.int32), out_rows)


def _wgrad_poisoned(R, K, A, G, table, gather_g):
    """the C-ABI call with `partial` filled with NaN: a partial that no workgroup writes (a split that owns no row) shows"""
    from unipre3d_amd import _lib
    Cin, Cout = A.shape[1], G.shape[1]
    lib = _load()
    part = torch.full((max(lib.u3d_spconv_wgrad_partial_floats(R, K, Cin, Cout), 1),), float("nan"), device=DEV)
    dW = torch.full((K, Cin, Cout), float("nan"), device=DEV)
    rc = lib.u3d_spconv_wgrad(R, K, Cin, Cout, _lib.ptr(table), int(gather_g), _lib.ptr(A), _lib.ptr(G), _lib.ptr(part), _lib.ptr(dW),
                              _lib.stream_ptr(DEV))
    assert rc == 0
    return dW


def _colsum_poisoned(G):
    from unipre3d_amd import _lib
    R, C = G.shape
    lib = _load()
    part = torch.full((max(lib.u3d_spconv_colsum_partial_floats(R, C), 1),), float("nan"), device=DEV)
    db = torch.full((C,), float("nan"), device=DEV)
    assert lib.u3d_spconv_colsum(R, C, _lib.ptr(G), _lib.ptr(part), _lib.ptr(db), _lib.stream_ptr(DEV)) == 0
    return db


def _n_src(R, i):
    """source tensors with as many rows as R, more, and fewer"""
    return (R, R + 37, max(1, R // 2))[i % 3]


# ---- b. GEMM, exact -------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=_id)
def test_gemm_table_mode_exact(shape):
    """every table pattern; the source tensor has R rows, more, or fewer; with a bias, and for `dense` and `empty` also without"""
    R, K, Cin, Cout = shape
    g = np.random.default_rng(R * 1000 + K * 100 + Cin)
    W, bias = _ints(g, K, Cin, Cout), _ints(g, Cout)
    for i, pattern in enumerate(KR.GEMM_PATTERNS):
        Ra = _n_src(R, i + R)
        A = _ints(g, Ra, Cin)
        T, _ = KR.build_table(pattern, R, K, Ra, TILE, seed=R + K + i)
        for b in ((bias, None) if pattern in ("dense", "empty") else (bias,)):
            got = _gemm(R, K, A, W, b, T)
            what = f"gemm[{gemm_class(Cin, Cout)}] {_id(shape)} {pattern}, A {Ra} rows, bias {b is not None}"
            _same(got, _exact(KR.gemm_ref(A, W, b, T)), what)
            if pattern == "empty":    # the bias bit for bit, or 0
                _same(got, torch.zeros(R, Cout) if b is None else bias.expand(R, Cout), what + " (no source anywhere)")


@gpu
@pytest.mark.parametrize("shape", LIST_SHAPES, ids=_id)
def test_gemm_list_mode_exact(shape):
    """list_row a permutation of the outputs; list_src tap-major, shuffled, all -1, one tap only; A has fewer rows than R, or more"""
    R, K, Cin, Cout = shape
    g = np.random.default_rng(R + K + Cout)
    W, bias = _ints(g, K, Cin, Cout), _ints(g, Cout)
    for i, pattern in enumerate(KR.LIST_PATTERNS):
        Ra = (max(1, R // 8), R + 11)[i % 2]
        A = _ints(g, Ra, Cin)
        list_row, list_src, claim = KR.build_list(pattern, R, K, Ra, seed=R + i)
        for b in (bias, None):
            got = _gemm(R, K, A, W, b, list_src, list_row=list_row, out_rows=R)
            what = f"gemm[{gemm_class(Cin, Cout)}] list mode {_id(shape)} {pattern}, A {Ra} rows, bias {b is not None}"
            _same(got, _exact(KR.gemm_ref(A, W, b, list_src, list_row=list_row, out_rows=R)), what)
            dead = sorted(set(range(R)) - set(claim["live_outputs"]))
            _same(got[dead], torch.zeros(len(dead), Cout) if b is None else bias.expand(len(dead), Cout), what + " (dropped entries)")


@gpu
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=_id)
def test_gemm_mask_zeroes_exactly_the_rows_it_names(shape):
    """rows with mask[o] != o are exactly 0 with and without a bias, the other rows are those of the unmasked run; table and list mode"""
    R, K, Cin, Cout = shape
    g = np.random.default_rng(R + Cin)
    A, W, bias = _ints(g, R, Cin), _ints(g, K, Cin, Cout), _ints(g, Cout) + 5.0     # a bias without zeros: a masked row that got it shows
    mask, kept = KR.build_mask(R, seed=K)
    gone = sorted(set(range(R)) - set(kept))
    assert gone and len(kept) > 1
    list_row, list_src, _ = KR.build_list("shuffled", R, K, R, seed=3)
    for pattern in ("dense", "sparse"):
        T, _ = KR.build_table(pattern, R, K, R, TILE, seed=K)
        for mode, tab, lr in (("table", T, None), ("list", list_src, list_row)):
            for b in (bias, None):
                plain = _gemm(R, K, A, W, b, tab, list_row=lr, out_rows=R)
                got = _gemm(R, K, A, W, b, tab, list_row=lr, mask=mask, out_rows=R)
                what = f"gemm[{gemm_class(Cin, Cout)}] mask {_id(shape)} {pattern} {mode}, bias {b is not None}"
                assert not got[gone].any(), what + ": a row with mask[o] != o is not 0"
                _same(got[kept], plain[kept], what + ": kept rows")
                _same(got, _exact(KR.gemm_ref(A, W, b, tab, list_row=lr, mask=mask, out_rows=R)), what)


@gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("shape", CONTAIN_SHAPES, ids=_id)
def test_gemm_reads_only_the_rows_its_table_names(shape, value):
    """A row of A that no entry references may hold NaN / +Inf: every output is bit-equal to the run with that row zeroed.  A row that exactly
    one output row references makes that output row non-finite, and only that one."""
    R, K, Cin, Cout = shape
    g = np.random.default_rng(R + Cout)
    Ra = R + 3
    A, W, bias = _ints(g, Ra, Cin), _ints(g, K, Cin, Cout), _ints(g, Cout)
    T, _ = KR.build_table("sparse", R, K, Ra - 1, TILE, seed=5)            # row Ra - 1 is referenced by no entry
    assert (T != Ra - 1).all()
    A[Ra - 1] = 0
    clean = _gemm(R, K, A, W, bias, T)
    _same(clean, _exact(KR.gemm_ref(A, W, bias, T)), f"gemm {_id(shape)} clean run")
    A[Ra - 1] = value
    _same(_gemm(R, K, A, W, bias, T), clean, f"gemm[{gemm_class(Cin, Cout)}] {_id(shape)}: an unreferenced row holding {value}")
    for o, k in ((TILE + 5, K - 1), (R - 1, 0), (0, K // 2)):               # inside a block, the last row (a block of one row), the first
        T1 = T.copy()
        T1[o, k] = Ra - 1
        got = _gemm(R, K, A, W, bias, T1)
        others = [r for r in range(R) if r != o]
        A[Ra - 1] = 0
        want = _gemm(R, K, A, W, bias, T1)
        A[Ra - 1] = value
        assert not torch.isfinite(got[o]).any(), f"{_id(shape)}: output row {o} reads the row holding {value}"
        _same(got[others], want[others], f"gemm[{gemm_class(Cin, Cout)}] {_id(shape)}: {value} referenced by row {o} alone")


# ---- c. weight gradient, exact ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_id)
def test_wgrad_exact(shape):
    """both gather sides (the gathered tensor holds more rows than R, or fewer), every table pattern; the wrapper and a call whose partial
    buffer starts as NaN"""
    from unipre3d_amd import sparseconv as sp
    R, K, Cin, Cout = shape
    splits, rps, used = wgrad_splits(*shape)
    print(f"[sparseconv] wgrad {_id(shape)}: {wgrad_class(Cin, Cout)}, {splits} splits of {rps} rows, {used} own a row")
    g = np.random.default_rng(R + K + Cin)
    for i, pattern in enumerate(KR.WGRAD_PATTERNS):
        for gather_g in (0, 1):
            n_src = (R + 5, max(1, R // 2))[(i + gather_g) % 2]
            T, claim = KR.build_table(pattern, R, K, n_src, KSTEP, seed=R + i)
            A, G = _ints(g, R if gather_g else n_src, Cin), _ints(g, n_src if gather_g else R, Cout)
            want = _exact(KR.wgrad_ref(A, G, T, gather_g))
            Ad, Gd, Td = _d(A), _d(G), _d(T)
            what = f"wgrad[{wgrad_class(Cin, Cout)}, {splits} splits] {_id(shape)} {pattern} gather_g {gather_g}"
            got = sp._wgrad(R, K, Ad, Gd, Td, gather_g)
            _same(got, want, what)
            _same(_wgrad_poisoned(R, K, Ad, Gd, Td, gather_g), want, what + " (partial buffer poisoned)")
            for k in range(K):
                if not claim["cells"][:, k].any():
                    assert not got[k].any(), what + f": tap {k} has no source, dW[{k}] must be 0"


# ---- d. bias gradient and chain sums, exact -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=_id)
def test_colsum_exact(shape):
    from unipre3d_amd import sparseconv as sp
    R, C = shape
    G = _ints(np.random.default_rng(R + C), R, C)
    want = _exact(KR.colsum_ref(G))
    Gd = _d(G)
    what = f"colsum {R}x{C}, {colsum_splits(R, C)} splits"
    _same(sp._colsum(Gd), want, what)
    _same(_colsum_poisoned(Gd), want, what + " (partial buffer poisoned)")


@gpu
@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("C", [1, 37])
def test_dupsum_exact(C, order):
    """chains of 1, 2 and 300 rows among 700 (the long one crosses 256-thread blocks), visited in ascending or descending memory order;
    rows with first[r] != r are exactly 0"""
    from unipre3d_amd import sparseconv as sp
    N = 700
    first, nxt, chains = KR.build_chains(N, [1, 2, 300], order, seed=C)
    long = chains[2]
    assert len({r * C // 256 for r in long}) >= 2 and len(long) == 300
    X = _ints(np.random.default_rng(C), N, C)
    got = sp._dupsum(_d(X), _d(first), _d(nxt))
    _same(got, _exact(KR.dupsum_ref(X, first, nxt)), f"dupsum C {C} {order}")
    tails = [r for c in chains for r in c[1:]]
    assert len(tails) == 300 and not got[tails].any()
    _same(got[long[0]], X[long].sum(0), "the chain of 300")


# ---- e. Gaussian values at one shape per kernel class, the project's bars -----------------------------------------------------------------------
def _within(got, ref, bound, tol, what):
    """|got - fp64| <= tol * sum |products| per element (tests/test_gpu_sparseconv.py's _within); prints the worst error / sum |products|"""
    err = (got.double().cpu() - ref).abs()
    worst = float((err / (bound + 1e-30)).max())
    print(f"[sparseconv-tolerance] {what}: worst error / sum|products| {worst:.3e}, bar {tol:.1e}, ratio to bar {worst / tol:.3f}")
    bad = err > tol * bound + 1e-30
    assert not bad.any(), f"{what}: {int(bad.sum())} elements out of bound, worst err/bound {worst:.2e} against {tol:.1e}"


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


@gpu
@pytest.mark.parametrize("case", VALUE_GEMM, ids=_id)
def test_gemm_gaussian_within_tol_x(case):
    mode, R, K, Cin, Cout = case
    A, W, bias = _randn(1, R + 9, Cin), _randn(2, K, Cin, Cout), _randn(3, Cout)
    if mode == "table":
        tab, lr = KR.build_table("dense", R, K, R + 9, TILE, seed=1)[0], None
    else:
        lr, tab, _ = KR.build_list("tap_major", R, K, R + 9, seed=1)
    got = _gemm(R, K, A, W, bias, tab, list_row=lr, out_rows=R)
    ref = KR.gemm_ref(A, W, bias, tab, list_row=lr, out_rows=R)
    bound = KR.gemm_ref(A.abs(), W.abs(), bias.abs(), tab, list_row=lr, out_rows=R)
    _within(got, ref, bound, TOL_X, f"gemm[{gemm_class(Cin, Cout)}] {mode} {R}x{K}x{Cin}x{Cout}")


@gpu
@pytest.mark.parametrize("shape", VALUE_WGRAD, ids=_id)
def test_wgrad_gaussian_within_tol_w(shape):
    from unipre3d_amd import sparseconv as sp
    R, K, Cin, Cout = shape
    T, _ = KR.build_table("dense", R, K, R + 5, KSTEP, seed=2)
    A, G = _randn(4, R + 5, Cin), _randn(5, R, Cout)
    got = sp._wgrad(R, K, _d(A), _d(G), _d(T), 0)
    _within(got, KR.wgrad_ref(A, G, T, 0), KR.wgrad_ref(A.abs(), G.abs(), T, 0), TOL_W,
            f"wgrad[{wgrad_class(Cin, Cout)}, {wgrad_splits(*shape)[0]} splits] {_id(shape)}")


@gpu
@pytest.mark.parametrize("shape", VALUE_COLSUM, ids=_id)
def test_colsum_gaussian_within_tol_w(shape):
    from unipre3d_amd import sparseconv as sp
    G = _randn(6, *shape)
    _within(sp._colsum(_d(G)), KR.colsum_ref(G), KR.colsum_ref(G.abs()), TOL_W, f"colsum[{colsum_splits(*shape)} splits] {_id(shape)}")


@gpu
def test_dupsum_gaussian_within_tol_x():
    from unipre3d_amd import sparseconv as sp
    first, nxt, _ = KR.build_chains(700, [1, 2, 300, 17, 64], "ascending", seed=2)
    X = _randn(7, 700, 37)
    _within(sp._dupsum(_d(X), _d(first), _d(nxt)), KR.dupsum_ref(X, first, nxt), KR.dupsum_ref(X.abs(), first, nxt), TOL_X, "dupsum 700x37, chains up to 300")
