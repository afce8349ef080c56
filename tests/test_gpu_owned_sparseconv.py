"""libunipre3d_sparseconv.so writes every element it owns and nothing else: its seven launching entry points called directly, with every
pointer inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrappers (sparseconv.subm_map,
down_map, _gemm, _dupsum, _wgrad, _colsum) on ordinary tensors, bit for bit -- the library is documented as free of float atomics, its
reductions run in a fixed order (tests/test_gpu_sparseconv*.py hold the wrappers to their references).

Scratch and `partial` buffers are guarded placements of exactly the size the library's query returns, at a 256-byte boundary, and stay
out of the bit comparison.  The sort tile (TILE = NT * ITEMS) is read from unipre3d_amd/csrc/u3d_sparseconv.hip and checked against
u3d_spconv_scratch_bytes, whose histogram grows by one 1 KiB line of digit counts exactly where a second tile begins; the channel and
split classes come from the header's U3D_SPCONV_* macros and the two partial_floats queries.

  entry point            cases (class query asserted)
  u3d_spconv_subm_map    k = 3, n_batch = 2, shape (7, 6, 9), N = 1, 300, TILE + 1 (two sort tiles: scratch_bytes); from N = 300 on sites
                         repeat, so first / next chains exist (asserted).  Outputs table (N, 27), first, next = sparseconv.subm_map.
  u3d_spconv_down_map    s = 2, the same N and shape: D0 = 7 and D2 = 9 are odd, the planes d0 = 6 and d2 = 8 are dropped.  meta: the 4 words the wrapper allocates,
  u3d_spconv_down_emit   all owned.  M is read from meta[0] after the first call; out_indices and table are placed with N rows, of which
                         M are owned.  list_src holds -1 for the dropped rows (asserted from N = 300 on).  = sparseconv.down_map.
  u3d_spconv_gemm        R = 65 (one row past a block tile), K = 27; (Cin, Cout) = (3, 16) and (16, 3): the VALU kernel by either channel
                         count; (33, 65): MFMA, one channel past a K stage, one column past a tile.  Table mode with and without bias,
                         table mode with mask, list mode (list_row given).  = sparseconv._gemm.
  u3d_spconv_dupsum      N = 300, C = 5, chains of length 1, 2 and 7.
  u3d_spconv_wgrad       both gather_g, the three kernel classes (Cin small: (3, 16); Cout small: (16, 3); MFMA: (33, 65)), each at: R = 65,
                         K = 27 (one split); the smallest R with trailing splits that own no row (K = 1 for the VALU classes, where the
                         split count must reach its cap of 256 first; K = 27 for MFMA); the smallest R for which
                         u3d_spconv_wgrad_partial_floats / (K * Cin * Cout) reaches U3D_SPCONV_WAVE_SUM_SPLITS, at K = 1.  `partial` is a
                         guarded placement of exactly the queried size.
  u3d_spconv_colsum      C = 5, the first R at which u3d_spconv_colsum_partial_floats / C reaches U3D_SPCONV_WAVE_SUM_SPLITS and the R before.
"""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import spconv_kernel_ref as KR
from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

MACROS = KR.header_macros()
SMALL_C, BLOCK, KSTEP, WAVE_SUM = MACROS["SMALL_C"], MACROS["TILE"], MACROS["KSTEP"], MACROS["WAVE_SUM_SPLITS"]
_SRC = (Path(__file__).resolve().parent.parent / "unipre3d_amd" / "csrc" / "u3d_sparseconv.hip").read_text()
SORT_TILE = int(re.search(r"constexpr int NT = (\d+);", _SRC).group(1)) * int(re.search(r"constexpr int ITEMS = (\d+);", _SRC).group(1))
assert re.search(r"constexpr int TILE = NT \* ITEMS;", _SRC)
B, D = 2, (7, 6, 9)
MAP_N = (1, 300, SORT_TILE + 1)
CHANNELS = {"cin_small": (3, 16), "cout_small": (16, 3), "mfma": (33, 65)}


def _sp():
    from unipre3d_amd import sparseconv
    return sparseconv


def _p(t):
    from unipre3d_amd import _lib
    return _lib.ptr(t)


def _stream():
    from unipre3d_amd import _lib
    return _lib.stream_ptr(torch.device("cuda:0"))


def _scratch_bytes(lib, N):
    """the queried size, after asserting that it counts the sort tiles the way SORT_TILE says: carve() takes two 8-byte and four 4-byte
    arrays of n rows, each rounded up to 256 bytes, and then (tiles + 1) lines of 256 digit counts"""
    a256 = lambda v: -(-v // 256) * 256
    tiles = lambda n: (int(lib.u3d_spconv_scratch_bytes(n)) - 2 * a256(8 * n) - 4 * a256(4 * n)) // 1024 - 1
    assert (tiles(1), tiles(SORT_TILE), tiles(SORT_TILE + 1)) == (1, 1, 2), "SORT_TILE is not where the second sort tile begins"
    assert tiles(N) == -(-N // SORT_TILE)
    return int(lib.u3d_spconv_scratch_bytes(N))


def _sites(N):
    """(N, 4) int32 rows drawn with repetition from the 2 x 7 x 6 x 9 grid (N = 1: one site that the strided map keeps)"""
    if N == 1:
        return torch.tensor([[1, 3, 2, 5]], dtype=torch.int32)
    g = np.random.default_rng(N)
    cells = g.integers(0, B * D[0] * D[1] * D[2], size=N)
    cells[:4] = [0, B * D[0] * D[1] * D[2] - 1, 5, 5]
    idx = np.stack([cells // (D[0] * D[1] * D[2]), cells // (D[1] * D[2]) % D[0], cells // D[2] % D[1], cells % D[2]], 1)
    return torch.from_numpy(idx.astype(np.int32))


# ---- maps --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", MAP_N)
def test_subm_map_writes_what_it_owns(N):
    sp = _sp()
    lib, k = sp.load(), 3
    K = k ** 3
    sites = _sites(N)
    nbytes = _scratch_bytes(lib, N)

    def case(arena):
        idx = arena.inp(sites, name="indices")
        table = arena.out((N, K), torch.int32, name="table")
        first, nxt = arena.out((N,), torch.int32, name="first"), arena.out((N,), torch.int32, name="next")
        scratch = arena.scratch(nbytes)
        assert idx.data_ptr() % 16 == 0
        assert lib.u3d_spconv_subm_map(N, _p(idx), B, *D, k, _p(table), _p(first), _p(nxt), _p(scratch), _stream()) == 0
        return [table, first, nxt]

    run, _ = run_twice(case, "cuda")
    m = sp.subm_map(sites.cuda(), D, B, k)
    assert same_bits(run[0], m.table) and same_bits(run[1], m.first) and same_bits(run[2], m.next)
    if N > 1:
        assert int((run[2] >= 0).sum()) > 0 and int((run[1] != torch.arange(N)).sum()) > 0, "no chains"


@pytest.mark.parametrize("N", MAP_N)
def test_down_map_and_emit_write_what_they_own(N):
    sp = _sp()
    lib, s = sp.load(), 2
    K = s ** 3
    sites = _sites(N)
    nbytes = _scratch_bytes(lib, N)
    assert D[0] % s == 1 and (N == 1 or int((sites[:, 1] == D[0] - 1).sum()) > 0)
    m = sp.down_map(sites.cuda(), D, B, s)
    M_want = m.out_indices.shape[0]
    meta_words = 4                                  # what sparseconv.down_map allocates: torch.empty(4, dtype=torch.int32)

    def case(arena):
        idx = arena.inp(sites, name="indices")
        meta = arena.out((meta_words,), torch.int32, name="meta")
        scratch = arena.scratch(nbytes)
        assert lib.u3d_spconv_down_map(N, _p(idx), B, *D, s, _p(meta), _p(scratch), _stream()) == 0
        torch.cuda.synchronize()
        M = int(meta[0].item())
        assert 0 < M <= N
        out_indices = arena.out((N, 4), torch.int32, name="out_indices")
        table = arena.out((N, K), torch.int32, name="table")
        rest = [arena.out((N,), torch.int32, name=nm) for nm in ("first", "next", "list_row", "list_src")]
        owned = [arena.own(out_indices, M), arena.own(table, M)]
        assert lib.u3d_spconv_down_emit(N, M, _p(idx), B, *D, s, _p(out_indices), _p(table), *(_p(t) for t in rest), _p(scratch), _stream()) == 0
        return [meta] + owned + rest

    run, _ = run_twice(case, "cuda")
    meta, out_indices, table, first, nxt, list_row, list_src = run
    assert meta[0] == M_want and out_indices.shape[0] == M_want
    for got, want, nm in ((out_indices, m.out_indices, "out_indices"), (table, m.table, "table"), (first, m.first, "first"), (nxt, m.next, "next"),
                          (list_row, m.list_row, "list_row"), (list_src, m.list_src, "list_src")):
        assert same_bits(got, want), nm
    dropped = int((sites[:, 1:] >= torch.tensor([(d - s) // s + 1 for d in D]) * s).any(1).sum())   # the planes d0 = 6 and d2 = 8
    assert int((list_src == -1).sum()) == dropped and (N == 1 or dropped > 0)


# ---- gemm ----------------------------------------------------------------------------------------------------------------------------------------
def _floats(g, *shape):
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32))


def _table(g, R, K, n_src):
    t = g.integers(0, n_src, size=(R, K)).astype(np.int32)
    t[g.random((R, K)) < 0.25] = -1
    t[R - 1, K - 1] = n_src - 1
    return torch.from_numpy(t)


@pytest.mark.parametrize("mode", ["table_bias", "table", "table_mask", "list_bias", "list"])
@pytest.mark.parametrize("cls", list(CHANNELS))
def test_gemm_writes_what_it_owns(cls, mode):
    sp = _sp()
    lib, R, K = sp.load(), BLOCK + 1, 27
    Cin, Cout = CHANNELS[cls]
    assert (Cin <= SMALL_C or Cout <= SMALL_C) == (cls != "mfma") and (cls != "mfma" or (Cin == KSTEP + 1 and Cout == BLOCK + 1))
    g = np.random.default_rng(Cin * 100 + Cout)
    n_src = R + 7
    A, W = _floats(g, n_src, Cin), _floats(g, K, Cin, Cout)
    bias = _floats(g, Cout) if mode.endswith("bias") else None
    mask = list_row = None
    if mode.startswith("list"):
        lr, ls, _ = KR.build_list("tap_major", R, K, n_src, seed=Cin)
        list_row, table = torch.from_numpy(lr), torch.from_numpy(ls)
        assert int((table < 0).sum()) > 0
    else:
        table = _table(g, R, K, n_src)
    if mode == "table_mask":
        mask = torch.from_numpy(KR.build_mask(R, seed=Cin)[0])
        assert 0 < int((mask != torch.arange(R)).sum()) < R

    def case(arena):
        t = {nm: (None if v is None else arena.inp(v, name=nm)) for nm, v in (("table", table), ("list_row", list_row), ("A", A), ("W", W),
                                                                              ("bias", bias), ("mask", mask))}
        Y = arena.out((R, Cout), torch.float32, name="Y")
        assert lib.u3d_spconv_gemm(R, K, Cin, Cout, _p(t["table"]), _p(t["list_row"]), _p(t["A"]), _p(t["W"]), _p(t["bias"]), _p(t["mask"]),
                                   _p(Y), _stream()) == 0
        return [Y]

    run, _ = run_twice(case, "cuda")
    c = lambda v: None if v is None else v.cuda()
    assert same_bits(run[0], sp._gemm(R, K, c(A), c(W), c(bias), c(table), c(list_row), c(mask)))
    if mask is not None:
        assert not run[0][mask != torch.arange(R)].any()


# ---- dupsum ----------------------------------------------------------------------------------------------------------------------------------------
def test_dupsum_writes_what_it_owns():
    sp = _sp()
    lib, N, C = sp.load(), 300, 5
    first, nxt, chains = KR.build_chains(N, [1, 2, 7, 7, 2], seed=5)
    assert {len(c) for c in chains} == {1, 2, 7}
    first, nxt = torch.from_numpy(first), torch.from_numpy(nxt)
    X = _floats(np.random.default_rng(5), N, C)

    def case(arena):
        f, n, x = arena.inp(first, name="first"), arena.inp(nxt, name="next"), arena.inp(X, name="in")
        out = arena.out((N, C), torch.float32, name="out")
        assert lib.u3d_spconv_dupsum(N, C, _p(f), _p(n), _p(x), _p(out), _stream()) == 0
        return [out]

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], sp._dupsum(X.cuda(), first.cuda(), nxt.cuda()))
    assert not run[0][first != torch.arange(N)].any()


# ---- wgrad / colsum ------------------------------------------------------------------------------------------------------------------------------
def _wgrad_splits(R, K, Cin, Cout):
    """(splits launched, splits that own a row)"""
    splits = int(_sp().load().u3d_spconv_wgrad_partial_floats(R, K, Cin, Cout)) // (K * Cin * Cout)
    rps = -(-(-(-R // splits)) // KSTEP) * KSTEP
    return splits, -(-R // rps)


@functools.lru_cache(maxsize=None)
def _wgrad_rows(cls, kind):
    """(R, K) of the case `kind` for the kernel class, found by asking the library"""
    Cin, Cout = CHANNELS[cls]
    if kind == "one_split":
        R, K = BLOCK + 1, 27
        assert _wgrad_splits(R, K, Cin, Cout) == (1, 1)
        return R, K
    K = 27 if (kind, cls) == ("empty_splits", "mfma") else 1
    hit = (lambda s, own: own < s) if kind == "empty_splits" else (lambda s, own: s >= WAVE_SUM)
    for R in range(1, 1 << 18):
        if hit(*_wgrad_splits(R, K, Cin, Cout)):
            if kind == "wave_sum":
                assert _wgrad_splits(R, K, Cin, Cout)[0] == WAVE_SUM and _wgrad_splits(R - 1, K, Cin, Cout)[0] == WAVE_SUM - 1
            return R, K
    raise AssertionError(f"no R below 2^18 gives {kind} for {cls}")


@pytest.mark.parametrize("gather_g", [0, 1])
@pytest.mark.parametrize("kind", ["one_split", "empty_splits", "wave_sum"])
@pytest.mark.parametrize("cls", list(CHANNELS))
def test_wgrad_writes_what_it_owns(cls, kind, gather_g):
    sp = _sp()
    lib = sp.load()
    Cin, Cout = CHANNELS[cls]
    assert (cls == "cin_small") == (Cin <= SMALL_C) and (cls == "cout_small") == (Cin > SMALL_C and Cout <= SMALL_C)
    R, K = _wgrad_rows(cls, kind)
    splits, owning = _wgrad_splits(R, K, Cin, Cout)
    print(f"wgrad {cls} {kind}: R = {R}, K = {K}, {splits} splits of which {owning} own a row")
    nfloats = int(lib.u3d_spconv_wgrad_partial_floats(R, K, Cin, Cout))
    assert nfloats == splits * K * Cin * Cout
    g = np.random.default_rng(R + gather_g)
    A, G, table = _floats(g, R, Cin), _floats(g, R, Cout), _table(g, R, K, R)

    def case(arena):
        t, a, gg = arena.inp(table, name="table"), arena.inp(A, name="A"), arena.inp(G, name="G")
        partial = arena.scratch(nfloats * 4, name="partial")
        dW = arena.out((K, Cin, Cout), torch.float32, name="dW")
        assert lib.u3d_spconv_wgrad(R, K, Cin, Cout, _p(t), gather_g, _p(a), _p(gg), _p(partial), _p(dW), _stream()) == 0
        return [dW]

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], sp._wgrad(R, K, A.cuda(), G.cuda(), table.cuda(), gather_g))


@pytest.mark.parametrize("side", ["below", "at"])
def test_colsum_writes_what_it_owns(side):
    sp = _sp()
    lib, C = sp.load(), 5
    splits = lambda R: int(lib.u3d_spconv_colsum_partial_floats(R, C)) // C
    R = next(r for r in range(1, 1 << 18) if splits(r) >= WAVE_SUM)
    assert splits(R) == WAVE_SUM and splits(R - 1) == WAVE_SUM - 1
    R -= side == "below"
    nfloats = int(lib.u3d_spconv_colsum_partial_floats(R, C))
    G = _floats(np.random.default_rng(R), R, C)

    def case(arena):
        g = arena.inp(G, name="G")
        partial = arena.scratch(nfloats * 4, name="partial")
        db = arena.out((C,), torch.float32, name="db")
        assert lib.u3d_spconv_colsum(R, C, _p(g), _p(partial), _p(db), _stream()) == 0
        return [db]

    run, _ = run_twice(case, "cuda")
    assert same_bits(run[0], sp._colsum(G.cuda()))
