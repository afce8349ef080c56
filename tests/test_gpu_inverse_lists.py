"""The inverse-list builder of csrc/u3d_group.h at its edges, through the two entry points that are made of it: u3d_local_grouper_lists (two
tables, no overflow list, L = N) and u3d_feature_propagation_lists (one table, overflow list, L = S), called directly on hand-built index
tables and held bit for bit to tests/local_grouper_ref.inverse_lists and tests/feature_propagation_ref.inverse_lists.

  The scan gives thread t of 1024 the words [t per, (t + 1) per) of ptr[0 .. L], per = ceil((L + 1) / 1024):
  L + 1 = 1024    one word per thread, none idle
  L + 1 = 1025    two words per thread: threads 0 .. 511 have two, thread 512 one, the others an empty slice
  L = 1           one thread has both words
  one list takes every entry, more than 64 of them and not a multiple of 64: the rank sort's wave runs a partial last pass, every other list
                  is empty
  feature propagation: every entry out of range (only the overflow list, which is not counted, is populated) and none (it is empty)
  LocalGrouper:   no fps with S == N; anchors that repeat, and anchors out of range (they count as point s)
  B = 2 throughout with tables that differ between the two, so a wrong batch offset shows.
  Every case: ent is a permutation of 0 .. n-1 per batch element, and a second call on fresh buffers gives the same bits (the order in
  which the atomic cursors drop entries is arbitrary and must not leak past the rank sort)."""
import numpy as np
import pytest
import torch

import feature_propagation_ref as FR
import local_grouper_ref as GR

pytestmark = pytest.mark.gpu

B = 2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _spread(shape, mod, mul, step):
    """Entry e of batch element b names (e mul + b step) % mod, every third one of the last four lists instead: short lists all over
    the range, longer ones where the scan ends, the two batch elements different."""
    n = int(np.prod(shape[1:]))
    e = np.arange(n, dtype=np.int64)[None, :] * mul + np.arange(shape[0], dtype=np.int64)[:, None] * step
    e[:, ::3] = mod - 1 - e[:, ::3] % min(4, mod)
    return (e % mod).astype(np.int32).reshape(shape)


def _lg_spread(N, S, K, fps=True):
    idx = _spread((B, S, K), N, 7, 13)
    idx[0, 0, 0], idx[0, S // 2, K - 1], idx[1, S - 1, 0], idx[1, 0, 1] = -1, N, I32_MIN, I32_MAX      # these name the row's anchor
    return (_spread((B, S), N, 29, 5) if fps else None), idx


def _one_list(shape, lists):
    """Batch element b's entries all name lists[b]."""
    return np.broadcast_to(np.asarray(lists, np.int32).reshape((B,) + (1,) * (len(shape) - 1)), shape).copy()


def _lg_repeated_anchors(N, S, K):
    fps = (np.arange(S, dtype=np.int32)[None, :] // 3 + np.arange(B, dtype=np.int32)[:, None]).astype(np.int32)      # each anchor three times
    fps[0, 4], fps[1, S - 1] = -5, N                                                                               # ... and two that count as s
    idx = _spread((B, S, K), N, 3, 1)
    idx[:, ::2, 0] = -1                                                                                            # every other row names its anchor
    return fps, idx


# (N, S, K, fps, idx)
LG_CASES = {
    "L+1=1024": (1023, 37, 3) + _lg_spread(1023, 37, 3),
    "L+1=1025": (1024, 37, 3) + _lg_spread(1024, 37, 3),
    "L=1": (1, 1, 2, np.zeros((B, 1), np.int32), np.array([[[0, -1]], [[7, 0]]], np.int32)),
    "one_list": (100, 100, 2, _one_list((B, 100), (7, 93)), _one_list((B, 100, 2), (7, 93))),      # 200 = 3 x 64 + 8 entries, 100 = 64 + 36 anchors
    "no_fps": (70, 70, 2) + _lg_spread(70, 70, 2, fps=False),
    "repeated_anchors": (40, 30, 2) + _lg_repeated_anchors(40, 30, 2),
}


def _fp_spread(N, S, bad):
    idx = _spread((B, N, 3), S, 11, 3)
    if bad:
        idx[0, 0, 0], idx[0, N // 2, 2], idx[1, N - 1, 1], idx[1, 1, 0] = -1, S, I32_MIN, I32_MAX
    return idx


def _fp_all_out(N, S):
    return np.tile(np.array([-1, S, S + 7, I32_MIN, I32_MAX, -S - 1], np.int32), B * N * 3 // 6).reshape(B, N, 3)


# (N, S, idx)
FP_CASES = {
    "L+1=1024": (50, 1023, _fp_spread(50, 1023, True)),
    "L+1=1025": (50, 1024, _fp_spread(50, 1024, True)),
    "L=1": (40, 1, _fp_spread(40, 1, True)),                              # list 0 has 118 entries in each batch element
    "one_list": (50, 5, _one_list((B, 50, 3), (3, 0))),                   # 150 = 2 x 64 + 22 entries
    "all_out_of_range": (50, 5, _fp_all_out(50, 5)),
    "none_out_of_range": (33, 7, _fp_spread(33, 7, False)),
}


def _held(name, got, want, n):
    ptr, ent = got
    assert torch.equal(torch.sort(ent.cpu(), dim=1)[0], torch.arange(n, dtype=torch.int32).expand(B, -1)), f"{name}: ent is no permutation"
    assert np.array_equal(ptr.cpu().numpy(), want[0]), f"{name}: ptr"
    assert np.array_equal(ent.cpu().numpy(), want[1]), f"{name}: ent"


@pytest.mark.parametrize("case", LG_CASES, ids=str)
def test_local_grouper_lists_at_the_builders_edges(case):
    from unipre3d_amd import _lib, local_grouper as lg
    lib = lg.load()
    N, S, K, fps_np, idx_np = LG_CASES[case]
    want = GR.inverse_lists(fps_np, idx_np, N)
    fps, idx = (None if fps_np is None else torch.from_numpy(fps_np).cuda()), torch.from_numpy(idx_np).cuda()
    nbytes = lib.u3d_local_grouper_scratch_bytes(B, N, S, K, 4, 0, 0, 2)
    assert nbytes == 4 * B * (N + S * K + S)
    st = _lib.stream_ptr(idx.device)

    def call():
        ptr, fptr = (torch.full((B, N + 1), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        ent, fent = torch.full((B, S * K), -1, dtype=torch.int32, device="cuda"), torch.full((B, S), -1, dtype=torch.int32, device="cuda")
        scratch = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        assert lib.u3d_local_grouper_lists(_lib.ptr(fps), _lib.ptr(idx), _lib.ptr(ptr), _lib.ptr(ent), _lib.ptr(fptr), _lib.ptr(fent),
                                           _lib.ptr(scratch), B, N, S, K, st) == 0
        torch.cuda.synchronize()
        return ptr, ent, fptr, fent

    for got in (call(), call()):
        _held("idx", got[:2], want[:2], S * K)
        _held("fps", got[2:], want[2:], S)


@pytest.mark.parametrize("case", FP_CASES, ids=str)
def test_feature_propagation_lists_at_the_builders_edges(case):
    from unipre3d_amd import _lib, feature_propagation as fp
    lib = fp.load()
    N, S, idx_np = FP_CASES[case]
    want = FR.inverse_lists(idx_np, S)
    if case.endswith("out_of_range"):                                    # the table is what its name says
        assert int(((idx_np < 0) | (idx_np >= S)).sum()) == (idx_np.size if case.startswith("all") else 0)
    idx = torch.from_numpy(idx_np).cuda()
    nbytes = lib.u3d_feature_propagation_scratch_bytes(B, N, S)
    assert nbytes == 4 * B * (S + 1 + 3 * N)
    st = _lib.stream_ptr(idx.device)

    def call():
        ptr, ent = torch.full((B, S + 1), -1, dtype=torch.int32, device="cuda"), torch.full((B, 3 * N), -1, dtype=torch.int32, device="cuda")
        scratch = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
        assert lib.u3d_feature_propagation_lists(_lib.ptr(idx), _lib.ptr(ptr), _lib.ptr(ent), _lib.ptr(scratch), B, N, S, st) == 0
        torch.cuda.synchronize()
        return ptr, ent

    for got in (call(), call()):
        _held("idx", got, want, 3 * N)
