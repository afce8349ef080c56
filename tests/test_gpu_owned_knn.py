"""libunipre3d_knn.so writes every element it owns and nothing else: its entry point called directly, with every pointer inside a
poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors, bit for bit
(tests/test_gpu_knn.py holds the wrapper to the fp64 restatement).

  entry point   cases
  u3d_knn       (b, n, m, k) = (2, 65, 17, 12): two workgroups per cloud, the second with one query, k < 64 (`lane < k` stores);
                (1, 2049, 5, 64): two LDS tiles, the second with one point, k = a full wave; each with dist2 and with dist2 = NULL
"""
import numpy as np
import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu


def _cloud(b, n, seed):
    # quantized coordinates: many equal distances, so the order among ties is part of what is compared
    return torch.from_numpy(np.random.default_rng(seed).integers(-8, 9, size=(b, n, 3)).astype(np.float32) * 0.125)


@pytest.mark.parametrize("with_dist2", [True, False])
@pytest.mark.parametrize("b, n, m, k", [(2, 65, 17, 12), (1, 2049, 5, 64)])
def test_knn_writes_what_it_owns(b, n, m, k, with_dist2):
    from unipre3d_amd import _lib, knn
    support, query = _cloud(b, n, 1), _cloud(b, m, 2)

    def case(arena):
        s, q = arena.inp(support, name="support"), arena.inp(query, name="query")
        d = arena.out((b, m, k), torch.float32, name="dist2") if with_dist2 else None
        idx = arena.out((b, m, k), torch.int32, name="idx")
        assert knn.load().u3d_knn(b, n, m, k, _lib.ptr(s), _lib.ptr(q), _lib.ptr(d), _lib.ptr(idx), _lib.stream_ptr(s.device)) == 0
        return [idx] + ([d] if with_dist2 else [])

    run, _ = run_twice(case, "cuda")
    want_d, want_i = knn.knn_query(k, support.cuda(), query.cuda())
    assert same_bits(run[0], want_i)
    if with_dist2:
        assert same_bits(run[1], want_d)
