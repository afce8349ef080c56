"""kNN without a GPU: the header against the module's binding table, the launch-path query, the CPU restatement (tests/knn_ref.py)
against the indices recorded from the reference's own functions (tests/golden/g16_knn.npz, made by tests/golden/make_g16_knn.py), and
the restatement's tie rule."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import knn_ref as KR
from conftest import ROOT

RECORDED_SORTED = ("layers_knn_point", "layers_knn_KNN", "group_KNN", "pcm_knn_point")
RECORDED_SET = ("pointmlp_knn_point",)
_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)


def _declared_functions():
    """{name: (return type, [parameter type, ...])} of every u3d_* function include/unipre3d_knn.h declares (comments and
    preprocessor lines stripped; a pointer parameter's type ends in '*')."""
    hdr = open(os.path.join(ROOT, "include", "unipre3d_knn.h")).read()
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
    knn = importlib.import_module("unipre3d_amd.knn")
    declared = _declared_functions()
    assert set(declared) == set(knn.EXPORTS) == {"u3d_knn", "u3d_knn_path"} and len(set(knn.EXPORTS)) == len(knn.EXPORTS)
    assert declared["u3d_knn"][1] == ["int"] * 4 + ["constfloat*", "constfloat*", "float*", "int32_t*", "void*"]
    assert declared["u3d_knn_path"][1] == ["int", "int"]
    handle = knn.load()
    for name, (ret, params) in declared.items():
        fn = getattr(handle, name)
        assert ret == "int" and fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == len(params), name
        for c_type, bound in zip(params, fn.argtypes):
            assert bound is (ctypes.c_void_p if c_type.endswith("*") else ctypes.c_int), (name, c_type, bound)
    hdr = open(os.path.join(ROOT, "include", "unipre3d_knn.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (U3D_KNN_\w+) (\d+)", hdr, re.M)}
    assert consts == {"U3D_KNN_MAX_K": knn.MAX_K, "U3D_KNN_TILE": knn.TILE, "U3D_KNN_QUERIES": knn.QUERIES}


def test_launch_path_boundaries():
    """u3d_knn_path is host arithmetic: 0 where u3d_knn refuses (n, k), else the LDS tiles walked -- one assertion on each side of
    every boundary the launch code has.  u3d_knn's own argument checks return before anything touches a device."""
    from unipre3d_amd import knn
    lib, T, K = knn.load(), knn.TILE, knn.MAX_K
    path = lib.u3d_knn_path
    assert (path(1, 1), path(0, 1), path(-1, 1)) == (1, 0, 0)                   # n >= 1
    assert (path(100, 1), path(100, 0), path(100, -3)) == (1, 0, 0)             # k >= 1
    assert (path(40, 40), path(40, 41)) == (1, 0)                               # k <= n
    assert (path(4096, K), path(4096, K + 1)) == (2, 0)                         # k <= U3D_KNN_MAX_K
    assert (path(T - 1, 12), path(T, 12), path(T + 1, 12)) == (1, 1, 2)         # one tile | two
    assert (path(2 * T, 12), path(2 * T + 1, 12), path(8192, 32), path(8193, 32)) == (2, 3, 4, 5)
    assert path(2**31 - 1, 64) == (2**31 - 1 + T - 1) // T                      # no 32-bit wrap in the tile count
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                                                  # never dereferenced: every call below returns first
    assert lib.u3d_knn(1, 8, 4, 0, one, one, null, one, null) == 1              # k < 1
    assert lib.u3d_knn(1, 8, 4, 9, one, one, null, one, null) == 1              # k > n
    assert lib.u3d_knn(1, 100, 4, K + 1, one, one, null, one, null) == 1        # k > U3D_KNN_MAX_K
    assert lib.u3d_knn(-1, 8, 4, 2, one, one, null, one, null) == 1             # negative sizes
    assert lib.u3d_knn(1, -8, 4, 2, one, one, null, one, null) == 1
    assert lib.u3d_knn(1, 8, -4, 2, one, one, null, one, null) == 1
    assert lib.u3d_knn(1, 8, 4, 2, null, one, null, one, null) == 1             # NULL mandatory pointers
    assert lib.u3d_knn(1, 8, 4, 2, one, one, null, null, null) == 1
    assert lib.u3d_knn(0, 8, 4, 2, null, null, null, null, null) == 0           # empty calls: no launch
    assert lib.u3d_knn(3, 8, 0, 2, null, null, null, null, null) == 0
    assert lib.u3d_knn(2**31 - 1, 8, 17, 2, one, one, null, one, null) == 1     # b * ceil(m / 16) beyond 2^31 - 1 workgroups


def _cases(golden):
    z = golden("g16_knn.npz")
    for i, (B, N, M, k) in enumerate(z["cases"].tolist()):
        support, qsel = z[f"c{i}_support"], z[f"c{i}_qsel"]
        assert support.shape == (B, N, 3) and support.dtype == np.float32 and qsel.shape == (B, M)
        query = np.take_along_axis(support, qsel.astype(np.int64)[:, :, None], 1)
        yield i, k, support, query, {n: z[f"c{i}_{n}"].astype(np.int32) for n in RECORDED_SORTED + RECORDED_SET}


def test_restatement_reproduces_the_recorded_reference_indices(golden):
    z = golden("g16_knn.npz")
    assert z["cases"].tolist() == [[2, 1024, 128, 32], [2, 128, 128, 8], [2, 300, 77, 12], [2, 512, 256, 12]]
    assert sorted(z.files) == sorted(["cases"] + [f"c{i}_{n}" for i in range(4) for n in ("support", "qsel") + RECORDED_SORTED + RECORDED_SET])
    for i, k, support, query, rec in _cases(golden):
        d2, idx = KR.knn(k, support, query)
        _, idx64 = KR.knn_f64(k, support, query)
        assert d2.dtype == np.float32 and idx.dtype == np.int32 and np.array_equal(idx, idx64), i
        for name in RECORDED_SORTED:
            assert np.array_equal(rec[name], idx), (i, name)                    # exact, every row, order included
        for name in RECORDED_SET:
            assert np.array_equal(np.sort(rec[name], -1), np.sort(idx, -1)), (i, name)    # topk(sorted=False): the set
        assert np.array_equal(d2, np.take_along_axis(KR.dist2(support, query), idx.astype(np.int64), -1))


def test_restatement_distance_is_the_direct_form_bit_for_bit():
    """d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded in fp32, is what `((src - dst) ** 2).sum(-1)` computes in torch."""
    import torch
    rng = np.random.default_rng(5)
    s, q = rng.uniform(-1, 1, (2, 97, 3)).astype(np.float32), rng.uniform(-1, 1, (2, 33, 3)).astype(np.float32)
    t = ((torch.from_numpy(q).unsqueeze(2) - torch.from_numpy(s).unsqueeze(1)) ** 2).sum(-1).numpy()
    assert np.array_equal(t.view(np.uint32), KR.dist2(s, q).view(np.uint32))


@pytest.mark.parametrize("cloud", ["lattice", "duplicated"])
def test_restatement_tie_rule(cloud):
    """Equal distances go to the lower index: within every row the (d2, index) keys increase strictly, and a self-query starts with the
    lowest index at distance 0."""
    p = KR.lattice() if cloud == "lattice" else KR.duplicated()
    n = p.shape[1]
    d2, idx = KR.knn(8, p, p)
    key = KR.keys(d2, idx)
    assert (np.diff(key.astype(object), axis=-1) > 0).all()
    full = KR.dist2(p, p)
    first = np.array([[np.flatnonzero(full[b, j] == 0)[0] for j in range(n)] for b in range(p.shape[0])])
    assert np.array_equal(idx[:, :, 0], first) and (d2[:, :, 0] == 0).all()
    if cloud == "lattice":
        assert np.array_equal(idx[0, :, 0], np.arange(64))
        assert idx[0, 0].tolist() == [0, 1, 4, 16, 5, 17, 20, 21] and d2[0, 0].tolist() == [0, 1, 1, 1, 2, 2, 2, 3]
    else:
        half = n // 2
        assert np.array_equal(idx[0, :, 0], np.arange(n) % half) and np.array_equal(idx[0, :, 1], np.arange(n) % half + half)
        assert (d2[:, :, 1] == 0).all() and (d2[:, :, 2] > 0).all()
    with pytest.raises(ValueError):
        KR.knn(n + 1, p, p)
