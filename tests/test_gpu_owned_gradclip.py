"""libunipre3d_gradclip.so writes every element it owns and nothing else: its three entry points called directly, with every pointer --
the gradient tensors, the pointer table, `numel`, `first_chunk`, `partials` and `state` -- inside a poisoned arena (tests/guarded.py),
under two poisons.

Layout: eight tensors of 1, 3, 4, 5, 65535, 65536, 65537 and 0 elements, each a placement of its own at 0, 4, 8 and 12 bytes past a
256-byte boundary in turn (the kernels read and write 16-byte vectors on the aligned middle of a chunk and single floats on its head
and tail); eight chunks of U3D_GC_CHUNK elements, the 65537-element tensor holding two, the empty tensor none.  `partials` is exactly
n_chunks * U3D_GC_PARTIAL_BYTES bytes and `state` exactly U3D_GC_STATE_BYTES; both are owned outputs, every byte of them.

  entry point             cases
  u3d_gradclip_stats      the layout above in three runs.  "clip": norm above max_norm.  "keep": the same values times 2^-14, norm below
  u3d_gradclip_finalize   max_norm.  "inf": +inf in the last element of the 65537-element tensor (the one element of the second chunk).
  u3d_gradclip_scale      clip: the tensors are owned outputs and every element is fl32(g * coef), coef read back from `state`;
                          keep and inf: the tensors are inputs, which the arena holds to the bytes copied in.

Expected values.  amax and found_inf are exact; `reserved` is 0; coef lies within one fp32 ulp of min(1, max_norm / (norm + 1e-6))
evaluated in fp64, and grad_scale within one ulp of that quotient's reciprocal.  total_norm against math.fsum over the fp64 squares: an
fp32 square is exact in fp64 and every term is non-negative, so a sum of n terms in any order lies within n * 2^-52 relative of the exact
sum, and the norm within half that: |total_norm - ref| <= ref * n * 2^-53, n = 196 611 elements.  (Derived, not measured.)
"""
import math
import re
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu

NUMEL = (1, 3, 4, 5, 65535, 65536, 65537, 0)
MISALIGN = (0, 4, 8, 12)
MAX_NORM = 1.0


def _macros():
    text = (Path(__file__).resolve().parent.parent / "include" / "unipre3d_gradclip.h").read_text()
    return {k: int(v) for k, v in re.findall(r"#define\s+U3D_GC_(\w+)\s+(\d+)", text)}


def _values(kind):
    rng = np.random.default_rng(20)
    g = [rng.standard_normal(n).astype(np.float32) for n in NUMEL]
    if kind == "keep":
        g = [a * np.float32(2.0 ** -14) for a in g]
    if kind == "inf":
        g[6][-1] = np.inf
    return g


@pytest.mark.parametrize("kind", ["clip", "keep", "inf"])
def test_gradclip_writes_what_it_owns(kind):
    from unipre3d_amd import _lib, gradcheck
    lib = gradcheck.load()
    M = _macros()
    chunk, pbytes, sbytes = M["CHUNK"], M["PARTIAL_BYTES"], M["STATE_BYTES"]
    assert chunk == gradcheck.GC_CHUNK and sbytes == 32 and pbytes == 16
    grads = _values(kind)
    first = np.concatenate([[0], np.cumsum([-(-n // chunk) for n in NUMEL])]).astype(np.int32)
    n_t, n_chunks = len(NUMEL), int(first[-1])
    assert n_chunks == 8 and list(first) == [0, 1, 2, 3, 4, 5, 6, 8, 8]
    writes = kind == "clip"

    def case(arena):
        ts = []
        for i, g in enumerate(grads):
            mis = MISALIGN[i % 4]
            if writes:
                t = arena.out(g.shape, torch.float32, misalign=mis, name=f"grad{i}")
                t.copy_(torch.from_numpy(g))
            else:
                t = arena.inp(torch.from_numpy(g), misalign=mis, name=f"grad{i}")
            assert arena.address(t) % 16 == mis and arena.address(t) % 256 == mis
            ts.append(t)
        ptrs = arena.inp(torch.tensor([arena.address(t) for t in ts], dtype=torch.int64), name="grad_ptrs")
        numel = arena.inp(torch.tensor(NUMEL, dtype=torch.int64), name="numel")
        fc = arena.inp(torch.from_numpy(first), name="first_chunk")
        partials = arena.out((n_chunks * pbytes,), torch.uint8, name="partials")
        state = arena.out((sbytes,), torch.uint8, name="state")
        st = _lib.stream_ptr(state.device)
        assert lib.u3d_gradclip_stats(ptrs.data_ptr(), numel.data_ptr(), fc.data_ptr(), n_t, n_chunks, partials.data_ptr(), st) == 0
        assert lib.u3d_gradclip_finalize(partials.data_ptr(), n_chunks, MAX_NORM, state.data_ptr(), st) == 0
        assert lib.u3d_gradclip_scale(ptrs.data_ptr(), numel.data_ptr(), fc.data_ptr(), n_t, n_chunks, state.data_ptr(), st) == 0
        return [partials, state] + (ts if writes else [])

    run, _ = run_twice(case, "cuda")
    total, amax, coef, gscale, found, reserved = struct.unpack("ddffff", run[1].numpy().tobytes())
    flat = np.concatenate(grads)
    finite = flat[np.isfinite(flat)]
    n = flat.size
    ref_norm = math.sqrt(math.fsum((finite.astype(np.float64) ** 2).tolist()))
    print(f"{kind}: total_norm {total!r} (reference {ref_norm!r}), amax {amax!r}, coef {coef!r}, grad_scale {gscale!r}, found_inf {found!r}")
    assert amax == float(np.abs(finite).max()) and reserved == 0.0 and struct.unpack("I", run[1].numpy().tobytes()[28:])[0] == 0
    # the partial records: the chunk's largest finite |g| and its non-finite flag are exact
    rec = [struct.unpack("dfI", run[0].numpy().tobytes()[16 * c:16 * c + 16]) for c in range(n_chunks)]
    pieces = [g[k * chunk:(k + 1) * chunk] for g in grads for k in range(-(-len(g) // chunk))]
    assert len(pieces) == n_chunks
    for (sumsq, m, bad), piece in zip(rec, pieces):
        fin = piece[np.isfinite(piece)]
        assert m == (float(np.abs(fin).max()) if fin.size else 0.0) and bad == int(fin.size != piece.size)
        if fin.size == piece.size:
            want = math.fsum((piece.astype(np.float64) ** 2).tolist())
            assert abs(sumsq - want) <= want * piece.size * 2.0 ** -52
    if kind == "inf":
        assert found == 1.0 and coef == 1.0 and gscale == 1.0
        return
    assert found == 0.0
    assert abs(total - ref_norm) <= ref_norm * n * 2.0 ** -53, (total, ref_norm)
    ref_coef = np.float32(min(1.0, MAX_NORM / (ref_norm + 1e-6)))
    assert abs(np.float32(coef) - ref_coef) <= np.spacing(ref_coef), (coef, ref_coef)
    ref_scale = np.float32(1.0 / min(1.0, MAX_NORM / (ref_norm + 1e-6)))
    assert abs(np.float32(gscale) - ref_scale) <= np.spacing(ref_scale), (gscale, ref_scale)
    if kind == "keep":
        assert ref_norm < MAX_NORM and coef == 1.0
        return
    assert ref_norm > MAX_NORM and coef < 1.0
    for i, g in enumerate(grads):
        assert same_bits(run[2 + i], torch.from_numpy(g * np.float32(coef))), f"grad{i}"
