"""unipre3d_amd.scatter.segment_csr on the MI355X against tests/attention_ref.segment_csr_ref: max / min and their argument rows bit-exact,
sum / mean within the fp32 sequential-sum bound 2^-23 * sum|terms| * segment length per element; gradients likewise."""
import numpy as np
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REDUCES = ("sum", "mean", "max", "min")


def _sc():
    from unipre3d_amd import scatter
    return scatter


def _indptr(kind, N, g):
    if kind == "ragged":      # segments of 0..8 rows, starting after row 0 and ending before N
        cuts = [2]
        while cuts[-1] < N - 3:
            cuts.append(min(cuts[-1] + int(g.integers(0, 9)), N - 3))
        return np.asarray(cuts, np.int64)
    if kind == "one":
        return np.asarray([0, N], np.int64)
    if kind == "none":
        return np.asarray([0], np.int64)
    return np.asarray([0, 0, N, N], np.int64)   # empty, all rows, empty


@pytest.mark.parametrize("C", [1, 3, 64, 512])
@pytest.mark.parametrize("kind", ["ragged", "one", "none", "edges"])
def test_against_loops(kind, C):
    g = np.random.default_rng(C * 7 + len(kind))
    N = 300 if C < 512 else 90
    src = g.normal(size=(N, C)).astype(np.float32)
    src[g.integers(0, N, 40), g.integers(0, C, 40)] = 1.5   # ties
    indptr = _indptr(kind, N, g)
    M = len(indptr) - 1
    dout = g.normal(size=(M, C)).astype(np.float32)
    seglen = np.diff(indptr).astype(np.float64)[:, None]
    for reduce in REDUCES:
        x = torch.as_tensor(src).to(DEV).requires_grad_(True)
        out = _sc().segment_csr(x, torch.as_tensor(indptr).to(DEV), reduce=reduce)
        assert out.shape == (M, C) and out.dtype == torch.float32
        out.backward(torch.as_tensor(dout).to(DEV))
        ref, arg = R.segment_csr_ref(src, indptr, reduce)
        dref = R.segment_csr_grad_ref(dout, indptr, arg, N, reduce)
        got, dgot = out.detach().cpu().numpy(), x.grad.cpu().numpy()
        if reduce in ("max", "min"):
            assert np.array_equal(got, ref), f"{reduce} {kind} C={C}"
            assert np.array_equal(dgot, dref), f"{reduce} {kind} C={C}: gradient rows (ties go to the lowest row)"
        else:
            sabs, _ = R.segment_csr_ref(np.abs(src), indptr, "sum")
            bound = 2.0 ** -23 * sabs.astype(np.float64) * seglen
            if reduce == "mean":
                bound = bound / np.maximum(seglen, 1) + 2.0 ** -23 * np.abs(ref)
            assert np.all(np.abs(got.astype(np.float64) - ref) <= bound), f"{reduce} {kind} C={C}"
            assert np.allclose(dgot, dref, rtol=2.0 ** -22, atol=0), f"{reduce} {kind} C={C}: gradient"


def test_ties_nan_and_repeat():
    src = np.array([[1, 5], [3, 5], [3, np.nan], [2, np.nan], [7, 0]], np.float32)
    indptr = np.array([0, 4, 4, 5], np.int64)
    for reduce in ("max", "min"):
        x = torch.as_tensor(src).to(DEV).requires_grad_(True)
        out = _sc().segment_csr(x, torch.as_tensor(indptr).to(DEV), reduce=reduce)
        out.backward(torch.ones_like(out))
        ref, arg = R.segment_csr_ref(src, indptr, reduce)
        assert np.array_equal(out.detach().cpu().numpy(), ref, equal_nan=True)
        want = R.segment_csr_grad_ref(np.ones((3, 2), np.float32), indptr, arg, 5, reduce)
        assert np.array_equal(x.grad.cpu().numpy(), want)
    assert arg.tolist() == [[0, 2], [-1, -1], [4, 4]]   # min: lowest row of the minimum; the lowest NaN row
    x = torch.randn(1000, 64, device=DEV)
    ip = torch.arange(0, 1001, 4, device=DEV)
    a, b = _sc().segment_csr(x, ip, reduce="mean"), _sc().segment_csr(x, ip, reduce="mean")
    assert torch.equal(a, b)
    buf = torch.empty(250, 64, device=DEV)
    assert _sc().segment_csr(x, ip, out=buf, reduce="sum") is buf and torch.equal(buf, _sc().segment_csr(x, ip))


def test_refusals():
    f = _sc().segment_csr
    x, ip = torch.zeros(8, 4, device=DEV), torch.tensor([0, 8], device=DEV)
    with pytest.raises(NotImplementedError):
        f(torch.zeros(2, 8, 4, device=DEV), ip)
    with pytest.raises(NotImplementedError):
        f(x, ip[None])
    with pytest.raises(ValueError, match="reduce"):
        f(x, ip, reduce="prod")
    with pytest.raises(RuntimeError, match="device"):
        f(x.cpu(), ip.cpu())


def test_ptv3_scale_with_one_long_segment():
    """N = 240 000 rows, C = 64: pooling segments of 1..16 rows and one segment of 50 000 rows, where the bound
    2^-23 * sum|terms| * segment length is not trivial; all four reductions, forward and backward."""
    g = np.random.default_rng(240)
    N, C, LONG = 240_000, 64, 50_000
    lens = []
    while sum(lens) < 100_000:
        lens.append(int(g.integers(1, 17)))
    lens.append(LONG)
    while sum(lens) < N - 16:
        lens.append(int(g.integers(1, 17)))
    lens.append(N - sum(lens))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert indptr[-1] == N and max(lens) == LONG and sorted(lens)[-2] <= 16 and min(lens) >= 1
    M = len(lens)
    src = g.normal(size=(N, C)).astype(np.float32)
    src[g.integers(0, N, 4000), g.integers(0, C, 4000)] = 1.5   # ties
    dout = g.normal(size=(M, C)).astype(np.float32)
    seglen = np.diff(indptr).astype(np.float64)[:, None]
    sabs, _ = R.segment_csr_ref(np.abs(src), indptr, "sum")
    for reduce in REDUCES:
        x = torch.as_tensor(src).to(DEV).requires_grad_(True)
        out = _sc().segment_csr(x, torch.as_tensor(indptr).to(DEV), reduce=reduce)
        assert out.shape == (M, C) and out.dtype == torch.float32
        out.backward(torch.as_tensor(dout).to(DEV))
        ref, arg = R.segment_csr_ref(src, indptr, reduce)
        dref = R.segment_csr_grad_ref(dout, indptr, arg, N, reduce)
        got, dgot = out.detach().cpu().numpy(), x.grad.cpu().numpy()
        if reduce in ("max", "min"):
            assert np.array_equal(got, ref), reduce
            assert np.array_equal(dgot, dref), f"{reduce}: gradient rows (ties go to the lowest row)"
        else:
            bound = 2.0 ** -23 * sabs.astype(np.float64) * seglen
            if reduce == "mean":
                bound = bound / np.maximum(seglen, 1) + 2.0 ** -23 * np.abs(ref)
            err = np.abs(got.astype(np.float64) - ref)
            print(f"[segment_csr] {reduce}: long segment worst error / bound {float((err[lens.index(LONG)] / bound[lens.index(LONG)]).max()):.3e}")
            assert np.all(err <= bound), reduce
            assert np.allclose(dgot, dref, rtol=2.0 ** -22, atol=0), f"{reduce}: gradient"
