"""_lib.call and the shared argument coercions, without a library or a device: `fn` is a Python function that records what it is given."""
import ctypes

import pytest
import torch
from torch import nn

from unipre3d_amd import _lib

SENTINEL = object()


def _recorder(code=0):
    """Stands in for a ctypes function: keeps its arguments in `.args`, returns the chosen code."""
    def u3d_fake_entry(*args):
        u3d_fake_entry.args = args
        return code
    return u3d_fake_entry


@pytest.fixture
def asked(monkeypatch):
    devs = []

    def fake_stream_ptr(dev=None):
        devs.append(dev)
        return SENTINEL

    monkeypatch.setattr(_lib, "stream_ptr", fake_stream_ptr)
    return devs


def test_arguments_arrive_marshalled_and_in_order(asked):
    t = torch.arange(6, dtype=torch.float32)
    p = nn.Parameter(torch.ones(3))
    empty = torch.empty(0, dtype=torch.int32)
    vp = ctypes.c_void_p(4096)
    dev = torch.device("cuda", 3)
    fn = _recorder()
    assert _lib.call(fn, t, p, None, 7, 0.5, True, vp, empty, dev=dev) == 0
    got = fn.args
    assert len(got) == 9
    assert type(got[0]) is int and got[0] == t.data_ptr() != 0
    assert type(got[1]) is int and got[1] == p.data_ptr() != 0
    assert got[2] is None
    assert type(got[3]) is int and got[3] == 7
    assert type(got[4]) is float and got[4] == 0.5
    assert got[5] is True
    assert got[6] is vp
    assert type(got[7]) is int and got[7] == 0          # a zero-element tensor is a NULL pointer
    assert got[8] is SENTINEL                           # the stream comes last
    assert len(asked) == 1 and asked[0] is dev


def test_no_arguments_but_the_stream(asked):
    fn = _recorder()
    assert _lib.call(fn, dev=None) == 0
    assert fn.args == (SENTINEL,) and asked == [None]


def test_return_codes(asked):
    assert _lib.call(_recorder(0), 1, dev=None) == 0
    with pytest.raises(RuntimeError) as e:
        _lib.call(_recorder(3), 1, dev=None)
    assert str(e.value) == "u3d_fake_entry failed with code 3"
    with pytest.raises(RuntimeError) as e:
        _lib.call(_recorder(3), 1, dev=None, what="fps (grid)")
    assert str(e.value) == "fps (grid) failed with code 3"
    assert _lib.call(_recorder(2), 1, dev=None, accept=(2,)) == 2
    with pytest.raises(RuntimeError) as e:
        _lib.call(_recorder(3), 1, dev=None, accept=(2,))
    assert str(e.value) == "u3d_fake_entry failed with code 3"
    # the text is check(..., named=False)'s
    with pytest.raises(RuntimeError) as e:
        _lib.check(3, "u3d_fake_entry", named=False)
    assert str(e.value) == "u3d_fake_entry failed with code 3"


def test_as_f32():
    view = torch.arange(24, dtype=torch.float64).reshape(4, 6)[:, ::2]          # float64, strided
    out = _lib.as_f32(view, "xyz")
    assert out.dtype == torch.float32 and out.is_contiguous() and torch.equal(out, view.float())
    half = _lib.as_f32(torch.ones(2, 3, dtype=torch.float16), "xyz")
    assert half.dtype == torch.float32 and half.is_contiguous()
    same = torch.ones(2, 3)
    assert _lib.as_f32(same, "xyz") is same                                     # nothing to do: no copy
    with pytest.raises(TypeError) as e:
        _lib.as_f32(torch.zeros(2, 3, dtype=torch.int64), "xyz")
    assert str(e.value) == "xyz must be a floating-point tensor, got torch.int64"


def test_as_i32():
    idx = torch.arange(12, dtype=torch.int64).reshape(3, 4)
    out = _lib.as_i32(idx, "idx")
    assert out.dtype == torch.int32 and out.is_contiguous() and torch.equal(out.long(), idx)
    strided = _lib.as_i32(idx.int().t(), "idx")
    assert strided.dtype == torch.int32 and strided.is_contiguous() and torch.equal(strided.long(), idx.t())
    same = idx.int()
    assert _lib.as_i32(same, "idx") is same
    for bad in (torch.float32, torch.int16, torch.bool):
        with pytest.raises(TypeError) as e:
            _lib.as_i32(torch.zeros(2, dtype=bad), "offset")
        assert str(e.value) == f"offset must be an int32 or int64 tensor, got {bad}"


def test_dense():
    base = torch.arange(64, dtype=torch.float32)
    start = 1 if base.data_ptr() % 16 == 0 else 0
    off = next(k for k in range(start, 8) if base[k:].data_ptr() % 16)          # a 4-byte aligned, not 16-byte aligned start
    p = nn.Parameter(base[off:off + 12].reshape(4, 3, 1))                       # a Conv1d weight (out, in, 1), unaligned
    assert p.data_ptr() % 16 != 0
    out = _lib.dense(p, (4, 3))
    assert out.shape == (4, 3) and out.dtype == torch.float32 and out.is_contiguous() and out.data_ptr() % 16 == 0
    assert not out.requires_grad and out.data_ptr() != p.data_ptr() and torch.equal(out, p.detach().reshape(4, 3))
    aligned = nn.Parameter(torch.ones(4, 3, 1))
    assert aligned.data_ptr() % 16 == 0
    view = _lib.dense(aligned, (4, 3))
    assert view.data_ptr() == aligned.data_ptr() and not view.requires_grad     # aligned and contiguous: a view, no copy
    t = _lib.dense(nn.Parameter(torch.ones(3, 4)).t(), (4, 3))                  # strided: made contiguous
    assert t.is_contiguous() and t.data_ptr() % 16 == 0 and t.shape == (4, 3)


def test_byte_buffer():
    for nbytes, want in ((0, 16), (1, 16), (16, 16), (17, 17), (4096, 4096)):
        buf = _lib.byte_buffer(nbytes, "cpu")
        assert buf.dtype == torch.uint8 and buf.numel() == want and buf.is_contiguous()
    assert _lib.byte_buffer(ctypes.c_size_t(40).value, torch.device("cpu")).numel() == 40
