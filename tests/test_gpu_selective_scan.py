"""unipre3d_amd.selective_scan on the MI355X against the sequential restatement (tests/selective_scan_ref.py): lengths around every
pass and lane-run boundary of the kernel, the option grid, the three analytic cases on structured inputs, all eight gradients,
determinism, the inner-function composition, the refusals, and the header against the binding.

Tolerance (selective_scan_ref's docstring): per tensor max |got - f64| / max |f64| <= max(4 x the fp32 loop's own figure, 4 ulp).
Every figure is printed before it is asserted; U3D_SSCAN_TOLERANCE_OUT=<file> collects them (profiles/selective_scan/tolerance.json).
"""
import ctypes
import functools
import json
import os
import re

import pytest
import torch

import selective_scan_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIGURES = []


@pytest.fixture(scope="module")
def ss():
    from unipre3d_amd import selective_scan
    selective_scan.load()
    yield selective_scan
    path = os.environ.get("U3D_SSCAN_TOLERANCE_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"unit": "max |got - f64| / max |f64| per tensor; bar = max(4 x yardstick, 4 * 2^-23); yardstick = the fp32 run of "
                               "the sequential restatement (tests/selective_scan_ref.py)", "cases": FIGURES}, f, indent=1)


def _check(case, name, got, want64, yardstick):
    err, b = R.norm_err(got, want64), R.bar(yardstick)
    FIGURES.append({"case": case, "tensor": name, "yardstick": yardstick, "bar": b, "device": err})
    print(f"[selective_scan] {case} {name}: yardstick {yardstick:.3e} bar {b:.3e} device {err:.3e}")
    return [] if err <= b else [f"{case} {name}: {err:.3e} > {b:.3e}"]


@functools.lru_cache(maxsize=None)
def _reference(batch, dim, L, groups, has_D, has_z, has_bias, softplus, seed=0):
    t, dout = R.make_inputs(batch, dim, L, groups, has_D, has_z, has_bias, softplus, seed)
    o64, g64, ys = R.yardstick_case(t, dout, delta_softplus=softplus)
    last64 = R.selective_scan(**t, delta_softplus=softplus, return_last_state=True)[1]
    last32 = R.selective_scan(**R.cast(t, torch.float32), delta_softplus=softplus, return_last_state=True)[1]
    ys["last_state"] = R.norm_err(last32, last64)
    return t, dout, o64, g64, last64, ys


def _device_case(ss, case, batch, dim, L, groups=None, has_D=True, has_z=True, has_bias=True, softplus=True):
    t, dout, o64, g64, last64, ys = _reference(batch, dim, L, groups, has_D, has_z, has_bias, softplus)
    td = R.cast(t, torch.float32, DEV)
    out, grads = R.run_with_grads(ss.selective_scan_fn, td, dout.float().to(DEV), delta_softplus=softplus)
    bad = _check(case, "out", out, o64, ys["out"])
    for k in R.GRAD_NAMES:
        if g64[k] is None:
            assert grads[k] is None
            continue
        assert grads[k].shape == t[k].shape, (k, grads[k].shape)
        bad += _check(case, "d" + k, grads[k], g64[k], ys[k])
    out2, last = ss.selective_scan_fn(**td, delta_softplus=softplus, return_last_state=True)
    assert torch.equal(out2, out) and not last.requires_grad
    bad += _check(case, "last_state", last, last64, ys["last_state"])
    assert not bad, bad
    return td, out, grads


def test_pass_lengths(ss):
    """One pass covers 64 lanes x 1, 2, 3 or 4 steps, chosen from L; above 256 the state is carried across passes of 256."""
    assert [ss.pass_len(L) for L in (1, 64, 65, 128, 129, 192, 193, 256, 257, 513, 4096)] == [64, 64, 128, 128, 192, 192] + [256] * 5


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 129, 257, 513])
def test_lengths_all_gradients(ss, L):
    """L = 257 is one step above a single pass, 513 one step above two; out, the last state and all eight gradients."""
    _device_case(ss, f"len_L{L}_D5", 2, 5, L)


@pytest.mark.parametrize("dim,groups,L", [(8, None, 129), (70, None, 129), (70, 1, 257), (70, 2, 129), (8, 2, 257), (8, 2, 513)])
def test_channels_and_groups(ss, dim, groups, L):
    """D = 70 with one group spans two channel slabs (64 + 6, the partials + reduce path); with two groups each slab holds 35 channels;
    3-D B / C (groups None) come back with 3-D gradients."""
    _device_case(ss, f"ch_D{dim}_G{groups}_L{L}", 2, dim, L, groups=groups)


@pytest.mark.parametrize("dim,groups,L", [(1, 1, 65), (3, 1, 65), (4, 1, 65), (17, 1, 65), (63, 1, 65), (64, 1, 65), (65, 1, 65), (129, 1, 65),
                                          (130, 2, 65), (192, 3, 65), (129, 1, 257)])
def test_backward_channel_classes(ss, dim, groups, L):
    """A backward workgroup is four waves on a slab of 64 channels of one group, 16 channels a wave: one wave alone (D = 1), a wave short
    of four (3), exactly four (4), one past a wave's 16 (17), one short of a slab (63), a full slab (64), slab + 1 (65), three slabs (129),
    two groups of two slabs with a one-channel tail each (130, 2), three groups of one slab (192, 3); and three slabs over two passes."""
    _device_case(ss, f"cls_D{dim}_G{groups}_L{L}", 2, dim, L, groups=groups)


@pytest.mark.parametrize("batch", [1, 3])
def test_batch_reduction_of_the_parameter_gradients(ss, batch):
    """dA, dD and ddelta_bias are summed over b from per-(b, d) partials, dB / dC come from (B, nslab, N, L) partials: one row and three."""
    _device_case(ss, f"batch_B{batch}_D70_G1_L129", batch, 70, 129, groups=1)


@pytest.mark.parametrize("softplus", [False, True])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("has_z", [False, True])
@pytest.mark.parametrize("has_D", [False, True])
def test_option_grid(ss, has_D, has_z, has_bias, softplus):
    _device_case(ss, f"opt_D{int(has_D)}_z{int(has_z)}_b{int(has_bias)}_sp{int(softplus)}", 2, 8, 129, has_D=has_D, has_z=has_z,
                 has_bias=has_bias, softplus=softplus)


def test_chunk_views(ss):
    """u and z as the two halves of one (B, 2 D, L) tensor, as Mamba passes them: same bits as the dense copies, gradients reach xz."""
    t, dout, o64, g64, _, ys = _reference(2, 8, 129, None, True, True, True, True)
    td = R.cast(t, torch.float32, DEV)
    xz = torch.cat([td["u"], td["z"]], dim=1).requires_grad_(True)
    u, z = xz.chunk(2, dim=1)
    assert not z.is_contiguous()
    out = ss.selective_scan_fn(u, td["delta"], td["A"], td["B"], td["C"], td["D"], z=z, delta_bias=td["delta_bias"], delta_softplus=True)
    dense = ss.selective_scan_fn(**td, delta_softplus=True)
    assert torch.equal(out, dense)
    (out * dout.float().to(DEV)).sum().backward()
    bad = _check("chunk_views", "du", xz.grad[:, :8], g64["u"], ys["u"]) + _check("chunk_views", "dz", xz.grad[:, 8:], g64["z"], ys["z"])
    assert not bad, bad


# ---- analytic cases on structured inputs -------------------------------------------------------------------------------------------
def _dev32(*ts):
    return [None if t is None else t.float().to(DEV) for t in ts]


@pytest.mark.parametrize("L", [129, 257])
def test_zero_A_running_sum_with_softplus_across_20(ss, L):
    """A = 0: y_l = sum_n C[n,l] sum_{k<=l} dt_k B[n,k] u_k, dt = softplus(raw) with raw on both sides of torch's threshold 20."""
    batch, dim = 2, 5
    s = R.structured(batch, dim, L)
    raw = -2.0 + 3.0 * s["z"]                                                      # -6.5 .. 2.5, differs per (b, d, l)
    raw[:, :, 5::7] = torch.tensor([19.5, 19.999, 20.0, 20.001, 20.5, 25.0, 60.0], dtype=torch.float64).repeat(L)[:raw[:, :, 5::7].shape[-1]]
    raw = raw.float().double()                                                     # the values the device sees
    dt = torch.nn.functional.softplus(raw)
    A0 = torch.zeros(dim, R.N, dtype=torch.float64)
    want = R.running_sum_answer(dt, s["B"].float().double(), s["C"].float().double(), s["u"].float().double())
    y32 = R.selective_scan(*[v.float() for v in (s["u"], raw, A0, s["B"], s["C"])], delta_softplus=True)
    u, rw, A, Bm, Cm = _dev32(s["u"], raw, A0, s["B"], s["C"])
    got = ss.selective_scan_fn(u, rw, A, Bm, Cm, delta_softplus=True)
    bad = _check(f"zeroA_L{L}", "out", got, want, R.norm_err(y32, want))
    swapped = ss.selective_scan_fn(u, rw, A, Cm, Bm, delta_softplus=True)
    assert R.norm_err(swapped, want) > 1e-2                                        # the inputs tell B from C
    assert not bad, bad


def test_zero_delta_is_the_skip_path(ss):
    """delta = 0 without softplus: the state never leaves 0 and out = D u silu(z); the last state is exactly 0; so are dB and dA."""
    batch, dim, L = 2, 5, 129
    s = R.structured(batch, dim, L)
    u, A, Bm, Cm, Dp, z = _dev32(s["u"], s["A"], s["B"], s["C"], s["D"], s["z"])
    td = {"u": u, "delta": torch.zeros_like(u), "A": A, "B": Bm, "C": Cm, "D": Dp, "z": z, "delta_bias": None}
    want = s["D"].float().double()[None, :, None] * s["u"].float().double() * torch.nn.functional.silu(s["z"].float().double())
    out, grads = R.run_with_grads(ss.selective_scan_fn, td, torch.ones(batch, dim, L))
    _, last = ss.selective_scan_fn(**td, return_last_state=True)
    bad = _check("zero_delta", "out", out, want, 0.0)
    assert not bad, bad
    assert float(last.abs().max()) == 0.0 and float(grads["B"].abs().max()) == 0.0 and float(grads["A"].abs().max()) == 0.0
    assert float(grads["C"].abs().max()) == 0.0


@pytest.mark.parametrize("L,k", [(129, (2, 3)), (129, (125, 128)), (257, (3, 4)), (257, (255, 256)), (513, (511, 512)), (65, (1, 2))])
def test_impulse_decay(ss, L, k):
    """One impulse in u at step k[b] (the two batch rows sit on the two sides of a lane-run boundary -- runs of 3 steps at L = 129, of 4
    at 257 and 513, of 2 at 65 -- or of a pass boundary, 256 | 512): y_l = C[l] dt_k B[k] u_k exp(A sum_{k<j<=l} dt_j), 0 before k.
    Channel 4's A is so negative that exp(dt A) underflows to 0 in fp32: its answer is the impulse step alone."""
    batch, dim = 2, 5
    s = R.structured(batch, dim, L)
    A = s["A"].clone()
    A[4] = -4000.0 * (1.0 + torch.arange(R.N, dtype=torch.float64))                # dt >= 0.05: exp(-200 ..) == 0 in fp32
    amp = 1.0 + 0.25 * torch.arange(batch * dim, dtype=torch.float64).reshape(batch, dim)
    u = torch.zeros(batch, dim, L, dtype=torch.float64)
    for b in range(batch):
        u[b, :, k[b]] = amp[b]
    f = lambda v: v.float().double()
    want = R.impulse_answer(f(s["dt"]), f(A), f(s["B"]), f(s["C"]), f(amp), k)
    y32 = R.selective_scan(*[v.float() for v in (u, s["dt"], A, s["B"], s["C"])])
    ud, dt, Ad, Bm, Cm = _dev32(u, s["dt"], A, s["B"], s["C"])
    got = ss.selective_scan_fn(ud, dt, Ad, Bm, Cm)
    assert torch.isfinite(got).all()
    for b in range(batch):
        assert float(got[b, :, :k[b]].abs().max()) == 0.0
        if k[b] + 1 < L:
            assert float(got[b, 4, k[b] + 1:].abs().max()) == 0.0                  # the underflowing channel
    bad = _check(f"impulse_L{L}_k{k[0]}_{k[1]}", "out", got, want, R.norm_err(y32, want))
    assert R.norm_err(got.flip(-1), want) > 1e-2
    assert not bad, bad


def test_two_runs_are_bit_identical(ss):
    """Multi-pass, multi-slab (the partials + reduce path), the single-slab direct path and three slabs over two passes: out and every
    gradient, twice."""
    for dim, groups, L in ((70, 1, 257), (70, 2, 129), (129, 1, 257)):
        t, dout, *_ = _reference(2, dim, L, groups, True, True, True, True)
        td = R.cast(t, torch.float32, DEV)
        a = R.run_with_grads(ss.selective_scan_fn, td, dout.float().to(DEV), delta_softplus=True)
        b = R.run_with_grads(ss.selective_scan_fn, td, dout.float().to(DEV), delta_softplus=True)
        assert torch.equal(a[0], b[0])
        for k in R.GRAD_NAMES:
            assert torch.equal(a[1][k], b[1][k]), k


def test_inner_function_composition(ss):
    """mamba_inner_fn_no_out_proj at d_model 24 (d_inner 48, dt_rank 2), L = 129, B = 2 against the restated composition: the output and
    the gradient of xz and of every parameter; mamba_inner_fn adds out_proj."""
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    d_model, d_inner, rank, L, width = 24, 48, 2, 129, 4
    p = {"xz": r(2, 2 * d_inner, L), "conv_w": 0.5 * r(d_inner, 1, width), "conv_b": 0.1 * r(d_inner),
         "x_proj": r(rank + 2 * R.N, d_inner) / d_inner ** 0.5, "dt_proj": r(d_inner, rank) / rank ** 0.5,
         "A": -torch.exp(0.3 * r(d_inner, R.N)) * (1.0 + torch.arange(R.N, dtype=torch.float64))[None], "D": r(d_inner),
         "dt_bias": -1.5 + 0.5 * r(d_inner)}
    dout = r(2, d_inner, L)

    def run(dtype, device, fn):
        q = {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in p.items()}
        out = fn(q)
        (out * dout.to(device=device, dtype=dtype)).sum().backward()
        return out.detach(), {k: v.grad.detach() for k, v in q.items()}

    ref = lambda q: R.mamba_inner_no_out_proj(q["xz"], q["conv_w"], q["conv_b"], q["x_proj"], q["dt_proj"], q["A"], q["D"], q["dt_bias"])
    o64, g64 = run(torch.float64, "cpu", ref)
    o32, g32 = run(torch.float32, "cpu", ref)
    dev = lambda q: ss.mamba_inner_fn_no_out_proj(q["xz"], q["conv_w"], q["conv_b"], q["x_proj"], q["dt_proj"], q["A"], None, None,
                                                  q["D"], q["dt_bias"], None, None, True)
    od, gd = run(torch.float32, DEV, dev)
    assert od.shape == (2, d_inner, L)
    bad = _check("inner", "out", od, o64, R.norm_err(o32, o64))
    for k in p:
        bad += _check("inner", "d" + k, gd[k], g64[k], R.norm_err(g32[k], g64[k]))
    assert not bad, bad
    w, bias = torch.randn(d_model, d_inner, generator=g).to(DEV), torch.randn(d_model, generator=g).to(DEV)
    q = {k: v.float().to(DEV) for k, v in p.items()}
    full = ss.mamba_inner_fn(q["xz"], q["conv_w"], q["conv_b"], q["x_proj"], q["dt_proj"], w, bias, q["A"], None, None, q["D"], q["dt_bias"])
    assert full.shape == (2, L, d_model)
    assert torch.allclose(full, torch.nn.functional.linear(od.transpose(1, 2), w, bias), rtol=1e-4, atol=1e-4)


def test_refusals(ss):
    t, _ = R.make_inputs(2, 8, 16, seed=2)
    td = R.cast(t, torch.float32, DEV)
    f = ss.selective_scan_fn
    with pytest.raises(NotImplementedError, match="complex"):
        f(**{**td, "A": torch.complex(td["A"], td["A"])})
    with pytest.raises(NotImplementedError, match="d_state == 16"):
        f(**{**td, "A": td["A"][:, :8].contiguous()})
    with pytest.raises(NotImplementedError, match="d_state == 16"):
        f(**{**td, "A": td["A"][:4]})
    with pytest.raises(NotImplementedError, match="constant"):
        f(**{**td, "B": td["A"]})
    with pytest.raises(NotImplementedError, match="constant"):
        f(**{**td, "C": td["A"]})
    for name in ("u", "delta", "z", "B"):
        with pytest.raises(NotImplementedError, match="fp32 only"):
            f(**{**td, name: td[name].half()})
    with pytest.raises(NotImplementedError, match="fp32 only"):
        f(**{**td, "A": td["A"].double()})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**R.cast(t, torch.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**{**td, "z": td["z"].cpu()})
    with pytest.raises(ValueError, match="do not divide"):
        f(**{**td, "B": td["B"][:, None].expand(2, 3, 16, 16).contiguous(), "C": td["C"][:, None].expand(2, 3, 16, 16).contiguous()})


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)


def test_header_and_binding_agree(ss):
    """include/unipre3d_selective_scan.h against the module's table and against what the loader set on the handle: the names, the
    parameter count, the return type and the class of every parameter."""
    hdr = open(os.path.join(ROOT, "include", "unipre3d_selective_scan.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    declared = {}
    for ret, name, params in _DECLARATION.findall(hdr):
        types = []
        for q in (s.strip() for s in params.split(",")):
            if q in ("", "void"):
                continue
            types.append(q[:q.rindex("*") + 1].replace(" ", "") if "*" in q else " ".join(q.split()[:-1]))
        assert name not in declared
        declared[name] = (" ".join(ret.split()), types)
    assert len(declared) == 5 and set(declared) == set(ss.EXPORTS) and len(set(ss.EXPORTS)) == len(ss.EXPORTS)
    handle = ss.load()
    assert handle.u3d_sscan_abi_version() == ss.ABI_VERSION == 1
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name, (ret, params) in declared.items():
        fn = getattr(handle, name)
        assert fn.restype is scalars[ret], (name, ret)
        assert len(fn.argtypes) == len(params), name
        assert params == [] or name in ("u3d_sscan_pass_len", "u3d_sscan_bwd_scratch_bytes") or params[-1] == "void*", name   # the stream
        for k, (c_type, bound) in enumerate(zip(params, fn.argtypes)):
            if c_type.endswith("*"):
                assert bound is ctypes.c_void_p, (name, k, c_type)
            else:
                assert bound is scalars[c_type], (name, k, c_type, bound)
