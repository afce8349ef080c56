"""unipre3d_amd.causal_conv1d and unipre3d_amd.layernorm on the MI355X against the restatement (tests/mambaops_ref.py): lengths around
every lane, 64-step group and chunk boundary of the conv kernel, row widths around every register layout of the norm kernel, row
counts on both sides of the backward's row split, the option grids, views, the exact cases, determinism, the refusals, PCM's block
prologue chain, and mamba_inner_fn_no_out_proj at every conv width.

Tolerance (mambaops_ref's docstring): per tensor max |got - f64| / max |f64| <= max(4 x the fp32 restatement's own figure, 4 ulp).
Every figure is printed before it is asserted; U3D_MAMBAOPS_TOLERANCE_OUT=<file> collects them (profiles/mambaops/tolerance.json).
"""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

import mambaops_ref as R
import selective_scan_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIGURES = []


@pytest.fixture(scope="module")
def cc():
    from unipre3d_amd import causal_conv1d
    causal_conv1d.load()
    yield causal_conv1d
    path = os.environ.get("U3D_MAMBAOPS_TOLERANCE_OUT")
    if path and FIGURES:
        worst = max(FIGURES, key=lambda f: f["ratio_to_bar"])
        with open(path, "w") as f:
            json.dump({"unit": "max |got - f64| / max |f64| per tensor; bar = max(4 x yardstick, 4 * 2^-23); yardstick = the fp32 run of "
                               "the restatement (tests/mambaops_ref.py; torch's F.layer_norm for the ill-conditioned rows)",
                       "worst": {k: worst[k] for k in ("case", "tensor", "ratio_to_bar")}, "cases": FIGURES}, f, indent=1)


@pytest.fixture(scope="module")
def ln(cc):
    from unipre3d_amd import layernorm
    return layernorm


def _check(case, name, got, want64, yardstick):
    err, b = R.norm_err(got, want64), R.bar(yardstick)
    FIGURES.append({"case": case, "tensor": name, "yardstick": yardstick, "bar": b, "device": err, "ratio_to_bar": err / b})
    print(f"[mambaops] {case} {name}: yardstick {yardstick:.3e} bar {b:.3e} device {err:.3e}")
    return [] if err <= b else [f"{case} {name}: {err:.3e} > {b:.3e}"]


def _compare(case, names, fn_ref, fn_dev, tensors, douts, fn_yard=None):
    """fn_ref in fp64 is the answer, fn_yard (default fn_ref) in fp32 the yardstick, fn_dev in fp32 on the device is checked: every
    output and the gradient of every given tensor.  names = (output names, tensor names).  Returns the device's (outs, grads)."""
    o64, g64 = R.run_with_grads(fn_ref, tensors, douts)
    o32, g32 = R.run_with_grads(fn_yard or fn_ref, R.cast(tensors, torch.float32), [d.float() for d in douts])
    od, gd = R.run_with_grads(fn_dev, R.cast(tensors, torch.float32, DEV), [d.float() for d in douts])
    bad = []
    for n, a, b, c in zip(names[0], od, o64, o32):
        assert a.shape == b.shape, (n, a.shape)
        bad += _check(case, n, a, b, R.norm_err(c, b))
    for n, a, b, c in zip(names[1], gd, g64, g32):
        assert (a is None) == (b is None), n
        if b is not None:
            assert a.shape == b.shape, (n, a.shape)
            bad += _check(case, "d" + n, a, b, R.norm_err(c, b))
    assert not bad, bad
    return od, gd


# ==== causal conv ===================================================================================================================
CONV_NAMES = (("out",), ("x", "weight", "bias"))


@functools.lru_cache(maxsize=None)
def _conv_inputs(batch, dim, L, width, has_bias):
    return R.conv_inputs(batch, dim, L, width, has_bias)


def _conv_case(cc, case, batch, dim, L, width=4, has_bias=True, activation="silu"):
    x, w, b, dout = _conv_inputs(batch, dim, L, width, has_bias)
    return _compare(case, CONV_NAMES, lambda x, w, b: R.causal_conv1d(x, w, b, activation),
                    lambda x, w, b: cc.causal_conv1d_fn(x, w, b, activation), (x, w, b), (dout,))


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 63, 64, 65, 129, 257])
def test_conv_lengths_all_gradients(cc, L):
    """D = 5 with odd L: rows start at every 4-byte phase.  L <= 3 is shorter than the taps, 63 | 64 | 65 straddle a 64-step group, 129 is
    Mamba3D's length (three steps per lane, one chunk), 257 one step into a second chunk."""
    _conv_case(cc, f"conv_len_L{L}", 2, 5, L)


@pytest.mark.parametrize("batch", [1, 3])
def test_conv_batch_reduction_of_dweight_and_dbias(cc, batch):
    """dweight and dbias are summed over b from per-(b, d) partials: one row and three."""
    _conv_case(cc, f"conv_batch_B{batch}_L129", batch, 5, 129)


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 130])
def test_conv_channel_counts(cc, dim):
    """One (b, d) row per wave, four waves a workgroup: a single channel, and row counts around one and two reduce workgroups."""
    _conv_case(cc, f"conv_D{dim}_L65", 2, dim, 65, 4)


def test_conv_lengths_around_the_chunk(cc):
    """The chunk a wave covers before it moves on (and carries the halo in registers), from the library: one below, at, one above, and
    one step into a third chunk."""
    chunk = cc.chunk_len(1 << 20)
    assert chunk % 64 == 0 and cc.chunk_len(chunk + 1) == chunk
    for L in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        _conv_case(cc, f"conv_chunk_L{L}", 2, 5, L)


@pytest.mark.parametrize("activation", [None, "silu", "swish"])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_option_grid(cc, width, has_bias, activation):
    od, gd = _conv_case(cc, f"conv_opt_W{width}_b{int(has_bias)}_{activation}", 2, 7, 129, width, has_bias, activation)
    assert (gd[2] is None) == (not has_bias)


def test_conv_chunk_views_are_read_in_place(cc):
    """Both halves of an xz of shape (2, 12, 67), as Mamba passes them: the same bits as their dense copies, the gradient reaches xz and
    the half that was not used gets zeros; a channel-last x (made dense inside) gives the same bits too."""
    x, w, b, dout = R.conv_inputs(2, 12, 67, 4)
    xd, wd, bd, dd = R.cast((x, w[:6], b[:6], dout[:, :6]), torch.float32, DEV)
    want64, g64 = {}, {}
    for half in (0, 1):
        (o,), g = R.run_with_grads(lambda x, w, b: R.causal_conv1d(x, w, b, "silu"), (x.chunk(2, dim=1)[half], w[:6], b[:6]), (dout[:, :6],))
        (o32,), g32 = R.run_with_grads(lambda x, w, b: R.causal_conv1d(x, w, b, "silu"),
                                       R.cast((x.chunk(2, dim=1)[half], w[:6], b[:6]), torch.float32), (dout[:, :6].float(),))
        want64[half], g64[half] = o, (g[0], R.norm_err(o32, o), R.norm_err(g32[0], g[0]))
    bad = []
    for half in (0, 1):
        xz = xd.clone().requires_grad_(True)
        view = xz.chunk(2, dim=1)[half]
        assert not view.is_contiguous() and view.stride(2) == 1
        out = cc.causal_conv1d_fn(view, wd, bd, "silu")
        assert out.is_contiguous() and torch.equal(out, cc.causal_conv1d_fn(view.detach().contiguous(), wd, bd, "silu"))
        (out * dd).sum().backward()
        lo, hi = 6 * half, 6 * half + 6
        bad += _check(f"conv_view_half{half}", "out", out, want64[half], g64[half][1])
        bad += _check(f"conv_view_half{half}", "dx", xz.grad[:, lo:hi], g64[half][0], g64[half][2])
        assert float(xz.grad[:, 6 - lo:12 - lo].abs().max()) == 0.0
        dense = view.detach().contiguous()
        last = dense.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert last.stride(2) == 6 and torch.equal(cc.causal_conv1d_fn(last, wd, bd, "silu"), out)
    assert not bad, bad


@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_one_hot_tap_is_the_shifted_input_bit_for_bit(cc, width):
    L = 300
    x = R.conv_inputs(2, 5, L, width)[0].float().to(DEV)
    for w in range(width):
        weight = torch.zeros(5, width, device=DEV)
        weight[:, w] = 1.0
        out, shift = cc.causal_conv1d_fn(x, weight), width - 1 - w
        assert torch.equal(out[..., shift:], x[..., :L - shift]), (width, w)
        assert shift == 0 or float(out[..., :shift].abs().max()) == 0.0


def test_conv_causality_and_row_independence_bit_for_bit(cc):
    """Changing x at step l0 leaves every output before l0 as it was (l0 on a lane, a group and a chunk boundary and inside); changing
    one (b, d) row leaves every other row as it was."""
    x, w, _, _ = R.cast(R.conv_inputs(2, 5, 300, 4), torch.float32, DEV)
    base = cc.causal_conv1d_fn(x, w)
    for l0 in (0, 1, 63, 64, 65, 255, 256, 257, 299):
        y = x.clone()
        y[:, :, l0] += 1.0
        out = cc.causal_conv1d_fn(y, w)
        assert torch.equal(out[..., :l0], base[..., :l0]), l0
        assert not torch.equal(out[..., l0], base[..., l0]), l0
        assert torch.equal(out[..., l0 + 4:], base[..., l0 + 4:]), l0
    y = x.clone()
    y[1, 2] += 1.0
    out = cc.causal_conv1d_fn(y, w)
    keep = torch.ones(2, 5, dtype=torch.bool, device=DEV)
    keep[1, 2] = False
    assert torch.equal(out[keep], base[keep]) and not torch.equal(out[1, 2], base[1, 2])


def test_conv_two_runs_are_bit_identical(cc):
    t = R.cast(R.conv_inputs(3, 5, 300, 4), torch.float32, DEV)
    f = lambda x, w, b: cc.causal_conv1d_fn(x, w, b, "silu")
    a, b = R.run_with_grads(f, t[:3], t[3:]), R.run_with_grads(f, t[:3], t[3:])
    assert torch.equal(a[0][0], b[0][0])
    for n, u, v in zip(CONV_NAMES[1], a[1], b[1]):
        assert torch.equal(u, v), n


def test_conv_refusals(cc):
    x, w, b, _ = R.cast(R.conv_inputs(2, 6, 9, 4), torch.float32, DEV)
    f = cc.causal_conv1d_fn
    for width in (1, 5):
        with pytest.raises(NotImplementedError, match="width"):
            f(x, torch.randn(6, width, device=DEV), b)
    for bad in ((x.half(), w, b), (x, w.double(), b), (x, w, b.half())):
        with pytest.raises(NotImplementedError, match="fp32 only"):
            f(*bad)
    with pytest.raises(NotImplementedError, match="activation must be None, silu, or swish"):
        f(x, w, b, "relu")
    for bad in ((x.cpu(), w.cpu(), b.cpu()), (x, w.cpu(), b), (x, w, b.cpu())):
        with pytest.raises(RuntimeError, match="no CPU fallback|different devices"):
            f(*bad)
    for bad in ((x, w[:5], b), (x, w, b[:5]), (x[0], w, b)):
        with pytest.raises(ValueError):
            f(*bad)
    assert cc.causal_conv1d_update is None


# ==== add + norm ====================================================================================================================
NORM_NAMES = (("y", "r"), ("x", "weight", "bias", "residual"))


@functools.lru_cache(maxsize=None)
def _norm_inputs(M, N, has_bias, has_residual):
    return R.norm_inputs(M, N, has_bias, has_residual)


def _norm_case(ln, case, M, N, is_rms, has_bias=True, has_residual=True, prenorm=True, eps=1e-5):
    x, w, b, res, dy, dr = _norm_inputs(M, N, has_bias, has_residual)
    names = NORM_NAMES if prenorm else (("y",), NORM_NAMES[1])
    od, gd = _compare(case, names, lambda x, w, b, res: R.layer_norm(x, w, b, res, eps, prenorm, is_rms),
                      lambda x, w, b, res: ln.layer_norm_fn(x, w, b, res, eps, prenorm, True, is_rms), (x, w, b, res), (dy, dr)[:len(names[0])])
    if prenorm:      # r is torch's own fp32 sum, bit for bit
        assert torch.equal(od[1].cpu(), x.float() + res.float() if has_residual else x.float())
    if has_residual:
        assert torch.equal(gd[0], gd[3])
    return od, gd


@pytest.mark.parametrize("N", [1, 3, 4, 63, 64, 65, 384, 385, 768, "cap"])
def test_norm_widths(ln, N):
    """A dword per lane below 4-element multiples (1, 3, 63, 65, 385: one, four and sixteen 64-lane groups), float4 per lane otherwise
    (4, 64: one group; 384: two; 768 and the cap: four), with M = 5 (two backward waves: four rows and one)."""
    N = ln.max_n() if N == "cap" else N
    for is_rms in (False, True):
        _norm_case(ln, f"norm_N{N}_{'rms' if is_rms else 'ln'}", 5, N, is_rms)


def test_norm_width_above_the_cap_raises(ln):
    n = ln.max_n() + 1
    with pytest.raises(NotImplementedError, match="at most"):
        ln.layer_norm_fn(torch.randn(2, n, device=DEV), torch.ones(n, device=DEV), None)


def test_norm_row_counts_around_the_backward_split(ln):
    """M = 1, M = 5, an M at which every backward wave owns at least two rows and some own one more (from the library's split), and an
    M beyond the wave cap (narrow rows: the split is by rows alone)."""
    split = next(M for M in range(8, 200) if M // ln.bwd_waves(M) >= 2 and M % ln.bwd_waves(M) != 0)
    capped = 4 * 2048 + 5
    assert ln.bwd_waves(capped) == ln.bwd_waves(2 * capped) and capped % ln.bwd_waves(capped) != 0
    for M, N in ((1, 384), (5, 384), (split, 384), (split, 65), (capped, 4)):
        for is_rms in (False, True):
            _norm_case(ln, f"norm_M{M}_N{N}_{'rms' if is_rms else 'ln'}", M, N, is_rms)


@pytest.mark.parametrize("prenorm", [False, True])
@pytest.mark.parametrize("has_residual", [False, True])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("is_rms", [False, True])
def test_norm_option_grid(ln, is_rms, has_bias, has_residual, prenorm):
    od, gd = _norm_case(ln, f"norm_opt_{'rms' if is_rms else 'ln'}_b{int(has_bias)}_r{int(has_residual)}_p{int(prenorm)}", 37, 384, is_rms,
                        has_bias, has_residual, prenorm)
    assert (gd[2] is None) == (not has_bias) and (gd[3] is None) == (not has_residual)


def test_norm_centred_variance_survives_a_large_offset(ln):
    """Rows of 1000 + 0.01 noise: E[r^2] - mean^2 would lose every digit of the variance in fp32.  The yardstick is torch's own fp32
    F.layer_norm (which centres), forward and backward."""
    g = torch.Generator().manual_seed(11)
    x = 1000.0 + 0.01 * torch.randn(5, 384, generator=g, dtype=torch.float64)
    x = x.float().double()                                                         # the values the device sees
    _, w, b, _, dy, _ = R.norm_inputs(5, 384)
    eps = 1e-6
    od, _ = _compare("norm_offset_1000", (("y",), ("x", "weight", "bias")), lambda x, w, b: R.layer_norm(x, w, b, None, eps),
                     lambda x, w, b: ln.layer_norm_fn(x, w, b, None, eps), (x, w, b), (dy,),
                     fn_yard=lambda x, w, b: F.layer_norm(x, (384,), w, b, eps))
    assert float(od[0].std()) > 0.5                                                # the rows were normalised, not flattened


def test_norm_exact_cases(ln):
    """A constant row gives the bias under LayerNorm, bit for bit; changing one row leaves every other row's y and dx as they were."""
    x, w, b, res, dy, _ = R.cast(R.norm_inputs(9, 384), torch.float32, DEV)
    const = torch.tensor([1000.0, -3.25, 0.0, 1e-3], device=DEV)[:, None].expand(4, 384)
    assert torch.equal(ln.layer_norm_fn(const, w, b), b[None].expand(4, 384))
    f = lambda x, w, b, res: ln.layer_norm_fn(x, w, b, res, 1e-5)
    (y0,), g0 = R.run_with_grads(f, (x, w, b, res), (dy,))
    x2 = x.clone()
    x2[4] += 1.0
    (y1,), g1 = R.run_with_grads(f, (x2, w, b, res), (dy,))
    keep = torch.arange(9, device=DEV) != 4
    assert torch.equal(y0[keep], y1[keep]) and not torch.equal(y0[4], y1[4])
    assert torch.equal(g0[0][keep], g1[0][keep]) and not torch.equal(g0[0][4], g1[0][4])


def test_norm_shapes_and_layouts(ln):
    """(B, L, N) in, (B, L, N) out, y, r and the gradients alike; an input whose last dimension is strided is made dense."""
    x, w, b, res, dy, dr = R.norm_inputs(6 * 7, 64)
    t3 = [x.reshape(6, 7, 64), w, b, res.reshape(6, 7, 64)]
    od, gd = _compare("norm_3d", NORM_NAMES, lambda x, w, b, res: R.rms_norm(x, w, b, res, True, 1e-5),
                      lambda x, w, b, res: ln.rms_norm_fn(x, w, b, res, True, False, 1e-5), t3, (dy.reshape(6, 7, 64), dr.reshape(6, 7, 64)))
    assert od[0].shape == od[1].shape == gd[0].shape == gd[3].shape == (6, 7, 64)
    wide = torch.randn(6, 7, 128, device=DEV)
    strided = wide[..., ::2]
    assert strided.stride(-1) == 2
    wd, bd = w.float().to(DEV), b.float().to(DEV)
    assert torch.equal(ln.layer_norm_fn(strided, wd, bd), ln.layer_norm_fn(strided.contiguous(), wd, bd))
    one = ln.layer_norm_fn(wide[0, 0, :64], wd, bd)                                # a single row, 1-D
    assert one.shape == (64,) and torch.equal(one, ln.layer_norm_fn(wide[:1, 0, :64], wd, bd)[0])


def test_norm_misaligned_pointers_take_the_dword_path(ln):
    """N = 64 allows float4 accesses only where every pointer is 16-byte aligned: an x that starts 4 bytes into its allocation, and a
    dy that arrives as such a view (the gradient of a concatenation is a narrow view of the incoming one)."""
    x, w, b, res, dy, dr = R.norm_inputs(42, 64)
    seen = []

    def dev(x, w, b, res):
        pad = x.new_zeros(1)
        xm = torch.cat([pad, x.flatten()])[1:].view_as(x)
        seen.append(xm.data_ptr() % 16)
        y, r = ln.layer_norm_fn(xm, w, b, res, 1e-5, True)
        return torch.cat([pad, y.flatten()])[1:].view_as(y), r

    _compare("norm_misaligned", NORM_NAMES, lambda x, w, b, res: R.layer_norm(x, w, b, res, 1e-5, True), dev, (x, w, b, res), (dy, dr))
    assert seen == [4]


def test_rms_norm_module(ln):
    """An nn.Module the reference's isinstance check accepts; its forward passes upstream's keywords (upstream's own forward adds an
    is_rms_norm= keyword its rms_norm_fn does not take); eps defaults: 1e-5 on the module, 1e-6 on the functions."""
    import inspect
    m = ln.RMSNorm(384, device=DEV)
    assert isinstance(m, torch.nn.Module) and isinstance(m, (torch.nn.LayerNorm, ln.RMSNorm)) and m.bias is None and m.eps == 1e-5
    assert torch.equal(m.weight.detach(), torch.ones(384, device=DEV)) and m.weight.requires_grad
    assert inspect.signature(ln.rms_norm_fn).parameters["eps"].default == 1e-6
    assert inspect.signature(ln.layer_norm_fn).parameters["eps"].default == 1e-6
    assert list(inspect.signature(ln.rms_norm_fn).parameters) == ["x", "weight", "bias", "residual", "prenorm", "residual_in_fp32", "eps"]
    assert list(inspect.signature(ln.layer_norm_fn).parameters) == ["x", "weight", "bias", "residual", "eps", "prenorm", "residual_in_fp32",
                                                                    "is_rms_norm"]
    x, _, _, res, _, _ = R.cast(R.norm_inputs(5, 384), torch.float32, DEV)
    y, r = m(x, residual=res, prenorm=True, residual_in_fp32=True)
    y2, r2 = ln.rms_norm_fn(x, m.weight, m.bias, residual=res, prenorm=True, residual_in_fp32=True, eps=m.eps)
    assert torch.equal(y, y2) and torch.equal(r, r2) and torch.equal(r, x + res)
    assert torch.equal(m(x), ln.rms_norm_fn(x, m.weight, None, eps=1e-5)) and not torch.equal(m(x * 1e-3), ln.rms_norm_fn(x * 1e-3, m.weight, None))
    y.sum().backward()
    assert m.weight.grad is not None and m.weight.grad.shape == (384,)


def test_block_prologue_chain(ln):
    """Two PCM block openings (rms_norm_fn, prenorm, residual carried, eps 1e-5) against the restated chain: hidden and residual as they
    enter the second mixer, and the gradients of the input, the stand-in mixer and both norm weights."""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    hidden, mix, w1, w2 = r(2, 37, 384), r(384, 384) / 384 ** 0.5, 1.0 + 0.2 * r(384), 1.0 + 0.2 * r(384)
    _compare("prologue_chain", (("hidden", "residual"), ("hidden_in", "mix", "w1", "w2")),
             lambda h, m, a, b: R.block_prologues(h, m, a, b), lambda h, m, a, b: R.block_prologues(h, m, a, b, norm=ln.rms_norm_fn),
             (hidden, mix, w1, w2), (r(2, 37, 384), r(2, 37, 384)))


def test_norm_two_runs_are_bit_identical(ln):
    t = R.cast(R.norm_inputs(301, 384), torch.float32, DEV)
    for is_rms in (False, True):
        f = lambda x, w, b, res: ln.layer_norm_fn(x, w, b, res, 1e-5, True, False, is_rms)
        a, b = R.run_with_grads(f, t[:4], t[4:]), R.run_with_grads(f, t[:4], t[4:])
        for u, v in zip(a[0] + a[1], b[0] + b[1]):
            assert torch.equal(u, v)


# ==== the mixer's inner function at every conv width and around the conv's chunk ====================================================
@pytest.mark.parametrize("L", [5, "chunk+1"])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_inner_function_composition_widths_and_lengths(cc, width, L):
    """mamba_inner_fn_no_out_proj (d_inner 48, dt_rank 2, B = 2) against selective_scan_ref's composition at every conv width, at a
    length barely above the taps and at one step into the conv's second chunk: the output and the gradient of xz and every parameter."""
    from unipre3d_amd import selective_scan as ss
    L = cc.chunk_len(1 << 20) + 1 if L == "chunk+1" else L
    g = torch.Generator().manual_seed(7 + width)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    d_inner, rank = 48, 2
    names = ("xz", "conv_w", "conv_b", "x_proj", "dt_proj", "A", "D", "dt_bias")
    t = (r(2, 2 * d_inner, L), 0.5 * r(d_inner, 1, width), 0.1 * r(d_inner), r(rank + 2 * S.N, d_inner) / d_inner ** 0.5,
         r(d_inner, rank) / rank ** 0.5, -torch.exp(0.3 * r(d_inner, S.N)) * (1.0 + torch.arange(S.N, dtype=torch.float64))[None], r(d_inner),
         -1.5 + 0.5 * r(d_inner))
    ref = lambda xz, cw, cb, xp, dp, A, D, db: S.mamba_inner_no_out_proj(xz, cw, cb, xp, dp, A, D, db)
    dev = lambda xz, cw, cb, xp, dp, A, D, db: ss.mamba_inner_fn_no_out_proj(xz, cw, cb, xp, dp, A, None, None, D, db, None, None, True)
    od, _ = _compare(f"inner_W{width}_L{L}", (("out",), names), ref, dev, t, (r(2, d_inner, L),))
    assert od[0].shape == (2, d_inner, L)
