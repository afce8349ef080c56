#!/usr/bin/env python3
"""Generates tests/golden/g14_mamba.npz: what the reference's OWN Mamba code computes on the CPU in fp32, for unipre3d_amd/selective_scan.py,
causal_conv1d.py and layernorm.py and for tests/mamba_mixer_ref.py.  Both trees are loaded by path under stub packages (their compiled
extensions `selective_scan_cuda` / `causal_conv1d_cuda` are empty stubs), and the names their modules call are bound to the reference's
own *_ref functions (selective_scan_ref, causal_conv1d_ref, mamba_inner_ref, layer_norm_ref, rms_norm_ref).  The adapters below only
rearrange arguments.  Only recorded data is stored; inputs are those of tests/selective_scan_ref.py / tests/mambaops_ref.py in fp32.

  scan_in_*                 u, z, dout (2, 8, 37), A (8, 16), D (8); delta_sp / bias_sp (raw, for softplus) and delta_raw / bias_raw (positive,
                            without); B3, C3 (2, 16, 37) and B4, C4 (2, 2, 16, 37).  A case drops what it does not have
  scan_{case}_*             selective_scan_ref(return_last_state=True): out, last_state, dA, dD, ddelta_bias, and for g0_sp and g2_sp also
                            du ddelta dB dC dz.  case = g{0|2}_{sp|raw} (3-D | G = 2 B / C, softplus on | off) and g0_sp_{noD|noz|nobias}
  conv_cases                the case of every row of the stacked conv arrays: {none|silu}_b{1|0}
  conv_x, conv_w{W}_*       x (2, 12, 19) (its first 6 channels are the input, given as a chunk view; the dense copy gives the same bits);
                            weight (6, W), bias, dout per width W = 2, 3, 4
  conv_w{W}_{out|dx|dweight|dbias}[_f64]   causal_conv1d_ref, one row per case (NaN rows where a case has no bias), in fp32 and in fp64
  norm_cases                the case of every row of the stacked norm arrays: {ln|rms}_r{0|1}_b{0|1}_p{0|1} (residual, bias, prenorm)
  norm_{M}x{N}_*            x, weight, bias, residual, dy, dr for (M, N) = (5, 24) and (3, 384); eps = 1e-5 (`eps`)
  norm_5x24_{y|r|dx|dweight|dbias}[_f64]   layer_norm_ref / rms_norm_ref, one row per case (NaN rows: r without prenorm, dbias without
                            bias), in fp32 and in fp64; dresidual is asserted to equal dx bit for bit and not stored
  norm_3x384_y              the fp32 y alone
  mix_w_*                   state_dict of Mamba3D's Mamba(d_model=24, bimamba_type="v4") after torch.manual_seed(14); every mixer below
                            loads it (PCM's module has the same parameters)
  mix_hidden, mix_cot       hidden_states and the cotangent (quarters), (2, 257, 24); the L = 129 cases use [:, :129]
  mix_{v4|v2|none|slow}_out L = 129.  v4: Mamba3D's fast path; v2 and none: PCM's fast paths (PCM's constructor asserts "v2", so `none` is
                            that module with bimamba_type set afterwards: mamba_inner_fn with out_proj); slow: Mamba3D, use_fast_path=False
  mix_{v4|v2}_dhidden, mix_v4_g_{name}   the gradient of hidden_states, and of every parameter for v4
  mix_v4_L257_out           the v4 mixer at L = 257
  block_*                   two chained PCM MambaBlock (v2 mixers that both load mix_w_*, RMSNorm weights block_w{1|2}_norm.weight seeded
                            away from ones, fused_add_norm, residual_in_fp32), L = 37: hidden_in, cot_hidden, cot_residual (quarters),
                            hidden, residual (out of the second block), dhidden_in, g1_{name} for every parameter of the first block
                            and g2_norm.weight

Size.  The inputs and outputs of these cases alone are about 400 KB of incompressible fp32, more than the largest golden so far (285 KB),
so the gradients are thinned, largest and least telling first (both sides of the comparison differentiate the same forward with
autograd, so a convention that a gradient shows, the output shows too): the L = 257 mixer's, the one-directional mixers', v2's and the
second block's parameters', the wide norm shape's, and the activation-sized ones of the scan's option cases.  main() prints the size.
"""
import importlib
import os
import sys
from functools import partial

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import make_g12_ptv3_boundary as g12  # noqa: E402
import mambaops_ref as MR  # noqa: E402
import selective_scan_ref as SR  # noqa: E402

MODELS = os.path.join(g12.REF, "openpoints/models")
EPS = 1e-5
SCAN_FULL_GRADS = ("g0_sp", "g2_sp")
CONV_CASES = [(act, has_b) for act in (None, "silu") for has_b in (1, 0)]
NORM_CASES = [(rms, r, b, p) for rms in (0, 1) for r in (0, 1) for b in (0, 1) for p in (0, 1)]


def _package(name, path):
    g12._stub(name).__path__ = [path]


def load_reference():
    """Returns ({tree: its mamba_simple module}, PCM's mamba_layer module, the reference's function table)."""
    g12._stub("selective_scan_cuda")
    g12._stub("causal_conv1d_cuda")
    cc = g12._load("causal_conv1d_interface_ref", "openpoints/models/PCM/causal-conv1d/causal_conv1d/causal_conv1d_interface.py")
    g12._stub("causal_conv1d", causal_conv1d_fn=cc.causal_conv1d_ref, causal_conv1d_update=None)
    g12._stub("timm")
    g12._stub("timm.models")
    g12._stub("timm.models.layers", DropPath=torch.nn.Identity)
    _package("bimamba_ssm", os.path.join(MODELS, "Mamba3D/bimamba_ssm"))
    _package("mamba_ssm", os.path.join(MODELS, "PCM/mamba/mamba_ssm"))
    simple, fns = {}, {"causal_conv1d_ref": cc.causal_conv1d_ref}
    for tree in ("bimamba_ssm", "mamba_ssm"):
        ssi = importlib.import_module(tree + ".ops.selective_scan_interface")
        ln = importlib.import_module(tree + ".ops.triton.layernorm")
        ssi.selective_scan_fn, ssi.causal_conv1d_fn = ssi.selective_scan_ref, cc.causal_conv1d_ref      # what mamba_inner_ref calls

        def no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B=None, C=None, D=None, delta_bias=None,
                        B_proj_bias=None, C_proj_bias=None, delta_softplus=True, ssi=ssi):
            eye = torch.eye(conv1d_weight.shape[0], dtype=xz.dtype)                                     # out_proj = identity, no bias
            return ssi.mamba_inner_ref(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, eye, None, A, B, C, D, delta_bias,
                                       B_proj_bias, C_proj_bias, delta_softplus).transpose(1, 2)

        def rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6, ln=ln):
            return ln.rms_norm_ref(x, weight, bias, residual=residual, eps=eps, prenorm=prenorm)

        def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False, ln=ln):
            return (ln.rms_norm_ref if is_rms_norm else ln.layer_norm_ref)(x, weight, bias, residual=residual, eps=eps, prenorm=prenorm)

        m = importlib.import_module(tree + ".modules.mamba_simple")
        m.selective_scan_fn, m.causal_conv1d_fn = ssi.selective_scan_ref, cc.causal_conv1d_ref
        m.mamba_inner_fn, m.mamba_inner_fn_no_out_proj = ssi.mamba_inner_ref, no_out_proj
        m.rms_norm_fn, m.layer_norm_fn = rms_norm_fn, layer_norm_fn
        simple[tree] = m
        fns[tree] = (ssi, ln, rms_norm_fn, layer_norm_fn)
    sys.path.insert(0, os.path.join(MODELS, "PCM"))
    layer = g12._load("pcm_mamba_layer_ref", "openpoints/models/PCM/mamba_layer.py")
    layer.rms_norm_fn, layer.layer_norm_fn = fns["mamba_ssm"][2], fns["mamba_ssm"][3]
    return simple, layer, fns


def _np(t):
    return t.detach().contiguous().numpy()


def _grads(fn, leaves, douts):
    """fn(*leaves) with every given leaf a fresh fp leaf; returns ([outs], [grad or None])."""
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in leaves]
    outs = fn(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * d.to(o.dtype)).sum() for o, d in zip(outs, douts) if d is not None).backward()
    return [o.detach() for o in outs], [None if t is None else t.grad for t in leaves]


def record_scan(out, ssi):
    f32 = lambda t: SR.cast(t, torch.float32)
    sets = {(g, sp): SR.make_inputs(2, 8, 37, groups=g, softplus=sp) for g in (None, 2) for sp in (True, False)}
    (base, dout) = sets[None, True]
    t, d = sets[None, False]                             # the G = 2 sets give B4 / C4 alone: every other tensor is the 3-D sets'
    assert torch.equal(d, dout) and all(torch.equal(t[k], base[k]) for k in ("u", "A", "D", "z"))
    for k in ("u", "A", "D", "z"):
        out["scan_in_" + k] = _np(base[k].float())
    out["scan_in_dout"] = _np(dout.float())
    for sp, tag in ((True, "sp"), (False, "raw")):
        out["scan_in_delta_" + tag], out["scan_in_bias_" + tag] = _np(sets[None, sp][0]["delta"].float()), _np(sets[None, sp][0]["delta_bias"].float())
    for g, tag in ((None, "3"), (2, "4")):
        out["scan_in_B" + tag], out["scan_in_C" + tag] = _np(sets[g, True][0]["B"].float()), _np(sets[g, True][0]["C"].float())
    cases = [(f"g{g or 0}_{'sp' if sp else 'raw'}", g, sp, ()) for g in (None, 2) for sp in (True, False)]
    cases += [("g0_sp_no" + n, None, True, (k,)) for n, k in (("D", "D"), ("z", "z"), ("bias", "delta_bias"))]
    for case, g, sp, absent in cases:
        t = f32({**sets[None, sp][0], "B": sets[g, True][0]["B"], "C": sets[g, True][0]["C"]})
        for k in absent:
            t[k] = None
        (o, last), grads = _grads(lambda u, dl, A, B, C, D, z, b: ssi.selective_scan_ref(u, dl, A, B, C, D, z, b, sp, True),
                                  [t[k] for k in SR.GRAD_NAMES], (dout.float(), None))
        assert o.dtype == torch.float32 and last.shape == (2, 8, 16)
        out[f"scan_{case}_out"], out[f"scan_{case}_last_state"] = _np(o), _np(last)
        for k, gr in zip(SR.GRAD_NAMES, grads):
            assert (gr is None) == (t[k] is None)
            if gr is not None and (case in SCAN_FULL_GRADS or k in ("A", "D", "delta_bias")):
                out[f"scan_{case}_d{k}"] = _np(gr)


def _stack(rows, like):
    """Rows of one tensor over the cases, NaN where a case has none."""
    return np.stack([np.full(like, np.nan, dtype=np.float64) if r is None else _np(r).astype(np.float64) for r in rows])


def record_conv(out, conv_ref):
    out["conv_cases"] = np.asarray([f"{act or 'none'}_b{has_b}" for act, has_b in CONV_CASES])
    for W in (2, 3, 4):
        x, w, b, dout = MR.conv_inputs(2, 12, 19, W)
        if "conv_x" in out:
            assert np.array_equal(out["conv_x"], _np(x.float()))
        out["conv_x"] = _np(x.float())
        w, b, dout = w[:6].float(), b[:6].float(), dout[:, :6].float()
        out[f"conv_w{W}_weight"], out[f"conv_w{W}_bias"], out[f"conv_w{W}_dout"] = _np(w), _np(b), _np(dout)
        for dtype, suffix in ((torch.float32, ""), (torch.float64, "_f64")):
            rows = {"out": [], "dx": [], "dweight": [], "dbias": []}
            for act, has_b in CONV_CASES:
                xz = x.float().to(dtype)
                f = lambda xz, w, b: conv_ref(xz.chunk(2, dim=1)[0], w, b, act)
                (o,), (dxz, dw, db) = _grads(f, (xz, w.to(dtype), b.to(dtype) if has_b else None), (dout.to(dtype),))
                (o2,), _ = _grads(lambda x, w, b: conv_ref(x, w, b, act), (xz[:, :6].contiguous(), w.to(dtype), b.to(dtype) if has_b else None),
                                  (dout.to(dtype),))
                assert o.dtype == dtype and torch.equal(o, o2) and float(dxz[:, 6:].abs().max()) == 0.0
                for k, v in (("out", o), ("dx", dxz[:, :6]), ("dweight", dw), ("dbias", db)):
                    rows[k].append(v)
            for k, v in rows.items():
                out[f"conv_w{W}_{k}{suffix}"] = _stack(v, tuple(next(r for r in v if r is not None).shape)).astype(_np(torch.zeros(0, dtype=dtype)).dtype)


def record_norm(out, ln):
    out["norm_cases"] = np.asarray([f"{'rms' if rms else 'ln'}_r{r}_b{b}_p{p}" for rms, r, b, p in NORM_CASES])
    for M, N in ((5, 24), (3, 384)):
        t = [v.float() for v in MR.norm_inputs(M, N)]
        for k, v in zip(("x", "weight", "bias", "residual", "dy", "dr"), t):
            out[f"norm_{M}x{N}_{k}"] = _np(v)
        for dtype, suffix in ((torch.float32, ""), (torch.float64, "_f64")):
            rows = {"y": [], "r": [], "dx": [], "dweight": [], "dbias": []}
            for rms, has_r, has_b, pre in NORM_CASES:
                ref = ln.rms_norm_ref if rms else ln.layer_norm_ref
                x, w, b, res, dy, dr = [v.to(dtype) for v in t]
                outs, (dx, dw, db, dres) = _grads(lambda x, w, b, res: ref(x, w, b, residual=res, eps=EPS, prenorm=bool(pre)),
                                                  (x, w, b if has_b else None, res if has_r else None), (dy, dr))
                assert outs[0].dtype == dtype and (dres is None or torch.equal(dres, dx))     # dresidual is dx and is not stored
                for k, v in (("y", outs[0]), ("r", outs[1] if pre else None), ("dx", dx), ("dweight", dw), ("dbias", db)):
                    rows[k].append(v)
            for k, v in rows.items():
                if N > 100 and (suffix or k != "y"):      # the wide shape keeps the fp32 y alone
                    continue
                out[f"norm_{M}x{N}_{k}{suffix}"] = _stack(v, tuple(next(r for r in v if r is not None).shape)).astype(_np(torch.zeros(0, dtype=dtype)).dtype)


def _module_run(module, hidden, cots, residual=None):
    module.zero_grad()
    h = hidden.clone().requires_grad_(True)
    outs = module(h) if residual is None else module(h, residual)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    return [o.detach() for o in outs], h.grad, {k: p.grad for k, p in module.named_parameters() if p.grad is not None}


def record_mixers(out, simple):
    torch.manual_seed(14)
    m3d, pcm = simple["bimamba_ssm"].Mamba, simple["mamba_ssm"].Mamba
    v4 = m3d(d_model=24, bimamba_type="v4")
    assert (v4.d_inner, v4.dt_rank, v4.d_conv) == (48, 2, 4)
    state = v4.state_dict()
    for k, v in state.items():
        out["mix_w_" + k] = _np(v)
    g = torch.Generator().manual_seed(14)
    hidden = torch.randn(2, 257, 24, generator=g) + 0.5 * SR._wave((2, 257, 24), 1.1, 0.07, 0.4).float()
    cot = torch.randint(-8, 9, (2, 257, 24), generator=g).float() / 4          # a cotangent may be anything: quarters compress
    out["mix_hidden"], out["mix_cot"] = _np(hidden), _np(cot)
    v2 = pcm(d_model=24, bimamba_type="v2")
    none = pcm(d_model=24, bimamba_type="v2")          # the constructor asserts "v2"; forward takes the mamba_inner_fn branch for any other value
    none.bimamba_type = "none"
    slow = m3d(d_model=24, bimamba_type="v4", use_fast_path=False)
    for name, mod in (("v4", v4), ("v2", v2), ("none", none), ("slow", slow)):
        mod.load_state_dict(state)
        (o,), dh, pg = _module_run(mod, hidden[:, :129], (cot[:, :129],))
        assert o.shape == (2, 129, 24) and o.dtype == torch.float32
        assert len(pg) == (16 if name in ("v4", "v2") else 9)                                 # the one-directional paths leave the *_b set alone
        out[f"mix_{name}_out"] = _np(o)
        if name in ("v4", "v2"):
            out[f"mix_{name}_dhidden"] = _np(dh)
        if name == "v4":
            for k, v in pg.items():
                out[f"mix_{name}_g_{k}"] = _np(v)
    (o,), _, _ = _module_run(v4, hidden, (cot,))
    out["mix_v4_L257_out"] = _np(o)
    return state


def record_blocks(out, layer, ln, state):
    mk = lambda i: layer.MambaBlock(24, i, "v2", norm_cls=partial(ln.RMSNorm, eps=EPS), fused_add_norm=True, residual_in_fp32=True,
                                    ssm_cfg={"bimamba_type": "v2"})
    b1, b2 = mk(0), mk(1)
    g = torch.Generator().manual_seed(15)
    with torch.no_grad():                                # RMSNorm starts at ones, which would hide the weight product
        for i, b in ((1, b1), (2, b2)):
            b.mixer.load_state_dict(state)               # both mixers are mix_w_*
            b.norm.weight.add_(0.3 * torch.randn(24, generator=g))
            assert b.norm.bias is None and b.norm.eps == EPS
            out[f"block_w{i}_norm.weight"] = _np(b.norm.weight)
    hidden = torch.randn(2, 37, 24, generator=g) + 0.5 * SR._wave((2, 37, 24), 1.1, 0.07, 0.4).float()
    cots = tuple(torch.randint(-8, 9, (2, 37, 24), generator=g).float() / 4 for _ in range(2))
    h = hidden.clone().requires_grad_(True)
    h1, r1 = b1(h, None)
    h2, r2 = b2(h1, r1)
    ((h2 * cots[0]).sum() + (r2 * cots[1]).sum()).backward()
    out.update(block_hidden_in=_np(hidden), block_cot_hidden=_np(cots[0]), block_cot_residual=_np(cots[1]), block_hidden=_np(h2),
               block_residual=_np(r2), block_dhidden_in=_np(h.grad))
    for k, p in b1.named_parameters():
        out[f"block_g1_{k}"] = _np(p.grad)
    out["block_g2_norm.weight"] = _np(b2.norm.weight.grad)


def main():
    simple, layer, fns = load_reference()
    ssi, ln = fns["mamba_ssm"][0], fns["mamba_ssm"][1]
    out = {"eps": np.float64(EPS)}
    record_scan(out, ssi)
    record_conv(out, fns["causal_conv1d_ref"])
    record_norm(out, ln)
    state = record_mixers(out, simple)
    record_blocks(out, layer, ln, state)
    path = os.path.join(OUT, "g14_mamba.npz")
    np.savez_compressed(path, **out)
    groups = {}
    for k, v in out.items():
        groups[k.split("_")[0]] = groups.get(k.split("_")[0], 0) + v.nbytes
    print("keys:", " ".join(sorted(out)))
    print("raw bytes per group:", groups)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "keys")


if __name__ == "__main__":
    main()
