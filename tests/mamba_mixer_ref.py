"""The Mamba mixers of the two backbones and PCM's block, restated around an `ops` namespace, in the dtype of their inputs.

    xz = in_proj(hidden) as (B, 2 d_inner, L), x in the first d_inner channels and z in the last
    none   out_proj(inner(xz))                                                      one direction, out_proj inside mamba_inner_fn
    v2     out_proj(inner(xz) + inner_b(xz.flip(-1)).flip(-1))                      PCM: the second direction runs back in TIME
    v4     out_proj(inner(xz) + inner_b(xz.flip(-2)).flip(-2))                      Mamba3D: the second direction runs on the CHANNEL axis
                                                                                    reversed, so z (reversed) is convolved and scanned and
                                                                                    x (reversed) gates it
    slow   conv + SiLU, x_proj split into dt | B | C, dt_proj's weight, the scan gated by z, out_proj, spelled out call by call
    block  (h, r) = rms_norm_fn(hidden, norm.weight, None, residual, prenorm=True, eps);  hidden' = mixer(h);  returns (hidden', r)

`ops` holds selective_scan_fn, mamba_inner_fn_no_out_proj, mamba_inner_fn, causal_conv1d_fn, rms_norm_fn and layer_norm_fn with
mamba_ssm's argument lists.  restated_ops() are the CPU restatements (tests/selective_scan_ref.py, tests/mambaops_ref.py): in fp64 the
arbiter, in fp32 the yardstick.  product_ops() are unipre3d_amd's, so that the same lines call the product with the views the
backbones hand it: xz as the permuted view of the in_proj product, flipped copies, chunk views, conv1d.weight as (d_inner, 1, W).
Weights come as a plain dict under the backbones' state_dict names.  tests/golden/g14_mamba.npz pins all of it to the backbones' code.
"""
import types

import numpy as np
import torch
import torch.nn.functional as F

import mambaops_ref as M
import selective_scan_ref as S

FLIP_AXIS = {"v2": -1, "v4": -2}
MIXER_KINDS = ("v4", "v2", "none", "slow")


def restated_ops():
    def no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B=None, C=None, D=None, delta_bias=None,
                    B_proj_bias=None, C_proj_bias=None, delta_softplus=True):
        assert B is None and C is None and B_proj_bias is None and C_proj_bias is None
        return S.mamba_inner_no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, D, delta_bias, delta_softplus)

    def with_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, B=None,
                      C=None, D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True):
        y = no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B, C, D, delta_bias, B_proj_bias, C_proj_bias,
                        delta_softplus)
        return F.linear(y.transpose(1, 2), out_proj_weight, out_proj_bias)

    def rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6):
        return M.rms_norm(x, weight, bias, residual, prenorm, eps)

    def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False):
        return M.layer_norm(x, weight, bias, residual, eps, prenorm, is_rms_norm)

    return types.SimpleNamespace(selective_scan_fn=S.selective_scan, mamba_inner_fn_no_out_proj=no_out_proj, mamba_inner_fn=with_out_proj,
                                 causal_conv1d_fn=M.causal_conv1d, rms_norm_fn=rms_norm_fn, layer_norm_fn=layer_norm_fn)


def product_ops():
    from unipre3d_amd import causal_conv1d, layernorm, selective_scan
    return types.SimpleNamespace(selective_scan_fn=selective_scan.selective_scan_fn,
                                 mamba_inner_fn_no_out_proj=selective_scan.mamba_inner_fn_no_out_proj,
                                 mamba_inner_fn=selective_scan.mamba_inner_fn, causal_conv1d_fn=causal_conv1d.causal_conv1d_fn,
                                 rms_norm_fn=layernorm.rms_norm_fn, layer_norm_fn=layernorm.layer_norm_fn)


def _f(t):
    """The backbones' `.float()` on A_log, D and dt_proj.bias; the fp64 arbiter keeps its precision."""
    return t if t.dtype == torch.float64 else t.float()


def in_proj(w, hidden):
    """(B, L, d_model) -> xz (B, 2 d_inner, L), as the permuted view of one (2 d_inner, B L) product."""
    b, L, d = hidden.shape
    xz = (w["in_proj.weight"] @ hidden.reshape(b * L, d).t()).reshape(-1, b, L).transpose(0, 1)
    if w.get("in_proj.bias") is not None:
        xz = xz + w["in_proj.bias"].to(xz.dtype)[:, None]
    return xz


def _direction(ops, w, xz, s):
    """One mamba_inner_fn_no_out_proj call; s is "" for the forward set of weights and "_b" for the second one."""
    return ops.mamba_inner_fn_no_out_proj(xz, w[f"conv1d{s}.weight"], w[f"conv1d{s}.bias"], w[f"x_proj{s}.weight"], w[f"dt_proj{s}.weight"],
                                          -torch.exp(_f(w[f"A{s}_log"])), None, None, _f(w[f"D{s}"]),
                                          delta_bias=_f(w[f"dt_proj{s}.bias"]), delta_softplus=True)


def _slow(ops, w, xz):
    b, _, L = xz.shape
    rank, n = w["dt_proj.weight"].shape[1], w["A_log"].shape[1]
    x, z = xz.chunk(2, dim=1)
    x = ops.causal_conv1d_fn(x, w["conv1d.weight"].squeeze(1), w["conv1d.bias"], "silu")
    x_dbl = F.linear(x.transpose(1, 2).reshape(b * L, -1), w["x_proj.weight"])
    dt, Bm, Cm = torch.split(x_dbl, [rank, n, n], dim=-1)
    dt = (w["dt_proj.weight"] @ dt.t()).reshape(-1, b, L).transpose(0, 1)
    Bm = Bm.reshape(b, L, n).transpose(1, 2).contiguous()
    Cm = Cm.reshape(b, L, n).transpose(1, 2).contiguous()
    y = ops.selective_scan_fn(x, dt, -torch.exp(_f(w["A_log"])), Bm, Cm, _f(w["D"]), z=z, delta_bias=_f(w["dt_proj.bias"]),
                              delta_softplus=True, return_last_state=False)
    return F.linear(y.transpose(1, 2), w["out_proj.weight"], w.get("out_proj.bias"))


def mixer(ops, w, hidden, kind, flip_axis=None):
    """hidden (B, L, d_model) -> (B, L, d_model).  flip_axis overrides the kind's own axis (the tests use it to show that they see it)."""
    xz = in_proj(w, hidden)
    if kind == "slow":
        return _slow(ops, w, xz)
    if kind == "none":
        return ops.mamba_inner_fn(xz, w["conv1d.weight"], w["conv1d.bias"], w["x_proj.weight"], w["dt_proj.weight"], w["out_proj.weight"],
                                  w.get("out_proj.bias"), -torch.exp(_f(w["A_log"])), None, None, _f(w["D"]),
                                  delta_bias=_f(w["dt_proj.bias"]), delta_softplus=True)
    axis = FLIP_AXIS[kind] if flip_axis is None else flip_axis
    out = _direction(ops, w, xz, "") + _direction(ops, w, xz.flip([axis]), "_b").flip([axis])
    return F.linear(out.transpose(1, 2), w["out_proj.weight"], w.get("out_proj.bias"))


def block(ops, w, hidden, residual=None, kind="v2", eps=1e-5):
    """PCM's block (fused add + RMSNorm, the residual kept): w holds "norm.weight" and the mixer's weights under "mixer."."""
    h, r = ops.rms_norm_fn(hidden, w["norm.weight"], w.get("norm.bias"), residual=residual, prenorm=True, residual_in_fp32=True, eps=eps)
    return mixer(ops, {k[len("mixer."):]: v for k, v in w.items() if k.startswith("mixer.")}, h, kind), r


def two_blocks(ops, w1, w2, hidden, kind="v2"):
    h, r = block(ops, w1, hidden, None, kind)
    return block(ops, w2, h, r, kind)


def run_with_grads(fn, tensors, douts):
    """tensors: dict name -> tensor; fn(dict of leaves) -> tensor or tuple.  Returns ([outs], {name: grad or None})."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in tensors.items()}
    outs = fn(leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * d.to(o.device, o.dtype)).sum() for o, d in zip(outs, douts)).backward()
    return [o.detach() for o in outs], {k: (None if v.grad is None else v.grad.detach()) for k, v in leaves.items()}


# ---- readers of tests/golden/g14_mamba.npz (g is the opened file) ---------------------------------------------------------------------
SCAN_CASES = [("g0_sp", "3", True, ()), ("g0_raw", "3", False, ()), ("g2_sp", "4", True, ()), ("g2_raw", "4", False, ()),
              ("g0_sp_noD", "3", True, ("D",)), ("g0_sp_noz", "3", True, ("z",)), ("g0_sp_nobias", "3", True, ("delta_bias",))]
MIX_WEIGHTS = ("in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D",
               "A_b_log", "conv1d_b.weight", "conv1d_b.bias", "x_proj_b.weight", "dt_proj_b.weight", "dt_proj_b.bias", "D_b", "out_proj.weight")


def _t(g, key, dtype=torch.float64):
    return torch.from_numpy(np.asarray(g[key])).to(dtype)


def scan_inputs(g, tag, softplus, absent, dtype=torch.float64):
    sp = "sp" if softplus else "raw"
    t = {"u": _t(g, "scan_in_u", dtype), "delta": _t(g, "scan_in_delta_" + sp, dtype), "A": _t(g, "scan_in_A", dtype),
         "B": _t(g, "scan_in_B" + tag, dtype), "C": _t(g, "scan_in_C" + tag, dtype), "D": _t(g, "scan_in_D", dtype),
         "z": _t(g, "scan_in_z", dtype), "delta_bias": _t(g, "scan_in_bias_" + sp, dtype)}
    for k in absent:
        t[k] = None
    return t, _t(g, "scan_in_dout", dtype)


def mix_weights(g, dtype=torch.float64, prefix="mix_w_"):
    """The recorded state_dict of the mixer, under its own names."""
    return {k: _t(g, prefix + k, dtype) for k in MIX_WEIGHTS}


def mixer_run(ops, weights, hidden, cot, kind, device="cpu", dtype=torch.float64, flip_axis=None):
    t = {k: v.to(device=device, dtype=dtype) for k, v in {**weights, "hidden": hidden}.items()}
    (out,), grads = run_with_grads(lambda q: mixer(ops, q, q["hidden"], kind, flip_axis), t, (cot,))
    return out, grads


def block_weights(g, i, dtype=torch.float64):
    w = {"mixer." + k: v for k, v in mix_weights(g, dtype).items()}
    w["norm.weight"] = _t(g, f"block_w{i}_norm.weight", dtype)
    return w


def blocks_run(ops, g, device="cpu", dtype=torch.float64):
    """The two recorded blocks chained: ([hidden, residual], gradients under "hidden" and "{1|2}.{state_dict name}")."""
    t = {"hidden": _t(g, "block_hidden_in")}
    for i in (1, 2):
        t.update({f"{i}.{k}": v for k, v in block_weights(g, i).items()})
    t = {k: v.to(device=device, dtype=dtype) for k, v in t.items()}
    pick = lambda q, i: {k[2:]: v for k, v in q.items() if k.startswith(f"{i}.")}
    return run_with_grads(lambda q: two_blocks(ops, pick(q, 1), pick(q, 2), q["hidden"]), t,
                          (_t(g, "block_cot_hidden"), _t(g, "block_cot_residual")))
