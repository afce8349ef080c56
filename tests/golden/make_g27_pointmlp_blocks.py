#!/usr/bin/env python3
"""Generates tests/golden/g27_pointmlp_blocks.npz: the reference's OWN ConvBNReLU1D, ConvBNReLURes1D, PreExtraction and PosExtraction
(openpoints/models/backbone/pointmlp.py:198-353, openpoints/models/PCM/PointMLP_layers.py:112-225), run in fp64 on the CPU, one training
step each (forward, backward, running buffers after it) and one module once more in eval mode (there the module and its pooled norm
only; the file stays under 1 MiB).  For unipre3d_amd/batchnorm_cf.py.
The two files are loaded as make_g21_local_grouper.py loads them.

Module cases (`modules`): <m>_x, <m>_dout, <m>_out, <m>_dx, <m>_p_<key> (the state_dict before the step), <m>_after_<key> (the buffers
after it), <m>_d_<key> (every parameter's gradient), <m>_keys (the state_dict key list), <m>_kind, <m>_act, <m>_training.
Per BatchNorm inside them (`cases`, named <m>/<norm key>): <c>_x, <c>_y, <c>_dy, <c>_dx, <c>_residual (or <c>_residual_is, the case whose _y it is) / <c>_dresidual (the last norm
of a residual block), <c>_gamma, <c>_beta, <c>_rm0, <c>_rv0, <c>_nbt0, <c>_rm1, <c>_rv1, <c>_nbt1, <c>_dgamma, <c>_dbeta, <c>_act, <c>_training,
and for the norm in front of PreExtraction's max (<c>_pool = 1): <c>_pooled, <c>_dpooled (B, C), <c>_arg (int32) and <c>_mask (pooled > 0);
there <c>_y / <c>_dy are the dense tensor the reference wrote and the gradient its max scattered into it.  Only arrays and names.

Every BatchNorm is unsettled as make_g26_batchnorm.py does it.  Seeds are drawn until, in every pooled case, every row's maximum
pre-activation lies at least 64 x dev from zero and, where it is positive, at least 64 x dev above the row's second largest value,
dev being the largest absolute deviation of the fp32 restatement's pre-activation (tests/batchnorm_cf_ref.py) from fp64 on that case:
the reference's arg and mask are then the only admissible ones.  Both figures are printed and recorded (<c>_dev, <c>_margin).
"""
import os
import sys

import numpy as np
import torch
from torch import nn

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import batchnorm_cf_ref as R  # noqa: E402
import make_g21_local_grouper as g21  # noqa: E402
from make_g26_batchnorm import _Tap, _bn_before, _unsettle  # noqa: E402

EPS, MOMENTUM, MARGIN = 1e-5, 0.1, 64.0
# name: (file, class, constructor args, kwargs, input shape, training)
CASES = {
    "pre_k24": ("pointmlp", "PreExtraction", (4, 8), dict(blocks=2, bias=False, use_xyz=False), (2, 6, 24, 8), True),
    "pre_k24_eval": ("pointmlp", "PreExtraction", (4, 8), dict(blocks=2, bias=False, use_xyz=False), (2, 6, 24, 8), False),
    "pcm_pre_k32": ("pcm", "PreExtraction", (4, 8), dict(blocks=1, bias=True, use_xyz=True, knn_grouper=False), (2, 5, 32, 7), True),
    "pos": ("pointmlp", "PosExtraction", (8,), dict(blocks=2), (2, 8, 40), True),
    "cbr_l50": ("pointmlp", "ConvBNReLU1D", (4, 8), dict(), (2, 4, 50), True),
    "res_groups": ("pointmlp", "ConvBNReLURes1D", (8,), dict(groups=2, res_expansion=0.5), (3, 8, 12), True),
    "cbr_gelu": ("pcm", "ConvBNReLU1D", (4, 8), dict(activation="gelu"), (2, 4, 50), True),
}


def _a(t):
    return t.detach().numpy().copy()


def run_case(rec, name, mods, seed):
    """One step of one case into rec; -> (dev, margin) of its pooled norm, or None."""
    file, cls, args, kw, shape, training = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    module = getattr(mods[file], cls)(*args, **kw)
    _unsettle(module, gen)
    module.train(training)
    act = "gelu" if kw.get("activation") == "gelu" else "relu"
    norms = {k: m for k, m in module.named_modules() if isinstance(m, nn.BatchNorm1d)}
    taps = {k: _Tap(m) for k, m in norms.items()}
    blocks = {k: _Tap(m) for k, m in module.named_modules() if type(m).__name__ in ("ConvBNReLURes1D", "ConvBNReLU1D")}
    if type(module).__name__ in ("ConvBNReLURes1D", "ConvBNReLU1D"):
        blocks[""] = _Tap(module)
    before = {k: _bn_before(m) for k, m in norms.items()}
    for k, v in module.state_dict().items():
        rec[f"{name}_p_{k}"] = _a(v)
    rec[f"{name}_keys"] = np.asarray(list(module.state_dict().keys()))
    x = (torch.randn(shape, generator=gen) + torch.linspace(-0.5, 0.5, shape[-1])).requires_grad_(True)
    out = module(x)
    dout = torch.randn(out.shape, generator=gen)
    out.backward(dout)
    rec.update({f"{name}_x": _a(x), f"{name}_dout": _a(dout), f"{name}_out": _a(out), f"{name}_dx": _a(x.grad),
                f"{name}_training": np.asarray(training), f"{name}_kind": np.asarray(cls), f"{name}_act": np.asarray(act)})
    for k, v in module.named_buffers():
        rec[f"{name}_after_{k}"] = _a(v)
    for k, p in module.named_parameters():
        rec[f"{name}_d_{k}"] = _a(p.grad)
    rec["modules"].append(name)

    pooled_norm = None
    if cls == "PreExtraction":
        pooled_norm = [k for k in norms][-1]
    for k, bn in norms.items():
        c = f"{name}/{k}"
        if k != pooled_norm and (not training or (file == "pcm" and k.startswith("transfer."))):
            continue                    # eval mode: the module and its pooled norm only; PCM's transfer has the shape of its net1.1
        owner = k.rsplit(".", 2)[0] if k.count(".") >= 2 else ""              # the ConvBNReLU(Res)1D that holds the norm
        xin, o = taps[k].calls[0]
        last_of_res = k.endswith("net2.4") or (k.endswith("net2.1") and not any(q == k[:-1] + "4" for q in norms))
        residual = None
        if last_of_res:
            residual, y = blocks[owner].calls[0]
        elif act == "gelu":
            y = blocks[owner].calls[0][1]
        else:
            y = o                                                              # (the in-place ReLU made it the activation's output)
        rec["cases"].append(c)
        for q, v in before[k].items():
            rec[f"{c}_{q}"] = _a(v)
        rec.update({f"{c}_x": _a(xin), f"{c}_y": _a(y), f"{c}_dy": _a(y.grad), f"{c}_dx": _a(xin.grad), f"{c}_dgamma": _a(bn.weight.grad),
                    f"{c}_dbeta": _a(bn.bias.grad), f"{c}_rm1": _a(bn.running_mean), f"{c}_rv1": _a(bn.running_var),
                    f"{c}_nbt1": _a(bn.num_batches_tracked), f"{c}_act": np.asarray(act), f"{c}_training": np.asarray(training),
                    f"{c}_pool": np.asarray(int(k == pooled_norm))})
        if residual is not None:
            rec[f"{c}_dresidual"] = _a(o.grad)                                 # d(bn output) = d(bn output + x) = g
            same = [q for q in rec["cases"][:-1] if np.array_equal(rec[f"{q}_y"], _a(residual))]
            if same:
                rec[f"{c}_residual_is"] = np.asarray(same[0])                  # the y of that case, not stored twice
            else:
                rec[f"{c}_residual"] = _a(residual)
    if pooled_norm is None:
        return None
    c = f"{name}/{pooled_norm}"
    b, n = shape[0], shape[1]
    y = rec[f"{c}_y"]
    pooled = _a(out).transpose(0, 2, 1).reshape(b * n, -1)
    assert np.array_equal(pooled, y.max(2))
    rec.update({f"{c}_pooled": pooled, f"{c}_dpooled": _a(dout).transpose(0, 2, 1).reshape(b * n, -1).copy(),
                f"{c}_arg": y.argmax(2).astype(np.int32), f"{c}_mask": pooled > 0})
    # the margins, from the restatement's pre-activation in fp64 and its fp32 deviation from it
    sd = {k[len(name) + 3:]: v for k, v in rec.items() if k.startswith(name + "_p_")}
    z = {}
    for dtype in (np.float64, np.float32):
        tape = R.Tape(sd, training=training, act=act, dtype=dtype, eps=EPS, momentum=MOMENTUM)
        got, _ = tape.pre_extraction(rec[f"{name}_x"])
        z[dtype] = tape.norms[pooled_norm]["z"].astype(np.float64)
        if dtype == np.float64:
            assert np.abs(got - rec[f"{name}_out"]).max() < 1e-12
    dev = float(np.abs(z[np.float32] - z[np.float64]).max())
    top = np.sort(z[np.float64], axis=2)
    first, second = top[:, :, -1], top[:, :, -2]
    margin = float(min(np.abs(first).min(), np.where(first > 0, first - second, np.inf).min()))
    rec[f"{c}_dev"], rec[f"{c}_margin"] = np.float64(dev), np.float64(margin)
    return dev, margin


def main():
    g21.load_reference()
    mods = {"pointmlp": sys.modules["g21.backbone.pointmlp"], "pcm": sys.modules["g21.PCM.PointMLP_layers"]}
    torch.set_default_dtype(torch.float64)
    rec = {"cases": [], "modules": [], "eps": np.float64(EPS), "momentum": np.float64(MOMENTUM)}
    for i, name in enumerate(CASES):
        seed = 2700 + 100 * i
        while True:
            trial = {"cases": [], "modules": []}
            m = run_case(trial, name, mods, seed)
            if m is None or m[1] >= MARGIN * m[0]:
                break
            print(f"{name}: seed {seed} rejected (deviation {m[0]:.3e}, margin {m[1]:.3e})")
            seed += 1
        rec["cases"] += trial.pop("cases")
        rec["modules"] += trial.pop("modules")
        rec.update(trial)
        rec[f"{name}_seed"] = np.int64(seed)
        if m is not None:
            print(f"{name}: seed {seed}, fp32 pre-activation deviation {m[0]:.3e}, margin kept {m[1]:.3e} = {m[1] / m[0]:.0f} x")
    rec["cases"], rec["modules"] = np.asarray(rec["cases"]), np.asarray(rec["modules"])
    path = os.path.join(OUT, "g27_pointmlp_blocks.npz")
    np.savez_compressed(path, **rec)
    print("wrote g27_pointmlp_blocks.npz:", len(rec["cases"]), "norm cases,", list(rec["modules"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
