#!/usr/bin/env python3
"""Generates tests/golden/g26_batchnorm.npz: the reference's OWN BasicBlock (pointcept/models/sparse_unet/spconv_unet_v1m1_base.py:25-104)
and its conv_input-style SparseSequential (:153-164: SubMConv3d k=5, BatchNorm1d(eps=1e-3, momentum=0.01), ReLU), run in fp64 on the CPU,
one training step each (forward, backward, running buffers after it), plus a PTv3 Embedding-style stem (the same sequence with nn.GELU,
point_transformer_v3m1_base.py:501-514) and the ReLU stem once more in eval mode.  For unipre3d_amd/batchnorm.py.

Stubs (the stubbing of make_g12_ptv3_boundary.py): spconv.pytorch (SparseConvTensor, SparseModule, a SparseSequential that hands plain
modules the features, and a SubMConv3d that applies tests/spconv_ref.subm over tests/spconv_ref.subm_table), torch_geometric's scatter,
timm's trunc_normal_, pointcept.models.utils.offset2batch and fusion.point_fusion (all unused here).

Recorded per module case `<m>`: <m>_indices, <m>_spatial_shape, <m>_x, <m>_dout, <m>_out, <m>_dx, <m>_p_<key> (the state_dict before
the step) / <m>_after_<key> (the buffers after it), <m>_d_<key> (every parameter's gradient), <m>_keys (the state_dict key list).
Per BatchNorm inside them, case `<c>` of `cases`: <c>_x, <c>_y, <c>_dy, <c>_dx, <c>_residual / <c>_dresidual (where there is one), <c>_gamma, <c>_beta,
<c>_rm0, <c>_rv0, <c>_nbt0, <c>_rm1, <c>_rv1, <c>_nbt1, <c>_dgamma, <c>_dbeta, <c>_act, <c>_training; eps and momentum once.
Only arrays and names are stored.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import spconv_ref  # noqa: E402

EPS, MOMENTUM = 1e-3, 0.01


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size

    def replace_feature(self, f):
        return SparseConvTensor(f, self.indices, self.spatial_shape, self.batch_size)


class SparseModule(nn.Module):
    pass


class SparseSequential(nn.Sequential):
    def forward(self, input):
        for module in self:
            input = module(input) if isinstance(module, SparseModule) else input.replace_feature(module(input.features))
        return input


class SubMConv3d(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        super().__init__()
        k = kernel_size
        self.k = k
        self.weight = nn.Parameter(torch.empty(out_channels, k, k, k, in_channels, dtype=torch.float64).uniform_(-1, 1) / np.sqrt(in_channels * k))
        self.bias = nn.Parameter(torch.zeros(out_channels, dtype=torch.float64)) if bias else None

    def forward(self, x):
        table = spconv_ref.subm_table(x.indices.numpy(), x.spatial_shape, self.k)
        return x.replace_feature(spconv_ref.subm(x.features, self.weight, self.bias, table))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _sites(rng, n, shape, batch):
    cells = rng.choice(batch * shape[0] * shape[1] * shape[2], size=n, replace=False)
    idx = np.stack(np.unravel_index(np.sort(cells), (batch,) + tuple(shape)), 1).astype(np.int32)
    return torch.from_numpy(idx)


def _unsettle(module, gen):
    """No BatchNorm at its default: gamma in [0.5, 1.5] with some negative, beta, running statistics, a count of 3."""
    for m in module.modules():
        if isinstance(m, nn.BatchNorm1d):
            c = m.num_features
            with torch.no_grad():
                m.weight.copy_((0.5 + torch.rand(c, generator=gen, dtype=torch.float64)) * torch.where(torch.arange(c) % 5 == 3, -1.0, 1.0))
                m.bias.copy_(torch.randn(c, generator=gen, dtype=torch.float64) * 0.3)
                m.running_mean.copy_(torch.randn(c, generator=gen, dtype=torch.float64) * 0.3)
                m.running_var.copy_(0.5 + torch.rand(c, generator=gen, dtype=torch.float64))
                m.num_batches_tracked.fill_(3)


class _Tap:
    """What goes into and comes out of one module, call by call, with gradients retained."""

    def __init__(self, module, pick=lambda t: t):
        self.calls = []
        module.register_forward_hook(self._hook)
        self.pick = pick

    def _hook(self, module, inputs, output):
        i, o = self.pick(inputs[0]), self.pick(output)
        for t in (i, o):
            if t.requires_grad and not t.is_leaf:
                t.retain_grad()
        self.calls.append((i, o))


def _bn_before(bn):
    return dict(gamma=bn.weight.detach().clone(), beta=bn.bias.detach().clone(), rm0=bn.running_mean.clone(), rv0=bn.running_var.clone(),
                nbt0=bn.num_batches_tracked.clone())


def _bn_case(rec, name, bn, before, x, y, act, training, residual=None):
    a = lambda t: t.detach().numpy().copy()
    rec["cases"].append(name)
    for k, v in before.items():
        rec[f"{name}_{k}"] = a(v)
    rec.update({f"{name}_x": a(x), f"{name}_y": a(y), f"{name}_dy": a(y.grad), f"{name}_dx": a(x.grad), f"{name}_dgamma": a(bn.weight.grad),
                f"{name}_dbeta": a(bn.bias.grad), f"{name}_rm1": a(bn.running_mean), f"{name}_rv1": a(bn.running_var),
                f"{name}_nbt1": a(bn.num_batches_tracked), f"{name}_act": np.asarray(act), f"{name}_training": np.asarray(training)})
    if residual is not None:
        rec[f"{name}_residual"], rec[f"{name}_dresidual"] = a(residual), a(residual.grad)


def _run(rec, name, module, x, training, gen):
    """One step of `module` on the sparse tensor x; the module-level record."""
    a = lambda t: t.detach().numpy().copy()
    module.train(training)
    for k, v in module.state_dict().items():
        rec[f"{name}_p_{k}"] = a(v)
    rec[f"{name}_keys"] = np.asarray(list(module.state_dict().keys()))
    out = module(x)
    dout = torch.randn(out.features.shape, generator=gen, dtype=torch.float64)
    out.features.retain_grad()
    out.features.backward(dout)
    rec.update({f"{name}_indices": x.indices.numpy(), f"{name}_spatial_shape": np.asarray(x.spatial_shape, np.int64),
                f"{name}_batch_size": np.int64(x.batch_size), f"{name}_x": a(x.features), f"{name}_dout": a(dout),
                f"{name}_out": a(out.features), f"{name}_dx": a(x.features.grad), f"{name}_training": np.asarray(training)})
    for k, v in module.named_buffers():
        rec[f"{name}_after_{k}"] = a(v)
    for k, p in module.named_parameters():
        rec[f"{name}_d_{k}"] = a(p.grad)
    return out


def main():
    sp = _stub("spconv")
    sp.pytorch = _stub("spconv.pytorch", SparseConvTensor=SparseConvTensor, SparseModule=SparseModule, SparseSequential=SparseSequential,
                       SubMConv3d=SubMConv3d)
    _stub("torch_geometric")
    _stub("torch_geometric.utils", scatter=None)
    _stub("timm")
    _stub("timm.models")
    _stub("timm.models.layers", trunc_normal_=None)
    _stub("pointcept")
    _stub("pointcept.models")
    _stub("pointcept.models.utils", offset2batch=None)
    _stub("fusion")
    _stub("fusion.point_fusion", PointFusion=object)
    ref = _load("spunet_ref", "pointcept/models/sparse_unet/spconv_unet_v1m1_base.py")

    torch.set_default_dtype(torch.float64)
    gen = torch.Generator().manual_seed(26)
    rng = np.random.default_rng(26)
    norm_fn = lambda c: nn.BatchNorm1d(c, eps=EPS, momentum=MOMENTUM)
    rec = {"cases": [], "modules": [], "eps": np.float64(EPS), "momentum": np.float64(MOMENTUM)}

    def sparse(n, cin, shape=(6, 6, 6), batch=2):
        f = (torch.randn(n, cin, generator=gen) + torch.linspace(-1, 1, cin)).requires_grad_(True)
        return SparseConvTensor(f, _sites(rng, n, shape, batch), list(shape), batch)

    # the reference's BasicBlock, in == embed (proj is the identity) and in != embed (proj = 1x1 conv + norm)
    for name, cin, cout in (("block_same", 8, 8), ("block_proj", 6, 10)):
        block = ref.BasicBlock(cin, cout, norm_fn=norm_fn, indice_key="k")
        _unsettle(block, gen)
        feats = lambda t: t.features if isinstance(t, SparseConvTensor) else t
        taps = {k: _Tap(getattr(block, k), feats) for k in ("bn1", "bn2", "relu", "proj")}
        if cin != cout:
            taps["proj.1"] = _Tap(block.proj[1])
        before = {k: _bn_before(m) for k, m in (("bn1", block.bn1), ("bn2", block.bn2))}
        if cin != cout:
            before["proj.1"] = _bn_before(block.proj[1])
        _run(rec, name, block, sparse(80, cin), True, gen)
        rec["modules"].append(name)
        _bn_case(rec, name + "_bn1", block.bn1, before["bn1"], taps["bn1"].calls[0][0], taps["relu"].calls[0][1], "relu", True)
        # (with the identity proj the residual IS the block's input, whose gradient also holds conv1's share: no dresidual record)
        residual = taps["proj"].calls[0][1] if cin != cout else None
        _bn_case(rec, name + "_bn2", block.bn2, before["bn2"], taps["bn2"].calls[0][0], taps["relu"].calls[1][1], "relu", True, residual)
        if cin == cout:
            rec[name + "_bn2_residual"] = taps["proj"].calls[0][1].detach().numpy().copy()
        else:
            x_p, y_p = taps["proj.1"].calls[0]
            _bn_case(rec, name + "_projnorm", block.proj[1], before["proj.1"], x_p, y_p, "none", True)

    # conv_input-style stems: ReLU (SpUNet) in training and eval mode, GELU (PTv3's Embedding)
    for name, act, training in (("stem_relu", nn.ReLU, True), ("stem_relu_eval", nn.ReLU, False), ("stem_gelu", nn.GELU, True)):
        stem = SparseSequential(SubMConv3d(3, 12, kernel_size=5, padding=1, bias=False, indice_key="stem"), norm_fn(12), act())
        _unsettle(stem, gen)
        bn_tap, act_tap = _Tap(stem[1]), _Tap(stem[2])
        before = _bn_before(stem[1])
        _run(rec, name, stem, sparse(100, 3), training, gen)
        rec["modules"].append(name)
        _bn_case(rec, name + "_bn", stem[1], before, bn_tap.calls[0][0], act_tap.calls[0][1], "relu" if act is nn.ReLU else "gelu", training)

    rec["cases"], rec["modules"] = np.asarray(rec["cases"]), np.asarray(rec["modules"])
    np.savez_compressed(os.path.join(OUT, "g26_batchnorm.npz"), **rec)
    print("wrote g26_batchnorm.npz:", list(rec["cases"]), list(rec["modules"]), os.path.getsize(os.path.join(OUT, "g26_batchnorm.npz")), "bytes")


if __name__ == "__main__":
    main()
