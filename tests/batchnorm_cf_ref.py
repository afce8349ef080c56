"""Restatement of the channels-first fused BatchNorm + activation + residual + max over L (unipre3d_amd/batchnorm_cf.py,
csrc/u3d_batchnorm_cf.hip) and of the reference's four modules built from it, in numpy.  (A plain helper module;
tests/test_batchnorm_cf_ref.py holds it to the reference's record, tests/golden/g27_pointmlp_blocks.npz.)

  forward / backward   dtype=np.float64: the arithmetic itself.  dtype=np.float32: every (B, C, L) tensor in fp32, one rounding per
                       operation and no contraction, in the kernels' order: y = act((x - mean) (invstd gamma) + beta [+ residual]);
                       the sums in f64 per lane (batch entries, sweeps and the lane's floats in ascending order), a butterfly over the
                       row's lanes, the batch lanes in ascending order (part_sums), then tests/batchnorm_ref.sum_partials over the parts;
                       mean, invstd and the running statistics in f64 from the block, rounded once.
                       pool=True: pooled (B, C) = max over L, arg = the lowest l that attains it, mask = pooled > 0 (relu);
                       decisions=(arg, mask) overrides both, so that an fp32 evaluation can be checked under the decisions it took.
  plan(C, L, aligned)  the kernels' dispatch class (u3d_bncf_plan), restated
  conv1d / Tape        a plain k = 1 (grouped) convolution and the four modules' forward and backward over a state_dict
"""
from __future__ import annotations

import collections
import os

import numpy as np

from batchnorm_ref import _act, _g, rel, sum_partials  # noqa: F401  (rel is re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g27_pointmlp_blocks.npz")
TOLERANCE = os.path.join(os.path.dirname(HERE), "profiles", "batchnorm_cf", "tolerance.json")
QUANTITIES = ("y", "dx", "dresidual", "dgamma", "dbeta", "running_mean", "running_var")
NT, MAXG, CHUNK_FLOATS, MAX_CHUNK = 256, 64, 8192, 4096

Plan = collections.namedtuple("Plan", "lanes_per_row channel_tile batch_chunk vec sweeps")


def plan(C, L, aligned=True):
    V = 4 if aligned and L % 4 == 0 else 1
    units = -(-L // V)
    G = 1
    while G < units and G < MAXG:
        G *= 2
    R = NT // G
    return Plan(G, min(C, R), min(max(CHUNK_FLOATS // (min(C, 32) * L), 1), MAX_CHUNK), V, -(-units // G))


def parts(B, C, L):
    return -(-B // plan(C, L).batch_chunk)


def part_sums(a, b, wide=None):
    """(parts, 2C) f64: per batch chunk the per-channel sums of a and of b (B, C, L), added as a workgroup adds them."""
    B, C, L = a.shape
    p = plan(C, L, (L % 4 == 0) if wide is None else wide)
    G, V, BC = p.lanes_per_row, p.vec, p.batch_chunk
    BS = (NT // G) // p.channel_tile
    lanes = [[l + j for l in range(gl * V, L, G * V) for j in range(V)] for gl in range(G)]
    out = []
    for b0 in range(0, B, BC):
        part = np.zeros(2 * C)
        for k, t in enumerate((a, b)):
            rows = np.asarray(t[b0:b0 + BC], np.float64)
            acc = np.zeros(C)
            for bs in range(BS):
                sub = rows[bs::BS]
                lane = np.zeros((G, C))
                for gl, idx in enumerate(lanes):
                    if idx and len(sub):
                        lane[gl] = np.cumsum(sub[:, :, idx].transpose(1, 0, 2).reshape(C, -1), axis=1)[:, -1]
                o = G // 2
                while o:
                    lane = lane + lane[np.arange(G) ^ o]
                    o //= 2
                acc = acc + lane[0]
            part[k * C:(k + 1) * C] = acc
        out.append(part)
    return np.stack(out)


def part_sums_pooled(a, b, L):
    """The pooled backward's partials: a, b (B, C) f64, one thread per channel, the chunk's batch entries in ascending order."""
    B, C = a.shape
    BC = plan(C, L).batch_chunk
    return np.stack([np.concatenate([np.cumsum(np.asarray(t[b0:b0 + BC], np.float64), axis=0)[-1] for t in (a, b)]) for b0 in range(0, B, BC)])


def to_groups(p, S):
    """(B, C) -> the (B / S, C, S) tensor of pool_groups = S."""
    B, C = p.shape
    return p if S == 1 else np.ascontiguousarray(p.reshape(B // S, S, C).transpose(0, 2, 1))


def from_groups(p, S):
    return p if S == 1 else np.ascontiguousarray(p.transpose(0, 2, 1).reshape(-1, p.shape[1]))


def forward(x, gamma, beta, running_mean=None, running_var=None, nbt=None, *, training, momentum, eps, act="none", residual=None,
            pool=False, decisions=None, dtype=np.float64, stat_reduce=None, wide=None):
    """-> dict: y (dense), z (the pre-activation), with pool also pooled, arg (B, C) and mask; mean, invstd, a, running_mean, running_var,
    nbt (after the step), and what backward() needs."""
    t = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    B, C, L = x.shape
    sh = (1, C, 1)
    gamma = np.ones(C, dtype) if gamma is None else np.asarray(gamma, dtype)
    beta = np.zeros(C, dtype) if beta is None else np.asarray(beta, dtype)
    rm = None if running_mean is None else np.asarray(running_mean, dtype).copy()
    rv = None if running_var is None else np.asarray(running_var, dtype).copy()
    count = float(B * L)
    if training:
        if dtype == np.float64 and stat_reduce is None:
            mean = x.mean((0, 2))
            var = ((x - mean.reshape(sh)) ** 2).mean((0, 2))
        else:
            xd = x.astype(np.float64)
            block = sum_partials(part_sums(xd, xd * xd, wide), count) if dtype == np.float32 else \
                np.concatenate([[count], xd.sum((0, 2)), (xd * xd).sum((0, 2))])
            if stat_reduce is not None:
                block = stat_reduce(block.copy())
            count = block[0]
            mean = block[1:1 + C] / count
            var = np.maximum(block[1 + C:] / count - mean * mean, 0.0)
        invstd = 1.0 / np.sqrt(var + float(eps))
        if nbt is not None and rm is not None:
            nbt = int(nbt) + 1
        if rm is not None:
            f = 1.0 / nbt if momentum is None else float(momentum)
            unbiased = var * (count / (count - 1.0)) if count > 1 else var
            rm = ((1.0 - f) * rm.astype(np.float64) + f * mean).astype(dtype)
            rv = ((1.0 - f) * rv.astype(np.float64) + f * unbiased).astype(dtype)
        mean, invstd = mean.astype(dtype), invstd.astype(dtype)
    else:
        mean, invstd = rm, (t(1) / np.sqrt(rv + t(eps))).astype(dtype)
    a = invstd * gamma
    z = (x - mean.reshape(sh)) * a.reshape(sh) + beta.reshape(sh)
    if residual is not None:
        z = z + np.asarray(residual, dtype)
    y = _act(z, act)
    out = dict(y=y, z=z, mean=mean, invstd=invstd, a=a, beta=beta, x=x, act=act, training=training, running_mean=rm, running_var=rv,
               nbt=nbt, dtype=dtype, stat_reduce=stat_reduce, wide=wide, count=count, pool=pool, has_residual=residual is not None)
    if pool:
        arg = np.argmax(y, axis=2).astype(np.int32) if decisions is None else np.asarray(decisions[0], np.int32)
        pooled = np.take_along_axis(y, arg[:, :, None].astype(np.int64), 2)[:, :, 0]
        mask = (pooled > 0) if decisions is None or decisions[1] is None else np.asarray(decisions[1], bool)
        out.update(pooled=pooled, arg=arg, mask=mask)
    return out


def backward(f, dy):
    """dy: (B, C, L), or with pool the (B, C) gradient of pooled.  -> dict: dx, dgamma, dbeta (this process's sums), dresidual."""
    dtype, x, act = f["dtype"], f["x"], f["act"]
    dy = np.asarray(dy, dtype)
    B, C, L = x.shape
    sh = (1, C, 1)
    mean, invstd, a = (f[k].reshape(sh) for k in ("mean", "invstd", "a"))
    xhat = (x - mean) * invstd
    if f["pool"]:
        at = f["arg"][:, :, None].astype(np.int64)
        xa = np.take_along_axis(x, at, 2)[:, :, 0]
        za = (xa - f["mean"]) * f["a"] + f["beta"]                                  # (gelu takes no residual)
        gp = np.where(f["mask"], dy, dtype(0)) if act == "relu" else _g(dy, za, None, act)
        g = np.zeros_like(x)
        np.put_along_axis(g, at, gp[:, :, None], 2)
        gd = gp.astype(np.float64)
        prod = gd * ((xa - f["mean"]) * f["invstd"]).astype(np.float64)
        partials = part_sums_pooled(gd, prod, L) if dtype == np.float32 else None
        sums = (gd.sum(0), prod.sum(0))
    else:
        z = (x - mean) * a + f["beta"].reshape(sh) if act == "gelu" else None
        g = _g(dy, z, f["y"], act)
        gd = g.astype(np.float64)
        prod = gd * xhat.astype(np.float64)
        partials = part_sums(gd, prod, f["wide"]) if dtype == np.float32 else None
        sums = (gd.sum((0, 2)), prod.sum((0, 2)))
    block = sum_partials(partials, B * L) if dtype == np.float32 else np.concatenate([[float(B * L)], *sums])
    dbeta, dgamma = block[1:1 + C].astype(dtype), block[1 + C:].astype(dtype)
    if f["training"]:
        if f["stat_reduce"] is not None:
            block = f["stat_reduce"](block.copy())
        b, d = (block[1:1 + C] / block[0]).astype(dtype), (block[1 + C:] / block[0]).astype(dtype)
        dx = a * ((g - b.reshape(sh)) - xhat * d.reshape(sh))
    else:
        dx = g * a
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dresidual=g if f["has_residual"] else None)


# ---- the four modules over a state_dict ---------------------------------------------------------------------------------------------

def conv1d(x, w, bias):
    """Conv1d(kernel_size=1, groups = C_in / w.shape[1]) -> (out, back(dout) -> (dx, dw, dbias))."""
    O, cg, _ = w.shape
    B, C, L = x.shape
    groups = C // cg
    og = O // groups
    xg, wg = x.reshape(B, groups, cg, L), w.reshape(groups, og, cg)
    out = np.einsum("goc,bgcl->bgol", wg, xg).reshape(B, O, L)
    if bias is not None:
        out = out + bias.reshape(1, O, 1)

    def back(d):
        dg = d.reshape(B, groups, og, L)
        return (np.einsum("goc,bgol->bgcl", wg, dg).reshape(B, C, L), np.einsum("bgol,bgcl->goc", dg, xg).reshape(w.shape),
                None if bias is None else d.sum((0, 2)))
    return out.astype(x.dtype), back


class Tape:
    """One training (or eval-mode) step of one of the four modules over the state_dict `sd` (numpy arrays under the reference's keys).
    After module(...) : .norms[<norm key>] is that norm's forward dict, .after the running buffers after the step; after the returned
    back(dout): .grads[<parameter key>] and .norm_dx[<conv key>], the gradient the norm behind that convolution hands it."""

    def __init__(self, sd, *, training, act="relu", dtype=np.float64, eps=1e-5, momentum=0.1, decisions=None):
        self.sd = {k: (np.asarray(v) if k.endswith("num_batches_tracked") else np.asarray(v, dtype)) for k, v in sd.items()}
        self.training, self.act, self.dtype, self.eps, self.momentum = training, act, dtype, eps, momentum
        self.decisions = decisions or {}
        self.norms, self.after, self.grads, self.norm_dx = {}, {}, {}, {}

    def conv_bn(self, conv, bn, x, residual=None, pool=False):
        sd = self.sd
        h, cback = conv1d(x, sd[conv + ".weight"], sd.get(conv + ".bias"))
        f = forward(h, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"],
                    sd[bn + ".num_batches_tracked"], training=self.training, momentum=self.momentum, eps=self.eps, act=self.act,
                    residual=residual, pool=pool, decisions=self.decisions.get(bn), dtype=self.dtype)
        self.norms[bn] = f
        self.after.update({bn + ".running_mean": f["running_mean"], bn + ".running_var": f["running_var"],
                           bn + ".num_batches_tracked": np.asarray(f["nbt"])})

        def back(d):
            g = backward(f, d)
            self.grads[bn + ".weight"], self.grads[bn + ".bias"] = g["dgamma"], g["dbeta"]
            self.norm_dx[conv] = g["dx"]                      # what the convolution in front receives: its bias gradient's terms
            dx, dw, db = cback(g["dx"])
            self.grads[conv + ".weight"] = dw
            if db is not None:
                self.grads[conv + ".bias"] = db
            return dx, g["dresidual"]
        return (f["pooled"] if pool else f["y"]), back

    def conv_bn_relu(self, prefix, x, pool=False):
        out, back = self.conv_bn(prefix + "net.0", prefix + "net.1", x, pool=pool)
        return out, lambda d: back(d)[0]

    def res_block(self, prefix, x, pool=False):
        h, b1 = self.conv_bn(prefix + "net1.0", prefix + "net1.1", x)
        b2 = None
        last = ("net2.0", "net2.1")
        if prefix + "net2.4.weight" in self.sd:
            h, b2 = self.conv_bn(prefix + "net2.0", prefix + "net2.1", h)
            last = ("net2.3", "net2.4")
        out, b3 = self.conv_bn(prefix + last[0], prefix + last[1], h, residual=x, pool=pool)

        def back(d):
            dh, dres = b3(d)
            if b2 is not None:
                dh = b2(dh)[0]
            return b1(dh)[0] + dres
        return out, back

    def blocks(self, prefix, x, pool=False):
        n = len({k[len(prefix):].split(".")[1] for k in self.sd if k.startswith(prefix + "operation.")})
        backs = []
        for i in range(n):
            x, b = self.res_block(f"{prefix}operation.{i}.", x, pool and i == n - 1)
            backs.append(b)

        def back(d):
            for b in reversed(backs):
                d = b(d)
            return d
        return x, back, n

    def pos_extraction(self, x):
        out, back, _ = self.blocks("", np.asarray(x, self.dtype))
        return out, back

    def pre_extraction(self, x):
        """x (b, n, s, d) -> (b, d', n)"""
        b, n, s, d = x.shape
        h = np.ascontiguousarray(np.asarray(x, self.dtype).transpose(0, 1, 3, 2)).reshape(-1, d, s)
        none = not any(k.startswith("operation.") for k in self.sd)
        h, bt = self.conv_bn_relu("transfer.", h, pool=none)
        bo = None
        if not none:
            h, bo, _ = self.blocks("", h, pool=True)

        def back(dout):
            dd = np.ascontiguousarray(np.asarray(dout, self.dtype).transpose(0, 2, 1)).reshape(b * n, -1)
            if bo is not None:
                dd = bo(dd)
            return bt(dd).reshape(b, n, d, s).transpose(0, 1, 3, 2)
        return h.reshape(b, n, -1).transpose(0, 2, 1), back


# ---- the record (tests/golden/g27_pointmlp_blocks.npz) ------------------------------------------------------------------------------
WANT = {"y": "_y", "dx": "_dx", "dresidual": "_dresidual", "dgamma": "_dgamma", "dbeta": "_dbeta", "running_mean": "_rm1", "running_var": "_rv1"}


def residual_of(g, c):
    if c + "_residual" in g.files:
        return g[c + "_residual"]
    return g[str(g[c + "_residual_is"]) + "_y"] if c + "_residual_is" in g.files else None


def norm_case(g, c, dtype, decisions=None):
    """The restatement on the recorded norm case c -> the quantities (y = pooled for a pooled case) and the forward dict."""
    pool = bool(g[c + "_pool"])
    f = forward(g[c + "_x"], g[c + "_gamma"], g[c + "_beta"], g[c + "_rm0"], g[c + "_rv0"], int(g[c + "_nbt0"]),
                  training=bool(g[c + "_training"]), momentum=float(g["momentum"]), eps=float(g["eps"]), act=str(g[c + "_act"]),
                  residual=residual_of(g, c), pool=pool, decisions=decisions, dtype=dtype)
    b = backward(f, g[c + ("_dpooled" if pool else "_dy")])
    return dict(y=f["pooled"] if pool else f["y"], dx=b["dx"], dresidual=b["dresidual"], dgamma=b["dgamma"], dbeta=b["dbeta"],
                running_mean=f["running_mean"], running_var=f["running_var"]), f


def wanted(g, c, q):
    if q == "y" and bool(g[c + "_pool"]):
        return g[c + "_pooled"]
    return g[c + WANT[q]] if c + WANT[q] in g.files else None


def module_case(g, m, dtype):
    """The restated module on the recorded module case m -> {quantity: value} under the record's names, and the tape."""
    sd = {k: g[f"{m}_p_{k}"] for k in map(str, g[f"{m}_keys"])}
    tape = Tape(sd, training=bool(g[f"{m}_training"]), act=str(g[f"{m}_act"]), dtype=dtype, eps=float(g["eps"]), momentum=float(g["momentum"]))
    kind = str(g[f"{m}_kind"])
    x = np.asarray(g[f"{m}_x"], dtype)
    if kind == "PreExtraction":
        out, back = tape.pre_extraction(x)
    elif kind == "PosExtraction":
        out, back = tape.pos_extraction(x)
    elif kind == "ConvBNReLU1D":
        out, back = tape.conv_bn_relu("", x)
    else:
        out, back = tape.res_block("", x)
    res = {"out": out, "dx": back(np.asarray(g[f"{m}_dout"], dtype))}
    res.update({"d_" + k: v for k, v in tape.grads.items()})
    res.update({"after_" + k: v for k, v in tape.after.items()})
    return res, tape


def reference_classes():
    """The four modules op by op over torch's own layers, restated from their description (Conv1d(k), BatchNorm1d, activation;
    act(net2(net1(x)) + x); transfer, blocks, adaptive_max_pool1d over the neighbours): the unfused form the fused classes are held
    against, under the class names fuse_pointmlp_blocks looks for.  -> {name: class}"""
    import torch.nn.functional as F
    from torch import nn

    def activation(name):
        return nn.GELU() if name.lower() == "gelu" else nn.ReLU(inplace=True)

    class ConvBNReLU1D(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size=1, bias=True, activation_name="relu"):
            super().__init__()
            self.act = activation(activation_name)
            self.net = nn.Sequential(nn.Conv1d(in_channels, out_channels, kernel_size, bias=bias), nn.BatchNorm1d(out_channels), self.act)

        def forward(self, x):
            return self.net(x)

    class ConvBNReLURes1D(nn.Module):
        def __init__(self, channel, kernel_size=1, groups=1, res_expansion=1.0, bias=True, activation_name="relu"):
            super().__init__()
            mid = int(channel * res_expansion)
            self.act = activation(activation_name)
            self.net1 = nn.Sequential(nn.Conv1d(channel, mid, kernel_size, groups=groups, bias=bias), nn.BatchNorm1d(mid), self.act)
            if groups > 1:
                self.net2 = nn.Sequential(nn.Conv1d(mid, channel, kernel_size, groups=groups, bias=bias), nn.BatchNorm1d(channel), self.act,
                                          nn.Conv1d(channel, channel, kernel_size, bias=bias), nn.BatchNorm1d(channel))
            else:
                self.net2 = nn.Sequential(nn.Conv1d(mid, channel, kernel_size, bias=bias), nn.BatchNorm1d(channel))

        def forward(self, x):
            return self.act(self.net2(self.net1(x)) + x)

    class PreExtraction(nn.Module):
        def __init__(self, in_channels, out_channels, blocks=1, groups=1, res_expansion=1, bias=True, activation_name="relu"):
            super().__init__()
            self.transfer = ConvBNReLU1D(in_channels, out_channels, bias=bias, activation_name=activation_name)
            self.operation = nn.Sequential(*[ConvBNReLURes1D(out_channels, groups=groups, res_expansion=res_expansion, bias=bias,
                                                             activation_name=activation_name) for _ in range(blocks)])

        def forward(self, x):
            b, n, s, d = x.size()
            x = self.operation(self.transfer(x.permute(0, 1, 3, 2).reshape(-1, d, s)))
            return F.adaptive_max_pool1d(x, 1).view(b * n, -1).reshape(b, n, -1).permute(0, 2, 1)

    class PosExtraction(nn.Module):
        def __init__(self, channels, blocks=1, groups=1, res_expansion=1, bias=True, activation_name="relu"):
            super().__init__()
            self.operation = nn.Sequential(*[ConvBNReLURes1D(channels, groups=groups, res_expansion=res_expansion, bias=bias,
                                                             activation_name=activation_name) for _ in range(blocks)])

        def forward(self, x):
            return self.operation(x)

    return {c.__name__: c for c in (ConvBNReLU1D, ConvBNReLURes1D, PreExtraction, PosExtraction)}


def reference_module(g, m):
    """The unfused torch module of the recorded module case m (fp32, the record's state_dict loaded) and its input shape."""
    import torch
    cls = reference_classes()
    sd = {k: torch.from_numpy(np.asarray(g[f"{m}_p_{k}"])) for k in map(str, g[f"{m}_keys"])}
    kind, act = str(g[f"{m}_kind"]), str(g[f"{m}_act"])
    bias = any(k.endswith("0.bias") for k in sd)
    n_blocks = len({k.split(".")[1] for k in sd if k.startswith("operation.")})
    block = next((k[:-len("net1.0.weight")] for k in sd if k.endswith("net1.0.weight")), None)
    groups, expansion = 1, 1.0
    if block is not None:
        w = sd[block + "net1.0.weight"]
        channel = sd[block + "net2.0.weight"].shape[0]
        groups = channel // w.shape[1]
        expansion = w.shape[0] / channel
    if kind == "ConvBNReLU1D":
        w = sd["net.0.weight"]
        mod = cls[kind](w.shape[1], w.shape[0], bias=bias, activation_name=act)
    elif kind == "ConvBNReLURes1D":
        mod = cls[kind](channel, groups=groups, res_expansion=expansion, bias=bias, activation_name=act)
    elif kind == "PosExtraction":
        mod = cls[kind](channel, blocks=n_blocks, groups=groups, res_expansion=expansion, bias=bias, activation_name=act)
    else:
        w = sd["transfer.net.0.weight"]
        mod = cls[kind](w.shape[1], w.shape[0], blocks=n_blocks, groups=groups, res_expansion=expansion, bias=bias, activation_name=act)
    mod.load_state_dict({k: v if k.endswith("num_batches_tracked") else v.float() for k, v in sd.items()})
    return mod.train(bool(g[f"{m}_training"]))
