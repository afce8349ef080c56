"""Restatement of the fused BatchNorm + activation + residual over point rows (unipre3d_amd/batchnorm.py, csrc/u3d_batchnorm.hip) in
numpy.  (A plain helper module; tests/test_batchnorm_ref.py holds it to torch's own modules in fp64 and to the reference's record,
tests/golden/g26_batchnorm.npz.)

  forward / backward   dtype=np.float64: the arithmetic itself (centred variance, plain sums).
                       dtype=np.float32: every row tensor in fp32, one rounding per operation and no contraction, in the kernels' order:
                       y = act((x - mean) (invstd gamma) + beta [+ residual]); the sums in f64 per row chunk (row lanes in ascending
                       order), the chunks in interleaved runs and a tree (sum_partials); mean, invstd and the running statistics in f64 from
                       the block `count | sum [C] | sum [C]`, rounded once.
                       stat_reduce is the hook of batch_norm_act(): it gets each f64 block and returns the reduced one.
  row_chunk(C)         rows one workgroup takes
"""
from __future__ import annotations

import os

import numpy as np
from scipy.special import erf

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g26_batchnorm.npz")
TOLERANCE = os.path.join(os.path.dirname(HERE), "profiles", "batchnorm", "tolerance.json")
QUANTITIES = ("y", "dx", "dresidual", "dgamma", "dbeta", "running_mean", "running_var")
NT, CHUNK_FLOATS, MIN_ROWS = 256, 4096, 32


def row_chunk(C):
    return max(CHUNK_FLOATS // C, MIN_ROWS)


def rel(got, want):
    """max|x - reference| / max|reference| (the unit of profiles/batchnorm/tolerance.json)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-300)) if want.size else 0.0


def chunk_sums(a, b, wide=None):
    """(parts, 2C) f64: per row chunk the column sums of a and of b, the row lanes of a column added in ascending order."""
    N, C = a.shape
    V = 4 if (C % 4 == 0 if wide is None else wide) else 1
    cols = C // V
    cpp = min(cols, NT)
    RP = NT // cpp
    ch = row_chunk(C)
    out = []
    for r0 in range(0, N, ch):
        part = np.zeros(2 * C)
        for k, t in enumerate((a, b)):
            rows = t[r0:r0 + ch].astype(np.float64)
            acc = np.zeros(C)
            for rl in range(RP):
                lane = np.zeros(C)
                for row in rows[rl::RP]:
                    lane = lane + row
                acc = acc + lane
            part[k * C:(k + 1) * C] = acc
        out.append(part)
    return np.stack(out)


def sum_partials(partials, count):
    """block = count | the partials added as sum_kernel does: 64 slots 64 chunks apart with 8 accumulators each, a pairwise sum per slot,
    a tree over the slots."""
    P, W = partials.shape
    acc = np.zeros((64, 8, W))
    for slot in range(min(64, P)):
        for k in range(8):
            for p in range(slot + 64 * k, P, 512):
                acc[slot, k] = acc[slot, k] + partials[p]
    t = ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])) + ((acc[:, 4] + acc[:, 5]) + (acc[:, 6] + acc[:, 7]))
    o = 32
    while o:
        t[:o] = t[:o] + t[o:2 * o]
        o //= 2
    return np.concatenate([[float(count)], t[0]])


def _act(z, act):
    if act == "relu":
        return np.where(z > 0, z, z.dtype.type(0))
    if act == "gelu":
        t = z.dtype.type
        return (t(0.5) * z) * (t(1) + erf(z * t(0.70710678118654752440)).astype(z.dtype))
    return z


def _g(dy, z, y, act):
    """dy act'(.): relu from the saved output's mask, gelu from the recomputed pre-activation z."""
    if act == "relu":
        return np.where(y > 0, dy, dy.dtype.type(0))
    if act == "gelu":
        t = z.dtype.type
        cdf = t(0.5) * (t(1) + erf(z * t(0.70710678118654752440)).astype(z.dtype))
        pdf = np.exp((t(-0.5) * z) * z) * t(0.39894228040143267794)
        return dy * (cdf + z * pdf)
    return dy


def forward(x, gamma, beta, running_mean=None, running_var=None, nbt=None, *, training, momentum, eps, act="none", residual=None,
            dtype=np.float64, stat_reduce=None, wide=None):
    """-> dict: y, mean, invstd, a (= invstd gamma), running_mean, running_var, nbt (after the step), and what backward() needs."""
    t = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    N, C = x.shape
    gamma = np.ones(C, dtype) if gamma is None else np.asarray(gamma, dtype)
    beta = np.zeros(C, dtype) if beta is None else np.asarray(beta, dtype)
    rm = None if running_mean is None else np.asarray(running_mean, dtype).copy()
    rv = None if running_var is None else np.asarray(running_var, dtype).copy()
    count = float(N)
    if training:
        if dtype == np.float64 and stat_reduce is None:
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
        else:
            xd = x.astype(np.float64)
            block = sum_partials(chunk_sums(x, xd * xd, wide), N) if dtype == np.float32 else \
                np.concatenate([[count], xd.sum(0), (xd * xd).sum(0)])
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
    z = (x - mean) * a + beta
    if residual is not None:
        z = z + np.asarray(residual, dtype)
    y = _act(z, act)
    return dict(y=y, mean=mean, invstd=invstd, a=a, beta=beta, x=x, act=act, training=training, running_mean=rm, running_var=rv,
                nbt=nbt, dtype=dtype, stat_reduce=stat_reduce, wide=wide, count=count)


def backward(f, dy):
    """-> dict: dx, dgamma, dbeta (this process's sums), dresidual."""
    dtype, x, act = f["dtype"], f["x"], f["act"]
    dy = np.asarray(dy, dtype)
    N, C = x.shape
    z = (x - f["mean"]) * f["a"] + f["beta"] if act == "gelu" else None
    g = _g(dy, z, f["y"], act)
    xhat = (x - f["mean"]) * f["invstd"]
    gd = g.astype(np.float64)
    prod = gd * xhat.astype(np.float64)
    block = sum_partials(chunk_sums(gd, prod, f["wide"]), N) if dtype == np.float32 else np.concatenate([[float(N)], gd.sum(0), prod.sum(0)])
    dbeta, dgamma = block[1:1 + C].astype(dtype), block[1 + C:].astype(dtype)
    if f["training"]:
        if f["stat_reduce"] is not None:
            block = f["stat_reduce"](block.copy())
        b, d = (block[1:1 + C] / block[0]).astype(dtype), (block[1 + C:] / block[0]).astype(dtype)
        dx = f["a"] * ((g - b) - xhat * d)
    else:
        dx = g * f["a"]
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dresidual=g)
