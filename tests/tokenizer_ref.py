"""Restatement of the group tokenizer (unipre3d_amd/tokenizer.py, csrc/u3d_tokenizer.hip) in numpy, phase by phase as the kernels run
it: BN1 folded from nine moments of the coordinates, the cat replaced by a per-group bias, and the closed-form backward in three phases
separated by BatchNorm's two global sums.  (A plain helper module; tests/test_tokenizer_ref.py holds it to the reference's own record,
tests/golden/g24_tokenizer.npz.)

  weights(C)            the closed-form fp64 recipe (no RNG) of the record's weights, BN affine and running statistics, rounded to fp32
  forward / backward    dtype=np.float64: the arithmetic itself.  dtype=np.float32: every tensor in fp32 and every product summed in the
                        kernels' order (one fp32 chain along k; weight gradients row by row inside a split, splits added in order), the
                        statistics in f64 as the kernels keep them.  arg2 / arg4 override the max decisions; stat_reduce is the hook of
                        tokenize(): it gets each phase's f64 block (count first) and returns the reduced one.
  reference_module      the reference's lines in torch (what unipre3d_amd.tokenizer.Encoder runs on the CPU), for yardsticks
"""
from __future__ import annotations

import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g24_tokenizer.npz")
TOLERANCE = os.path.join(os.path.dirname(HERE), "profiles", "tokenizer", "tolerance.json")
C1, C2, C3 = 128, 256, 512
PARAMS = ("W1", "b1", "g1", "be1", "W2", "b2", "W3", "b3", "g2", "be2", "W4", "b4")
RUNNING = ("rm1", "rv1", "rm2", "rv2")
STATE_KEYS = {"W1": "first_conv.0.weight", "b1": "first_conv.0.bias", "g1": "first_conv.1.weight", "be1": "first_conv.1.bias",
              "rm1": "first_conv.1.running_mean", "rv1": "first_conv.1.running_var", "W2": "first_conv.3.weight", "b2": "first_conv.3.bias",
              "W3": "second_conv.0.weight", "b3": "second_conv.0.bias", "g2": "second_conv.1.weight", "be2": "second_conv.1.bias",
              "rm2": "second_conv.1.running_mean", "rv2": "second_conv.1.running_var", "W4": "second_conv.3.weight",
              "b4": "second_conv.3.bias"}
CASES = ("train", "eval", "padded", "strided")
QUANTITIES = ("out", "dparams", "dx", "running")
SUBSET_STEP = {"W2": 37, "W3": 293, "W4": 3}   # dW2, dW3 and dW4 are recorded at the flat indices 0, step, 2 step, ...
EPS, MOMENTUM = 1e-5, 0.1
NBT0 = 3                                  # num_batches_tracked before the recorded step


# ---- the record's weights ------------------------------------------------------------------------------------------------------------
def _wave(shape, a, b, c, scale, offset=0.0):
    i = np.arange(shape[0], dtype=np.float64)[:, None]
    j = np.arange(shape[1] if len(shape) > 1 else 1, dtype=np.float64)[None, :]
    v = offset + scale * np.sin(a * i + b * j + c + 0.37 * np.cos(0.61 * i * j + c))
    return v.reshape(shape).astype(np.float32)


def weights(C):
    """{name: fp32 array}: Conv weights (out, in) of about +-1.7 / sqrt(fan in), biases, gamma in [0.6, 1.4] with some negative, beta,
    running means and positive running variances -- none at its default."""
    w = {"W1": _wave((C1, 3), 0.731, 1.913, 0.2, 0.9), "b1": _wave((C1,), 0.377, 0, 1.1, 0.2),
         "g1": _wave((C1,), 1.117, 0, 0.5, 0.4, 1.0), "be1": _wave((C1,), 0.893, 0, 2.3, 0.3),
         "W2": _wave((C2, C1), 0.517, 1.291, 0.7, 1.7 / np.sqrt(C1)), "b2": _wave((C2,), 0.291, 0, 0.9, 0.1),
         "W3": _wave((C3, C3), 0.443, 1.577, 1.3, 1.7 / np.sqrt(C3)), "b3": _wave((C3,), 0.613, 0, 0.1, 0.1),
         "g2": _wave((C3,), 0.971, 0, 1.9, 0.4, 1.0), "be2": _wave((C3,), 0.559, 0, 0.4, 0.3),
         "W4": _wave((C, C3), 0.659, 1.181, 2.1, 1.7 / np.sqrt(C3)), "b4": _wave((C,), 0.787, 0, 1.7, 0.1),
         "rm1": _wave((C1,), 0.411, 0, 0.3, 0.3), "rv1": _wave((C1,), 0.233, 0, 0.8, 0.3, 0.6),
         "rm2": _wave((C3,), 0.347, 0, 1.5, 0.3), "rv2": _wave((C3,), 0.199, 0, 2.2, 0.15, 0.3)}
    w["g1"][5::11] *= -1
    w["g2"][3::13] *= -1
    return w


def checksums(w):
    return np.array([[float(np.sum(w[k], dtype=np.float64)), float(np.sum(np.abs(w[k]), dtype=np.float64))] for k in PARAMS + RUNNING])


def state_dict(w):
    import torch
    sd = {STATE_KEYS[k]: torch.from_numpy(np.ascontiguousarray(v)).reshape(v.shape + (1,) if k in ("W1", "W2", "W3", "W4") else v.shape)
          for k, v in w.items()}
    sd["first_conv.1.num_batches_tracked"] = torch.tensor(NBT0)
    sd["second_conv.1.num_batches_tracked"] = torch.tensor(NBT0)
    return sd


def dist(x, ref, scale=None):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(x - ref)) / max(float(np.max(np.abs(ref))) if scale is None else scale, 1e-300))


# ---- products in the kernels' order ------------------------------------------------------------------------------------------------
def wgrad_rows_per_split(rows):
    s = max(1, min(64, (rows + 255) // 256))
    return ((rows + s - 1) // s + 31) // 32 * 32


def wgrad_splits(rows):
    rps = wgrad_rows_per_split(rows)
    return (rows + rps - 1) // rps


def _mm(a, b, dt):
    """a (R, K) b (K, N): fp64 a plain product, fp32 one chain along k."""
    if dt == np.float64:
        return a @ b
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * b[k:k + 1, :]
    return acc


def _mm_rows(a, g, dt, rps=None):
    """a (R, I)^T g (R, J) summed over the rows: fp32 row by row inside a split of rps rows, the splits added in order."""
    if dt == np.float64:
        return a.T @ g
    R = a.shape[0]
    rps = wgrad_rows_per_split(R) if rps is None else rps
    total = np.zeros((a.shape[1], g.shape[1]), np.float32)
    for r0 in range(0, R, rps):
        acc = np.zeros_like(total)
        for r in range(r0, min(R, r0 + rps)):
            acc += a[r][:, None] * g[r][None, :]
        total += acc
    return total


def _colsum(a, dt):
    return np.sum(a, axis=0, dtype=np.float64).astype(dt)


def _seqsum(a, dt):
    """(M, n, J) summed over n, in order."""
    s = np.zeros((a.shape[0], a.shape[2]), dt)
    for i in range(a.shape[1]):
        s += a[:, i]
    return s


def _bn_update(run, mean, var, N, momentum, nbt):
    f = 1.0 / nbt if momentum is None else momentum
    return (1.0 - f) * run[0] + f * mean, (1.0 - f) * run[1] + f * var * (N / (N - 1.0))


# ---- forward -----------------------------------------------------------------------------------------------------------------------
def forward(x, w, *, training, dtype=np.float64, eps=EPS, momentum=MOMENTUM, nbt=NBT0, stat_reduce=None, arg2=None, arg4=None,
            mask1=None, mask3=None):
    """x (B, G, n, 3); w as weights() gives them.  Returns the saved state: out (B, G, C), f2, y3, g, arg2, arg4, the folds, and in
    training mode the running statistics after the step (`running`: rm1, rv1, rm2, rv2 in f64, and `nbt`).  arg2 / arg4 override the
    two max decisions and mask1 / mask3 (rows, 128) / (rows, 512) the two ReLU decisions the backward uses: all four are discontinuous,
    so a gradient is compared under the compared side's own decisions."""
    dt = dtype
    B, G, n, _ = x.shape
    M, R = B * G, B * G * n
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    X = np.ascontiguousarray(x).reshape(R, 3).astype(dt)
    s = {"shape": (B, G, n), "training": training, "dtype": dt, "X": X, "w": w, "stat_reduce": stat_reduce if training else None}
    red = s["stat_reduce"] or (lambda b: b)
    running = {k: W[k].copy() for k in RUNNING}
    if training:
        X64 = X.astype(np.float64)
        s1 = np.concatenate([[R], X64.sum(0), [(X64[:, a] * X64[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]])
        s1_loc, s1 = s1.copy(), red(s1)
        N, m = s1[0], s1[1:4] / s1[0]
        S = np.zeros((3, 3))
        for q, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            S[a, b] = S[b, a] = s1[4 + q] / N - m[a] * m[b]
        wm = W["W1"] @ m
        var1 = np.maximum(np.einsum("ka,ab,kb->k", W["W1"], S, W["W1"]), 0.0)
        mean1, inv1 = wm + W["b1"], 1.0 / np.sqrt(var1 + eps)
        dh = -inv1 * wm
        running["rm1"], running["rv1"] = _bn_update((W["rm1"], W["rv1"]), mean1, var1, N, momentum, nbt + 1)
    else:
        mean1, inv1 = W["rm1"], 1.0 / np.sqrt(W["rv1"] + eps)
        dh = inv1 * (W["b1"] - mean1)
    Ah, dhat = (inv1[:, None] * W["W1"]).astype(dt), dh.astype(dt)
    A, d = ((W["g1"] * inv1)[:, None] * W["W1"]).astype(dt), (W["g1"] * dh + W["be1"]).astype(dt)
    pre1 = ((A[None, :, 2] * X[:, 2:3] + d[None, :]) + A[None, :, 1] * X[:, 1:2]) + A[None, :, 0] * X[:, 0:1]
    xh1 = ((Ah[None, :, 2] * X[:, 2:3] + dhat[None, :]) + Ah[None, :, 1] * X[:, 1:2]) + Ah[None, :, 0] * X[:, 0:1]
    h1 = np.maximum(pre1, 0)
    cast = lambda k: W[k].astype(dt)
    f2 = _mm(h1, cast("W2").T, dt) + cast("b2")
    f2g = f2.reshape(M, n, C2)
    arg2 = np.argmax(f2g, axis=1).astype(np.int32) if arg2 is None else np.asarray(arg2, np.int32).reshape(M, C2)
    g = np.take_along_axis(f2g, arg2[:, None, :].astype(np.int64), 1)[:, 0]
    W3 = cast("W3")
    u = _mm(g, W3[:, :C2].T, dt) + cast("b3")
    y3 = _mm(f2, W3[:, C2:].T, dt) + np.repeat(u, n, axis=0)
    if training:
        y64 = y3.astype(np.float64)
        s2_loc = np.concatenate([[R], y64.sum(0), (y64 * y64).sum(0)])
        s2 = red(s2_loc.copy())
        s["fwd_sums"] = (s1_loc, s1, s2_loc, s2)
        N = s2[0]
        mean2 = s2[1:1 + C3] / N
        var2 = np.maximum(s2[1 + C3:] / N - mean2 * mean2, 0.0)
        inv2 = 1.0 / np.sqrt(var2 + eps)
        running["rm2"], running["rv2"] = _bn_update((W["rm2"], W["rv2"]), mean2, var2, N, momentum, nbt + 1)
    else:
        mean2, inv2 = W["rm2"], 1.0 / np.sqrt(W["rv2"] + eps)
    sc2 = W["g2"] * inv2
    s2c, t2 = sc2.astype(dt), (W["be2"] - mean2 * sc2).astype(dt)
    pre3 = s2c * y3 + t2
    h3 = np.maximum(pre3, 0)
    f4 = _mm(h3, cast("W4").T, dt) + cast("b4")
    C = f4.shape[1]
    f4g = f4.reshape(M, n, C)
    arg4 = np.argmax(f4g, axis=1).astype(np.int32) if arg4 is None else np.asarray(arg4, np.int32).reshape(M, C)
    out = np.take_along_axis(f4g, arg4[:, None, :].astype(np.int64), 1)[:, 0]
    s.update(mask1=pre1 > 0 if mask1 is None else np.asarray(mask1, bool).reshape(R, C1),
             mask3=pre3 > 0 if mask3 is None else np.asarray(mask3, bool).reshape(R, C3))
    s.update(out=out.reshape(B, G, C), f2=f2, y3=y3, g=g, arg2=arg2, arg4=arg4, f4=f4, pre1=pre1, xh1=xh1, h1=h1, pre3=pre3, h3=h3,
             inv1=inv1.astype(dt), inv2=inv2.astype(dt), mean2=mean2.astype(dt), running=running, nbt=nbt + 1 if training else nbt)
    return s


# ---- backward ----------------------------------------------------------------------------------------------------------------------
def backward(s, dout):
    """The closed-form gradients under s's arg2 / arg4: {name: array} for the twelve parameters (in the (out, in) shapes) and 'x'."""
    dt = s["dtype"]
    B, G, n = s["shape"]
    M, R = B * G, B * G * n
    W = {k: np.asarray(v, np.float64).astype(dt) for k, v in s["w"].items()}
    red = s["stat_reduce"] or (lambda b: b)
    training = s["training"]
    dout = np.asarray(dout).reshape(M, -1).astype(dt)
    C = dout.shape[1]
    rows4 = (np.arange(M)[:, None] * n + s["arg4"]).astype(np.int64)
    rows2 = (np.arange(M)[:, None] * n + s["arg2"]).astype(np.int64)
    dF4 = np.zeros((R, C), dt)
    dF4[rows4, np.arange(C)[None, :]] = dout
    grads = {"b4": _colsum(dout, dt)}
    if dt == np.float64:
        grads["W4"] = dF4.T @ s["h3"]
    else:
        acc = np.zeros((C, C3), np.float32)
        for gi in range(M):                                  # (one split of groups up to 64 groups)
            acc += dout[gi][:, None] * s["h3"][rows4[gi]]
        grads["W4"] = acc
    dh3m = np.where(s["mask3"], _mm(dF4, W["W4"], dt), 0).astype(dt)
    xh3 = (s["y3"] - s["mean2"]) * s["inv2"]
    d64 = dh3m.astype(np.float64)
    s3 = np.concatenate([[R], d64.sum(0), (d64 * xh3.astype(np.float64)).sum(0)])
    r3 = red(s3.copy())
    grads["be2"], grads["g2"] = s3[1:1 + C3].astype(dt), s3[1 + C3:].astype(dt)
    p = W["g2"] * s["inv2"]
    q = (r3[1:1 + C3] / r3[0]).astype(dt) if training else np.zeros(C3, dt)
    ww = (r3[1 + C3:] / r3[0]).astype(dt) if training else np.zeros(C3, dt)
    dy3 = p * (dh3m - q - xh3 * ww)
    dS = _seqsum(dy3.reshape(M, n, C3), dt)
    # the three biases that feed only a BatchNorm: the sum of dy over this rank's rows in closed form, in f64, from the sums alone
    # (p (S1 - N q - w sum(xhat)); in one process the exact zero it is mathematically, where a sum of fp32 dy would be rounding noise)
    s1_loc, s1_red, s2_loc, s2_red = s.get("fwd_sums", (None,) * 4)
    xsum3 = s2_loc[1:1 + C3] - s2_loc[0] * (s2_red[1:1 + C3] / s2_red[0]) if training else 0.0
    q64, w64 = (r3[1:1 + C3] / r3[0], r3[1 + C3:] / r3[0]) if training else (0.0, 0.0)
    db3 = p.astype(np.float64) * (s3[1:1 + C3] - s3[0] * q64 - w64 * s["inv2"].astype(np.float64) * xsum3)
    grads["b3"] = db3.astype(dt)
    grads["W3"] = np.concatenate([_mm_rows(dS, s["g"], dt), _mm_rows(dy3, s["f2"], dt)], axis=1)
    dg = _mm(dS, W["W3"][:, :C2], dt)
    df2 = _mm(dy3, W["W3"][:, C2:], dt)
    df2[rows2, np.arange(C2)[None, :]] += dg
    W3_64 = W["W3"].astype(np.float64)
    grads["b2"] = (db3 @ (W3_64[:, :C2] + W3_64[:, C2:])).astype(dt)
    grads["W2"] = _mm_rows(df2, s["h1"], dt)
    dh1m = np.where(s["mask1"], _mm(df2, W["W2"], dt), 0).astype(dt)
    d64 = dh1m.astype(np.float64)
    s1b = np.concatenate([[R], d64.sum(0), (d64 * s["xh1"].astype(np.float64)).sum(0)])
    r1 = red(s1b.copy())
    grads["be1"], grads["g1"] = s1b[1:1 + C1].astype(dt), s1b[1 + C1:].astype(dt)
    p1 = W["g1"] * s["inv1"]
    q1 = (r1[1:1 + C1] / r1[0]).astype(dt) if training else np.zeros(C1, dt)
    w1 = (r1[1 + C1:] / r1[0]).astype(dt) if training else np.zeros(C1, dt)
    dy1 = p1 * (dh1m - q1 - s["xh1"] * w1)
    grads["W1"] = (dy1.astype(np.float64).T @ s["X"].astype(np.float64)).astype(dt)
    xsum1 = W["W1"].astype(np.float64) @ (s1_loc[1:4] - s1_loc[0] * (s1_red[1:4] / s1_red[0])) if training else 0.0
    q64, w64 = (r1[1:1 + C1] / r1[0], r1[1 + C1:] / r1[0]) if training else (0.0, 0.0)
    grads["b1"] = (p1.astype(np.float64) * (s1b[1:1 + C1] - s1b[0] * q64 - w64 * s["inv1"].astype(np.float64) * xsum1)).astype(dt)
    grads["x"] = _mm(dy1, W["W1"], dt).reshape(B, G, n, 3)
    return grads


ZERO_IN_TRAINING = {"b1": "be1", "b2": "be2", "b3": "be2"}     # a bias that feeds only a BatchNorm: held on the scale of that BN's dbeta


def distances(got, ref, training):
    """{quantity: max|x - ref| / max|ref|} for out, dparams (the worst parameter), dx and running (the worst of the four buffers).
    got / ref: {'out', the twelve parameter names, 'x', 'rm1', 'rv1', 'rm2', 'rv2'}; missing entries of got are skipped."""
    d = {"out": dist(got["out"], ref["out"]), "dparams": 0.0, "dx": 0.0, "running": 0.0}
    for k in PARAMS:
        if k in got:
            scale = float(np.max(np.abs(ref[ZERO_IN_TRAINING[k]]))) if training and k in ZERO_IN_TRAINING else None
            d["dparams"] = max(d["dparams"], dist(got[k], ref[k], scale))
    if "x" in got:
        d["dx"] = dist(got["x"], ref["x"])
    for k in RUNNING:
        if k in got:
            d["running"] = max(d["running"], dist(got[k], ref[k]))
    return d


def recorded(grads):
    """The gradients as the record keeps them: dW2, dW3 and dW4 at every SUBSET_STEP-th flat index."""
    return {k: (np.asarray(v).reshape(-1)[::SUBSET_STEP[k]] if k in SUBSET_STEP else np.asarray(v)) for k, v in grads.items()}


# ---- two ranks in lock step -----------------------------------------------------------------------------------------------------------
def run_ranks(fns):
    """Runs fns[rank](stat_reduce) in one thread per rank; stat_reduce adds the ranks' blocks in rank order.  Returns the results and the
    list of blocks every rank contributed, in call order."""
    n = len(fns)
    barrier, slots, results, sent, errors = threading.Barrier(n), [None] * n, [None] * n, [[] for _ in range(n)], []

    def reducer(rank):
        def reduce(block):
            slots[rank] = np.array(block, np.float64)
            sent[rank].append(slots[rank].copy())
            barrier.wait()
            total = sum(slots[1:], slots[0].copy())
            barrier.wait()
            return total
        return reduce

    def work(rank):
        try:
            results[rank] = fns[rank](reducer(rank))
        except BaseException as e:      # a failing rank must not leave the other one waiting
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return results, sent


# ---- the reference's lines in torch ---------------------------------------------------------------------------------------------------
def reference_module(C, w, dtype, training):
    import torch
    from unipre3d_amd.tokenizer import Encoder
    m = Encoder(C)
    m.load_state_dict(state_dict(w), strict=True)
    m = m.to(dtype)
    m.train(training)
    return m


def reference_run(module, x, dout):
    """(out, {name: grad}, running after the step) of a module with the reference's forward on CPU tensors."""
    import torch
    dtype = next(module.parameters()).dtype
    t = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    module.zero_grad()
    out = module(t)
    (out * torch.from_numpy(np.asarray(dout)).to(dtype)).sum().backward()
    sd = module.state_dict()
    inv = {v: k for k, v in STATE_KEYS.items()}
    grads = {inv[k]: p.grad.numpy().reshape(p.shape[:2] if p.dim() == 3 else p.shape) for k, p in module.named_parameters()}
    grads["x"] = t.grad.numpy()
    running = {k: sd[STATE_KEYS[k]].numpy().copy() for k in RUNNING}
    return out.detach().numpy(), grads, running, int(sd["first_conv.1.num_batches_tracked"])


def golden_case(z, name):
    """(x as the module is fed it, dout, training) of a recorded case; `strided` comes back as the transformer's permuted view."""
    x = z[f"{name}_x"]
    if name == "strided":
        x = np.transpose(x, (0, 2, 3, 1))          # recorded as (B, 3, G, n)
    return x, z[f"{name}_dout"], name != "eval"


def record_of(z, name):
    """{quantity name: the recorded fp64 array} of a case."""
    ref = {k: z[f"{name}_d{k}64"] for k in PARAMS}
    ref.update(out=z[f"{name}_out64"], x=z[f"{name}_dx64"], **{k: z[f"{name}_{k}64"] for k in RUNNING})
    return ref


def floors(z):
    """{case: {quantity: distance}} of the fp32 restatement in the kernels' order from the fp64 record.  Gradients under the fp32 run's own
    max and ReLU decisions are compared with the fp64 arithmetic under the same decisions."""
    w = weights(int(z["C"]))
    rows = {}
    for name in (str(n) for n in z["names"]):
        x, dout, training = golden_case(z, name)
        s = forward(x, w, training=training, dtype=np.float32)
        s64 = forward(x, w, training=training, arg2=s["arg2"], arg4=s["arg4"], mask1=s["mask1"], mask3=s["mask3"])
        got = dict(recorded(backward(s, dout)), out=s["out"], **s["running"])
        ref = dict(recorded(backward(s64, dout)), out=z[f"{name}_out64"], **{k: z[f"{name}_{k}64"] for k in RUNNING})
        rows[name] = distances(got, ref, training)
    return rows


def tolerance():
    import json
    with open(TOLERANCE) as f:
        return json.load(f)


# ---- shapes without a recorded case ---------------------------------------------------------------------------------------------------
# (B, G, n, C); tests/test_gpu_tokenizer.py says which constant of the kernels each one comes from
EDGES = ((1, 1, 2, 40), (2, 5, 24, 40), (1, 3, 33, 384), (2, 2, 1, 40), (1, 2, 256, 16), (2, 5, 30, 40), (1, 2, 3, 1), (1, 2, 4, 1024),
         (1, 9, 64, 72), (4, 128, 32, 384))
EDGE_MODES = tuple((s, t) for s in EDGES for t in (True, False) if t or s != EDGES[-1])    # the workload-shaped one in training mode only


def edge_inputs(shape):
    """(x, dout) of an edge shape: uniform coordinates, the last quarter of every group repeating its first row (ball-query padding)."""
    B, G, n, C = shape
    rng = np.random.default_rng(B * 1000 + G * 10 + n)
    x = rng.uniform(-1, 1, (B, G, n, 3)).astype(np.float32)
    if n >= 4:
        x[:, :, n - n // 4:] = x[:, :, :1]
    return x, rng.uniform(-1, 1, (B, G, C)).astype(np.float32)


def edge_floor(shape, training):
    """{quantity: distance} of the fp32 restatement in the kernels' order from the fp64 restatement at an edge shape (gradients under the
    fp32 run's own max and ReLU decisions on both sides)."""
    x, dout = edge_inputs(shape)
    w = weights(shape[3])
    s = forward(x, w, training=training, dtype=np.float32)
    s64 = forward(x, w, training=training, arg2=s["arg2"], arg4=s["arg4"], mask1=s["mask1"], mask3=s["mask3"])
    free = forward(x, w, training=training)
    got = dict(backward(s, dout), out=s["out"], **s["running"])
    ref = dict(backward(s64, dout), out=free["out"], **free["running"])
    return distances(got, ref, training)


def edge_key(shape, training):
    return "x".join(map(str, shape)) + ("-train" if training else "-eval")


def kernel_masks(x, fold1, fold2, y3):
    """The two ReLU decisions as the kernels take them, from what they keep: [fma(A0, a, fma(A1, b, fma(A2, c, d))) > 0] (rows, 128) and
    [fma(s2, y3, t2) > 0] (rows, 512).  A product of two fp32 numbers is exact in f64 and rounding keeps the sign of a sum, so the last
    fma's sign is computed exactly; the two inner fmas are rounded to fp32 as the device rounds them."""
    X = np.ascontiguousarray(x).reshape(-1, 3).astype(np.float64)
    f1, f2c = np.asarray(fold1, np.float32).astype(np.float64), np.asarray(fold2, np.float32).astype(np.float64)
    A, d = f1[:3 * C1].reshape(C1, 3), f1[3 * C1:4 * C1]
    t = (A[None, :, 2] * X[:, 2:3] + d[None, :]).astype(np.float32).astype(np.float64)
    t = (A[None, :, 1] * X[:, 1:2] + t).astype(np.float32).astype(np.float64)
    mask1 = (A[None, :, 0] * X[:, 0:1] + t) > 0
    mask3 = (f2c[None, :C3] * np.asarray(y3, np.float64).reshape(-1, C3) + f2c[None, C3:2 * C3]) > 0
    return mask1, mask3


def mask_gap(s64, mask1, mask3):
    """The largest |fp64 pre-activation| / max|fp64 pre-activation| over the elements where a given ReLU decision differs from the fp64
    arithmetic's own: how far from the kink a differing decision was taken (0 when none differs)."""
    gap = 0.0
    for pre, mask in ((s64["pre1"], mask1), (s64["pre3"], mask3)):
        flipped = (pre > 0) != mask
        if flipped.any():
            gap = max(gap, float(np.abs(pre[flipped]).max() / np.abs(pre).max()))
    return gap
