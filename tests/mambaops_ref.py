"""The two operators of a Mamba block around its scan, restated on CPU torch in the dtype of their inputs (fp64 is the arbiter, fp32
the yardstick): the causal depthwise conv1d (+ SiLU) as explicit padding plus a tap loop, the residual-add + LayerNorm / RMSNorm as the
formulae read, and PCM's block prologue chaining (hidden, residual) through two add + norm calls.

    conv:  out[b,d,l] = act(bias[d] + sum_w weight[d,w] x[b,d,l-(W-1)+w]),  x zero at negative steps;  act = silu for "silu" | "swish"
    norm:  r = x (+ residual);  LayerNorm  y = (r - mean) / sqrt(var + eps) w (+ b),  var = mean((r - mean)^2)  (centred)
                                RMSNorm    y = r / sqrt(mean(r^2) + eps) w (+ b);        returns y, or (y, r) under prenorm

The error measure and the bar are the selective scan's (tests/selective_scan_ref.py): per tensor max |got - f64| / max |f64| against
max(4 x the fp32 run's own figure, 4 fp32 ulps of the tensor maximum): the device may fuse the tap sum into FMAs and sums rows in a tree.
"""

import torch
import torch.nn.functional as F

from selective_scan_ref import FACTOR, FLOOR, _wave, bar, norm_err  # noqa: F401  (re-exported for the tests)


def causal_conv1d(x, weight, bias=None, activation=None):
    """x (B, D, L), weight (D, W), bias (D,) or None."""
    if activation not in (None, "silu", "swish"):
        raise NotImplementedError("activation must be None, silu, or swish")
    L, W = x.shape[-1], weight.shape[1]
    xp = F.pad(x, (W - 1, 0))
    out = torch.zeros_like(x)
    for w in range(W):
        out = out + weight[None, :, w, None] * xp[:, :, w:w + L]
    if bias is not None:
        out = out + bias[None, :, None]
    return out if activation is None else out * torch.sigmoid(out)


def layer_norm(x, weight, bias, residual=None, eps=1e-6, prenorm=False, is_rms_norm=False):
    r = x if residual is None else x + residual
    if is_rms_norm:
        y = r / torch.sqrt((r * r).mean(-1, keepdim=True) + eps) * weight
    else:
        c = r - r.mean(-1, keepdim=True)
        y = c / torch.sqrt((c * c).mean(-1, keepdim=True) + eps) * weight
    if bias is not None:
        y = y + bias
    return (y, r) if prenorm else y


def rms_norm(x, weight, bias, residual=None, prenorm=False, eps=1e-6):
    return layer_norm(x, weight, bias, residual, eps, prenorm, True)


def block_prologues(hidden, mix, w1, w2, norm=rms_norm, eps=1e-5):
    """Two PCM blocks' openings (mamba_layer.py's fused_add_norm branch) with a stand-in mixer: the first block has no residual yet, the
    second adds what the first one's mixer produced.  mix (N, N) is the stand-in (a linear map keeps the chain differentiable and cheap).
    Returns (hidden, residual) as they enter the second block's mixer."""
    h, r = norm(hidden, w1, None, residual=None, prenorm=True, eps=eps)
    h = torch.tanh(h @ mix)
    return norm(h, w2, None, residual=r, prenorm=True, eps=eps)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def conv_inputs(batch, dim, L, width, has_bias=True, seed=0):
    """fp64 (x, weight, bias, dout): O(1) noise plus a pattern that differs along every axis."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = r(batch, dim, L) + _wave((batch, dim, L), 1.3, 0.37, 0.05)
    weight = 0.5 * r(dim, width) + 0.3 * _wave((dim, width), 0.7, 1.1)
    bias = 0.3 * r(dim) if has_bias else None
    dout = r(batch, dim, L) + _wave((batch, dim, L), 0.4, 0.19, 0.13)
    return x, weight, bias, dout


def norm_inputs(M, N, has_bias=True, has_residual=True, seed=0):
    """fp64 (x, weight, bias, residual, dy, dr)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = r(M, N) + 0.5 * _wave((M, N), 0.9, 0.13)
    weight = 1.0 + 0.3 * r(N)
    bias = 0.3 * r(N) if has_bias else None
    residual = 2.0 * r(M, N) + _wave((M, N), 0.3, 0.21, phase=1.0) if has_residual else None
    return x, weight, bias, residual, r(M, N) + 0.3 * _wave((M, N), 0.5, 0.07), r(M, N)


def run_with_grads(fn, tensors, douts):
    """fn(*leaves) -> tensor or tuple; backward of sum_i (out_i * douts_i); returns (outs, grads), None staying None."""
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in tensors]
    outs = fn(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * d.to(o.device, o.dtype)).sum() for o, d in zip(outs, douts)).backward()
    return [o.detach() for o in outs], [None if v is None else v.grad.detach() for v in leaves]


def cast(tensors, dtype, device="cpu"):
    return [None if t is None else t.to(device=device, dtype=dtype) for t in tensors]
