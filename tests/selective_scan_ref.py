"""The selective scan (Mamba's S6 recurrence) restated as a sequential loop on CPU torch, in the dtype of its inputs (fp64 is the
arbiter, fp32 the yardstick), the torch composition of the Mamba inner function around it, the structured inputs the tests share and
the error measure they use.

    dt = delta (+ delta_bias[d]); softplus when asked (torch's rule: identity above 20)
    x_l = exp(dt_l A) x_{l-1} + dt_l B_l u_l, x_{-1} = 0;   y_l = sum_n C_l x_l (+ D u_l);   out = y (* silu(z))

Error measure: per tensor, max |got - f64| / max |f64|.  The yardstick of a case is that measure for the fp32 run of this loop; the
device may be 4 x the yardstick (its scan reassociates the products of exp terms), with a floor of FLOOR_ULPS fp32 ulps of the tensor
maximum: one exp, one softplus / sigmoid and a three-term product each contribute up to an ulp even where the sequential fp32 loop
happens to be exact (the analytic cases with zeros).
"""

import torch
import torch.nn.functional as F

N = 16
FLOOR_ULPS = 4
FLOOR = FLOOR_ULPS * 2.0 ** -23
FACTOR = 4.0
GRAD_NAMES = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")


def selective_scan(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, return_last_state=False):
    """u, delta, z (B, D, L); A (D, N); B, C (B, N, L) or (B, G, N, L); D, delta_bias (D).  One step at a time."""
    batch, dim, L = u.shape
    dt = delta if delta_bias is None else delta + delta_bias[None, :, None]
    if delta_softplus:
        dt = F.softplus(dt)
    Bx = B[:, None] if B.dim() == 3 else B
    Cx = C[:, None] if C.dim() == 3 else C
    Bx = Bx.repeat_interleave(dim // Bx.shape[1], dim=1)          # (B, D, N, L): channel d reads group d // (D / G)
    Cx = Cx.repeat_interleave(dim // Cx.shape[1], dim=1)
    x = u.new_zeros(batch, dim, A.shape[1])
    ys = []
    for l in range(L):
        step = dt[:, :, l, None]
        x = torch.exp(step * A[None]) * x + step * Bx[:, :, :, l] * u[:, :, l, None]
        ys.append((Cx[:, :, :, l] * x).sum(-1))
    y = torch.stack(ys, dim=2)
    if D is not None:
        y = y + D[None, :, None] * u
    if z is not None:
        y = y * F.silu(z)
    return (y, x) if return_last_state else y


def mamba_inner_no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, D=None, delta_bias=None,
                            delta_softplus=True, scan=selective_scan):
    """The mixer between in_proj and out_proj: causal depthwise conv + SiLU, x_proj, dt_proj's weight, the scan gated by z."""
    L = xz.shape[-1]
    rank = delta_proj_weight.shape[1]
    x, z = xz.chunk(2, dim=1)
    d_inner, width = conv1d_weight.shape[0], conv1d_weight.shape[-1]
    x = F.silu(F.conv1d(F.pad(x, (width - 1, 0)), conv1d_weight.reshape(d_inner, 1, width), conv1d_bias, groups=d_inner))
    x_dbl = torch.einsum("bdl,rd->blr", x, x_proj_weight)                       # (B, L, rank + 2 N)
    delta = torch.einsum("dr,blr->bdl", delta_proj_weight, x_dbl[..., :rank])
    Bm = x_dbl[..., rank:rank + N].permute(0, 2, 1)
    Cm = x_dbl[..., rank + N:].permute(0, 2, 1)
    return scan(x, delta, A, Bm, Cm, D, z=z, delta_bias=delta_bias, delta_softplus=delta_softplus)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _wave(shape, *freqs, phase=0.0):
    """A smooth pattern that differs along every axis: sin of a weighted index sum (irrational-ish weights, no two axes alike)."""
    acc = torch.full(shape, phase, dtype=torch.float64)
    for ax, f in enumerate(freqs):
        idx = torch.arange(shape[ax], dtype=torch.float64).reshape([-1 if i == ax else 1 for i in range(len(shape))])
        acc = acc + f * idx
    return torch.sin(acc)


def make_inputs(batch, dim, L, groups=None, has_D=True, has_z=True, has_bias=True, softplus=True, seed=0):
    """fp64 inputs of Mamba-like ranges: A negative and different per (d, n), dt after softplus around 0.01 .. 1, everything else
    O(1) noise plus a pattern.  groups None: 3-D B / C.  Without softplus nothing keeps dt positive but the inputs themselves, so the
    bias is positive there (a negative dt makes exp(dt A) grow without bound over L steps: inf in every precision, nothing to compare)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    t = {"u": r(batch, dim, L) + _wave((batch, dim, L), 1.3, 0.37, 0.05)}
    raw = 0.8 * r(batch, dim, L) + _wave((batch, dim, L), 0.7, 0.21, 0.11)
    t["delta"] = raw - 1.5 if softplus else 0.02 + 0.3 * torch.sigmoid(raw)
    t["A"] = -torch.exp(0.3 * r(dim, N)) * (1.0 + torch.arange(N, dtype=torch.float64))[None]
    bshape = (batch, N, L) if groups is None else (batch, groups, N, L)
    t["B"] = r(*bshape) + _wave(bshape, *(0.9, 0.45, 0.17, 0.06)[-len(bshape):])
    t["C"] = r(*bshape) + _wave(bshape, *(0.5, 0.33, 0.23, 0.09)[-len(bshape):], phase=1.0)
    t["D"] = r(dim) if has_D else None
    t["z"] = r(batch, dim, L) if has_z else None
    bias = r(dim)
    t["delta_bias"] = (0.5 * bias if softplus else 0.1 * bias.abs()) if has_bias else None
    dout = r(batch, dim, L) + _wave((batch, dim, L), 0.4, 0.19, 0.13)
    return t, dout


def structured(batch, dim, L):
    """Deterministic values that differ per channel, per state and per step (no two of B, C, u, dt alike)."""
    t = {"u": 0.5 + 0.4 * _wave((batch, dim, L), 1.1, 0.37, 0.05),
         "B": 1.0 + 0.5 * _wave((batch, N, L), 0.9, 0.41, 0.07),
         "C": -0.7 + 0.6 * _wave((batch, N, L), 0.3, 0.29, 0.13, phase=2.0),
         "dt": 0.05 + 0.04 * (1.0 + _wave((batch, dim, L), 0.6, 0.23, 0.17, phase=0.5)),
         "A": -(0.2 + 0.1 * torch.arange(N, dtype=torch.float64))[None] * (1.0 + 0.05 * torch.arange(dim, dtype=torch.float64))[:, None],
         "D": 0.3 + 0.1 * torch.arange(dim, dtype=torch.float64),
         "z": 1.5 * _wave((batch, dim, L), 0.8, 0.31, 0.19, phase=1.0)}
    return t


def running_sum_answer(dt, B, C, u):
    """A = 0: y_l = sum_n C[n,l] sum_{k<=l} dt_k B[n,k] u_k."""
    inner = torch.cumsum(dt[:, :, None, :] * B[:, None] * u[:, :, None, :], dim=-1)
    return (C[:, None] * inner).sum(2)


def impulse_answer(dt, A, B, C, amp, k):
    """u = amp[b,d] at step k[b] and 0 elsewhere: y_l = sum_n C[n,l] dt_k B[n,k] amp exp(A sum_{k<j<=l} dt_j) for l >= k, else 0."""
    batch, dim, L = dt.shape
    y = torch.zeros(batch, dim, L, dtype=dt.dtype)
    for b in range(batch):
        kb = int(k[b])
        decay = torch.cumsum(dt[b, :, kb:], dim=-1) - dt[b, :, kb:kb + 1]          # sum_{k<j<=l} dt_j, (D, L-k)
        x = dt[b, :, kb, None, None] * B[b, None, :, kb, None] * amp[b, :, None, None] * torch.exp(A[:, :, None] * decay[:, None, :])
        y[b, :, kb:] = (C[b, None, :, kb:] * x).sum(1)
    return y


# ---- the error measure -------------------------------------------------------------------------------------------------------------
def norm_err(got, want64):
    want64, got = want64.detach().double(), got.detach()
    scale = float(want64.abs().max())
    return float((got.double().cpu() - want64).abs().max()) / scale if scale > 0 else float(got.double().abs().max())


def bar(yardstick):
    return max(FACTOR * yardstick, FLOOR)


def run_with_grads(fn, t, dout, **kw):
    """out and the gradient of every given tensor of t (dict in GRAD_NAMES order) for d(sum out * dout), detached."""
    leaves = {k: (v.detach().clone().requires_grad_(True) if v is not None else None) for k, v in t.items()}
    out = fn(leaves["u"], leaves["delta"], leaves["A"], leaves["B"], leaves["C"], leaves["D"], z=leaves["z"],
             delta_bias=leaves["delta_bias"], **kw)
    (out * dout.to(out.device, out.dtype)).sum().backward()
    return out.detach(), {k: (v.grad.detach() if v is not None else None) for k, v in leaves.items()}


def cast(t, dtype, device="cpu"):
    return {k: (v.to(device=device, dtype=dtype) if v is not None else None) for k, v in t.items()}


def yardstick_case(t64, dout64, **kw):
    """(out64, grads64, {'out' | name: yardstick}) of a case: the fp32 run of the loop against its fp64 run."""
    o64, g64 = run_with_grads(selective_scan, t64, dout64, **kw)
    o32, g32 = run_with_grads(selective_scan, cast(t64, torch.float32), dout64.float(), **kw)
    ys = {"out": norm_err(o32, o64)}
    for k in GRAD_NAMES:
        if g64[k] is not None:
            ys[k] = norm_err(g32[k], g64[k])
    return o64, g64, ys
