"""CPU restatement of unipre3d_amd/metrics.py (include/unipre3d_metrics.h), in numpy.

  ssim_f32        fp32, in the kernel's order: the 11-tap window applied separably (row pass, then column pass, taps 0..10 in turn,
                  every product and sum rounded in fp32), zero padding of 5 without renormalisation, then the map and its mean
  ssim_f64        fp64 with the reference's own 2-D window -- the fp32 outer product of the fp32 taps, as utils/loss_utils.py
                  `create_window` builds it -- so it reproduces the reference's fp64 result to rounding; the arbiter of the GPU tests
  ssim_grad       the analytic gradient of sum_i weight[i] * ssim[i] with respect to img1, the formula the kernel uses:
                  s_i (blur(d_mu1) + 2 img1 blur(d_sigma1^2) + img2 blur(d_sigma12)), s_i = weight[i] / (C H W); fp64 (2-D window)
                  or fp32 (separable)
  psnr            eval.py:28-30 per image, in the given precision
  all_zero        eval.py:122's `torch.all(target == 0)` per image
  evaluate_views_lists   the list-based aggregation of eval.py:121-176 over per-image values, with the one deviation of
                  unipre3d_amd.metrics.evaluate_views: an example without a valid view of a class is left out of that class's mean
  bars / distances       the tolerance rule of profiles/metrics/tolerance.json, shared by the CPU and the GPU tests"""
import json
import os

import numpy as np

WINDOW = np.array([float.fromhex(h) for h in ("0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3",
                                              "0x1.10656p-2", "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8",
                                              "0x1.0d956cp-10")], dtype=np.float32)     # gaussian(11, 1.5), recorded in g18_metrics.npz
R = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2
TOLERANCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "metrics", "tolerance.json")
DEGENERATE = ("identical", "constant_constant")


def _as4(x, dtype):
    x = np.asarray(x, dtype=dtype)
    return x[None] if x.ndim == 3 else x


def window2d():
    """create_window's (11, 11): the outer product of the fp32 taps, rounded in fp32."""
    return (WINDOW[:, None] * WINDOW[None, :]).astype(np.float32)


def blur_2d(x):
    """fp64, the reference's 2-D window, zero padding."""
    H, W = x.shape[-2:]
    w2 = window2d().astype(np.float64)
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(R, R), (R, R)])
    out = np.zeros_like(x)
    for i in range(11):
        for j in range(11):
            out += w2[i, j] * p[..., i:i + H, j:j + W]
    return out


def blur_separable(x):
    """The kernel's order in x's own precision: rows first (over the padded rows too: they are zero), then columns; tap k = 0..10."""
    H, W = x.shape[-2:]
    g = WINDOW.astype(x.dtype)
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(R, R), (R, R)])
    rows = np.zeros(p.shape[:-1] + (W,), dtype=x.dtype)
    for k in range(11):
        rows = rows + g[k] * p[..., :, k:k + W]
    out = np.zeros_like(x)
    for k in range(11):
        out = out + g[k] * rows[..., k:k + H, :]
    return out


def _maps(a, b, blur, want_grad):
    t = a.dtype.type
    c1, c2 = t(C1), t(C2)
    mu1, mu2 = blur(a), blur(b)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(a * a) - mu1_sq, blur(b * b) - mu2_sq, blur(a * b) - mu12
    A1, A2, B1, B2 = t(2) * mu12 + c1, t(2) * s12 + c2, mu1_sq + mu2_sq + c1, s1 + s2 + c2
    S = (A1 * A2) / (B1 * B2)
    if not want_grad:
        return S, None
    inv = t(1) / (B1 * B2)
    d_s1, d_s12 = -S / B2, t(2) * A1 * inv
    d_mu1 = t(2) * mu2 * A2 * inv - t(2) * mu1 * S / B1 - t(2) * mu1 * d_s1 - mu2 * d_s12
    return S, (d_mu1, d_s1, d_s12)


def ssim_f32(img1, img2):
    a, b = _as4(img1, np.float32), _as4(img2, np.float32)
    S, _ = _maps(a, b, blur_separable, False)
    return (S.reshape(S.shape[0], -1).sum(1, dtype=np.float32) / np.float32(S[0].size)).astype(np.float32)


def ssim_f64(img1, img2):
    a, b = _as4(img1, np.float64), _as4(img2, np.float64)
    S, _ = _maps(a, b, blur_2d, False)
    return S.reshape(S.shape[0], -1).mean(1)


def ssim_grad(img1, img2, weight=None, dtype=np.float64):
    """d(sum_i weight[i] * ssim[i]) / d img1 (weight None: ones), shaped like img1 as (N,C,H,W)."""
    a, b = _as4(img1, dtype), _as4(img2, dtype)
    blur = blur_2d if dtype == np.float64 else blur_separable
    w = np.ones(a.shape[0], dtype=dtype) if weight is None else np.asarray(weight, dtype=dtype)
    _, (d_mu1, d_s1, d_s12) = _maps(a, b, blur, True)
    scale = (w / a.dtype.type(a[0].size)).reshape(-1, 1, 1, 1)
    return scale * (blur(d_mu1) + a.dtype.type(2) * a * blur(d_s1) + b * blur(d_s12))


def psnr(images, targets, dtype=np.float64):
    a, b = _as4(images, dtype), _as4(targets, dtype)
    d = a - b
    with np.errstate(divide="ignore"):
        return (dtype(-10) * np.log10((d * d).reshape(d.shape[0], -1).mean(1, dtype=dtype))).astype(dtype)


def all_zero(targets):
    b = _as4(targets, np.float32)
    return (b == 0).reshape(b.shape[0], -1).all(1)


def evaluate_views_lists(psnr_n, ssim_n, valid_n, n_views, input_images):
    """eval.py:121-176 over per-image values (item-major): lists per example, `sum / len` per class, then `sum / len` over examples."""
    ex = {k: [] for k in ("PSNR_cond", "SSIM_cond", "PSNR_novel", "SSIM_novel")}
    for d in range(len(psnr_n) // n_views):
        views = {k: [] for k in ex}
        for r in range(n_views):
            i = d * n_views + r
            if valid_n[i]:
                cls = "cond" if r < input_images else "novel"
                views["PSNR_" + cls].append(float(psnr_n[i]))
                views["SSIM_" + cls].append(float(ssim_n[i]))
        for k, v in views.items():
            if v:                                              # (the reference divides by zero here)
                ex[k].append(sum(v) / len(v))
    return {k: (sum(v) / len(v) if v else float("nan")) for k, v in ex.items()}


# ---- the tolerance rule (profiles/metrics/tolerance.json) ----

def case_names(z):
    return [str(n) for n in z["names"]]


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


def _max_abs(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    both_inf = np.isinf(x) & np.isinf(ref) & (np.sign(x) == np.sign(ref))
    with np.errstate(invalid="ignore"):
        return float(np.max(np.where(both_inf, 0.0, np.abs(x - ref)), initial=0.0))


def distances(name, ssim_n, psnr_n, grad, z):
    """The three distances of one golden case's results from its fp64 record: max |ssim - ssim64| over images, max |psnr - psnr64|
    over images (two infinities of one sign are 0 apart), and the gradient's relative L2 -- its max-abs distance for a degenerate
    pair, whose true gradient is 0.  None entries are skipped."""
    out = {}
    if ssim_n is not None:
        out["ssim"] = _max_abs(ssim_n, z[f"{name}_ssim64"])
    if psnr_n is not None:
        out["psnr"] = _max_abs(psnr_n, z[f"{name}_psnr64"])
    if grad is not None:
        g64 = z[f"{name}_grad64"]
        out["grad"] = _max_abs(grad, g64) if name in DEGENERATE else rel_l2(grad, g64)
    return out


def yardsticks(name, z):
    """The distance of the reference's OWN fp32 results from its fp64 record.  For a degenerate pair the gradient's yardstick is the
    reference's fp32 max-abs gradient."""
    return distances(name, z[f"{name}_ssim32"], z[f"{name}_psnr32"], z[f"{name}_grad32"], z)


def load_tolerance():
    with open(TOLERANCE) as f:
        return json.load(f)


def bars(name, z, tol=None):
    """bar = 2 x yardstick + floor per quantity; the floors are recorded in tolerance.json (the fp32 restatement's largest distance from
    the fp64 record over the golden cases, measured on the CPU)."""
    tol = tol or load_tolerance()
    y, f = yardsticks(name, z), tol["floors"]
    return {"ssim": 2 * y["ssim"] + f["ssim"], "psnr": 2 * y["psnr"] + f["psnr"],
            "grad": 2 * y["grad"] + (f["grad_max_abs_degenerate"] if name in DEGENERATE else f["grad_rel_l2"])}


def restatement_distances(name, z):
    a, b = z[f"{name}_img1"], z[f"{name}_img2"]
    return distances(name, ssim_f32(a, b), psnr(a, b, np.float32), ssim_grad(a, b, None, np.float32), z)
