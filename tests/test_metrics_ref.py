"""PSNR / SSIM without a GPU: the header against the module's binding table, the library's host arithmetic, the CPU restatement
(tests/metrics_ref.py) against what the reference's own `ssim` and PSNR line returned (tests/golden/g18_metrics.npz, made by
tests/golden/make_g18_metrics.py), the analytic gradient against finite differences, the tolerance record and the aggregation."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest

import metrics_ref as MR
from conftest import ROOT

CASES = ("noise", "smooth", "render", "identical", "constant_constant", "constant_zero", "one_channel", "small", "pixel")
_DECLARATION = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s+\w+)?\s*\*?)\s*\b(u3d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", re.M)


def _declared_functions():
    """{name: (return type, [parameter type, ...])} of every u3d_* function include/unipre3d_metrics.h declares (comments and
    preprocessor lines stripped; a pointer parameter's type ends in '*')."""
    hdr = open(os.path.join(ROOT, "include", "unipre3d_metrics.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    out = {}
    for ret, name, params in _DECLARATION.findall(hdr):
        types = []
        for p in (q.strip() for q in params.split(",")):
            if p in ("", "void"):
                continue
            types.append(p[:p.rindex("*") + 1].replace(" ", "") if "*" in p else " ".join(p.split()[:-1]))
        assert name not in out, name
        out[name] = (" ".join(ret.split()), types)
    return out


def test_header_and_binding_agree():
    metrics = importlib.import_module("unipre3d_amd.metrics")
    declared = _declared_functions()
    assert set(declared) == set(metrics.EXPORTS) == {"u3d_metrics_tiles", "u3d_metrics_forward", "u3d_metrics_ssim_backward"}
    assert len(set(metrics.EXPORTS)) == len(metrics.EXPORTS)
    assert declared["u3d_metrics_tiles"][1] == ["int"] * 3
    assert declared["u3d_metrics_forward"][1] == ["int"] * 4 + ["constfloat*", "constfloat*", "float*", "float*", "float*", "int32_t*",
                                                                  "float*", "void*"]
    assert declared["u3d_metrics_ssim_backward"][1] == ["int"] * 4 + ["constfloat*"] * 4 + ["float*", "void*"]
    handle = metrics.load()
    for name, (ret, params) in declared.items():
        fn = getattr(handle, name)
        assert ret == "int" and fn.restype is ctypes.c_int, name
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for c_type, bound in zip(params, fn.argtypes):
            assert bound is (ctypes.c_void_p if c_type.endswith("*") else ctypes.c_int), (name, c_type, bound)
    hdr = open(os.path.join(ROOT, "include", "unipre3d_metrics.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (U3D_METRICS_\w+) (\d+)", hdr, re.M)}
    assert consts == {"U3D_METRICS_TILE": metrics.TILE, "U3D_METRICS_HALO": metrics.HALO} and metrics.HALO == MR.R == 5


def test_library_carries_no_switches():
    from unipre3d_amd import metrics
    blob = open(metrics.LIB_PATH, "rb").read()
    assert b"U3D_" not in blob and b"getenv" not in blob


def test_host_arithmetic_and_refusals():
    """u3d_metrics_tiles is host arithmetic; the launchers' argument checks return before anything touches a device."""
    from unipre3d_amd import metrics
    lib, T = metrics.load(), metrics.TILE
    tiles = lib.u3d_metrics_tiles
    assert (tiles(1, 1, 1), tiles(3, T, T), tiles(3, T + 1, T), tiles(3, T, T + 1), tiles(1, 2 * T + 3, 2 * T + 3)) == (1, 3, 6, 6, 9)
    assert (tiles(3, 128, 128), tiles(3, 120, 160), tiles(3, 480, 640)) == (48, 60, 900)
    assert (tiles(0, 8, 8), tiles(3, 0, 8), tiles(3, 8, 0), tiles(-1, 8, 8), tiles(3, -8, 8)) == (0, 0, 0, 0, 0)
    assert tiles(1, 2**31 - 1, 1) == (2**31 - 1 + T - 1) // T                   # no 32-bit wrap in the tile count
    assert tiles(1, 2**31 - 1, 2**31 - 1) == 0 and tiles(2**31 - 1, 2**31 - 1, 2**31 - 1) == 0 and tiles(2**31 - 1, T, T + 1) == 0
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)                        # never dereferenced: every call below returns first
    fwd, bwd = lib.u3d_metrics_forward, lib.u3d_metrics_ssim_backward
    assert fwd(-1, 3, 8, 8, one, one, one, one, one, one, null, null) == 1
    assert fwd(1, 0, 8, 8, one, one, one, one, one, one, null, null) == 1
    assert fwd(1, 3, 0, 8, one, one, one, one, one, one, null, null) == 1
    assert fwd(2**31 - 1, 3, 8, 8, one, one, one, one, one, one, null, null) == 1         # n * tiles beyond 2^31 - 1
    for k in range(6):                                                          # each mandatory pointer
        args = [one] * 6
        args[k] = null
        assert fwd(1, 3, 8, 8, *args, null, null) == 1, k
    assert fwd(0, 3, 8, 8, null, null, null, null, null, null, null, null) == 0           # empty call: no launch
    assert bwd(-1, 3, 8, 8, one, one, one, one, one, null) == 1 and bwd(1, 3, 8, 0, one, one, one, one, one, null) == 1
    for k in range(5):
        args = [one] * 5
        args[k] = null
        assert bwd(1, 3, 8, 8, *args, null) == 1, k
    assert bwd(0, 3, 8, 8, null, null, null, null, null, null) == 0


def test_python_surface_refuses_before_any_launch():
    import torch
    from unipre3d_amd import metrics
    a = torch.zeros(2, 3, 8, 8)
    for fn in (metrics.ssim, metrics.psnr, metrics.image_metrics):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.evaluate_views(a, a, 2, 1)
    with pytest.raises(NotImplementedError, match="11-tap"):
        metrics.ssim(a, a, window_size=7)
    with pytest.raises(NotImplementedError, match="swap"):
        metrics.ssim(a, a.clone().requires_grad_(True))


def test_golden_layout(golden):
    z = golden("g18_metrics.npz")
    assert MR.case_names(z) == list(CASES)
    keys = ("img1", "img2", "ssim32", "ssim64", "grad32", "grad64", "psnr32", "psnr64")
    assert sorted(z.files) == sorted(["names", "window"] + [f"{c}_{k}" for c in CASES for k in keys])
    assert z["window"].dtype == np.float32 and np.array_equal(z["window"], MR.WINDOW)     # the reference's gaussian(11, 1.5)
    src = open(os.path.join(ROOT, "unipre3d_amd", "csrc", "u3d_metrics.hip")).read()
    taps = [float.fromhex(h) for h in re.findall(r"(0x1\.[0-9a-f]+p-\d+)f", re.search(r"#define U3D_METRICS_WINDOW(.*?)\n\n", src, re.S).group(1))]
    assert taps == [float(v) for v in MR.WINDOW]                                # the kernel's taps, bit for bit
    for c in CASES:
        a = z[f"{c}_img1"]
        assert a.dtype == np.float32 and a.ndim == 4 and z[f"{c}_img2"].shape == a.shape and max(a.shape[2:]) <= 53
        for tag, dt in (("32", np.float32), ("64", np.float64)):
            assert z[f"{c}_ssim{tag}"].dtype == dt and z[f"{c}_ssim{tag}"].shape == a.shape[:1]
            assert z[f"{c}_grad{tag}"].dtype == dt and z[f"{c}_grad{tag}"].shape == a.shape
            assert z[f"{c}_psnr{tag}"].dtype == dt and z[f"{c}_psnr{tag}"].shape == a.shape[:1]
    assert z["noise_img1"].shape == (2, 3, 37, 53) and z["one_channel_img1"].shape[1] == 1
    assert z["small_img1"].shape[2:] == (9, 7) and z["pixel_img1"].shape[2:] == (1, 1)
    assert np.array_equal(z["identical_img1"], z["identical_img2"]) and not z["constant_zero_img2"].any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g18_metrics.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_mamba.npz"))


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_is_the_references_fp64(golden, case):
    """Same 2-D window, same formula: agreement to fp64 rounding, forward, gradient and PSNR."""
    z = golden("g18_metrics.npz")
    a, b = z[f"{case}_img1"], z[f"{case}_img2"]
    assert np.abs(MR.ssim_f64(a, b) - z[f"{case}_ssim64"]).max() < 1e-12
    g = MR.ssim_grad(a, b)
    assert np.abs(g - z[f"{case}_grad64"]).max() < 1e-12 * max(1.0, np.abs(g).max())
    p, want = MR.psnr(a, b), z[f"{case}_psnr64"]
    assert np.array_equal(np.isinf(p), np.isinf(want)) and np.allclose(p[np.isfinite(p)], want[np.isfinite(want)], rtol=0, atol=1e-11)
    if case in ("identical", "constant_constant"):
        assert np.isposinf(want).all() and np.abs(z[f"{case}_ssim64"] - 1).max() < 1e-12 and np.abs(z[f"{case}_grad64"]).max() < 1e-12


@pytest.mark.parametrize("case", CASES)
def test_fp32_restatement_within_the_bars(golden, case):
    """The fp32 separable form and its gradient against bar = 2 x yardstick + floor, and the recorded floors against what the
    restatement measures now (the floors may not be smaller than the distance they were set from)."""
    z, tol = golden("g18_metrics.npz"), MR.load_tolerance()
    d, bar, y = MR.restatement_distances(case, z), MR.bars(case, z, tol), MR.yardsticks(case, z)
    row = {r["case"]: r for r in tol["cases"]}[case]
    for k in ("ssim", "psnr", "grad"):
        print(f"{case} {k}: restatement {d[k]:.3e}  yardstick {y[k]:.3e}  bar {bar[k]:.3e}")
        assert d[k] <= bar[k], (case, k, d[k], bar[k])
        assert row[f"{k}_yardstick"] == pytest.approx(y[k], rel=1e-9, abs=1e-30)
        floor = tol["floors"]["grad_max_abs_degenerate" if k == "grad" and case in MR.DEGENERATE else "grad_rel_l2" if k == "grad" else k]
        assert d[k] <= floor * (1 + 1e-6)
    if case in MR.DEGENERATE:
        a, b = z[f"{case}_img1"], z[f"{case}_img2"]
        assert np.abs(MR.ssim_f32(a, b).astype(np.float64) - 1).max() <= bar["ssim"]


def test_tolerance_record():
    tol = MR.load_tolerance()
    assert [r["case"] for r in tol["cases"]] == list(CASES)
    assert set(tol["floors"]) == {"ssim", "psnr", "grad_rel_l2", "grad_max_abs_degenerate"}
    for k, v in tol["floors"].items():
        assert 0 < v < (1e-4 if k == "grad_rel_l2" else 1e-5), (k, v)           # fp32 rounding, not a licence
    for r in tol["cases"]:
        for k in ("ssim", "psnr", "grad"):
            assert r[f"{k}_restatement_f32"] <= tol["floors"]["grad_max_abs_degenerate" if k == "grad" and r["case"] in MR.DEGENERATE
                                                               else "grad_rel_l2" if k == "grad" else k]
            assert f"{k}_kernel_worst" in r


def test_analytic_gradient_against_finite_differences():
    """The fp64 analytic form is pinned by central differences of the fp64 forward on a shape with borders everywhere (the window
    leaves the image on both sides at once) and non-uniform per-image weights."""
    rng = np.random.default_rng(7)
    a, b = rng.uniform(0, 1, (2, 2, 7, 9)), rng.uniform(0, 1, (2, 2, 7, 9))
    w = np.array([0.7, -1.3])
    g = MR.ssim_grad(a, b, w)
    f = lambda x: float((w * MR.ssim_f64(x, b)).sum())
    eps, worst = 1e-6, 0.0
    for idx in [tuple(i) for i in np.argwhere(np.ones(a.shape, bool))][::5]:
        hi, lo = a.copy(), a.copy()
        hi[idx] += eps
        lo[idx] -= eps
        worst = max(worst, abs((f(hi) - f(lo)) / (2 * eps) - g[idx]))
    assert worst < 1e-8 * max(1.0, np.abs(g).max()), worst
    # the fp32 separable gradient is the same formula
    assert MR.rel_l2(MR.ssim_grad(a.astype(np.float32), b.astype(np.float32), w, np.float32), g) < 1e-5


def test_all_zero_counts_negative_zero():
    b = np.zeros((3, 1, 4, 4), np.float32)
    b[1] = -0.0
    b[2, 0, 3, 3] = 1e-30
    assert MR.all_zero(b).tolist() == [True, True, False]


def test_aggregation_hand_worked():
    """Two examples of four views, two of them conditioning; an invalid view in each class, and an example with no valid cond view."""
    psnr = [10.0, 20.0, 30.0, 40.0, 12.0, 14.0, 16.0, 18.0]
    ssim = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
    valid = [True, False, True, False, True, True, True, True]
    got = MR.evaluate_views_lists(psnr, ssim, valid, 4, 2)
    assert got["PSNR_cond"] == pytest.approx((10.0 + (12.0 + 14.0) / 2) / 2) and got["PSNR_novel"] == pytest.approx((30.0 + 17.0) / 2)
    assert got["SSIM_cond"] == pytest.approx((0.1 + 0.55) / 2) and got["SSIM_novel"] == pytest.approx((0.3 + 0.75) / 2)
    valid = [False, False, True, False, True, True, True, True]                 # example 0 has no valid cond view: left out of cond
    got = MR.evaluate_views_lists(psnr, ssim, valid, 4, 2)
    assert got["PSNR_cond"] == pytest.approx(13.0) and got["PSNR_novel"] == pytest.approx((30.0 + 17.0) / 2)
    got = MR.evaluate_views_lists(psnr, ssim, [False] * 8, 4, 2)
    assert all(math.isnan(v) for v in got.values())
    got = MR.evaluate_views_lists([float("inf"), 20.0], [1.0, 0.5], [True, True], 2, 1)
    assert got["PSNR_cond"] == float("inf") and got["PSNR_novel"] == 20.0
