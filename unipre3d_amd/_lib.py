"""ctypes binding of libunipre3d_rasterizer.so (the C-ABI declared in include/unipre3d_rasterizer.h), and the loader and call helpers
every native library of the package is bound through (`open_library`, `call`, `on_device`, the argument coercions; `check`, `ptr` and
`stream_ptr` are the pieces the rasterizer path and the tests use directly).

The product path has NO CPU or PyTorch fallback: if the HIP library is missing or cannot be loaded,
`load()` raises.  `import torch` must precede the dlopen so that the library's libamdhip64.so.7
dependency resolves to the HIP runtime PyTorch-ROCm already loaded (one runtime per process, so torch's
streams and device pointers are valid inside the library).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import torch  # noqa: F401  (must be imported before the library is opened, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (experiments only: U3D_LIB_DIRNAME selects a kernel-variant build directory made with `make LIBDIR=../lib_x EXTRA=...`)
LIB_DIR = os.path.join(_HERE, os.environ.get("U3D_LIB_DIRNAME", "lib"))
LIB_PATH = os.path.join(LIB_DIR, "libunipre3d_rasterizer.so")
CSRC = os.path.join(_HERE, "csrc")

ABI_VERSION = 5   # include/unipre3d_rasterizer.h: U3D_ABI_VERSION
FLAG_PREFILTERED, FLAG_ANTIALIASING, FLAG_DEBUG, FLAG_EXACT_AA_GRAD, FLAG_STATS, FLAG_ACC_CLEAN, FLAG_SPARSE_BWD = 1, 2, 4, 8, 16, 32, 64

PROFILE_KINDS = ("preprocess_fwd", "depth_sort", "render_fwd", "render_bwd", "preprocess_bwd", "render_fb")


class RasterDesc(ctypes.Structure):
    _fields_ = [("n_items", ctypes.c_int32), ("views_per_item", ctypes.c_int32), ("P", ctypes.c_int32),
                ("image_height", ctypes.c_int32), ("image_width", ctypes.c_int32), ("tanfovx", ctypes.c_float),
                ("tanfovy", ctypes.c_float), ("scale_modifier", ctypes.c_float), ("sh_degree", ctypes.c_int32),
                ("sh_coeffs", ctypes.c_int32), ("flags", ctypes.c_int32),
                # ragged batches: sum of the sets' sizes (0 = every set has P) and the DEVICE pointer to the n_items + 1 prefix sums
                ("total_P", ctypes.c_int32), ("item_offsets", ctypes.c_void_p)]


class ScratchSizes(ctypes.Structure):
    _fields_ = [("geom_bytes", ctypes.c_size_t), ("binning_bytes", ctypes.c_size_t), ("image_bytes", ctypes.c_size_t),
                ("backward_bytes", ctypes.c_size_t), ("num_rendered_offset", ctypes.c_size_t),
                ("fused_bytes", ctypes.c_size_t)]


class HeadDesc(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("channels", ctypes.c_int32), ("offset_scale", ctypes.c_float),
                ("isotropic", ctypes.c_int32)]


class LossDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("non_bg_color_loss_rate", ctypes.c_float),
                ("bg_color_loss_rate", ctypes.c_float)]


LOSS_KINDS = {"l2": 1, "focal_l2": 2, "l1": 3}


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc build of libunipre3d_rasterizer.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout[-2000:])
    return LIB_PATH


_handles = {}


def open_library(file_name: str, signatures: dict, abi=None) -> ctypes.CDLL:
    """The library `file_name` of LIB_DIR, opened once and bound from its table: `signatures` maps every exported name to
    (restype, argtypes) and both are set for every entry; `abi` = (symbol, expected) is checked where the library exports a version.
    No fallback: a missing file raises."""
    key = (LIB_DIR, file_name)
    lib = _handles.get(key)
    if lib is None:
        path = os.path.join(LIB_DIR, file_name)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing (no fallback): run `make -C unipre3d_amd/csrc`")
        lib = ctypes.CDLL(path)
        for name, (restype, argtypes) in signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        if abi is not None:
            found = getattr(lib, abi[0])()
            if found != abi[1]:
                raise RuntimeError(f"{path}: ABI {found}, this module binds ABI {abi[1]}: rebuild (`make -C unipre3d_amd/csrc`)")
        _handles[key] = lib
    return lib


_vp, _int, _i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32
_desc, _head, _loss = ctypes.POINTER(RasterDesc), ctypes.POINTER(HeadDesc), ctypes.POINTER(LossDesc)
SIGNATURES = {   # include/unipre3d_rasterizer.h
    "u3d_abi_version": (_int, []),
    "u3d_error_string": (ctypes.c_char_p, [_int]),
    "u3d_scratch_query": (_int, [_desc, ctypes.POINTER(ScratchSizes)]),
    "u3d_rasterize_forward": (_int, [_desc] + [_vp] * 18),
    "u3d_rasterize_backward": (_int, [_desc] + [_vp] * 27),
    "u3d_render_loss_forward": (_int, [_desc, _head, _loss] + [_vp] * 15),
    "u3d_render_loss_backward": (_int, [_desc, _head, _loss] + [_vp] * 18),
    "u3d_render_loss_step": (_int, [_desc, _head, _loss] + [_vp] * 16),
    "u3d_render_loss_step_forward": (_int, [_desc, _head, _loss] + [_vp] * 16),
    "u3d_render_loss_step_backward": (_int, [_desc, _head] + [_vp] * 13),
    "u3d_render_view_forward": (_int, [_desc] + [_vp] * 17),
    "u3d_render_view_backward": (_int, [_desc] + [_vp] * 24),
    "u3d_mark_visible": (_int, [_i32, _vp, _vp, _vp, _vp, _vp]),
    "u3d_profile_begin": (_int, [_i32]),
    "u3d_profile_end": (_int, [_vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def load() -> ctypes.CDLL:
    return open_library("libunipre3d_rasterizer.so", SIGNATURES, ("u3d_abi_version", ABI_VERSION))


def check(code: int, what: str, named: bool = True) -> None:
    """Raises on a non-zero return code.  The rasterizer names its codes (u3d_error_string); the other libraries export no such
    table (named=False) and are called through `call`."""
    if code != 0:
        if named:
            raise RuntimeError(f"{what} failed: {load().u3d_error_string(code).decode()} (code {code})")
        raise RuntimeError(f"{what} failed with code {code}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(dev=None):
    """torch's CURRENT stream on the current device as a hipStream_t (the raw-handle query costs ~0.3 us, the Stream object
    route ~10 us per call).  The kernels are launched on the calling thread's current HIP device, so tensors on another
    device are refused instead of being launched against the wrong queue."""
    cur = torch.cuda.current_device()
    if dev is not None and dev.index is not None and dev.index != cur:
        raise RuntimeError(f"tensors live on cuda:{dev.index} but the current device is cuda:{cur}; "
                           f"call under torch.cuda.device({dev.index}) (one process per GPU sets it once)")
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(cur))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(module_name: str, *tensors):
    """The one HIP device the tensors (None entries skipped) live on; anything else raises -- there is no CPU path."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"unipre3d_amd.{module_name} needs tensors on a HIP device; there is no CPU fallback")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"unipre3d_amd.{module_name}: tensors on different devices ({dev}, {t.device})")
        dev = t.device
    return dev


def ptr(t) -> ctypes.c_void_p:
    """Device pointer of a tensor (None -> NULL)."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def call(fn, *args, dev, what=None, accept=()):
    """One launching entry point of a library opened by open_library: fn(*args, stream).  A tensor goes in as its device pointer
    (None stays NULL, everything else passes through), torch's current stream on `dev` comes last, as in every prototype under
    include/.  Returns the code when it is 0 or listed in `accept`; any other code raises under the name `what` (default: the symbol)."""
    code = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], stream_ptr(dev))
    if code != 0 and code not in accept:
        raise RuntimeError(f"{what or fn.__name__} failed with code {code}")
    return code


def scratch(nbytes: int, dev):
    """(tensor that owns the bytes, 256-byte aligned device pointer into it)."""
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return buf, ctypes.c_void_p((buf.data_ptr() + 255) & ~255)


def byte_buffer(nbytes: int, dev):
    """A uint8 tensor of `nbytes` bytes, at least 16 (a zero-size query still gets a real pointer), as the allocator aligns it."""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def as_f32(t, what):
    """The kernels read raw contiguous fp32: anything else (fp16/bf16 under autocast, float64, a strided view) is cast or copied,
    never reinterpreted."""
    if not t.is_floating_point():
        raise TypeError(f"{what} must be a floating-point tensor, got {t.dtype}")
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def as_i32(t, what):
    """Contiguous int32 indices from int32 or int64 (narrowed)."""
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what} must be an int32 or int64 tensor, got {t.dtype}")
    return (t if t.dtype == torch.int32 else t.int()).contiguous()


def dense(t, shape):
    """A contiguous, 16-byte aligned view (or copy) of a parameter in the library's shape, detached."""
    t = t.detach().reshape(shape).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def profile_begin(max_records: int = 65536, kinds=None, stride: int = 1) -> None:
    """kinds: iterable of PROFILE_KINDS names to record (None = all); stride: sample every stride-th launch of a kind (1..15).
    Each recorded scope costs ~4-5 us on the stream."""
    arg = max_records
    if kinds is not None or stride != 1:
        mask = 0
        for k in (kinds if kinds is not None else PROFILE_KINDS):
            mask |= 1 << PROFILE_KINDS.index(k)
        arg = -((max(1, min(int(stride), 15)) << 26) | (mask << 20) | min(max_records, 0xfffff))
    check(load().u3d_profile_begin(arg), "u3d_profile_begin")


def profile_end() -> dict:
    """{kind: (total_ms, launches)} for the kernels enqueued since profile_begin()."""
    ms = (ctypes.c_float * len(PROFILE_KINDS))()
    cnt = (ctypes.c_int32 * len(PROFILE_KINDS))()
    check(load().u3d_profile_end(ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(cnt, ctypes.c_void_p)), "u3d_profile_end")
    return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(PROFILE_KINDS)}
