"""Every launching entry point of the bindings' EXPORTS tables is named in some tests/test_gpu_owned_*.py (the guard-zone tests of
tests/guarded.py), so that a library or an entry point added later cannot stay outside them unnoticed.  No GPU and no built library:
the binding modules are imported, nothing is loaded.

Two lists are exempt.  HOST_ONLY: entry points that launch nothing and write no device memory (versions, size and class queries, process
state).  RASTERIZER: the ten render entry points of libunipre3d_rasterizer.so, which take up to 27 pointers and four scratch regions sized
by u3d_scratch_query -- a sitting of its own; they leave the list when their test is written.  Neither list may hold a name that no
module exports."""
import importlib
import pkgutil
import re
from pathlib import Path

HOST_ONLY = {
    # versions, error text, profiling hooks (host state and host pointers)
    "u3d_abi_version", "u3d_error_string", "u3d_profile_begin", "u3d_profile_end", "u3d_attn_abi_version", "u3d_mambaops_abi_version",
    "u3d_feature_propagation_abi_version", "u3d_fusion_abi_version", "u3d_lnp_abi_version", "u3d_local_grouper_abi_version",
    "u3d_mha_abi_version", "u3d_pointfusion_abi_version", "u3d_sscan_abi_version", "u3d_ser_abi_version", "u3d_spconv_abi_version",
    # sizes of caller-provided buffers
    "u3d_scratch_query", "u3d_cconv_bwd_scratch_bytes", "u3d_addnorm_bwd_scratch_bytes", "u3d_feature_propagation_scratch_bytes",
    "u3d_zbuffer_fusion_zbuf_bytes", "u3d_lnp_scratch_bytes", "u3d_local_grouper_scratch_bytes", "u3d_pointfusion_scratch_bytes",
    "u3d_fps_grid_workspace_bytes", "u3d_sscan_bwd_scratch_bytes", "u3d_ser_scratch_bytes", "u3d_spconv_scratch_bytes",
    "u3d_spconv_wgrad_partial_floats", "u3d_spconv_colsum_partial_floats",
    # which kernel a shape launches, and the constants behind that choice
    "u3d_cconv_chunk_len", "u3d_addnorm_max_n", "u3d_addnorm_bwd_waves", "u3d_knn_path", "u3d_metrics_tiles", "u3d_sscan_pass_len",
    "u3d_fps_grid_points_per_workgroup", "u3d_group_points_grad_rows", "u3d_three_interpolate_grad_rows", "u3d_group_points_form",
    "u3d_three_interpolate_form",
    # process-wide mode of the point operators
    "u3d_pointops_set_contraction", "u3d_pointops_get_contraction",
}
# up to 27 pointers and four scratch regions sized by u3d_scratch_query per call: their guard-zone tests are a pull request of their own
RASTERIZER = {
    "u3d_rasterize_forward", "u3d_rasterize_backward", "u3d_render_loss_forward", "u3d_render_loss_backward", "u3d_render_loss_step",
    "u3d_render_loss_step_forward", "u3d_render_loss_step_backward", "u3d_render_view_forward", "u3d_render_view_backward", "u3d_mark_visible",
}

TESTS = Path(__file__).resolve().parent


def _exports():
    """{binding module name: its EXPORTS}"""
    import unipre3d_amd
    out = {}
    for m in pkgutil.iter_modules(unipre3d_amd.__path__):
        text = (Path(unipre3d_amd.__path__[0]) / f"{m.name}.py")
        if m.ispkg or not text.exists() or not re.search(r"^EXPORTS\s*=", text.read_text(), re.M):
            continue
        out[m.name] = tuple(importlib.import_module(f"unipre3d_amd.{m.name}").EXPORTS)
    return out


def _owned_text():
    files = sorted(TESTS.glob("test_gpu_owned_*.py"))
    assert len(files) >= 16, [f.name for f in files]
    return {f.name: f.read_text() for f in files}


def test_every_launching_entry_point_is_named_in_an_owned_test():
    exports, text = _exports(), _owned_text()
    assert len(exports) >= 19 and {"pointops", "sparseconv", "fusion", "gradcheck", "_lib"} <= set(exports), sorted(exports)
    missing = {}
    for mod, names in exports.items():
        assert names and all(n.startswith("u3d_") for n in names), mod
        for n in names:
            if n in HOST_ONLY or n in RASTERIZER:
                continue
            if not any(re.search(rf"\b{n}\b", t) for t in text.values()):
                missing.setdefault(mod, []).append(n)
    assert not missing, f"entry points that no tests/test_gpu_owned_*.py names: {missing}"


def test_the_exempt_lists_hold_only_exported_names():
    exported = {n for names in _exports().values() for n in names}
    assert HOST_ONLY <= exported, sorted(HOST_ONLY - exported)
    assert RASTERIZER <= exported and len(RASTERIZER) == 10, sorted(RASTERIZER - exported)
    assert not HOST_ONLY & RASTERIZER


def test_every_owned_test_file_is_marked_gpu_and_runs_under_both_poisons():
    for name, t in _owned_text().items():
        assert re.search(r"^pytestmark = (\[)?pytest\.mark\.gpu", t, re.M), name
        assert "run_twice" in t, name
