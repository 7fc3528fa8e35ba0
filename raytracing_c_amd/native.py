"""Loads librt_hip.so (built in-tree by raytracing_c_amd/csrc/Makefile) and declares prototypes.

There is no Python or CPU implementation behind this module: if the shared library is missing
the import of `lib` raises NativeLibraryMissing.
"""
import ctypes as C
import os

from . import ctypes_abi as abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_LIB_PATH: A/B a differently built librt_hip.so (tools/exp_ab.sh); the default is the in-tree build.
LIB_PATH = os.environ.get("RT_LIB_PATH") or os.path.join(_HERE, "librt_hip.so")
# The diagnostic build (make diag): unit-test entry points (include/rt_hip_diag.h), the wavefront pipeline, host units
# that read the RT_* experiment knobs.  Tests and experiments load it BESIDE the product library as `raytracing_c_amd.diag`.
DIAG_PATH = os.path.join(_HERE, "librt_hip_diag.so")


class NativeLibraryMissing(RuntimeError):
    pass


def _preload_hip_runtime():
    """One HIP runtime per process.

    librt_hip.so needs `libamdhip64.so.7`; PyTorch-ROCm ships its own copy of that library and
    loads it by the unversioned name, so whichever is mapped first must serve both (two HSA
    runtimes in one process cannot both own the GPU: the second reports "No HIP GPUs").
    When torch is installed, map ITS copy first -- the multi-GPU launcher and the tests share
    device buffers with torch.  RT_HIP_RUNTIME=system keeps the ROCm installation's runtime
    (for processes that never import torch).
    """
    import importlib.util
    import sys
    if os.environ.get("RT_HIP_RUNTIME", "torch") != "torch":
        return
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


class _Lazy:
    """Resolves the shared library on first attribute access."""

    def __init__(self, path, diag=False):
        self._dll = None
        self._path = path
        self._diag = diag

    def _load(self):
        if self._dll is not None:
            return self._dll
        if not os.path.exists(self._path):
            raise NativeLibraryMissing(
                f"{self._path} not found: build it with `make -C raytracing_c_amd/csrc{' diag' if self._diag else ''}` "
                "(or __graft_entry__.build()); there is no CPU fallback for the render path")
        _preload_hip_runtime()
        dll = C.CDLL(self._path)
        _declare(dll)
        if self._diag or hasattr(dll, "rt_test_math"):
            _declare_diag(dll)
        if self._diag and os.path.realpath(self._path) != os.path.realpath(LIB_PATH):
            # scenes are built with the PRODUCT library's material tokens (scene.py): make the diagnostic library accept them
            dll.rt_diag_set_tokens(symbol_address("disney_shader_proc"), symbol_address("debug_shader_proc"),
                                   symbol_address("sample_background"))
        self._dll = dll
        return dll

    def __getattr__(self, name):
        return getattr(self._load(), name)


def _declare(d):
    P = C.POINTER
    vp = C.c_void_p
    d.rt_last_error.restype = C.c_char_p
    d.rt_clear_error.restype = None
    d.rt_init.argtypes = [C.c_int]
    d.rt_set_seed.argtypes = [C.c_uint32]
    d.rt_set_seed.restype = None
    d.rt_get_seed.restype = C.c_uint32
    d.scene_init.argtypes = [P(abi.Scene), abi.Triangle_Slice, abi.Allocator]
    d.scene_init.restype = None
    d.scene_init_sah.argtypes = [P(abi.Scene), abi.Triangle_Slice, abi.Allocator]
    d.scene_init_sah.restype = None
    d.scene_init_gpu.argtypes = [P(abi.Scene), abi.Triangle_Slice, abi.Allocator]
    if hasattr(d, "scene_refit"):                          # (absent from older builds loaded as A/B partners)
        d.rt_scene_slot_map.argtypes = [P(abi.Scene), abi.Triangle_Slice, vp]
        d.rt_scene_slot_map.restype = C.c_ssize_t
        d.scene_refit.argtypes = [P(abi.Scene), abi.Triangle_Slice, vp]
        d.scene_refit_gpu.argtypes = [P(abi.Scene), abi.Triangle_Slice, vp]
    d.rt_scene_alloc.argtypes = [P(abi.Scene), abi.isize, abi.Allocator]
    d.rt_scene_alloc.restype = C.c_bool
    d.rt_scene_free.argtypes = [P(abi.Scene)]
    d.rt_scene_free.restype = None
    d.scene_load_bytes.argtypes = [abi.Byte_Slice, P(abi.Scene)]
    d.scene_load_bytes.restype = C.c_bool
    d.scene_save_bytes.argtypes = [P(abi.Scene), vp, C.c_ssize_t]
    d.scene_save_bytes.restype = C.c_ssize_t
    d.scene_file_size.argtypes = [P(abi.Scene)]
    d.scene_file_size.restype = C.c_ssize_t
    d.rt_scene_upload.argtypes = [P(abi.Scene)]
    d.rt_scene_upload.restype = vp
    d.rt_scene_release.argtypes = [vp]
    d.rt_scene_release.restype = None
    d.rt_scene_invalidate.argtypes = [P(abi.Scene)]
    d.rt_scene_invalidate.restype = None
    d.rt_scene_device_bytes.argtypes = [vp]
    d.rt_scene_device_bytes.restype = C.c_int64
    d.rt_set_camera.argtypes = [vp, P(abi.Camera)]
    d.rt_chunk_count.argtypes = [C.c_int32, C.c_int32]
    d.rt_local_chunk_count.argtypes = [C.c_int32] * 4
    d.rt_chunk_owner.argtypes = [C.c_int32] * 4
    d.rt_max_local_chunk_count.argtypes = [C.c_int32] * 3
    d.rt_local_chunk_list.argtypes = [C.c_int32] * 4 + [P(C.c_int32), C.c_int32]
    d.rt_render_accumulate.argtypes = [vp, P(abi.RT_Render_Params), vp, vp]
    d.rt_resolve.argtypes = [P(abi.RT_Render_Params), vp, vp, vp, vp, vp]
    d.rt_untile.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    d.rt_render_frame.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize, vp, vp]
    if hasattr(d, "rt_frame_begin"):                       # (absent from older builds loaded as A/B partners)
        d.rt_frame_begin.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize]
        d.rt_frame_end.argtypes = [C.c_int]
    if hasattr(d, "rt_render_views"):
        d.rt_render_views.argtypes = [P(abi.Scene), C.c_int32, P(abi.RT_View), P(abi.Image), abi.isize, abi.isize, vp, vp]
        d.rt_render_accumulate_views.argtypes = [vp, P(abi.RT_Render_Params), C.c_int32, P(abi.RT_View), vp, vp]
    if hasattr(d, "rt_query_closest"):
        d.rt_query_closest.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp]
        d.rt_query_occluded.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
        d.rt_scene_hits.argtypes = [P(abi.Scene), C.c_int64, vp, vp, vp]
        d.rt_scene_closest.argtypes = [P(abi.Scene), C.c_int64, vp, vp, vp]
        d.rt_scene_occluded.argtypes = [P(abi.Scene), C.c_int64, vp, vp, vp]
        d.rt_get_query_counters.argtypes = [P(abi.RT_Query_Counters)]
    if hasattr(d, "rt_render_features"):
        d.rt_render_accumulate_features.argtypes = [vp, P(abi.RT_Render_Params), vp, vp]
        d.rt_resolve_features.argtypes = [P(abi.RT_Render_Params), vp, vp, vp, vp, vp, vp]
        d.rt_render_features.argtypes = [P(abi.Scene), C.c_int32, C.c_int32, abi.isize, abi.isize, P(abi.RT_Features), vp]
    if hasattr(d, "rt_scene_probes"):                      # (absent from older builds loaded as A/B partners)
        d.rt_probe_trace.argtypes = [vp, P(abi.RT_Probe_Params), C.c_int64, vp, vp, vp]
        d.rt_probe_project.argtypes = [P(abi.RT_Probe_Params), C.c_int64, vp, vp, vp]
        d.rt_probe_resolve.argtypes = [P(abi.RT_Probe_Params), C.c_int64, vp, vp, vp]
        d.rt_scene_probes.argtypes = [P(abi.Scene), P(abi.RT_Probe_Params), C.c_int64, vp, vp, vp, vp]
        d.rt_get_probe_counters.argtypes = [P(abi.RT_Counters)]
    if hasattr(d, "rt_scene_lightmap"):
        d.rt_lightmap_texels.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        d.rt_lightmap_trace.argtypes = [vp, P(abi.RT_Lightmap_Params), vp, C.c_int64, C.c_int64, vp, vp]
        d.rt_lightmap_resolve.argtypes = [P(abi.RT_Lightmap_Params), C.c_int64, vp, vp, vp, vp]
        d.rt_lightmap_work_bytes.argtypes = [C.c_int32, C.c_int32]
        d.rt_lightmap_work_bytes.restype = C.c_int64
        d.rt_lightmap_dilate.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
        d.rt_scene_lightmap.argtypes = [P(abi.Scene), P(abi.RT_Lightmap_Params), C.c_int32, vp, vp, vp, P(C.c_int64)]
        d.rt_get_lightmap_counters.argtypes = [P(abi.RT_Counters)]
    if hasattr(d, "rt_guided_denoise"):
        d.rt_guided_work_bytes.argtypes = [C.c_int32, C.c_int32]
        d.rt_guided_work_bytes.restype = C.c_int64
        d.rt_guided_denoise.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Guided_Params)] + [vp] * 9
        d.rt_guided_denoise_host.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Guided_Params), vp, P(abi.RT_Features), vp, vp]
        d.rt_render_denoised.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize, P(abi.RT_Guided_Params), vp, vp]
    if hasattr(d, "rt_temporal_accumulate"):
        d.rt_temporal_history_bytes.argtypes = [C.c_int32, C.c_int32]
        d.rt_temporal_history_bytes.restype = C.c_int64
        d.rt_temporal_accumulate.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Temporal_Params), P(abi.Camera), P(abi.Camera)] + [vp] * 11
        d.rt_temporal_accumulate_host.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Temporal_Params), P(abi.Camera), P(abi.Camera), vp,
                                                  P(abi.RT_Features), P(abi.RT_History_Planes), P(abi.RT_History_Planes), vp, vp, vp]
        d.rt_history_create.argtypes = [C.c_int32, C.c_int32]
        d.rt_history_create.restype = vp
        d.rt_history_reset.argtypes = [vp]
        d.rt_history_destroy.argtypes = [vp]
        d.rt_history_destroy.restype = None
        d.rt_render_temporal.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize, vp, P(abi.RT_Temporal_Params),
                                         P(abi.RT_Guided_Params), vp, vp, vp]
    if hasattr(d, "rt_render_svgf"):
        d.rt_temporal_moments_bytes.argtypes = [C.c_int32, C.c_int32]
        d.rt_temporal_moments_bytes.restype = C.c_int64
        d.rt_temporal_accumulate_moments.argtypes = ([C.c_int32, C.c_int32, P(abi.RT_Temporal_Params), P(abi.Camera), P(abi.Camera)]
                                                     + [vp] * 10 + [P(abi.RT_Variance_Params)] + [vp] * 4)
        d.rt_temporal_accumulate_moments_host.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Temporal_Params), P(abi.Camera), P(abi.Camera),
                                                          vp, P(abi.RT_Features), P(abi.RT_History_Planes), P(abi.RT_History_Planes),
                                                          vp, vp, vp, P(abi.RT_Variance_Params), vp, vp, vp]
        d.rt_guided_variance_work_bytes.argtypes = [C.c_int32, C.c_int32]
        d.rt_guided_variance_work_bytes.restype = C.c_int64
        d.rt_guided_denoise_variance.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Guided_Params)] + [vp] * 11
        d.rt_guided_denoise_variance_host.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Guided_Params), vp, P(abi.RT_Features), vp, vp, vp,
                                                      vp]
        d.rt_render_svgf.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize, vp, P(abi.RT_Temporal_Params),
                                     P(abi.RT_Variance_Params), P(abi.RT_Guided_Params), vp, vp, vp, vp]
    if hasattr(d, "rt_render_upsampled"):                  # (absent from older builds loaded as A/B partners)
        d.rt_guided_upsample_work_bytes.argtypes = [C.c_int32, C.c_int32]
        d.rt_guided_upsample_work_bytes.restype = C.c_int64
        d.rt_guided_upsample.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Upsample_Params)] + [vp] * 13
        d.rt_guided_upsample_host.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Upsample_Params), vp, P(abi.RT_Features),
                                              P(abi.RT_Features), vp, vp]
        d.rt_render_upsampled.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize, P(abi.RT_Upsample_Params),
                                          P(abi.RT_Guided_Params), vp, vp, vp]
    if hasattr(d, "rt_render_adaptive"):                   # (absent from older builds loaded as A/B partners)
        d.rt_render_accumulate_chunks.argtypes = [vp, P(abi.RT_Render_Params), C.c_int32, vp, vp, vp]
        d.rt_adaptive_merge.argtypes = [C.c_int32] * 4 + [vp] * 5
        d.rt_resolve_adaptive.argtypes = [C.c_int32, C.c_int32] + [vp] * 6
        d.rt_render_adaptive.argtypes = [P(abi.Scene), P(abi.Image), P(abi.RT_Adaptive_Params), abi.isize, vp, vp, vp]
    if hasattr(d, "rt_scene_keep_geometry"):               # (absent from older builds loaded as A/B partners)
        d.rt_device_scene_keep_geometry.argtypes = [vp, vp]
        d.rt_scene_keep_geometry.argtypes = [P(abi.Scene)]
        d.rt_scene_has_kept_geometry.argtypes = [P(abi.Scene)]
        d.rt_render_accumulate_features_motion.argtypes = [vp, P(abi.RT_Render_Params), vp, vp, vp]
        d.rt_resolve_motion.argtypes = [P(abi.RT_Render_Params), vp, vp, vp]
        d.rt_render_features_motion.argtypes = [P(abi.Scene), C.c_int32, C.c_int32, abi.isize, abi.isize, P(abi.RT_Features), vp, vp, vp]
        d.rt_temporal_accumulate_motion.argtypes = ([C.c_int32, C.c_int32, P(abi.RT_Temporal_Params), P(abi.Camera), P(abi.Camera)]
                                                    + [vp] * 10 + [P(abi.RT_Variance_Params)] + [vp] * 5)
        d.rt_temporal_accumulate_motion_host.argtypes = [C.c_int32, C.c_int32, P(abi.RT_Temporal_Params), P(abi.Camera), P(abi.Camera),
                                                         vp, P(abi.RT_Features), P(abi.RT_History_Planes), P(abi.RT_History_Planes),
                                                         vp, vp, vp, P(abi.RT_Variance_Params), vp, vp, vp, vp]
        d.rt_history_set_motion.argtypes = [vp, C.c_int]
    d.rt_get_counters.argtypes = [P(abi.RT_Counters)]
    if hasattr(d, "rt_get_skipped_root_visits"):           # (absent from older builds that tools/exp_small_ab.sh loads as A/B partners)
        d.rt_get_skipped_root_visits.argtypes = [P(C.c_uint64)]
    if hasattr(d, "rt_get_leafless_paths"):
        d.rt_get_leafless_paths.argtypes = [P(C.c_uint64)]
    if hasattr(d, "rt_get_triangleless_paths"):
        d.rt_get_triangleless_paths.argtypes = [P(C.c_uint64)]
    if hasattr(d, "rt_get_fused_root_visits"):
        d.rt_get_fused_root_visits.argtypes = [P(C.c_uint64)]
    if hasattr(d, "rt_get_shade_taps_form"):               # (absent from older builds loaded as A/B partners)
        d.rt_get_shade_taps_form.argtypes = []
        d.rt_materials_share_taps.argtypes = [vp, C.c_int32]
    d.rt_math_contract.restype = C.c_int
    d.rt_last_kernel_ms.restype = C.c_float
    d.rt_kernel_timing_reset.restype = None
    d.rt_kernel_timing_mean_ms.argtypes = [P(C.c_int32)]
    d.rt_kernel_timing_mean_ms.restype = C.c_float
    d.rt_set_devices.argtypes = [C.c_int32, C.c_int32]
    d.rt_device_count.restype = C.c_int32
    d.rt_scene_verify.argtypes = [P(abi.Scene)]
    d.rt_scene_touch.argtypes = [P(abi.Scene), vp, C.c_size_t]
    d.rt_scene_set_static.argtypes = [P(abi.Scene), C.c_int32]
    d.rt_scene_set_static.restype = None
    d.rt_get_frame_timing.argtypes = [P(abi.RT_Frame_Timing)]
    d.render_thread_proc.argtypes = [P(abi.Rendering_Context)]
    d.render_thread_proc.restype = None
    d.rendering_context_is_finished.argtypes = [P(abi.Rendering_Context)]
    d.rendering_context_is_finished.restype = C.c_bool
    d.rendering_context_finish.argtypes = [P(abi.Rendering_Context)]
    d.rendering_context_finish.restype = None
    d.render.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize]
    d.lightmap_bake.argtypes = [P(abi.Image), P(abi.Scene), abi.isize]
    d.lightmap_bake.restype = None
    d.denoise_image.argtypes = [P(abi.Image), P(abi.Image), abi.isize]
    d.denoise_image.restype = None
    d.rt_denoise.argtypes = [C.c_int32, C.c_int32, vp, vp, vp]


def _declare_diag(d):
    """include/rt_hip_diag.h"""
    vp = C.c_void_p
    d.rt_test_math.argtypes = [C.c_int32, C.c_int32, vp, vp, vp]
    d.rt_test_rcp_sweep.argtypes = [vp]
    d.rt_test_srgb_sweep.argtypes = [vp]
    d.rt_test_env_sweep.argtypes = [C.c_int32, C.c_uint32, vp]
    d.rt_test_quantize_sweep.argtypes = [vp]
    d.rt_test_encode_sweep.argtypes = [vp]
    d.rt_test_group_sum.argtypes = [C.c_int32, C.c_int32, vp, vp, vp]
    d.rt_test_sky_add_group.argtypes = []
    d.rt_test_node_order.argtypes = [C.c_int32, vp, vp, vp]
    d.rt_test_trace.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    d.rt_test_texture.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
    d.rt_test_shade.argtypes = [vp, C.c_int32, C.c_int32] + [vp] * 7
    d.rt_test_shade_hit.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32] + [vp] * 8
    d.rt_test_feature_hit.argtypes = [vp, C.c_int32] + [vp] * 5
    d.rt_test_brdf.argtypes = [C.c_int32] + [vp] * 6
    d.rt_test_background.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
    d.rt_test_primary_ray.argtypes = [C.POINTER(abi.Camera), C.c_int32, C.c_int32, C.c_int32, vp, vp]
    d.rt_test_trace_stream.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    d.rt_test_tile_order.argtypes = [C.c_int32, vp, vp]
    d.rt_set_pipeline.argtypes = [C.c_int32]
    d.rt_get_pipeline.restype = C.c_int32
    d.rt_set_wavefront_capacity.argtypes = [C.c_int64]
    d.rt_set_wavefront_capacity.restype = None
    d.rt_get_wave_times.argtypes = [vp, C.c_int32]
    d.rt_get_ledger.argtypes = [vp, C.c_int32]
    d.rt_diag_device_bytes_live.argtypes = []
    d.rt_diag_device_bytes_live.restype = C.c_int64
    d.rt_diag_release_staging.argtypes = []
    d.rt_diag_cached_scene.argtypes = [C.POINTER(abi.Scene)]
    d.rt_diag_cached_scene.restype = vp
    d.rt_diag_multi_fault.argtypes = [C.c_int32, C.c_int32]
    d.rt_diag_multi_fault.restype = None
    d.rt_diag_set_tokens.argtypes = [vp, vp, vp]
    d.rt_diag_set_tokens.restype = None


lib = _Lazy(LIB_PATH)
diag = _Lazy(DIAG_PATH, diag=True)


def symbol_address(name):
    """Address of an exported function (used as Shader.proc / Background.proc token)."""
    return C.cast(getattr(lib, name), C.c_void_p).value


def last_error(which=None):
    return ((which or lib).rt_last_error() or b"").decode("utf-8", "replace")
