"""MI355X-native render hot path behind the raytracing_c scene.h / raytracer.h boundary.

Python here is plumbing only (ctypes mirror of include/*.h, asset loading, the
multi-GPU launcher); every pixel is computed by librt_hip.so on gfx950.
"""
from . import ctypes_abi as abi          # noqa: F401
from .native import lib, diag, NativeLibraryMissing, last_error   # noqa: F401
from .scene import HostScene, build_scene, Material   # noqa: F401
from .background import procedural_background   # noqa: F401
from .loaders import load_model, default_camera, camera_from_trs   # noqa: F401
from .render import render_frame, render_views, render_context, frame_begin, frame_end, Counters   # noqa: F401
from .query import closest_hits, occluded, closest_hits_device, occluded_device, get_query_counters, QueryCounters   # noqa: F401
from .features import render_features   # noqa: F401
from .probes import (bake_probes, bake_probes_device, probe_grid, sh9_basis, sh9_radiance, sh9_irradiance, probe_visibility,   # noqa: F401
                     get_probe_counters)
from .lightmap import (bake_lightmap, bake_lightmap_device, lightmap_texels, dilate_lightmap, lightmap_vertices,   # noqa: F401
                       get_lightmap_counters)
from .guided import guided_denoise, render_denoised   # noqa: F401
from .temporal import temporal_accumulate, render_temporal, History   # noqa: F401
from .variance import temporal_accumulate_moments, guided_denoise_variance, render_svgf   # noqa: F401
from .upsample import guided_upsample, render_upsampled   # noqa: F401
from .adaptive import render_adaptive, render_accumulate_chunks, adaptive_merge, resolve_adaptive   # noqa: F401
