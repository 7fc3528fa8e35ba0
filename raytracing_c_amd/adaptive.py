"""Python view of adaptive sampling (include/rt_hip.h: rt_render_adaptive, rt_render_accumulate_chunks, rt_adaptive_merge,
rt_resolve_adaptive): chunks double their samples until their error settles.  Plumbing only: every sum, error and pixel is computed
by the library.
"""
import ctypes as C

import numpy as np

from . import ctypes_abi as abi
from .native import lib as _lib, last_error
from .render import get_counters
from .scene import HostScene, make_image

CHUNK = 32


def _chunk_array(chunks):
    a = np.ascontiguousarray(chunks, np.int32).reshape(-1)
    return a, (a.ctypes.data if a.size else None)


def render_accumulate_chunks(dscene, params, chunks, accum, stream=None, lib=None):
    """rt_render_accumulate with the caller's chunk list: `chunks` a strictly ascending sequence of global chunk indices, `accum` a
    torch int64 GPU tensor (h, w, 3) holding the u64 sums, `dscene` what rt_scene_upload returned.  Only enqueues work."""
    lib = lib or _lib
    a, ptr = _chunk_array(chunks)
    if lib.rt_render_accumulate_chunks(dscene, C.byref(params), a.size, ptr, accum.data_ptr(), stream) != 0:
        raise RuntimeError("rt_render_accumulate_chunks failed: " + last_error(lib))


def adaptive_merge(width, height, n, chunks, accum, fresh, err, stream=None, lib=None):
    """rt_adaptive_merge on torch int64 GPU tensors: accum, fresh (h, w, 3) and err (rt_chunk_count,) hold u64 values; the listed
    chunks' err entries are overwritten, accum += fresh and fresh = 0 in their pixels.  Only enqueues work."""
    lib = lib or _lib
    a, ptr = _chunk_array(chunks)
    if lib.rt_adaptive_merge(width, height, n, a.size, ptr, accum.data_ptr(), fresh.data_ptr(), err.data_ptr(), stream) != 0:
        raise RuntimeError("rt_adaptive_merge failed: " + last_error(lib))


def resolve_adaptive(width, height, chunk_samples, accum, image=None, linear=None, sample_map=None, stream=None, lib=None):
    """rt_resolve_adaptive on torch GPU tensors: chunk_samples int32 (rt_chunk_count,), accum int64 (h, w, 3); the outputs that are
    given are written: image uint8 (h, w, 3), linear float32 (h, w, 3), sample_map int32 (h, w).  Only enqueues work."""
    lib = lib or _lib
    ptr = lambda t: None if t is None else t.data_ptr()
    if lib.rt_resolve_adaptive(width, height, chunk_samples.data_ptr(), accum.data_ptr(), ptr(image), ptr(linear), ptr(sample_map),
                               stream) != 0:
        raise RuntimeError("rt_resolve_adaptive failed: " + last_error(lib))


def render_adaptive(hs: HostScene, width, height, min_samples, max_samples, threshold, max_bounces, seed=0x1234ABCD, lib=None) -> dict:
    """One frame through rt_render_adaptive: dict(image uint8 (h, w, 3), linear float32 (h, w, 3), accum uint64 (h, w, 3),
    chunk_samples int32 (chunks_y, chunks_x) = the samples every 32 x 32 chunk ended with, sample_map int32 (h, w) = the same per
    pixel, counters = rt_get_counters(), summed over the frame's launches)."""
    lib = lib or _lib
    lib.rt_set_seed(seed)
    params = abi.RT_Adaptive_Params(min_samples=min_samples, max_samples=max_samples, threshold=threshold, reserved=0)
    out = np.zeros((height, width, 3), np.uint8)
    img, _keep = make_image(out)
    img.pixels.data = out.ctypes.data
    linear = np.zeros((height, width, 3), np.float32)
    accum = np.zeros((height, width, 3), np.uint64)
    cy, cx = (height + CHUNK - 1) // CHUNK, (width + CHUNK - 1) // CHUNK
    counts = np.zeros((cy, cx), np.int32)
    if lib.rt_render_adaptive(C.byref(hs.scene), C.byref(img), C.byref(params), max_bounces, linear.ctypes.data, accum.ctypes.data,
                              counts.ctypes.data) != 0:
        raise RuntimeError("rt_render_adaptive failed: " + last_error(lib))
    sample_map = np.ascontiguousarray(np.repeat(np.repeat(counts, CHUNK, axis=0), CHUNK, axis=1)[:height, :width])
    return dict(image=out, linear=linear, accum=accum, chunk_samples=counts, sample_map=sample_map, counters=get_counters(lib))
