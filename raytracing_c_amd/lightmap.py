"""Python view of the HDR lightmaps (include/rt_hip.h, "HDR lightmaps"): the light arriving at the texels of a UV layout as a
float image, its order-free 32.32 sums, the texel list behind it and seam padding around the charts.

bake_lightmap takes a HostScene (rt_scene_lightmap); bake_lightmap_device takes an uploaded device scene, torch tensors and a stream
(rt_lightmap_texels / rt_lightmap_trace / rt_lightmap_resolve / rt_lightmap_dilate).  Plumbing only: every list entry, sum, texel
and filled texel is computed by the library.
"""
import ctypes as C

import numpy as np

from . import ctypes_abi as abi
from .native import lib as _lib, last_error
from .render import Counters
from .scene import HostScene


def get_lightmap_counters(lib=None) -> Counters:
    """Counters of the last lightmap trace of this process (rt_get_lightmap_counters)."""
    lib = lib or _lib
    c = abi.RT_Counters()
    if lib.rt_get_lightmap_counters(C.byref(c)) != 0:
        raise RuntimeError(last_error(lib))
    return Counters(*[int(getattr(c, f[0])) for f in c._fields_])


def _params(lib, width, height, samples, max_bounces, scale, seed, sample_range):
    first, count = sample_range if sample_range is not None else (0, 0)
    return abi.RT_Lightmap_Params(width=width, height=height, samples=samples, sample_first=first, sample_count=count,
                                  max_bounces=max_bounces, seed=lib.rt_get_seed() if seed is None else seed, scale=scale)


def lightmap_vertices(hs: HostScene):
    """(slots, 9) float32: per triangle slot x0 x1 x2 y0 y1 y2 z0 z1 z2 of the ORIGINAL vertices (triangles.x/y/z[k][i]) -- what
    rt_lightmap_texels reads as d_vertices."""
    T = hs.scene.triangles
    n = int(T.len)
    out = np.empty((n, 9), np.float32)
    for a, ax in enumerate("xyz"):
        for k in range(3):
            out[:, a * 3 + k] = np.ctypeslib.as_array(getattr(T, ax)[k], (n,))
    return out


def bake_lightmap(hs: HostScene, width, height, samples, max_bounces=8, scale=1.0, dilate=0, seed=None, *, sample_range=None,
                  return_sums=False, return_texels=False, lib=None):
    """The lightmap (height, width, 4) float32 of the scene's UV layout: per owned texel the mean over `samples` cosine-weighted
    paths times `scale` (1.0: the number the reference computes before its u8 store; 2 pi: the irradiance) and .w = 1; texels nobody
    owns are 0 with .w = 0, or -- after `dilate` passes of seam padding -- the mean of their filled neighbours with .w = 1 + pass.
    seed: default rt_get_seed(); sample_range = (first, count): trace only those samples (the image is then that range's share of
    the mean).  return_sums: also the (n, 3) uint64 sums per list entry; return_texels: also the list, (n,) of
    abi.LIGHTMAP_TEXEL_DTYPE.  Returns the image, or a tuple in that order."""
    lib = lib or _lib
    p = _params(lib, width, height, samples, max_bounces, scale, seed, sample_range)
    room = max(width, 0) * max(height, 0)
    image = np.zeros((max(height, 0), max(width, 0), 4), np.float32)
    sums = np.zeros((room, 3), np.uint64) if return_sums else None
    texels = np.zeros(room, abi.LIGHTMAP_TEXEL_DTYPE) if return_texels else None
    n = C.c_int64(0)
    if lib.rt_scene_lightmap(C.byref(hs.scene), C.byref(p), dilate, image.ctypes.data, sums.ctypes.data if return_sums else None,
                             texels.ctypes.data if return_texels else None, C.byref(n)) != 0:
        raise RuntimeError("rt_scene_lightmap failed: " + last_error(lib))
    out = (image,) + ((sums[:n.value],) if return_sums else ()) + ((texels[:n.value],) if return_texels else ())
    return out[0] if len(out) == 1 else out


def lightmap_texels(dscene, vertices, width, height, *, stream=None, lib=None):
    """The texel list of a width x height map on the device: `vertices` a contiguous float32 GPU tensor (slots, 9)
    (lightmap_vertices), `dscene` what rt_scene_upload returned.  Returns (texels, n): a float32 tensor (n, 8) holding the
    RT_Lightmap_Texel entries (a view of the front of a width x height buffer) and the list's length.  Synchronises the stream to
    read the length."""
    import torch
    lib = lib or _lib
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 9 or not vertices.is_cuda \
            or not vertices.is_contiguous():
        raise ValueError("vertices must be a contiguous float32 GPU tensor of shape (slots, 9)")
    st = stream if stream is not None else torch.cuda.current_stream(vertices.device)
    room = max(width, 0) * max(height, 0)
    with torch.cuda.stream(st):
        owner = torch.empty(room + max(height, 0), dtype=torch.int32, device=vertices.device)
        texels = torch.empty((room, 8), dtype=torch.float32, device=vertices.device)
        count = torch.zeros(1, dtype=torch.int64, device=vertices.device)
    if lib.rt_lightmap_texels(dscene, vertices.data_ptr(), width, height, owner.data_ptr(), texels.data_ptr(), count.data_ptr(),
                              st.cuda_stream) != 0:
        raise RuntimeError("rt_lightmap_texels failed: " + last_error(lib))
    st.synchronize()
    n = int(count.item())
    return texels[:n], n


def dilate_lightmap(image, passes, *, stream=None, lib=None):
    """`passes` passes of seam padding over `image`, a contiguous float32 GPU tensor (height, width, 4), in place
    (rt_lightmap_dilate); returns it."""
    import torch
    lib = lib or _lib
    if image.dtype != torch.float32 or image.dim() != 3 or image.shape[2] != 4 or not image.is_cuda or not image.is_contiguous():
        raise ValueError("image must be a contiguous float32 GPU tensor of shape (height, width, 4)")
    st = stream if stream is not None else torch.cuda.current_stream(image.device)
    with torch.cuda.stream(st):
        work = torch.empty_like(image)
    if lib.rt_lightmap_dilate(image.shape[1], image.shape[0], passes, image.data_ptr(), work.data_ptr(), st.cuda_stream) != 0:
        raise RuntimeError("rt_lightmap_dilate failed: " + last_error(lib))
    work.record_stream(st)
    return image


def bake_lightmap_device(dscene, vertices, width, height, samples, max_bounces=8, scale=1.0, dilate=0, seed=None, *,
                         sample_range=None, texels=None, sums=None, return_sums=False, return_texels=False, stream=None, lib=None):
    """bake_lightmap on torch tensors.  texels: the (n, 8) list of an earlier lightmap_texels call for this map (default: built
    here); sums: an int64 tensor (n, 3) to ADD this sample range to (default: a zeroed one).  Enqueues trace, resolve and dilation on
    `stream` (default: torch's current stream) and returns the image, a float32 tensor (height, width, 4), plus -- return_sums --
    the int64 tensor holding the u64 sums and -- return_texels -- the list."""
    import torch
    lib = lib or _lib
    p = _params(lib, width, height, samples, max_bounces, scale, seed, sample_range)
    st = stream if stream is not None else torch.cuda.current_stream(vertices.device)
    if texels is None:
        texels, n = lightmap_texels(dscene, vertices, width, height, stream=st, lib=lib)
    n = int(texels.shape[0])
    with torch.cuda.stream(st):
        if sums is None:
            sums = torch.zeros((n, 3), dtype=torch.int64, device=vertices.device)
        elif sums.dtype != torch.int64 or tuple(sums.shape) != (n, 3) or not sums.is_cuda or not sums.is_contiguous():
            raise ValueError("sums must be a contiguous int64 GPU tensor of shape (n, 3)")
        image = torch.empty((height, width, 4), dtype=torch.float32, device=vertices.device)
    if n and lib.rt_lightmap_trace(dscene, C.byref(p), texels.data_ptr(), 0, n, sums.data_ptr(), st.cuda_stream) != 0:
        raise RuntimeError("rt_lightmap_trace failed: " + last_error(lib))
    if lib.rt_lightmap_resolve(C.byref(p), n, texels.data_ptr() if n else None, sums.data_ptr() if n else None, image.data_ptr(),
                               st.cuda_stream) != 0:
        raise RuntimeError("rt_lightmap_resolve failed: " + last_error(lib))
    if dilate:
        dilate_lightmap(image, dilate, stream=st, lib=lib)
    out = (image,) + ((sums,) if return_sums else ()) + ((texels,) if return_texels else ())
    return out[0] if len(out) == 1 else out
