"""Python view of the batch ray queries (include/rt_hip.h): closest hit, occlusion and full hit records.

Host forms take numpy arrays and a HostScene (rt_scene_hits / rt_scene_closest / rt_scene_occluded); device forms take torch tensors on the GPU, an
uploaded device scene and a stream (rt_query_closest / rt_query_occluded).  Plumbing only: every hit is computed by the library.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import ctypes_abi as abi
from .native import lib as _lib, last_error
from .scene import HostScene


@dataclass
class QueryCounters:
    rays: int = 0
    hits: int = 0
    node_visits: int = 0
    leaf_visits: int = 0


def get_query_counters(lib=None) -> QueryCounters:
    lib = lib or _lib
    c = abi.RT_Query_Counters()
    if lib.rt_get_query_counters(C.byref(c)) != 0:
        raise RuntimeError(last_error(lib))
    return QueryCounters(*[int(getattr(c, f[0])) for f in c._fields_])


def _host_rays(rays):
    rays = np.ascontiguousarray(rays, np.float32)
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("rays must have shape (n, 6): origin, direction")
    return rays


def _host_bounds(t_max, n):
    if t_max is None:
        return None
    t_max = np.ascontiguousarray(t_max, np.float32)
    if t_max.shape != (n,):
        raise ValueError("t_max must have shape (n,)")
    return t_max


def closest_hits(hs: HostScene, rays, t_max=None, full=False, lib=None):
    """ray_scene_hit for every row of `rays` (n x 6 float32) with the upper bound t_max[i] (default: infinity).

    Returns a structured array of abi.RAY_HIT_DTYPE (t, triangle, u, v; a miss has triangle -1, t = its bound, u = v = 0) through
    rt_scene_closest, or with full=True a pair (hits of abi.HIT_DTYPE, triangles int32) through rt_scene_hits: the reference's
    Hit records, filled for the rays that hit and left as they were prepared (distance = the bound, everything else zero) for
    the others."""
    lib = lib or _lib
    rays = _host_rays(rays)
    n = len(rays)
    t_max = _host_bounds(t_max, n)
    if not full:
        out = np.zeros(n, abi.RAY_HIT_DTYPE)
        if lib.rt_scene_closest(C.byref(hs.scene), n, rays.ctypes.data, None if t_max is None else t_max.ctypes.data,
                                out.ctypes.data) != 0:
            raise RuntimeError("rt_scene_closest failed: " + last_error(lib))
        return out
    hits = np.zeros(n, abi.HIT_DTYPE)
    hits["distance"] = np.inf if t_max is None else t_max
    tri = np.zeros(n, np.int32)
    if lib.rt_scene_hits(C.byref(hs.scene), n, rays.ctypes.data, hits.ctypes.data, tri.ctypes.data) != 0:
        raise RuntimeError("rt_scene_hits failed: " + last_error(lib))
    return hits, tri


def occluded(hs: HostScene, rays, t_max=None, lib=None):
    """One uint8 per ray: 1 when the ray hits anything within (EPSILON, t_max[i]) (default bound: infinity)."""
    lib = lib or _lib
    rays = _host_rays(rays)
    n = len(rays)
    t_max = _host_bounds(t_max, n)
    flags = np.zeros(n, np.uint8)
    if lib.rt_scene_occluded(C.byref(hs.scene), n, rays.ctypes.data, None if t_max is None else t_max.ctypes.data,
                             flags.ctypes.data) != 0:
        raise RuntimeError("rt_scene_occluded failed: " + last_error(lib))
    return flags


def _device_args(rays, t_max, stream):
    import torch
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6 or not rays.is_cuda or not rays.is_contiguous():
        raise ValueError("rays must be a contiguous float32 GPU tensor of shape (n, 6)")
    n = rays.shape[0]
    if t_max is not None and (t_max.dtype != torch.float32 or tuple(t_max.shape) != (n,) or not t_max.is_cuda
                              or not t_max.is_contiguous()):
        raise ValueError("t_max must be a contiguous float32 GPU tensor of shape (n,)")
    s = stream if stream is not None else torch.cuda.current_stream(rays.device)
    return n, (t_max.data_ptr() if t_max is not None else None), s.cuda_stream


def closest_hits_device(dscene, rays, t_max=None, full=False, stream=None, lib=None):
    """rt_query_closest on torch tensors: enqueues on `stream` (default: torch's current stream) and returns a float32 tensor
    (n, 4) holding RT_Ray_Hit records (column 1 is the triangle index as int bits: .view(torch.int32)), and with full=True also
    an int32 tensor (n, 22) holding RT_Device_Hit records.  `dscene`: what rt_scene_upload returned."""
    import torch
    lib = lib or _lib
    n, tp, sp = _device_args(rays, t_max, stream)
    hits = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
    rec = torch.empty((n, 22), dtype=torch.int32, device=rays.device) if full else None
    if lib.rt_query_closest(dscene, n, rays.data_ptr(), tp, hits.data_ptr(), rec.data_ptr() if full else None, sp) != 0:
        raise RuntimeError("rt_query_closest failed: " + last_error(lib))
    return (hits, rec) if full else hits


def occluded_device(dscene, rays, t_max=None, stream=None, lib=None):
    """rt_query_occluded on torch tensors: enqueues on `stream` and returns a uint8 tensor (n,)."""
    import torch
    lib = lib or _lib
    n, tp, sp = _device_args(rays, t_max, stream)
    flags = torch.empty((n,), dtype=torch.uint8, device=rays.device)
    if lib.rt_query_occluded(dscene, n, rays.data_ptr(), tp, flags.data_ptr(), sp) != 0:
        raise RuntimeError("rt_query_occluded failed: " + last_error(lib))
    return flags
