"""Python view of the first-hit feature buffers (include/rt_hip.h: rt_render_features): coverage, albedo, shading normal and world
position of what the camera sees.  Plumbing only: every value is computed by the library.
"""
import ctypes as C

import numpy as np

from . import ctypes_abi as abi
from .native import lib as _lib, last_error
from .scene import HostScene


def render_features(hs: HostScene, width, height, samples, max_bounces, lib=None, motion=False) -> dict:
    """The feature buffers of the frame (hs, width, height, samples, max_bounces) from hs.scene.camera: float32 arrays `coverage`
    (h, w), `albedo`, `normal`, `position` (h, w, 3) -- per pixel the mean over the frame's own samples -- and `sums` (h, w, 10)
    uint64, the 32.32 fixed-point sums they are resolved from (position: two's complement).  motion=True
    (rt_render_features_motion): also `motion` (h, w, 3) float32 and `motion_sums` (h, w, 3) uint64 -- where the first hits WERE in
    the scene's kept geometry (HostScene.keep_geometry) minus where they are, the mean over ALL samples like position; zero without
    kept geometry."""
    lib = lib or _lib
    out = dict(coverage=np.zeros((height, width), np.float32), albedo=np.zeros((height, width, 3), np.float32),
               normal=np.zeros((height, width, 3), np.float32), position=np.zeros((height, width, 3), np.float32),
               sums=np.zeros((height, width, abi.RT_FEATURE_CHANNELS), np.uint64))
    planes = abi.RT_Features(*[out[n].ctypes.data_as(C.POINTER(C.c_float)) for n in ("coverage", "albedo", "normal", "position")])
    if motion:
        out["motion"] = np.zeros((height, width, abi.RT_MOTION_CHANNELS), np.float32)
        out["motion_sums"] = np.zeros((height, width, abi.RT_MOTION_CHANNELS), np.uint64)
        if lib.rt_render_features_motion(C.byref(hs.scene), width, height, samples, max_bounces, C.byref(planes), out["sums"].ctypes.data,
                                         out["motion"].ctypes.data, out["motion_sums"].ctypes.data) != 0:
            raise RuntimeError("rt_render_features_motion failed: " + last_error(lib))
        return out
    if lib.rt_render_features(C.byref(hs.scene), width, height, samples, max_bounces, C.byref(planes), out["sums"].ctypes.data) != 0:
        raise RuntimeError("rt_render_features failed: " + last_error(lib))
    return out
