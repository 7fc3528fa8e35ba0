"""Python view of temporal accumulation (include/rt_hip.h: rt_temporal_accumulate, rt_temporal_accumulate_host, rt_history_*,
rt_render_temporal): the frame blended with the history of the frames before it, reprojected through the first hits.  Plumbing
only: every pixel is accumulated by the library.
"""
import ctypes as C

import numpy as np

from . import ctypes_abi as abi
from .guided import _device_frame, _device_plane, _host_frame, _host_plane, _params as _guided_params
from .native import lib as _lib, last_error
from .scene import HostScene, make_image

HISTORY_PLANES = ("color", "length", "coverage", "normal", "position")


def _params(alpha, max_history, normal_tolerance, plane_tolerance, demodulate):
    return abi.RT_Temporal_Params(alpha=alpha, max_history=int(max_history), normal_tolerance=normal_tolerance,
                                  plane_tolerance=plane_tolerance, demodulate=1 if demodulate else 0)


def as_camera(cam):
    """abi.Camera from an abi.Camera or a pair (view matrix (4, 4), focal_length)."""
    if isinstance(cam, abi.Camera):
        return cam
    matrix, focal = cam
    out = abi.Camera()
    m = np.asarray(matrix, dtype=np.float32).reshape(4, 4)
    for i in range(4):
        for j in range(4):
            out.view_matrix.rows[i][j] = float(m[i, j])
    out.focal_length = float(np.float32(focal))                 # (fov is not read by the accumulation)
    return out


def _history_planes(h, w, given=None):
    """(abi.RT_History_Planes, the arrays it points to) -- of `given` (a dict) or fresh."""
    fp = C.POINTER(C.c_float)
    arrays = {}
    for k in HISTORY_PLANES:
        shape = (h, w) if k in ("length", "coverage") else (h, w, 3)
        arrays[k] = np.zeros(shape, np.float32) if given is None else _host_plane(given[k], shape, "history " + k)
    return abi.RT_History_Planes(*[arrays[k].ctypes.data_as(fp) for k in HISTORY_PLANES]), arrays


def temporal_accumulate(color, coverage, albedo, normal, position, camera, previous_camera=None, history=None, alpha=0.05,
                        max_history=64, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=True, image=False, lib=None,
                        motion=None) -> dict:
    """One accumulation step: dict(out float32 (h, w, 3), length float32 (h, w), history, and with image=True image uint8 (h, w, 3)).
    numpy arrays go through rt_temporal_accumulate_host, and a history is a dict of the planes HISTORY_PLANES; torch GPU tensors go
    through rt_temporal_accumulate on torch's current stream (the call only enqueues), and a history is a float32 tensor
    (3, h, w, 4): the three planes of float4 records.  history=None: no history (previous_camera is not read).  `albedo` may be
    None when demodulate is False.  Cameras: abi.Camera or (view matrix, focal_length).  motion: None, or the (h, w, 3) float32
    motion plane of render_features(motion=True) -- THE ACCUMULATION WITH MOTION, through rt_temporal_accumulate_motion(_host)."""
    lib = lib or _lib
    params = _params(alpha, max_history, normal_tolerance, plane_tolerance, demodulate)
    cam = as_camera(camera)
    prev = None if previous_camera is None else as_camera(previous_camera)
    h, w = coverage.shape
    if isinstance(color, np.ndarray):
        col, planes, _keep_frame = _host_frame(color, coverage, albedo, normal, position)
        h_in, _keep = (None, None) if history is None else _history_planes(h, w, history)
        h_out, new = _history_planes(h, w)
        out = np.zeros((h, w, 3), np.float32)
        length = np.zeros((h, w), np.float32)
        img = np.zeros((h, w, 3), np.uint8) if image else None
        if motion is not None:
            mot = _host_plane(motion, (h, w, 3), "motion")
            if lib.rt_temporal_accumulate_motion_host(w, h, C.byref(params), C.byref(cam), None if prev is None else C.byref(prev), col,
                                                      C.byref(planes), None if h_in is None else C.byref(h_in), C.byref(h_out),
                                                      out.ctypes.data, length.ctypes.data, img.ctypes.data if image else None,
                                                      None, None, None, None, mot.ctypes.data) != 0:
                raise RuntimeError("rt_temporal_accumulate_motion_host failed: " + last_error(lib))
        elif lib.rt_temporal_accumulate_host(w, h, C.byref(params), C.byref(cam), None if prev is None else C.byref(prev), col,
                                           C.byref(planes), None if h_in is None else C.byref(h_in), C.byref(h_out), out.ctypes.data,
                                           length.ctypes.data, img.ctypes.data if image else None) != 0:
            raise RuntimeError("rt_temporal_accumulate_host failed: " + last_error(lib))
        res = dict(out=out, length=length, history=new)
        if image:
            res["image"] = img
        return res
    import torch
    dev = color.device
    frame = _device_frame(color, coverage, albedo, normal, position)
    h_in = None if history is None else _device_plane(history, (3, h, w, 4), "history", dev)
    mot = None if motion is None else _device_plane(motion, (h, w, 3), "motion", dev)
    with torch.cuda.device(dev):
        new = torch.empty((3, h, w, 4), dtype=torch.float32, device=dev)
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        length = torch.empty((h, w), dtype=torch.float32, device=dev)
        img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev) if image else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        if motion is not None:
            if lib.rt_temporal_accumulate_motion(w, h, C.byref(params), C.byref(cam), None if prev is None else C.byref(prev), *frame,
                                                 h_in, new.data_ptr(), out.data_ptr(), length.data_ptr(),
                                                 img.data_ptr() if image else None, None, None, None, None, stream, mot) != 0:
                raise RuntimeError("rt_temporal_accumulate_motion failed: " + last_error(lib))
        elif lib.rt_temporal_accumulate(w, h, C.byref(params), C.byref(cam), None if prev is None else C.byref(prev), *frame, h_in,
                                      new.data_ptr(), out.data_ptr(), length.data_ptr(), img.data_ptr() if image else None, stream) != 0:
            raise RuntimeError("rt_temporal_accumulate failed: " + last_error(lib))
    res = dict(out=out, length=length, history=new)
    if image:
        res["image"] = img
    return res


class History:
    """rt_history_create / rt_history_reset / rt_history_destroy: the history of one sequence, for render_temporal().
    motion=True: for a mesh deformed between the frames (rt_history_set_motion)."""

    def __init__(self, width, height, lib=None, motion=False):
        self.lib = lib or _lib
        self.width, self.height = int(width), int(height)
        self.handle = self.lib.rt_history_create(self.width, self.height)
        if not self.handle:
            raise RuntimeError("rt_history_create failed: " + last_error(self.lib))
        if motion:
            self.set_motion(True)

    def set_motion(self, on):
        """rt_history_set_motion: frames on this history use the motion feature pass and THE ACCUMULATION WITH MOTION, against the
        scene's kept geometry (HostScene.keep_geometry)."""
        if self.lib.rt_history_set_motion(self.handle, 1 if on else 0) != 0:
            raise RuntimeError("rt_history_set_motion failed: " + last_error(self.lib))

    def reset(self):
        if self.lib.rt_history_reset(self.handle) != 0:
            raise RuntimeError("rt_history_reset failed: " + last_error(self.lib))

    def close(self):
        if self.handle:
            self.lib.rt_history_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_temporal(hs: HostScene, width, height, samples, max_bounces, history: History, seed=0x1234ABCD, alpha=0.05, max_history=64,
                    normal_tolerance=0.3, plane_tolerance=0.02, demodulate=True, guided=None) -> dict:
    """One frame of a sequence through rt_render_temporal: dict(image uint8 (h, w, 3) = the encoding of the last stage,
    linear_noisy, linear_out float32 (h, w, 3), length float32 (h, w)).  guided: None, or a dict of guided_denoise()'s parameters
    (iterations, sigma_color, sigma_normal, sigma_position -- a world-space length, required -- and demodulate) to filter the
    accumulated frame."""
    lib = history.lib
    lib.rt_set_seed(seed)
    params = _params(alpha, max_history, normal_tolerance, plane_tolerance, demodulate)
    gp = None
    if guided is not None:
        g = dict(iterations=4, sigma_color=1.0, sigma_normal=0.2, demodulate=True)
        g.update(guided)
        gp = _guided_params(g["iterations"], g["sigma_color"], g["sigma_normal"], g["sigma_position"], g["demodulate"])
    out = np.zeros((height, width, 3), np.uint8)
    img, _keep = make_image(out)
    img.pixels.data = out.ctypes.data
    noisy = np.zeros((height, width, 3), np.float32)
    linear = np.zeros((height, width, 3), np.float32)
    length = np.zeros((height, width), np.float32)
    if lib.rt_render_temporal(C.byref(hs.scene), C.byref(img), samples, max_bounces, history.handle, C.byref(params),
                              None if gp is None else C.byref(gp), noisy.ctypes.data, linear.ctypes.data, length.ctypes.data) != 0:
        raise RuntimeError("rt_render_temporal failed: " + last_error(lib))
    return dict(image=out, linear_noisy=noisy, linear_out=linear, length=length)
