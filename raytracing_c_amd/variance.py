"""Python view of variance-guided denoising (include/rt_hip.h: rt_temporal_accumulate_moments, rt_guided_denoise_variance,
rt_render_svgf and their host-level forms): the accumulation that carries luminance moments, the variance estimated from them and
the a-trous filter steered by that variance.  Plumbing only: every pixel is computed by the library.
"""
import ctypes as C

import numpy as np

from . import ctypes_abi as abi
from .guided import _device_frame, _device_plane, _host_frame, _host_plane, _params as _guided_params, default_sigma_position
from .native import lib as _lib, last_error
from .scene import HostScene, make_image
from .temporal import History, _history_planes, _params as _temporal_params, as_camera


def _variance_params(sigma_normal, sigma_position):
    return abi.RT_Variance_Params(sigma_normal=sigma_normal, sigma_position=sigma_position)


def temporal_accumulate_moments(color, coverage, albedo, normal, position, camera, previous_camera=None, history=None, moments=None,
                                alpha=0.05, max_history=64, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=True,
                                sigma_normal=0.2, sigma_position=None, image=False, lib=None, motion=None) -> dict:
    """temporal_accumulate() with the moments and the variance: dict(out, length, history, moments, variance float32 (h, w), and
    with image=True image).  numpy arrays go through rt_temporal_accumulate_moments_host and moments are float32 (h, w, 2); torch
    GPU tensors go through rt_temporal_accumulate_moments on torch's current stream and moments are float32 (h, w, 4): the records
    (m1, m2, 0, 0).  history and moments are given both or neither.  sigma_position=None: default_sigma_position(position,
    coverage).  motion: None, or the (h, w, 3) float32 motion plane of render_features(motion=True) -- the moments form of THE
    ACCUMULATION WITH MOTION, through rt_temporal_accumulate_motion(_host)."""
    lib = lib or _lib
    if sigma_position is None:
        sigma_position = default_sigma_position(position, coverage)
    params = _temporal_params(alpha, max_history, normal_tolerance, plane_tolerance, demodulate)
    vparams = _variance_params(sigma_normal, sigma_position)
    cam = as_camera(camera)
    prev = None if previous_camera is None else as_camera(previous_camera)
    h, w = coverage.shape
    if isinstance(color, np.ndarray):
        col, planes, _keep_frame = _host_frame(color, coverage, albedo, normal, position)
        h_in, _keep = (None, None) if history is None else _history_planes(h, w, history)
        h_out, new = _history_planes(h, w)
        m_in = None if moments is None else _host_plane(moments, (h, w, 2), "moments")
        out = np.zeros((h, w, 3), np.float32)
        length = np.zeros((h, w), np.float32)
        m_out = np.zeros((h, w, 2), np.float32)
        var = np.zeros((h, w), np.float32)
        img = np.zeros((h, w, 3), np.uint8) if image else None
        args = (w, h, C.byref(params), C.byref(cam), None if prev is None else C.byref(prev), col, C.byref(planes),
                None if h_in is None else C.byref(h_in), C.byref(h_out), out.ctypes.data, length.ctypes.data,
                img.ctypes.data if image else None, C.byref(vparams), None if m_in is None else m_in.ctypes.data, m_out.ctypes.data,
                var.ctypes.data)
        if motion is not None:
            mot = _host_plane(motion, (h, w, 3), "motion")
            if lib.rt_temporal_accumulate_motion_host(*args, mot.ctypes.data) != 0:
                raise RuntimeError("rt_temporal_accumulate_motion_host failed: " + last_error(lib))
        elif lib.rt_temporal_accumulate_moments_host(*args) != 0:
            raise RuntimeError("rt_temporal_accumulate_moments_host failed: " + last_error(lib))
        res = dict(out=out, length=length, history=new, moments=m_out, variance=var)
        if image:
            res["image"] = img
        return res
    import torch
    dev = color.device
    frame = _device_frame(color, coverage, albedo, normal, position)
    h_in = None if history is None else _device_plane(history, (3, h, w, 4), "history", dev)
    m_in = None if moments is None else _device_plane(moments, (h, w, 4), "moments", dev)
    mot = None if motion is None else _device_plane(motion, (h, w, 3), "motion", dev)
    with torch.cuda.device(dev):
        new = torch.empty((3, h, w, 4), dtype=torch.float32, device=dev)
        m_out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        length = torch.empty((h, w), dtype=torch.float32, device=dev)
        var = torch.empty((h, w), dtype=torch.float32, device=dev)
        img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev) if image else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (w, h, C.byref(params), C.byref(cam), None if prev is None else C.byref(prev), *frame, h_in, new.data_ptr(),
                out.data_ptr(), length.data_ptr(), img.data_ptr() if image else None, C.byref(vparams), m_in, m_out.data_ptr(),
                var.data_ptr(), stream)
        if motion is not None:
            if lib.rt_temporal_accumulate_motion(*args, mot) != 0:
                raise RuntimeError("rt_temporal_accumulate_motion failed: " + last_error(lib))
        elif lib.rt_temporal_accumulate_moments(*args) != 0:
            raise RuntimeError("rt_temporal_accumulate_moments failed: " + last_error(lib))
    res = dict(out=out, length=length, history=new, moments=m_out, variance=var)
    if image:
        res["image"] = img
    return res


def guided_denoise_variance(color, coverage, albedo, normal, position, variance, iterations=4, sigma_color=4.0, sigma_normal=0.2,
                            sigma_position=None, demodulate=True, image=False, lib=None) -> dict:
    """The variance-guided filter: dict(out float32 (h, w, 3), variance float32 (h, w) = the filtered variance, and with image=True
    image uint8 (h, w, 3)).  numpy arrays go through rt_guided_denoise_variance_host; torch GPU tensors through
    rt_guided_denoise_variance on torch's current stream.  sigma_color is a multiple of the pixel's standard deviation."""
    lib = lib or _lib
    if sigma_position is None:
        sigma_position = default_sigma_position(position, coverage)
    params = _guided_params(iterations, sigma_color, sigma_normal, sigma_position, demodulate)
    h, w = coverage.shape
    if isinstance(color, np.ndarray):
        col, planes, _keep = _host_frame(color, coverage, albedo, normal, position)
        var = _host_plane(variance, (h, w), "variance")
        out = np.zeros((h, w, 3), np.float32)
        var_out = np.zeros((h, w), np.float32)
        img = np.zeros((h, w, 3), np.uint8) if image else None
        if lib.rt_guided_denoise_variance_host(w, h, C.byref(params), col, C.byref(planes), out.ctypes.data,
                                               img.ctypes.data if image else None, var.ctypes.data, var_out.ctypes.data) != 0:
            raise RuntimeError("rt_guided_denoise_variance_host failed: " + last_error(lib))
    else:
        import torch
        dev = color.device
        frame = _device_frame(color, coverage, albedo, normal, position)
        var = _device_plane(variance, (h, w), "variance", dev)
        with torch.cuda.device(dev):
            n_work = lib.rt_guided_variance_work_bytes(w, h)
            if n_work < 0:
                raise RuntimeError("rt_guided_variance_work_bytes failed: " + last_error(lib))
            work = torch.empty((n_work,), dtype=torch.uint8, device=dev)
            out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            var_out = torch.empty((h, w), dtype=torch.float32, device=dev)
            img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev) if image else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            if lib.rt_guided_denoise_variance(w, h, C.byref(params), *frame, out.data_ptr(), img.data_ptr() if image else None,
                                              work.data_ptr(), stream, var, var_out.data_ptr()) != 0:
                raise RuntimeError("rt_guided_denoise_variance failed: " + last_error(lib))
    res = dict(out=out, variance=var_out)
    if image:
        res["image"] = img
    return res


def render_svgf(hs: HostScene, width, height, samples, max_bounces, history: History, seed=0x1234ABCD, alpha=0.05, max_history=64,
                normal_tolerance=0.3, plane_tolerance=0.02, demodulate=True, iterations=4, sigma_color=4.0, sigma_normal=0.2,
                sigma_position=None, variance_sigma_normal=None, variance_sigma_position=None) -> dict:
    """One frame of a sequence through rt_render_svgf: dict(image uint8 (h, w, 3) = the encoded filtered frame, linear_noisy,
    linear_out float32 (h, w, 3), length, variance float32 (h, w) = the filter's INPUT variance).  sigma_position is a world-space
    length and required; the variance estimate's sigmas default to the filter's."""
    if sigma_position is None:
        raise ValueError("render_svgf needs sigma_position, a world-space length (guided.default_sigma_position)")
    lib = history.lib
    lib.rt_set_seed(seed)
    params = _temporal_params(alpha, max_history, normal_tolerance, plane_tolerance, demodulate)
    gp = _guided_params(iterations, sigma_color, sigma_normal, sigma_position, demodulate)
    vparams = _variance_params(sigma_normal if variance_sigma_normal is None else variance_sigma_normal,
                               sigma_position if variance_sigma_position is None else variance_sigma_position)
    out = np.zeros((height, width, 3), np.uint8)
    img, _keep = make_image(out)
    img.pixels.data = out.ctypes.data
    noisy = np.zeros((height, width, 3), np.float32)
    linear = np.zeros((height, width, 3), np.float32)
    length = np.zeros((height, width), np.float32)
    var = np.zeros((height, width), np.float32)
    if lib.rt_render_svgf(C.byref(hs.scene), C.byref(img), samples, max_bounces, history.handle, C.byref(params), C.byref(vparams),
                          C.byref(gp), noisy.ctypes.data, linear.ctypes.data, length.ctypes.data, var.ctypes.data) != 0:
        raise RuntimeError("rt_render_svgf failed: " + last_error(lib))
    return dict(image=out, linear_noisy=noisy, linear_out=linear, length=length, variance=var)
