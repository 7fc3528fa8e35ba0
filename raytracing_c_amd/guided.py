"""Python view of the guided denoiser (include/rt_hip.h: rt_guided_denoise, rt_guided_denoise_host, rt_render_denoised): the
edge-stopping a-trous filter of a linear frame over its first-hit feature buffers.  Plumbing only: every pixel is filtered by the
library; the one number computed here is the default sigma_position, a length taken from the position plane.
"""
import ctypes as C
import math

import numpy as np

from . import ctypes_abi as abi
from .native import lib as _lib, last_error
from .scene import HostScene, make_image


def default_sigma_position(position, coverage):
    """0.02 x the diagonal of the bounding box of `position` over the pixels with coverage 1; 1.0 when there is no such pixel (or
    the box has no extent).  numpy arrays or torch tensors."""
    if isinstance(position, np.ndarray):
        full = np.asarray(coverage) == 1.0
        if not full.any():
            return 1.0
        pts = position[full]
        lo, hi = pts.min(axis=0), pts.max(axis=0)
    else:
        full = coverage == 1.0
        if not bool(full.any()):
            return 1.0
        pts = position[full]
        lo, hi = pts.min(dim=0).values.cpu().numpy(), pts.max(dim=0).values.cpu().numpy()
    d = [float(hi[k]) - float(lo[k]) for k in range(3)]
    diag = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return 0.02 * diag if diag > 0.0 else 1.0


def _params(iterations, sigma_color, sigma_normal, sigma_position, demodulate):
    return abi.RT_Guided_Params(iterations=int(iterations), sigma_color=sigma_color, sigma_normal=sigma_normal,
                                sigma_position=sigma_position, demodulate=1 if demodulate else 0)


def _host_plane(a, shape, name):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {shape}, not {a.shape}")
    return a


def _device_plane(t, shape, name, device):
    import torch
    if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_cuda or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 GPU tensor of shape {shape} on {device}")
    return t.data_ptr()


def _frame(color, coverage, albedo, normal, position, plane):
    """(colour, coverage, albedo, normal, position), each through plane(array, shape, name); `albedo` may be None and stays None."""
    h, w = coverage.shape
    cov = plane(coverage, (h, w), "coverage")
    col, alb, nrm, pos = [None if a is None else plane(a, (h, w, 3), n)
                          for a, n in zip((color, albedo, normal, position), ("color", "albedo", "normal", "position"))]
    return col, cov, alb, nrm, pos


def _host_frame(*frame):
    """Of a frame in numpy arrays: (pointer to the colour, abi.RT_Features, the arrays the two point to)."""
    arrays = _frame(*frame, _host_plane)
    fp = C.POINTER(C.c_float)
    return arrays[0].ctypes.data, abi.RT_Features(*[None if a is None else a.ctypes.data_as(fp) for a in arrays[1:]]), arrays


def _device_frame(color, *planes):
    """Of a frame in torch GPU tensors on the colour's device: the five device pointers, in the C calls' order."""
    return _frame(color, *planes, lambda t, shape, name: _device_plane(t, shape, name, color.device))


def guided_denoise(color, coverage, albedo, normal, position, iterations=4, sigma_color=1.0, sigma_normal=0.2, sigma_position=None,
                   demodulate=True, image=False, lib=None):
    """The filtered frame: float32 (h, w, 3), and with image=True the pair (filtered, its uint8 encoding (h, w, 3)).
    numpy arrays go through rt_guided_denoise_host; torch GPU tensors through rt_guided_denoise on torch's current stream, with a
    torch tensor as the work buffer (the call only enqueues).  `albedo` may be None when demodulate is False.  sigma_position=None:
    default_sigma_position(position, coverage)."""
    lib = lib or _lib
    if sigma_position is None:
        sigma_position = default_sigma_position(position, coverage)
    params = _params(iterations, sigma_color, sigma_normal, sigma_position, demodulate)
    h, w = coverage.shape
    if isinstance(color, np.ndarray):
        col, planes, _keep = _host_frame(color, coverage, albedo, normal, position)
        out = np.zeros((h, w, 3), np.float32)
        img = np.zeros((h, w, 3), np.uint8) if image else None
        if lib.rt_guided_denoise_host(w, h, C.byref(params), col, C.byref(planes), out.ctypes.data,
                                      img.ctypes.data if image else None) != 0:
            raise RuntimeError("rt_guided_denoise_host failed: " + last_error(lib))
        return (out, img) if image else out
    import torch
    dev = color.device
    frame = _device_frame(color, coverage, albedo, normal, position)
    with torch.cuda.device(dev):
        n_work = lib.rt_guided_work_bytes(w, h)
        if n_work < 0:
            raise RuntimeError("rt_guided_work_bytes failed: " + last_error(lib))
        # (allocated under the current stream, on which the launches run: the caching allocator reuses it in stream order)
        work = torch.empty((n_work,), dtype=torch.uint8, device=dev)
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev) if image else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        if lib.rt_guided_denoise(w, h, C.byref(params), *frame, out.data_ptr(), img.data_ptr() if image else None, work.data_ptr(),
                                 stream) != 0:
            raise RuntimeError("rt_guided_denoise failed: " + last_error(lib))
    return (out, img) if image else out


def render_denoised(hs: HostScene, width, height, samples, max_bounces, seed=0x1234ABCD, iterations=4, sigma_color=1.0,
                    sigma_normal=0.2, sigma_position=None, demodulate=True, lib=None) -> dict:
    """One denoised frame through rt_render_denoised: dict(image uint8 (h, w, 3) = the encoded denoised frame, linear_noisy,
    linear_denoised float32 (h, w, 3)).  sigma_position=None: default_sigma_position() of a feature pass of the same frame
    shape, rendered first for that number alone -- give a world-space length to save it."""
    lib = lib or _lib
    if sigma_position is None:
        from .features import render_features
        planes = render_features(hs, width, height, samples, max_bounces, lib=lib)
        sigma_position = default_sigma_position(planes["position"], planes["coverage"])
    lib.rt_set_seed(seed)
    params = _params(iterations, sigma_color, sigma_normal, sigma_position, demodulate)
    out = np.zeros((height, width, 3), np.uint8)
    img, _keep = make_image(out)
    img.pixels.data = out.ctypes.data
    noisy = np.zeros((height, width, 3), np.float32)
    clean = np.zeros((height, width, 3), np.float32)
    if lib.rt_render_denoised(C.byref(hs.scene), C.byref(img), samples, max_bounces, C.byref(params), noisy.ctypes.data,
                              clean.ctypes.data) != 0:
        raise RuntimeError("rt_render_denoised failed: " + last_error(lib))
    return dict(image=out, linear_noisy=noisy, linear_denoised=clean)
