"""Python view of feature-guided upsampling (include/rt_hip.h: rt_guided_upsample, rt_guided_upsample_host, rt_render_upsampled):
a frame traced at half the width and half the height, brought to full size over full-resolution first-hit feature buffers.
Plumbing only: every pixel is computed by the library.
"""
import ctypes as C

import numpy as np

from . import ctypes_abi as abi
from .guided import _device_frame, _device_plane, _host_frame, _host_plane, _params as _guided_params, default_sigma_position
from .native import lib as _lib, last_error
from .scene import HostScene, make_image


def _params(sigma_normal, sigma_position, demodulate, guide_samples=0):
    return abi.RT_Upsample_Params(sigma_normal=sigma_normal, sigma_position=sigma_position, demodulate=1 if demodulate else 0,
                                  guide_samples=int(guide_samples))


def guided_upsample(color_low, low, full, sigma_normal=0.2, sigma_position=None, demodulate=True, image=False, out=True, lib=None):
    """The upsampled frame: float32 (h, w, 3), and with image=True the pair (upsampled, its uint8 encoding (h, w, 3)); out=False
    (with image=True): (None, the encoding).  color_low is (h / 2, w / 2, 3); low and full are dicts of coverage (.., ..), albedo,
    normal, position (.., .., 3) at the low and at the full size (albedo may be None when demodulate is False; full needs no
    colour).  numpy arrays go through rt_guided_upsample_host; torch GPU tensors through rt_guided_upsample on torch's current
    stream, with a torch tensor as the work buffer (the call only enqueues).  sigma_position=None: default_sigma_position() of the
    full-resolution planes."""
    lib = lib or _lib
    if sigma_position is None:
        sigma_position = default_sigma_position(full["position"], full["coverage"])
    params = _params(sigma_normal, sigma_position, demodulate)
    h, w = full["coverage"].shape
    if tuple(low["coverage"].shape) != (h // 2, w // 2) or (w | h) & 1:
        raise ValueError(f"the low planes must be ({h} / 2, {w} / 2) and the full size even, not {tuple(low['coverage'].shape)}")
    order = ("coverage", "albedo", "normal", "position")
    if isinstance(color_low, np.ndarray):
        col, low_planes, _keep_low = _host_frame(color_low, *[low[k] for k in order])
        fp = C.POINTER(C.c_float)
        arrays = [_host_plane(full["coverage"], (h, w), "coverage")] + [
            None if full[k] is None else _host_plane(full[k], (h, w, 3), k) for k in order[1:]]
        full_planes = abi.RT_Features(*[None if a is None else a.ctypes.data_as(fp) for a in arrays])
        res = np.zeros((h, w, 3), np.float32) if out else None
        img = np.zeros((h, w, 3), np.uint8) if image else None
        if lib.rt_guided_upsample_host(w, h, C.byref(params), col, C.byref(low_planes), C.byref(full_planes),
                                       res.ctypes.data if out else None, img.ctypes.data if image else None) != 0:
            raise RuntimeError("rt_guided_upsample_host failed: " + last_error(lib))
        return (res, img) if image else res
    import torch
    dev = color_low.device
    low_frame = _device_frame(color_low, *[low[k] for k in order])
    full_frame = [_device_plane(full["coverage"], (h, w), "coverage", dev)] + [
        None if full[k] is None else _device_plane(full[k], (h, w, 3), k, dev) for k in order[1:]]
    with torch.cuda.device(dev):
        n_work = lib.rt_guided_upsample_work_bytes(w, h)
        if n_work < 0:
            raise RuntimeError("rt_guided_upsample_work_bytes failed: " + last_error(lib))
        # (allocated under the current stream, on which the launches run: the caching allocator reuses it in stream order)
        work = torch.empty((n_work,), dtype=torch.uint8, device=dev)
        res = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if out else None
        img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev) if image else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        if lib.rt_guided_upsample(w, h, C.byref(params), *low_frame, *full_frame, res.data_ptr() if out else None,
                                  img.data_ptr() if image else None, work.data_ptr(), stream) != 0:
            raise RuntimeError("rt_guided_upsample failed: " + last_error(lib))
    return (res, img) if image else res


def render_upsampled(hs: HostScene, width, height, samples, max_bounces, seed=0x1234ABCD, guide_samples=0, sigma_normal=0.2,
                     sigma_position=None, demodulate=True, guided=None, lib=None) -> dict:
    """One frame through rt_render_upsampled: the path frame at (width / 2, height / 2), upsampled to (width, height) over a
    full-resolution feature pass of guide_samples samples (0: samples).  dict(image uint8 (h, w, 3) = the encoding of the last
    stage, linear_low float32 (h / 2, w / 2, 3), linear_upsampled float32 (h, w, 3), and with guided linear_out float32 (h, w, 3)).
    guided: None, or a dict of guided_denoise()'s parameters (iterations, sigma_color, sigma_normal, sigma_position, demodulate)
    for the filter over the upsampled frame.  sigma_position is a world-space length and required (of `guided` too)."""
    lib = lib or _lib
    if sigma_position is None:
        raise ValueError("render_upsampled needs sigma_position, a world-space length (guided.default_sigma_position)")
    lib.rt_set_seed(seed)
    params = _params(sigma_normal, sigma_position, demodulate, guide_samples)
    gp = None
    if guided is not None:
        kw = dict(iterations=4, sigma_color=1.0, sigma_normal=0.2, sigma_position=sigma_position, demodulate=True)
        kw.update(guided)
        gp = _guided_params(**kw)
    out = np.zeros((height, width, 3), np.uint8)
    img, _keep = make_image(out)
    img.pixels.data = out.ctypes.data
    low = np.zeros((height // 2, width // 2, 3), np.float32)
    up = np.zeros((height, width, 3), np.float32)
    clean = np.zeros((height, width, 3), np.float32) if gp is not None else None
    if lib.rt_render_upsampled(C.byref(hs.scene), C.byref(img), samples, max_bounces, C.byref(params),
                               None if gp is None else C.byref(gp), low.ctypes.data, up.ctypes.data,
                               None if clean is None else clean.ctypes.data) != 0:
        raise RuntimeError("rt_render_upsampled failed: " + last_error(lib))
    res = dict(image=out, linear_low=low, linear_upsampled=up)
    if clean is not None:
        res["linear_out"] = clean
    return res
