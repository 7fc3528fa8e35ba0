"""The refusals of the frame post passes (raytracing_c_amd/csrc/rt_post.cpp: the guided denoiser, temporal accumulation, the moments
and the variance-guided filter, the accumulation with motion, feature-guided upsampling) without a GPU: a table of bad calls at 4 x 4, every one of which fails before the device is
touched, and for each the return value and the WHOLE rt_last_error() text, as tests/golden/post_refusals.json recorded them.  A
row with two faults pins which check fires first, so the table is what a restructuring of the host side has to leave as it is.
The outputs are pre-filled with a sentinel and stay untouched.

The fixture was recorded once (`python -m tests.test_post_refusals record` writes the rows it has none for) from the library as it
was before rt_post.cpp's stages took a frame value and one struct of optional outputs each, and the rows of the motion and
upsampling entry points from the library as it was before upsampling was folded into the shared checks, uploads and stages; rows
are added to it, never changed."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

F32 = np.float32
W = H = 4
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_refusals.json")
NAN, INF = float("nan"), float("inf")
BIG = (1 << 15, (1 << 13) + 1)                      # more than 2^28 pixels


ENTRIES = ("rt_guided_work_bytes", "rt_temporal_history_bytes", "rt_guided_variance_work_bytes", "rt_temporal_moments_bytes",
           "rt_history_create", "rt_history_reset", "rt_guided_denoise", "rt_guided_denoise_variance", "rt_temporal_accumulate",
           "rt_temporal_accumulate_moments", "rt_guided_denoise_host", "rt_guided_denoise_variance_host",
           "rt_temporal_accumulate_host", "rt_temporal_accumulate_moments_host", "rt_render_denoised", "rt_render_temporal",
           "rt_render_svgf",
           "rt_history_set_motion", "rt_temporal_accumulate_motion", "rt_temporal_accumulate_motion_host",
           "rt_guided_upsample_work_bytes", "rt_guided_upsample", "rt_guided_upsample_host", "rt_render_upsampled")


class _Marker:
    """An argument built per call: a params struct, the planes, an Image -- with some fields replaced."""

    def __init__(self, kind, **fields):
        self.kind, self.fields = kind, fields


def G(**kw):
    return _Marker("guided", **kw)


def T(**kw):
    return _Marker("temporal", **kw)


def V(**kw):
    return _Marker("variance", **kw)


def U(**kw):
    return _Marker("upsample", **kw)


def FEATS(**kw):
    return _Marker("features", **kw)


def LOW(**kw):
    return _Marker("features_low", **kw)


def HIN(**kw):
    return _Marker("history_in", **kw)


def HOUT(**kw):
    return _Marker("history_out", **kw)


def IMG(**kw):
    return _Marker("image", **kw)


class Context:
    """The arrays the calls name (none is read or written: every row fails first) and the good value of every argument."""

    def __init__(self):
        import raytracing_c_amd as rt
        from raytracing_c_amd import ctypes_abi as abi
        self.rt, self.abi, self.lib = rt, abi, rt.lib
        self.inputs = {"color": np.full((H, W, 3), 7.0, F32), "plane": np.full((H, W, 3), 0.5, F32),
                       "variance_in": np.full((H, W), 0.25, F32), "moments_in": np.full((H, W, 2), 0.5, F32),
                       "motion": np.full((H, W, 3), 0.125, F32), "color_low": np.full((H // 2, W // 2, 3), 7.0, F32),
                       "plane_low": np.full((H // 2, W // 2, 3), 0.5, F32)}
        self.outputs = {"out": np.full((H, W, 3), 7.0, F32), "length": np.full((H, W), 7.0, F32), "variance": np.full((H, W), 7.0, F32),
                        "moments": np.full((H, W, 2), 7.0, F32), "history_out": np.full((H, W, 3), 7.0, F32),
                        "image": np.full((H, W, 3), 0x55, np.uint8), "work": np.full(64 * W * H + 16, 0x55, np.uint8),
                        "hist": np.full(2 * 48 * W * H + 16, 0x55, np.uint8), "mom": np.full(2 * 16 * W * H + 16, 0x55, np.uint8),
                        "up": np.full(UP_SLOT * len(UP_ARRAYS) + 16, 0x55, np.uint8)}
        self.before = {k: v.copy() for k, v in {**self.inputs, **self.outputs}.items()}
        a = {k: v.ctypes.data for k, v in {**self.inputs, **self.outputs}.items()}
        self.addr = a
        self.work = a["work"] + (-a["work"]) % 16
        self.hist_a = a["hist"] + (-a["hist"]) % 16
        self.hist_b = self.hist_a + 48 * W * H
        self.mom_a = a["mom"] + (-a["mom"]) % 16
        self.mom_b = self.mom_a + 16 * W * H
        self.up = a["up"] + (-a["up"]) % 16
        self.camera = abi.Camera()
        self.scene = abi.Scene()
        self.history = self.lib.rt_history_create(W, H)           # (touches no device)
        assert self.history
        self.keep = []
        cam, p = C.byref(self.camera), a["plane"]
        frame_dev = dict(d_color=a["color"], d_coverage=p, d_albedo=p, d_normal=p, d_position=p)
        size = dict(width=W, height=H)
        guided_dev = dict(**size, params=G(), **frame_dev, d_out=a["out"], d_image=a["image"], d_work=self.work, stream=None)
        temporal_dev = dict(**size, params=T(), camera=cam, previous_camera=cam, **frame_dev, d_history_in=self.hist_a,
                            d_history_out=self.hist_b, d_out=a["out"], d_length=a["length"], d_image=a["image"])
        guided_host = dict(**size, params=G(), color=a["color"], planes=FEATS(), out=a["out"], image=a["image"])
        temporal_host = dict(**size, params=T(), camera=cam, previous_camera=cam, color=a["color"], planes=FEATS(), history_in=HIN(),
                             history_out=HOUT(), out=a["out"], length=a["length"], image=a["image"])
        frame = dict(scene=C.byref(self.scene), image=IMG(), samples=2, max_bounces=2)
        moments_dev = dict(vp=V(), d_moments_in=self.mom_a, d_moments_out=self.mom_b, d_variance=a["variance"], stream=None)
        moments_host = dict(vp=V(), moments_in=a["moments_in"], moments_out=a["moments"], variance=a["variance"])
        self.good = {
            "rt_guided_work_bytes": size, "rt_temporal_history_bytes": size, "rt_guided_variance_work_bytes": size,
            "rt_temporal_moments_bytes": size, "rt_history_create": size, "rt_history_reset": dict(history=self.history),
            "rt_guided_denoise": guided_dev,
            "rt_guided_denoise_variance": dict(**guided_dev, d_variance=a["variance_in"], d_variance_out=a["variance"]),
            "rt_temporal_accumulate": dict(**temporal_dev, stream=None),
            "rt_temporal_accumulate_moments": dict(**temporal_dev, **moments_dev),
            "rt_guided_denoise_host": guided_host,
            "rt_guided_denoise_variance_host": dict(**guided_host, variance=a["variance_in"], variance_out=a["variance"]),
            "rt_temporal_accumulate_host": temporal_host,
            "rt_temporal_accumulate_moments_host": dict(**temporal_host, **moments_host),
            "rt_render_denoised": dict(**frame, params=G(), linear_noisy=a["out"], linear_denoised=a["out"]),
            "rt_render_temporal": dict(**frame, history=self.history, temporal_params=T(), guided_params=G(), linear_noisy=a["out"],
                                       linear_out=a["out"], length=a["length"]),
            "rt_render_svgf": dict(**frame, history=self.history, temporal_params=T(), variance_params=V(), guided_params=G(),
                                   linear_noisy=a["out"], linear_out=a["out"], length=a["length"], variance=a["variance"]),
            "rt_history_set_motion": dict(history=self.history, on=1),
            "rt_temporal_accumulate_motion": dict(**temporal_dev, **moments_dev, d_motion=a["motion"]),
            "rt_temporal_accumulate_motion_host": dict(**temporal_host, **moments_host, motion=a["motion"]),
            "rt_guided_upsample_work_bytes": size,
            "rt_guided_upsample": dict(**size, params=U(), **{"d_" + k: self.up_at(k) for k in UP_ARRAYS}, stream=None),
            "rt_guided_upsample_host": dict(**size, params=U(), color_low=a["color_low"], low=LOW(), full=FEATS(), out=a["out"],
                                            image=a["image"]),
            "rt_render_upsampled": dict(**frame, upsample_params=U(), guided_params=G(), linear_low=a["out"], linear_upsampled=a["out"],
                                        linear_out=a["out"]),
        }

    def up_at(self, k, offset=0):
        """Where rt_guided_upsample's array `k` lies in a good call (UP_SLOT bytes apart: none overlaps at 4 x 4), plus `offset`."""
        return self.up + UP_SLOT * UP_ARRAYS.index(k) + offset

    def close(self):
        self.lib.rt_history_destroy(self.history)
        self.lib.rt_clear_error()

    def build(self, m):
        abi, a = self.abi, self.addr
        fp = C.POINTER(C.c_float)
        if m.kind == "guided":
            s = abi.RT_Guided_Params(iterations=2, sigma_color=1.0, sigma_normal=0.2, sigma_position=1.0, demodulate=1)
        elif m.kind == "temporal":
            s = abi.RT_Temporal_Params(alpha=0.1, max_history=32, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
        elif m.kind == "variance":
            s = abi.RT_Variance_Params(0.2, 1.0)
        elif m.kind == "upsample":
            s = abi.RT_Upsample_Params(sigma_normal=0.2, sigma_position=0.5, demodulate=1, guide_samples=0)
        elif m.kind == "features":
            s = abi.RT_Features(*[self.inputs["plane"].ctypes.data_as(fp)] * 4)
        elif m.kind == "features_low":
            s = abi.RT_Features(*[self.inputs["plane_low"].ctypes.data_as(fp)] * 4)
        elif m.kind == "history_in":
            s = abi.RT_History_Planes(*[self.inputs["plane"].ctypes.data_as(fp)] * 5)
        elif m.kind == "history_out":
            s = abi.RT_History_Planes(*[self.outputs["history_out"].ctypes.data_as(fp)] * 5)
        else:
            s = abi.Image()
            s.components, s.pixel_type, s.width, s.stride, s.height = 3, 0, W, W, H
            s.pixels.data, s.pixels.len = a["image"], self.outputs["image"].size
        for k, v in m.fields.items():
            if k == "pixels":
                s.pixels.data = v
            else:
                setattr(s, k, v)
        self.keep.append(s)
        return C.byref(s)

    def call(self, entry, overrides):
        args = dict(self.good[entry])
        for k, v in overrides.items():
            assert k in args, (entry, k)
            args[k] = v
        values = []
        for v in args.values():
            if callable(v):
                v = v(self)
            values.append(self.build(v) if isinstance(v, _Marker) else v)
        self.lib.rt_clear_error()
        rc = getattr(self.lib, entry)(*values)
        msg = self.rt.last_error()
        self.lib.rt_clear_error()
        self.keep.clear()
        return {"rc": rc, "error": msg}

    def untouched(self):
        return all(v.tobytes() == self.before[k].tobytes() for k, v in {**self.inputs, **self.outputs}.items())


# ---- the table: (row, entry point, the arguments that differ from a good call) ---------------------------------------------------

GUIDED_PARAMS = [("iterations 0", dict(iterations=0)), ("iterations 9", dict(iterations=9)), ("sigma_color 0", dict(sigma_color=0.0)),
                 ("sigma_color nan", dict(sigma_color=NAN)), ("sigma_normal -1", dict(sigma_normal=-1.0)),
                 ("sigma_normal nan", dict(sigma_normal=NAN)), ("sigma_position 0", dict(sigma_position=0.0)),
                 ("sigma_position nan", dict(sigma_position=NAN)), ("demodulate 2", dict(demodulate=2)),
                 # two faults: the fields in the struct's order
                 ("iterations and sigma_color", dict(iterations=0, sigma_color=0.0)),
                 ("sigma_color and sigma_normal", dict(sigma_color=-1.0, sigma_normal=0.0)),
                 ("sigma_normal and sigma_position", dict(sigma_normal=NAN, sigma_position=NAN)),
                 ("sigma_position and demodulate", dict(sigma_position=0.0, demodulate=-1))]
TEMPORAL_PARAMS = [("alpha 0", dict(alpha=0.0)), ("alpha 1.5", dict(alpha=1.5)), ("alpha nan", dict(alpha=NAN)),
                   ("max_history 0", dict(max_history=0)), ("max_history 2^20 + 1", dict(max_history=(1 << 20) + 1)),
                   ("normal_tolerance 0", dict(normal_tolerance=0.0)), ("normal_tolerance nan", dict(normal_tolerance=NAN)),
                   ("plane_tolerance -inf", dict(plane_tolerance=-INF)), ("plane_tolerance nan", dict(plane_tolerance=NAN)),
                   ("demodulate -1", dict(demodulate=-1)),
                   ("alpha and max_history", dict(alpha=0.0, max_history=0)),
                   ("max_history and normal_tolerance", dict(max_history=-3, normal_tolerance=0.0)),
                   ("normal_tolerance and plane_tolerance", dict(normal_tolerance=NAN, plane_tolerance=0.0)),
                   ("plane_tolerance and demodulate", dict(plane_tolerance=0.0, demodulate=2))]
VARIANCE_PARAMS = [("variance sigma_normal 0", dict(sigma_normal=0.0)), ("variance sigma_normal nan", dict(sigma_normal=NAN)),
                   ("variance sigma_position -1", dict(sigma_position=-1.0)), ("variance sigma_position nan", dict(sigma_position=NAN)),
                   ("both variance sigmas", dict(sigma_normal=0.0, sigma_position=0.0))]
UPSAMPLE_PARAMS = [("sigma_normal 0", dict(sigma_normal=0.0)), ("sigma_normal nan", dict(sigma_normal=NAN)),
                   ("sigma_normal -1", dict(sigma_normal=-1.0)), ("sigma_position 0", dict(sigma_position=0.0)),
                   ("sigma_position nan", dict(sigma_position=NAN)), ("demodulate 2", dict(demodulate=2)),
                   ("demodulate -1", dict(demodulate=-1)),
                   ("sigma_normal and sigma_position", dict(sigma_normal=NAN, sigma_position=-0.5)),
                   ("sigma_position and demodulate", dict(sigma_position=0.0, demodulate=3))]
SIZES = [("width 0", dict(width=0)), ("height -2", dict(height=-2)), ("too large", dict(width=BIG[0], height=BIG[1]))]
# (BIG's height is odd: for the upsampling its "too large" row is "odd and too large together", and this one is too large alone)
UPSAMPLE_SIZES = SIZES + [("odd width", dict(width=W - 1)), ("odd height", dict(height=H + 1)), ("1 x 1", dict(width=1, height=1)),
                          ("width 0 and height 0", dict(width=0, height=0)), ("width 1", dict(width=1)),
                          ("even and too large", dict(width=BIG[0], height=BIG[1] + 1))]
DEVICE_PLANES = ("d_color", "d_coverage", "d_albedo", "d_normal", "d_position")
HOST_PLANES = ("coverage", "albedo", "normal", "position")
HISTORY_PLANES = ("color", "length", "coverage", "normal", "position")
# rt_guided_upsample's arrays in its arguments' order -- the low frame, the full planes, the outputs, the work area -- and how far
# apart a good call has them
UP_ARRAYS = ("color_low", "coverage_low", "albedo_low", "normal_low", "position_low", "coverage", "albedo", "normal", "position", "out",
             "image", "work")
UP_PLANES = UP_ARRAYS[:9]
UP_SLOT = 256
PLAIN_DEV = dict(vp=None, d_moments_in=None, d_moments_out=None, d_variance=None)     # rt_temporal_accumulate_motion's plain form
PLAIN_HOST = dict(vp=None, moments_in=None, moments_out=None, variance=None)          # ... and rt_temporal_accumulate_motion_host's


def _rows():
    rows = []

    def row(entry, name, **overrides):
        rows.append((entry + ": " + name, entry, overrides))

    # ---- the sizes and the history object
    for entry in ("rt_guided_work_bytes", "rt_temporal_history_bytes", "rt_guided_variance_work_bytes", "rt_temporal_moments_bytes",
                  "rt_history_create"):
        for name, kw in SIZES:
            row(entry, name, **kw)
        row(entry, "width 0 and height 0", width=0, height=0)
    row("rt_history_reset", "history NULL", history=None)
    for name, kw in UPSAMPLE_SIZES:
        row("rt_guided_upsample_work_bytes", name, **kw)
    row("rt_history_set_motion", "history NULL", history=None)
    row("rt_history_set_motion", "on 2", on=2)
    row("rt_history_set_motion", "on -1", on=-1)
    row("rt_history_set_motion", "history and on", history=None, on=2)

    # ---- the guided denoiser, device level
    for entry in ("rt_guided_denoise", "rt_guided_denoise_variance"):
        for name, kw in SIZES:
            row(entry, name, **kw)
        row(entry, "params NULL", params=None)
        for name, kw in GUIDED_PARAMS:
            row(entry, name, params=G(**kw))
        for k in DEVICE_PLANES:
            row(entry, k + " NULL", **{k: None})
        row(entry, "d_albedo NULL without demodulate, d_work NULL", params=G(demodulate=0), d_albedo=None, d_work=None)
        row(entry, "d_work NULL", d_work=None)
        row(entry, "d_work unaligned", d_work=lambda c: c.work + 4)
        # two faults
        row(entry, "size and params NULL", width=0, params=None)
        row(entry, "too large and params NULL", width=BIG[0], height=BIG[1], params=None)
        row(entry, "params and d_color", params=G(iterations=9), d_color=None)
        row(entry, "d_color and d_normal", d_color=None, d_normal=None)
        row(entry, "d_coverage and d_albedo", d_coverage=None, d_albedo=None)
        row(entry, "d_albedo and d_position", d_albedo=None, d_position=None)
        row(entry, "d_normal and d_position", d_normal=None, d_position=None)
        row(entry, "d_position and d_work", d_position=None, d_work=None)
    row("rt_guided_denoise", "no output", d_out=None, d_image=None)
    row("rt_guided_denoise", "no output and d_work NULL", d_out=None, d_image=None, d_work=None)
    v = "rt_guided_denoise_variance"
    row(v, "d_variance NULL", d_variance=None)
    row(v, "no output", d_out=None, d_image=None, d_variance_out=None)
    row(v, "d_position and d_variance", d_position=None, d_variance=None)
    row(v, "d_variance and no output", d_variance=None, d_out=None, d_image=None, d_variance_out=None)
    row(v, "no output and d_work NULL", d_out=None, d_image=None, d_variance_out=None, d_work=None)
    row(v, "d_variance_out alone is an output, d_work NULL", d_out=None, d_image=None, d_work=None)

    # ---- the guided denoiser, host level
    for entry in ("rt_guided_denoise_host", "rt_guided_denoise_variance_host"):
        for name, kw in SIZES:
            row(entry, name, **kw)
        row(entry, "params NULL", params=None)
        for name, kw in GUIDED_PARAMS:
            row(entry, name, params=G(**kw))
        row(entry, "color NULL", color=None)
        row(entry, "planes NULL", planes=None)
        for k in HOST_PLANES:
            row(entry, "planes->" + k + " NULL", planes=FEATS(**{k: None}))
        row(entry, "size and params NULL", height=0, params=None)
        row(entry, "params and color", params=G(demodulate=2), color=None)
        row(entry, "color and planes", color=None, planes=None)
        row(entry, "coverage and normal", planes=FEATS(coverage=None, normal=None))
        row(entry, "albedo and position", planes=FEATS(albedo=None, position=None))
        row(entry, "normal and position", planes=FEATS(normal=None, position=None))
    row("rt_guided_denoise_host", "no output", out=None, image=None)
    row("rt_guided_denoise_host", "albedo NULL without demodulate, no output", params=G(demodulate=0), planes=FEATS(albedo=None),
        out=None, image=None)
    row("rt_guided_denoise_host", "position and no output", planes=FEATS(position=None), out=None, image=None)
    v = "rt_guided_denoise_variance_host"
    row(v, "variance NULL", variance=None)
    row(v, "no output", out=None, image=None, variance_out=None)
    row(v, "position and variance", planes=FEATS(position=None), variance=None)
    row(v, "variance and no output", variance=None, out=None, image=None, variance_out=None)

    # ---- the accumulation, device level
    for entry in ("rt_temporal_accumulate", "rt_temporal_accumulate_moments", "rt_temporal_accumulate_motion"):
        for name, kw in SIZES:
            row(entry, name, **kw)
        row(entry, "params NULL", params=None)
        for name, kw in TEMPORAL_PARAMS:
            row(entry, name, params=T(**kw))
        row(entry, "camera NULL", camera=None)
        row(entry, "previous_camera NULL", previous_camera=None)
        for k in DEVICE_PLANES:
            row(entry, k + " NULL", **{k: None})
        row(entry, "d_history_out NULL", d_history_out=None)
        row(entry, "d_history_out unaligned", d_history_out=lambda c: c.hist_b + 4)
        row(entry, "d_history_in unaligned", d_history_in=lambda c: c.hist_a + 8)
        row(entry, "histories equal", d_history_out=lambda c: c.hist_a)
        row(entry, "d_history_out inside d_history_in", d_history_out=lambda c: c.hist_b - 16)
        row(entry, "d_history_in inside d_history_out", d_history_in=lambda c: c.hist_b - 16, d_history_out=lambda c: c.hist_a)
        # two faults
        row(entry, "size and params NULL", width=0, params=None)
        row(entry, "params and camera", params=T(alpha=2.0), camera=None)
        row(entry, "camera and previous_camera", camera=None, previous_camera=None)
        row(entry, "previous_camera and d_color", previous_camera=None, d_color=None)
        row(entry, "d_color and d_coverage", d_color=None, d_coverage=None)
        row(entry, "d_albedo and d_normal", d_albedo=None, d_normal=None)
        row(entry, "d_position and d_history_out", d_position=None, d_history_out=None)
        row(entry, "d_history_out NULL and d_history_in unaligned", d_history_out=None, d_history_in=lambda c: c.hist_a + 8)
        row(entry, "unaligned and overlapping", d_history_out=lambda c: c.hist_a + 8)
    for m in ("rt_temporal_accumulate_moments", "rt_temporal_accumulate_motion"):
        for name, kw in VARIANCE_PARAMS:
            row(m, name, vp=V(**kw))
        row(m, "variance wanted without its params", vp=None)
        row(m, "bad variance params although no variance is wanted", vp=V(sigma_normal=0.0), d_variance=None)
        row(m, "d_moments_out NULL", d_moments_out=None)
        row(m, "history without moments", d_moments_in=None)
        row(m, "moments without history", d_history_in=None)
        row(m, "d_moments_out unaligned", d_moments_out=lambda c: c.mom_b + 4)
        row(m, "d_moments_in unaligned", d_moments_in=lambda c: c.mom_a + 8)
        row(m, "moments equal", d_moments_out=lambda c: c.mom_a)
        row(m, "d_moments_out inside d_moments_in", d_moments_out=lambda c: c.mom_b - 16)
        row(m, "d_moments_in inside d_moments_out", d_moments_in=lambda c: c.mom_b - 16, d_moments_out=lambda c: c.mom_a)
        row(m, "temporal params and variance params", params=T(alpha=0.0), vp=None)
        row(m, "variance params and camera", vp=None, camera=None)
        row(m, "histories overlap and d_moments_out NULL", d_history_out=lambda c: c.hist_a, d_moments_out=None)
        row(m, "d_moments_out NULL and history without moments", d_moments_out=None, d_moments_in=None)
        row(m, "history without moments and d_moments_out unaligned", d_moments_in=None, d_moments_out=lambda c: c.mom_b + 4)
        row(m, "moments unaligned and overlapping", d_moments_out=lambda c: c.mom_a + 8)
    # the motion plane, in the moments form and in the plain one (vp, both moments and the variance all NULL)
    m = "rt_temporal_accumulate_motion"
    for form, kw in (("", {}), ("plain: ", PLAIN_DEV)):
        row(m, form + "d_motion NULL", d_motion=None, **kw)
        row(m, form + "d_position and d_motion", d_position=None, d_motion=None, **kw)
        row(m, form + "d_motion and d_history_out", d_motion=None, d_history_out=None, **kw)
        row(m, form + "d_motion and histories overlap", d_motion=None, d_history_out=lambda c: c.hist_a, **kw)
    row(m, "d_motion and d_moments_out", d_motion=None, d_moments_out=None)
    row(m, "plain: d_history_out NULL", **{**PLAIN_DEV, "d_history_out": None})
    row(m, "plain: histories equal", **{**PLAIN_DEV, "d_history_out": lambda c: c.hist_a})
    # exactly one of the four given: the moments form, by its rules
    row(m, "plain but for vp", **{**PLAIN_DEV, "vp": V()})
    row(m, "plain but for bad vp", **{**PLAIN_DEV, "vp": V(sigma_normal=0.0)})
    row(m, "plain but for d_moments_in", **{**PLAIN_DEV, "d_moments_in": lambda c: c.mom_a})
    row(m, "plain but for d_moments_out", **{**PLAIN_DEV, "d_moments_out": lambda c: c.mom_b})
    row(m, "plain but for d_variance", **{**PLAIN_DEV, "d_variance": lambda c: c.addr["variance"]})

    # ---- the accumulation, host level
    for entry in ("rt_temporal_accumulate_host", "rt_temporal_accumulate_moments_host", "rt_temporal_accumulate_motion_host"):
        for name, kw in SIZES:
            row(entry, name, **kw)
        row(entry, "params NULL", params=None)
        for name, kw in TEMPORAL_PARAMS:
            row(entry, name, params=T(**kw))
        row(entry, "camera NULL", camera=None)
        row(entry, "previous_camera NULL", previous_camera=None)
        row(entry, "color NULL", color=None)
        row(entry, "planes NULL", planes=None)
        for k in HOST_PLANES:
            row(entry, "planes->" + k + " NULL", planes=FEATS(**{k: None}))
        for k in HISTORY_PLANES:
            row(entry, "history_in->" + k + " NULL", history_in=HIN(**{k: None}))
            row(entry, "history_out->" + k + " NULL", history_out=HOUT(**{k: None}))
        row(entry, "size and params NULL", width=0, params=None)
        row(entry, "params and camera", params=T(max_history=0), camera=None)
        row(entry, "camera and previous_camera", camera=None, previous_camera=None)
        row(entry, "previous_camera and color", previous_camera=None, color=None)
        row(entry, "color and planes->coverage", color=None, planes=FEATS(coverage=None))
        row(entry, "planes->position and history_in->color", planes=FEATS(position=None), history_in=HIN(color=None))
        row(entry, "history_in: color and length", history_in=HIN(color=None, length=None))
        row(entry, "history_in: length and coverage", history_in=HIN(length=None, coverage=None))
        row(entry, "history_in: coverage and normal", history_in=HIN(coverage=None, normal=None))
        row(entry, "history_in: normal and position", history_in=HIN(normal=None, position=None))
        row(entry, "history_in->position and history_out->color", history_in=HIN(position=None), history_out=HOUT(color=None))
    h = "rt_temporal_accumulate_host"
    row(h, "no output", history_out=None, out=None, length=None, image=None)
    row(h, "history_in->normal and no output", history_in=HIN(normal=None), history_out=None, out=None, length=None, image=None)
    for m in ("rt_temporal_accumulate_moments_host", "rt_temporal_accumulate_motion_host"):
        for name, kw in VARIANCE_PARAMS:
            row(m, name, vp=V(**kw))
        row(m, "variance wanted without its params", vp=None)
        row(m, "bad variance params although no variance is wanted", vp=V(sigma_position=0.0), variance=None)
        row(m, "history without moments", moments_in=None)
        row(m, "moments without history", history_in=None)
        row(m, "no output", history_out=None, out=None, length=None, image=None, moments_out=None, variance=None, vp=None)
        row(m, "temporal params and variance params", params=T(demodulate=2), vp=None)
        row(m, "variance params and camera", vp=V(sigma_normal=NAN), camera=None)
        row(m, "history_out->length and history without moments", history_out=HOUT(length=None), moments_in=None)
        row(m, "moments without history and no output", history_in=None, history_out=None, out=None, length=None, image=None,
            moments_out=None, variance=None, vp=None)
    # the motion plane, in the moments form and in the plain one (vp, both moments and the variance all NULL)
    m = "rt_temporal_accumulate_motion_host"
    no_output = dict(history_out=None, out=None, length=None, image=None)
    for form, kw in (("", {}), ("plain: ", PLAIN_HOST)):
        row(m, form + "motion NULL", motion=None, **kw)
        row(m, form + "planes->position and motion", planes=FEATS(position=None), motion=None, **kw)
        row(m, form + "motion and history_in->color", motion=None, history_in=HIN(color=None), **kw)
        row(m, form + "motion and history_out->position", motion=None, history_out=HOUT(position=None), **kw)
    row(m, "motion and history without moments", motion=None, moments_in=None)
    row(m, "plain: no output", **PLAIN_HOST, **no_output)
    row(m, "plain: motion and no output", motion=None, **PLAIN_HOST, **no_output)
    row(m, "plain: history_in->length NULL", history_in=HIN(length=None), **PLAIN_HOST)
    # exactly one of the four given: the moments form, by its rules (moments_in alone is a good call, so it comes without its history)
    row(m, "plain but for vp", **{**PLAIN_HOST, "vp": V()})
    row(m, "plain but for bad vp", **{**PLAIN_HOST, "vp": V(sigma_position=NAN)})
    row(m, "plain but for moments_in, without a history", history_in=None, **{**PLAIN_HOST, "moments_in": lambda c: c.addr["moments_in"]})
    row(m, "plain but for moments_out", **{**PLAIN_HOST, "moments_out": lambda c: c.addr["moments"]})
    row(m, "plain but for variance", **{**PLAIN_HOST, "variance": lambda c: c.addr["variance"]})

    # ---- the upsampling, device level (UP_ARRAYS: a good call's arrays lie UP_SLOT apart in one area that is never read)
    u = "rt_guided_upsample"
    for name, kw in UPSAMPLE_SIZES:
        row(u, name, **kw)
    row(u, "params NULL", params=None)
    for name, kw in UPSAMPLE_PARAMS:
        row(u, name, params=U(**kw))
    for k in UP_PLANES + ("work",):
        row(u, "d_" + k + " NULL", **{"d_" + k: None})
    row(u, "no output", d_out=None, d_image=None)
    row(u, "d_work unaligned", d_work=lambda c: c.up_at("work", 4))
    # two faults
    row(u, "size and params NULL", width=0, params=None)
    row(u, "odd and params NULL", width=W + 1, params=None)
    row(u, "params and d_color_low", params=U(demodulate=2), d_color_low=None)
    for k, k2 in zip(UP_PLANES, UP_PLANES[1:]):
        row(u, "d_" + k + " and d_" + k2, **{"d_" + k: None, "d_" + k2: None})
    row(u, "d_albedo_low NULL without demodulate, d_position_low NULL", params=U(demodulate=0), d_albedo_low=None, d_position_low=None)
    row(u, "d_albedo NULL without demodulate, d_work NULL", params=U(demodulate=0), d_albedo=None, d_work=None)
    row(u, "both albedos NULL without demodulate, no output", params=U(demodulate=0), d_albedo_low=None, d_albedo=None, d_out=None,
        d_image=None)
    row(u, "d_position and no output", d_position=None, d_out=None, d_image=None)
    row(u, "no output and d_work NULL", d_out=None, d_image=None, d_work=None)
    row(u, "d_work NULL and d_out over d_color_low", d_work=None, d_out=lambda c: c.up_at("color_low"))
    row(u, "d_work unaligned and under d_out", d_work=lambda c: c.up_at("out", 4))
    # an output over an input or the work area: at its start, at its first and at its last byte; the image over the f32 output
    n3 = W * H * 3 * 4
    for k in UP_PLANES + ("work",):
        row(u, "d_out over d_" + k, d_out=lambda c, k=k: c.up_at(k))
        row(u, "d_image over d_" + k, d_image=lambda c, k=k: c.up_at(k))
    row(u, "d_out ends on the first byte of d_coverage", d_out=lambda c: c.up_at("coverage", 1 - n3))
    row(u, "d_out begins on the last byte of d_coverage", d_out=lambda c: c.up_at("coverage", W * H * 4 - 1))
    row(u, "d_image begins on the last byte of d_out", d_image=lambda c: c.up_at("out", n3 - 1))
    row(u, "d_image ends on the first byte of d_out", d_image=lambda c: c.up_at("out", 1 - W * H * 3))
    row(u, "d_work under d_out", d_work=lambda c: c.up_at("out", 16))
    row(u, "d_work begins on the last 16 bytes of d_image", d_work=lambda c: c.up_at("image", W * H * 3 - 16))
    # which one is named: the first in the order of the arguments, not in memory; the inputs before the other output
    row(u, "d_out over d_albedo and d_normal", d_out=lambda c: c.up_at("albedo", 100))
    row(u, "d_out over d_albedo and d_normal, d_albedo behind d_normal", d_albedo=lambda c: c.up_at("normal"),
        d_normal=lambda c: c.up_at("albedo"), d_out=lambda c: c.up_at("albedo", 100))
    row(u, "d_out and d_image over inputs", d_out=lambda c: c.up_at("position"), d_image=lambda c: c.up_at("color_low"))
    row(u, "d_image over d_position and d_out", d_out=lambda c: c.up_at("position", 200), d_image=lambda c: c.up_at("position", 170))
    row(u, "a NULL albedo overlaps nothing, d_image over d_out", params=U(demodulate=0), d_albedo_low=None, d_albedo=None,
        d_image=lambda c: c.up_at("out", 8))

    # ---- the upsampling, host level
    u = "rt_guided_upsample_host"
    for name, kw in UPSAMPLE_SIZES:
        row(u, name, **kw)
    row(u, "params NULL", params=None)
    for name, kw in UPSAMPLE_PARAMS:
        row(u, name, params=U(**kw))
    row(u, "color_low NULL", color_low=None)
    row(u, "low NULL", low=None)
    row(u, "full NULL", full=None)
    for k in HOST_PLANES:
        row(u, "low->" + k + " NULL", low=LOW(**{k: None}))
        row(u, "full->" + k + " NULL", full=FEATS(**{k: None}))
        row(u, k + " missing in low and full", low=LOW(**{k: None}), full=FEATS(**{k: None}))
    row(u, "no output", out=None, image=None)
    # two faults
    row(u, "size and params NULL", height=0, params=None)
    row(u, "odd and params NULL", height=H - 1, params=None)
    row(u, "params and color_low", params=U(sigma_normal=0.0), color_low=None)
    row(u, "color_low and low", color_low=None, low=None)
    row(u, "low and full", low=None, full=None)
    row(u, "full and low->coverage", full=None, low=LOW(coverage=None))
    for k, k2 in zip(HOST_PLANES, HOST_PLANES[1:]):
        row(u, "low: " + k + " and " + k2, low=LOW(**{k: None, k2: None}))
        row(u, "full: " + k + " and " + k2, full=FEATS(**{k: None, k2: None}))
    row(u, "low->position and full->coverage", low=LOW(position=None), full=FEATS(coverage=None))
    row(u, "low->normal and full->albedo", low=LOW(normal=None), full=FEATS(albedo=None))
    row(u, "low->albedo NULL without demodulate, full->position NULL", params=U(demodulate=0), low=LOW(albedo=None),
        full=FEATS(position=None))
    row(u, "both albedos NULL without demodulate, no output", params=U(demodulate=0), low=LOW(albedo=None), full=FEATS(albedo=None),
        out=None, image=None)
    row(u, "full->position and no output", full=FEATS(position=None), out=None, image=None)

    # ---- behind a frame (the scene is never read)
    for entry, stage, first, first_params in (("rt_render_denoised", "params", G, GUIDED_PARAMS),
                                              ("rt_render_temporal", "temporal_params", T, TEMPORAL_PARAMS),
                                              ("rt_render_svgf", "temporal_params", T, TEMPORAL_PARAMS),
                                              ("rt_render_upsampled", "upsample_params", U, UPSAMPLE_PARAMS)):
        row(entry, "scene NULL", scene=None)
        row(entry, "image NULL", image=None)
        row(entry, "scene and image", scene=None, image=None)
        row(entry, "width 0", image=IMG(width=0))
        row(entry, "height -1", image=IMG(height=-1))
        row(entry, "width 2^31", image=IMG(width=1 << 31, stride=1 << 31))
        row(entry, "too large", image=IMG(width=BIG[0], stride=BIG[0], height=BIG[1]))
        row(entry, "stage params NULL", **{stage: None})
        for name, kw in first_params:
            row(entry, name, **{stage: first(**kw)})
        row(entry, "2 components", image=IMG(components=2))
        row(entry, "stride < width", image=IMG(stride=W - 1))
        row(entry, "samples 0", samples=0)
        row(entry, "samples 2^31", samples=1 << 31)
        row(entry, "max_bounces -1", max_bounces=-1)
        row(entry, "max_bounces 2^31", max_bounces=1 << 31)
        # two faults
        row(entry, "image size and stage params", image=IMG(width=0), **{stage: None})
        row(entry, "stage params and layout", image=IMG(components=2), **{stage: first(demodulate=2)})
        row(entry, "components and stride", image=IMG(components=2, stride=W - 1))
        row(entry, "stride and samples", image=IMG(stride=W - 1), samples=0)
        row(entry, "samples and max_bounces", samples=0, max_bounces=-1)
    d = "rt_render_denoised"
    row(d, "no output", image=IMG(pixels=None), linear_denoised=None)
    row(d, "max_bounces and no output", max_bounces=-1, image=IMG(pixels=None), linear_denoised=None)
    for entry in ("rt_render_temporal", "rt_render_svgf"):
        row(entry, "history NULL", history=None)
        row(entry, "image and history", image=None, history=None)
        row(entry, "history and image size", history=None, image=IMG(width=0))
        for name, kw in GUIDED_PARAMS:
            row(entry, "guided " + name, guided_params=G(**kw))
        row(entry, "temporal params and guided params", temporal_params=T(alpha=0.0), guided_params=G(iterations=0))
        row(entry, "guided params and layout", guided_params=G(iterations=0), image=IMG(components=2))
        row(entry, "the image is not the history's size", image=IMG(width=W + 1, stride=W + 1))
    t = "rt_render_temporal"
    row(t, "no output", image=IMG(pixels=None), linear_out=None, length=None)
    row(t, "max_bounces and no output", max_bounces=-1, image=IMG(pixels=None), linear_out=None, length=None)
    row(t, "no output and the history's size", image=IMG(width=W + 1, stride=W + 1, pixels=None), linear_out=None, length=None)
    s = "rt_render_svgf"
    for name, kw in VARIANCE_PARAMS:
        row(s, name, variance_params=V(**kw))
    row(s, "variance params NULL", variance_params=None)
    row(s, "guided params NULL", guided_params=None)
    row(s, "temporal params and variance params", temporal_params=T(alpha=0.0), variance_params=None)
    row(s, "variance params and guided params", variance_params=None, guided_params=None)
    row(s, "no output", image=IMG(pixels=None), linear_out=None, length=None, variance=None)
    row(s, "variance alone is an output: the history's size", image=IMG(width=W + 1, stride=W + 1, pixels=None), linear_out=None,
        length=None)
    u = "rt_render_upsampled"
    no_output = dict(image=IMG(pixels=None), linear_upsampled=None, linear_out=None)
    row(u, "odd width", image=IMG(width=W - 1, stride=W - 1))
    row(u, "odd height", image=IMG(height=H + 1))
    row(u, "1 high", image=IMG(height=1))
    row(u, "1 x 1", image=IMG(width=1, stride=1, height=1))
    row(u, "width 2^32", image=IMG(width=1 << 32, stride=1 << 32))
    row(u, "even and too large", image=IMG(width=BIG[0], stride=BIG[0], height=BIG[1] + 1))
    row(u, "odd and upsample params NULL", image=IMG(height=H - 1), upsample_params=None)
    for name, kw in GUIDED_PARAMS:
        row(u, "guided " + name, guided_params=G(**kw))
    row(u, "guide_samples -1", upsample_params=U(guide_samples=-1))
    row(u, "guide_samples samples + 1", upsample_params=U(guide_samples=3))
    row(u, "linear_out without guided params", guided_params=None)
    row(u, "no output", **no_output)
    row(u, "no output and no guided params", guided_params=None, **no_output)
    # two faults, in the order of the checks: image size, upsample params, guided params, layout, samples, max_bounces,
    # guide_samples, linear_out without a filter, no output (the first pair and layout / samples / max_bounces are above)
    row(u, "upsample params and guided params", upsample_params=U(sigma_normal=0.0), guided_params=G(iterations=0))
    row(u, "upsample params NULL and guided params", upsample_params=None, guided_params=G(iterations=0))
    row(u, "guided params and layout", guided_params=G(iterations=0), image=IMG(components=2))
    row(u, "layout and samples", image=IMG(components=2), samples=0)
    row(u, "max_bounces and guide_samples", max_bounces=-1, upsample_params=U(guide_samples=-1))
    row(u, "samples and guide_samples", samples=0, upsample_params=U(guide_samples=1))
    row(u, "guide_samples and linear_out without guided params", upsample_params=U(guide_samples=3), guided_params=None)
    row(u, "guide_samples and no output", upsample_params=U(guide_samples=-1), **no_output)
    row(u, "linear_out without guided params and no other output", guided_params=None, image=IMG(pixels=None), linear_upsampled=None)
    row(u, "max_bounces and no output", max_bounces=-1, **no_output)
    assert len({r[0] for r in rows}) == len(rows)
    return rows


ROWS = _rows()


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_entry_point_with_a_refusal_has_rows_and_every_row_a_record(recorded):
    assert {r[1] for r in ROWS} == set(ENTRIES)
    assert set(recorded) == {r[0] for r in ROWS}


@pytest.mark.parametrize("name,entry,overrides", ROWS, ids=[r[0] for r in ROWS])
def test_the_call_is_refused_as_recorded(ctx, recorded, name, entry, overrides):
    got = ctx.call(entry, overrides)
    print(got)
    assert got["rc"] in (-1, None) and got["error"].startswith(entry + ": ")
    assert got == recorded[name]
    assert ctx.untouched()


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    have = {}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            have = json.load(f)
    c = Context()
    for name_, entry_, overrides_ in ROWS:
        if name_ not in have:
            have[name_] = c.call(entry_, overrides_)
            assert have[name_]["rc"] in (-1, None) and c.untouched(), (name_, have[name_])
    c.close()
    with open(FIXTURE, "w") as f:
        json.dump(have, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(have), "rows in", FIXTURE)
