"""Feature-guided upsampling without a GPU: the exported names in all four libraries, the struct's layout against the C header, the
Python mirror and entry points, the size the library reports, and every refusal -- each reported before a device is touched, with
the outputs untouched."""
import ctypes as C
import os
import subprocess

import numpy as np

NAMES = ["rt_guided_upsample_work_bytes", "rt_guided_upsample", "rt_guided_upsample_host", "rt_render_upsampled"]
FIELDS = ["sigma_normal", "sigma_position", "demodulate", "guide_samples"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN, INF = float("nan"), float("inf")


def test_symbols_in_all_four_libraries_and_python_entry_points():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    for n in NAMES:
        assert n in abi.EXPORTED_SYMBOLS
        for lib in (rt.lib, rt.diag):
            assert getattr(lib, n) is not None
    for path in ("librt_hip_v1.so", "librt_hip_v2.so"):
        dll = C.CDLL(os.path.join(os.path.dirname(rt.native.LIB_PATH), path))
        for n in NAMES:
            assert getattr(dll, n) is not None
    assert callable(rt.guided_upsample) and callable(rt.render_upsampled)


def test_work_bytes_is_48_per_low_pixel_and_refuses_bad_sizes():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    f = rt.lib.rt_guided_upsample_work_bytes
    assert f(1920, 1080) == 48 * 960 * 540 == abi.RT_UPSAMPLE_WORK_PER_LOW_PIXEL * 960 * 540
    assert f(2, 2) == 48 and f(6, 10) == 48 * 3 * 5 and f(1 << 14, 1 << 14) == 48 << 26
    for w, h, word in ((0, 4, "invalid"), (4, 0, "invalid"), (-2, 4, "invalid"), (3, 4, "odd"), (4, 5, "odd"), (1, 1, "invalid"),
                       (1 << 15, (1 << 13) + 2, "too large")):
        rt.lib.rt_clear_error()
        assert f(w, h) == -1 and "rt_guided_upsample_work_bytes" in rt.last_error() and word in rt.last_error(), (w, h, rt.last_error())
    rt.lib.rt_clear_error()


def test_the_struct_is_the_headers(tmp_path):
    """sizeof and the field offsets of RT_Upsample_Params as the C compiler lays include/rt_hip.h out, against the ctypes mirror."""
    from raytracing_c_amd import ctypes_abi as abi
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(RT_Upsample_Params));\n'
                   + "".join(f'  printf(" %zu", offsetof(RT_Upsample_Params, {n}));\n' for n in FIELDS) + '  return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    mirror = [C.sizeof(abi.RT_Upsample_Params)] + [getattr(abi.RT_Upsample_Params, n).offset for n in FIELDS]
    assert got == mirror == [16, 0, 4, 8, 12]
    assert [n for n, _ in abi.RT_Upsample_Params._fields_] == FIELDS


def test_every_refusal_comes_before_the_device_and_leaves_the_outputs_untouched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    w, h = 8, 4
    fp = C.POINTER(C.c_float)
    low3, full3 = np.full((h // 2, w // 2, 3), 0.5, F32), np.full((h, w, 3), 0.5, F32)
    lp, fpl = low3.ctypes.data_as(fp), full3.ctypes.data_as(fp)
    low, full = abi.RT_Features(lp, lp, lp, lp), abi.RT_Features(fpl, fpl, fpl, fpl)
    out = np.full((h, w, 3), 7.0, F32)
    img = np.full((h, w, 3), 0x55, np.uint8)
    good = abi.RT_Upsample_Params(0.2, 0.5, 1, 0)

    def fails(call, who, *words):
        lib.rt_clear_error()
        assert call() == -1
        for word in (who + ":",) + words:
            assert word in rt.last_error(), (word, rt.last_error())

    # ---- the host level
    def host(width=w, height=h, p=good, color=low3.ctypes.data, lo=low, fu=full, o=out.ctypes.data, im=img.ctypes.data):
        return lib.rt_guided_upsample_host(width, height, None if p is None else C.byref(p), color, None if lo is None else C.byref(lo),
                                           None if fu is None else C.byref(fu), o, im)
    who = "rt_guided_upsample_host"
    fails(lambda: host(p=None), who, "upsample params are NULL")
    fails(lambda: host(color=None), who, "color_low is NULL")
    fails(lambda: host(lo=None), who, "low is NULL")
    fails(lambda: host(fu=None), who, "full is NULL")
    for name in ("coverage", "albedo", "normal", "position"):
        for which, word in (("lo", "low->"), ("fu", "full->")):
            planes = abi.RT_Features(*[None if k == name else (lp if which == "lo" else fpl) for k in ("coverage", "albedo", "normal", "position")])
            fails(lambda: host(**{which: planes}), who, word + name)
    for width, height, word in ((7, 4, "odd"), (8, 3, "odd"), (0, 4, "invalid"), (8, 0, "invalid"), (1, 4, "invalid"), (-8, 4, "invalid"),
                                (1 << 15, (1 << 13) + 2, "too large")):
        fails(lambda: host(width=width, height=height), who, word)
    for bad, word in ((abi.RT_Upsample_Params(0.0, 0.5, 1, 0), "sigma_normal"), (abi.RT_Upsample_Params(NAN, 0.5, 1, 0), "sigma_normal"),
                      (abi.RT_Upsample_Params(-1.0, 0.5, 1, 0), "sigma_normal"), (abi.RT_Upsample_Params(0.2, 0.0, 1, 0), "sigma_position"),
                      (abi.RT_Upsample_Params(0.2, NAN, 1, 0), "sigma_position"), (abi.RT_Upsample_Params(0.2, 0.5, 2, 0), "demodulate"),
                      (abi.RT_Upsample_Params(0.2, 0.5, -1, 0), "demodulate")):
        fails(lambda: host(p=bad), who, word)
    fails(lambda: host(o=None, im=None), who, "no output is wanted")
    # (without demodulate a missing albedo is no refusal: that call would reach the device, and is not made here)

    # ---- the device level: addresses that are never read
    A = 1 << 20                                                                  # twelve arrays, 1 MiB apart: none overlaps at 8 x 4

    def device(width=w, height=h, p=good, **kw):
        a = dict(color_low=1 * A, coverage_low=2 * A, albedo_low=3 * A, normal_low=4 * A, position_low=5 * A, coverage=6 * A,
                 albedo=7 * A, normal=8 * A, position=9 * A, out=10 * A, image=11 * A, work=12 * A)
        a.update(kw)
        return lib.rt_guided_upsample(width, height, None if p is None else C.byref(p), *[a[k] for k in (
            "color_low", "coverage_low", "albedo_low", "normal_low", "position_low", "coverage", "albedo", "normal", "position", "out",
            "image", "work")], None)
    who = "rt_guided_upsample"
    fails(lambda: device(p=None), who, "upsample params are NULL")
    for k in ("color_low", "coverage_low", "albedo_low", "normal_low", "position_low", "coverage", "albedo", "normal", "position", "work"):
        fails(lambda: device(**{k: None}), who, "d_" + k + " is NULL")
    fails(lambda: device(out=None, image=None), who, "no output is wanted")
    fails(lambda: device(work=12 * A + 4), who, "aligned")
    for width, height, word in ((7, 4, "odd"), (8, 3, "odd"), (0, 4, "invalid"), (1 << 15, (1 << 13) + 2, "too large")):
        fails(lambda: device(width=width, height=height), who, word)
    fails(lambda: device(p=abi.RT_Upsample_Params(0.2, NAN, 1, 0)), who, "sigma_position")
    fails(lambda: device(p=abi.RT_Upsample_Params(0.2, 0.5, 3, 0)), who, "demodulate")
    # an output over an input or the scratch: at its start, at its first and at its last byte; the image over the f32 output
    n3 = w * h * 3 * 4
    for k in ("color_low", "coverage_low", "albedo_low", "normal_low", "position_low", "coverage", "albedo", "normal", "position", "work"):
        fails(lambda: device(out=device_address(k, A)), who, "d_out overlaps d_" + k)
        fails(lambda: device(image=device_address(k, A)), who, "d_image overlaps d_" + k)
    fails(lambda: device(out=6 * A - n3 + 1), who, "d_out overlaps d_coverage")
    fails(lambda: device(out=6 * A + w * h * 4 - 1), who, "d_out overlaps d_coverage")
    fails(lambda: device(image=10 * A + n3 - 1), who, "d_image overlaps d_out")
    fails(lambda: device(work=10 * A + 16), who, "d_out overlaps d_work")

    # ---- behind a frame
    scene = abi.Scene()
    pixels = np.full((h, w, 3), 0x55, np.uint8)
    image = abi.Image()
    image.width, image.height, image.stride, image.components = w, h, w, 3
    image.pixels.data, image.pixels.len = pixels.ctypes.data, pixels.size
    gp = abi.RT_Guided_Params(2, 1.0, 0.2, 0.5, 1)
    lin_low, lin_up, lin_out = np.full((h // 2, w // 2, 3), 7.0, F32), np.full((h, w, 3), 7.0, F32), np.full((h, w, 3), 7.0, F32)

    def frame(sc=scene, im=image, samples=16, bounces=8, p=good, g=gp, lo=lin_low.ctypes.data, up=lin_up.ctypes.data,
              fo=lin_out.ctypes.data):
        return lib.rt_render_upsampled(None if sc is None else C.byref(sc), None if im is None else C.byref(im), samples, bounces,
                                       None if p is None else C.byref(p), None if g is None else C.byref(g), lo, up, fo)
    who = "rt_render_upsampled"
    fails(lambda: frame(sc=None), who, "scene is NULL")
    fails(lambda: frame(im=None), who, "image is NULL")
    fails(lambda: frame(p=None), who, "upsample params are NULL")

    def sized(width, height):
        im = abi.Image()
        im.width, im.height, im.stride, im.components = width, height, max(width, 1), 3
        return im
    for width, height, word in ((7, 4, "odd"), (8, 5, "odd"), (0, 4, "invalid"), (8, 1, "invalid"), (1 << 32, 4, "invalid"),
                                (1 << 15, (1 << 13) + 2, "too large")):
        fails(lambda: frame(im=sized(width, height)), who, word)
    fails(lambda: frame(p=abi.RT_Upsample_Params(INF, -0.5, 1, 0)), who, "sigma_position")
    fails(lambda: frame(p=abi.RT_Upsample_Params(NAN, 0.5, 1, 0)), who, "sigma_normal")
    fails(lambda: frame(p=abi.RT_Upsample_Params(0.2, 0.5, 7, 0)), who, "demodulate")
    fails(lambda: frame(p=abi.RT_Upsample_Params(0.2, 0.5, 1, -1)), who, "guide_samples")
    fails(lambda: frame(p=abi.RT_Upsample_Params(0.2, 0.5, 1, 17)), who, "guide_samples")
    fails(lambda: frame(samples=0), who, "samples")
    fails(lambda: frame(bounces=-1), who, "max_bounces")
    fails(lambda: frame(g=abi.RT_Guided_Params(9, 1.0, 0.2, 0.5, 1)), who, "iterations")
    fails(lambda: frame(g=None), who, "linear_out", "guided params are NULL")
    fails(lambda: frame(im=sized(w, h), up=None, fo=None), who, "no output is wanted")
    fails(lambda: frame(im=sized(w, h), g=None, up=None, fo=None), who, "no output is wanted")
    narrow = sized(w, h)
    narrow.pixels.data = image.pixels.data
    narrow.stride = w - 1
    fails(lambda: frame(im=narrow), who, "stride")

    assert (out == 7.0).all() and (img == 0x55).all() and (pixels == 0x55).all()
    assert (lin_low == 7.0).all() and (lin_up == 7.0).all() and (lin_out == 7.0).all()
    lib.rt_clear_error()


def device_address(k, A):
    order = ("color_low", "coverage_low", "albedo_low", "normal_low", "position_low", "coverage", "albedo", "normal", "position", "out",
             "image", "work")
    return (order.index(k) + 1) * A
