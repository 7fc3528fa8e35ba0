"""Variance-guided denoising without a GPU: the exported names in all four libraries, the struct size against the C header, the
Python mirror and entry points, the sizes the library reports, and argument errors that are reported before a device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np

NAMES = ["rt_temporal_moments_bytes", "rt_temporal_accumulate_moments", "rt_temporal_accumulate_moments_host",
         "rt_guided_variance_work_bytes", "rt_guided_denoise_variance", "rt_guided_denoise_variance_host", "rt_render_svgf"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


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
    assert callable(rt.temporal_accumulate_moments) and callable(rt.guided_denoise_variance) and callable(rt.render_svgf)
    assert rt.lib.rt_temporal_moments_bytes(1920, 1080) == 16 * 1920 * 1080 == abi.RT_TEMPORAL_MOMENTS_PER_PIXEL * 1920 * 1080
    assert rt.lib.rt_guided_variance_work_bytes(1920, 1080) == 64 * 1920 * 1080
    for f in (rt.lib.rt_temporal_moments_bytes, rt.lib.rt_guided_variance_work_bytes):
        rt.lib.rt_clear_error()
        assert f(0, 4) == -1 and "image size" in rt.last_error()
        assert f(1 << 15, (1 << 13) + 1) == -1
    rt.lib.rt_clear_error()


def test_the_struct_is_the_headers(tmp_path):
    """sizeof and the field offsets of RT_Variance_Params as the C compiler lays include/rt_hip.h out, against the ctypes mirror."""
    from raytracing_c_amd import ctypes_abi as abi
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(RT_Variance_Params), offsetof(RT_Variance_Params, sigma_normal),'
                   ' offsetof(RT_Variance_Params, sigma_position)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.RT_Variance_Params), abi.RT_Variance_Params.sigma_normal.offset,
                   abi.RT_Variance_Params.sigma_position.offset] == [8, 0, 4]


def test_argument_errors_before_the_device_is_touched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    w = h = 4
    plane = np.full((h, w, 3), 0.5, F32)
    out = np.full((h, w, 3), 7.0, F32)
    fp = C.POINTER(C.c_float)
    pp = plane.ctypes.data_as(fp)
    cam = abi.Camera()
    tp = abi.RT_Temporal_Params(alpha=0.1, max_history=32, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
    gp = abi.RT_Guided_Params(2, 4.0, 0.2, 1.0, 1)
    feats = abi.RT_Features(pp, pp, pp, pp)
    hp = abi.RT_History_Planes(pp, pp, pp, pp, pp)

    def fails(call, *words):
        lib.rt_clear_error()
        assert call() == -1
        for word in words:
            assert word in rt.last_error(), rt.last_error()

    def host(vp, history, moments, variance=out.ctypes.data, moments_out=None):
        return lib.rt_temporal_accumulate_moments_host(w, h, C.byref(tp), C.byref(cam), C.byref(cam), plane.ctypes.data, C.byref(feats),
                                                       history, None, None, None, None, vp, moments, moments_out, variance)
    good = abi.RT_Variance_Params(0.2, 1.0)
    fails(lambda: host(None, None, None), "rt_temporal_accumulate_moments_host", "variance params are NULL")
    for bad, word in ((abi.RT_Variance_Params(0.0, 1.0), "sigma_normal"), (abi.RT_Variance_Params(float("nan"), 1.0), "sigma_normal"),
                      (abi.RT_Variance_Params(0.2, -1.0), "sigma_position"), (abi.RT_Variance_Params(0.2, float("nan")), "sigma_position")):
        fails(lambda: host(C.byref(bad), None, None), word)
    fails(lambda: host(C.byref(good), C.byref(hp), None), "without its moments")
    fails(lambda: host(C.byref(good), None, plane.ctypes.data), "without their history")
    fails(lambda: host(C.byref(good), None, None, variance=None), "no output is wanted")
    fails(lambda: lib.rt_temporal_accumulate_moments(w, h, C.byref(tp), C.byref(cam), None, 16, 16, 16, 16, 16, None, 32, None, None, None,
                                                     None, None, None, None, None), "d_moments_out is NULL")
    fails(lambda: lib.rt_temporal_accumulate_moments(w, h, C.byref(tp), C.byref(cam), C.byref(cam), 16, 16, 16, 16, 16, 4096, 8192, None,
                                                     None, None, None, 1 << 20, (1 << 20) + 64, None, None), "overlap")
    fails(lambda: lib.rt_guided_denoise_variance(w, h, C.byref(gp), 16, 16, 16, 16, 16, 16, None, 4096, None, None, None),
          "rt_guided_denoise_variance", "d_variance is NULL")
    fails(lambda: lib.rt_guided_denoise_variance(w, h, C.byref(gp), 16, 16, 16, 16, 16, None, None, 4096, None, 16, None), "no output is wanted")
    fails(lambda: lib.rt_guided_denoise_variance_host(w, h, C.byref(gp), plane.ctypes.data, C.byref(feats), out.ctypes.data, None, None, None),
          "variance is NULL")
    fails(lambda: lib.rt_render_svgf(None, None, 1, 1, None, None, None, None, None, None, None, None), "rt_render_svgf", "scene is NULL")
    assert (out == 7.0).all()
    lib.rt_clear_error()
