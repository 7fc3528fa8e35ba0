"""Batch ray queries (include/rt_hip.h: rt_query_closest, rt_query_occluded, rt_scene_hits, rt_scene_closest, rt_scene_occluded,
rt_get_query_counters) without a GPU: the symbols are exported by both libraries, the records have the same layout in C, in the
ctypes mirror and in the numpy dtypes, RT_Device_Hit is the reference's Hit up to tex_coords, every argument error is reported
before the device is touched, and without a device the host forms fail loudly and leave the caller's arrays alone."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_query_closest", "rt_query_occluded", "rt_scene_hits", "rt_scene_closest", "rt_scene_occluded", "rt_get_query_counters"]
HEAD = ["distance", "normal", "normal_geo", "point", "tangent", "bitangent", "tex_coords"]


@pytest.fixture(scope="module")
def lib():
    import raytracing_c_amd as rt
    return rt.lib


def _exported(path):
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_both_libraries_export_the_query_entry_points():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    for path in (rt.native.LIB_PATH, rt.native.DIAG_PATH):
        names = _exported(path)
        for n in NAMES:
            assert n in names, (path, n)
    for n in NAMES:
        assert n in abi.EXPORTED_SYMBOLS
        assert getattr(rt.lib, n) is not None and getattr(rt.diag, n) is not None


def test_record_layouts_match_the_c_header(tmp_path):
    from raytracing_c_amd import ctypes_abi as abi
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    exe = str(tmp_path / "query_layout")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "query_layout.c"), "-o", exe], check=True)
    got = {k: int(v) for k, v in (line.split() for line in
                                  subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["sizeof.RT_Ray_Hit"] == 16
    assert got["sizeof.RT_Device_Hit"] == 88 == got["sizeof.Hit"]
    assert got["sizeof.Ray"] == 24
    for f in HEAD:                                   # RT_Device_Hit IS Hit up to tex_coords, in C ...
        assert got["RT_Device_Hit." + f] == got["Hit." + f], f
    assert got["RT_Device_Hit.triangle"] == got["Hit.shader"] == 72
    for T in (abi.RT_Ray_Hit, abi.RT_Device_Hit, abi.Hit, abi.RT_Query_Counters):      # ... and the ctypes mirror is the C layout
        assert got["sizeof." + T.__name__] == C.sizeof(T)
        for f, *_ in T._fields_:
            assert got[f"{T.__name__}.{f}"] == getattr(T, f).offset, (T.__name__, f)
    for f in HEAD:                                   # ... and so are the numpy dtypes
        assert abi.DEVICE_HIT_DTYPE.fields[f][1] == abi.HIT_DTYPE.fields[f][1] == getattr(abi.Hit, f).offset
    assert abi.DEVICE_HIT_DTYPE.fields["triangle"][1] == 72 and abi.DEVICE_HIT_DTYPE.fields["material"][1] == 76
    assert abi.HIT_DTYPE.fields["shader_data"][1] == 72 and abi.HIT_DTYPE.fields["shader_proc"][1] == 80
    assert [abi.RAY_HIT_DTYPE.fields[f][1] for f in ("t", "triangle", "u", "v")] == [0, 4, 8, 12]


def _fails(lib, call, *words):
    from raytracing_c_amd.native import last_error
    lib.rt_clear_error()
    assert call() == -1
    msg = last_error(lib)
    for w in words:
        assert w in msg, msg
    lib.rt_clear_error()


def test_device_level_argument_errors(lib):
    fake = (C.c_uint8 * 4096)()                     # (never read: every case fails before the scene is dereferenced)
    d = C.addressof(fake)
    buf = (C.c_uint8 * 1024)()
    b = C.addressof(buf)
    _fails(lib, lambda: lib.rt_query_closest(None, 4, b, None, b, None, None), "rt_query_closest", "scene is NULL")
    _fails(lib, lambda: lib.rt_query_closest(d, 0, b, None, b, None, None), "n must be positive")
    _fails(lib, lambda: lib.rt_query_closest(d, -5, b, None, b, None, None), "n must be positive")
    _fails(lib, lambda: lib.rt_query_closest(d, (1 << 30) + 1, b, None, b, None, None), "too many rays")
    _fails(lib, lambda: lib.rt_query_closest(d, 4, None, None, b, None, None), "d_rays")
    _fails(lib, lambda: lib.rt_query_closest(d, 4, b, None, None, None, None), "d_hits")
    _fails(lib, lambda: lib.rt_query_occluded(None, 4, b, None, b, None), "rt_query_occluded", "scene is NULL")
    _fails(lib, lambda: lib.rt_query_occluded(d, 0, b, None, b, None), "n must be positive")
    _fails(lib, lambda: lib.rt_query_occluded(d, 1 << 31, b, None, b, None), "too many rays")
    _fails(lib, lambda: lib.rt_query_occluded(d, 4, None, None, b, None), "d_rays")
    _fails(lib, lambda: lib.rt_query_occluded(d, 4, b, None, None, None), "d_flags")


def test_host_level_argument_errors(lib):
    from raytracing_c_amd import ctypes_abi as abi
    scene = abi.Scene()                             # (never read: every case fails before the scene or the device is touched)
    s = C.byref(scene)
    buf = (C.c_uint8 * 1024)()
    b = C.addressof(buf)
    _fails(lib, lambda: lib.rt_scene_hits(None, 4, b, b, None), "rt_scene_hits", "scene is NULL")
    _fails(lib, lambda: lib.rt_scene_hits(s, 0, b, b, None), "n must be positive")
    _fails(lib, lambda: lib.rt_scene_hits(s, (1 << 30) + 1, b, b, None), "too many rays")
    _fails(lib, lambda: lib.rt_scene_hits(s, 4, None, b, None), "rays is NULL")
    _fails(lib, lambda: lib.rt_scene_hits(s, 4, b, None, None), "hits is NULL")
    _fails(lib, lambda: lib.rt_scene_closest(None, 4, b, None, b), "rt_scene_closest", "scene is NULL")
    _fails(lib, lambda: lib.rt_scene_closest(s, 0, b, None, b), "n must be positive")
    _fails(lib, lambda: lib.rt_scene_closest(s, (1 << 30) + 1, b, None, b), "too many rays")
    _fails(lib, lambda: lib.rt_scene_closest(s, 4, None, None, b), "rays is NULL")
    _fails(lib, lambda: lib.rt_scene_closest(s, 4, b, None, None), "hits is NULL")
    _fails(lib, lambda: lib.rt_scene_occluded(None, 4, b, None, b), "rt_scene_occluded", "scene is NULL")
    _fails(lib, lambda: lib.rt_scene_occluded(s, -1, b, None, b), "n must be positive")
    _fails(lib, lambda: lib.rt_scene_occluded(s, 1 << 40, b, None, b), "too many rays")
    _fails(lib, lambda: lib.rt_scene_occluded(s, 4, None, None, b), "rays is NULL")
    _fails(lib, lambda: lib.rt_scene_occluded(s, 4, b, None, None), "flags is NULL")
    _fails(lib, lambda: lib.rt_get_query_counters(None), "rt_get_query_counters")
    assert all(v == 0 for v in buf)


def test_host_forms_fail_loudly_without_a_device_and_touch_nothing(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("quad")
    n = 100
    rays = np.zeros((n, 6), np.float32)
    rays[:, 2], rays[:, 5] = 3.0, -1.0
    hits = np.frombuffer(bytes([0xA5]) * (88 * n), abi.HIT_DTYPE).copy()
    tri = np.full(n, 0x5A5A5A5A, np.int32)
    flags = np.full(n, 0x77, np.uint8)
    before = hits.tobytes()
    rt.lib.rt_clear_error()
    assert rt.lib.rt_scene_hits(C.byref(hs.scene), n, rays.ctypes.data, hits.ctypes.data, tri.ctypes.data) == -1
    assert "no HIP device" in rt.last_error()
    assert hits.tobytes() == before and (tri == 0x5A5A5A5A).all()
    rt.lib.rt_clear_error()
    rec = np.frombuffer(bytes([0x3C]) * (16 * n), abi.RAY_HIT_DTYPE).copy()
    assert rt.lib.rt_scene_closest(C.byref(hs.scene), n, rays.ctypes.data, None, rec.ctypes.data) == -1
    assert "no HIP device" in rt.last_error()
    assert rec.tobytes() == bytes([0x3C]) * (16 * n)
    rt.lib.rt_clear_error()
    assert rt.lib.rt_scene_occluded(C.byref(hs.scene), n, rays.ctypes.data, None, flags.ctypes.data) == -1
    assert "no HIP device" in rt.last_error()
    assert (flags == 0x77).all()
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.closest_hits(hs, rays)
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.occluded(hs, rays)
    rt.lib.rt_clear_error()
