"""rt_render_views / rt_render_accumulate_views (include/rt_hip.h) without a GPU: the symbols are exported, RT_View has the
same layout in C and in the ctypes mirror, and every argument error is reported before the device is touched."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracing_c_amd", "librt_hip.so")


@pytest.fixture(scope="module")
def lib():
    import raytracing_c_amd as rt
    return rt.lib


def test_both_entry_points_are_exported():
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "rt_render_views" in names
    assert "rt_render_accumulate_views" in names


def test_rt_view_layout_matches_the_c_header(tmp_path):
    from raytracing_c_amd import ctypes_abi as abi
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    exe = str(tmp_path / "views_layout")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "views_layout.c"), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {"sizeof": C.sizeof(abi.RT_View), "align": C.alignment(abi.RT_View), "camera": abi.RT_View.camera.offset,
            "seed": abi.RT_View.seed.offset, "camera.focal_length": abi.RT_View.camera.offset + abi.Camera.focal_length.offset}
    assert {k: int(v) for k, v in got.items()} == want


def _images(sizes, components=3, stride_minus=0):
    from raytracing_c_amd import ctypes_abi as abi
    images = (abi.Image * len(sizes))()
    keep = []
    for i, (w, h) in enumerate(sizes):
        buf = (C.c_uint8 * (w * h * 4))()
        keep.append(buf)
        images[i].components = components
        images[i].width = w
        images[i].stride = w - stride_minus
        images[i].height = h
        images[i].pixels.data = C.addressof(buf)
        images[i].pixels.len = len(buf)
    return images, keep


def _views(n):
    from raytracing_c_amd import ctypes_abi as abi
    views = (abi.RT_View * n)()
    for v in range(n):
        views[v].camera.focal_length = 1.0
        views[v].seed = v
    return views


def _fails(lib, call, *words):
    from raytracing_c_amd.native import last_error
    lib.rt_clear_error()
    assert call() == -1
    msg = last_error(lib)
    for w in words:
        assert w in msg, msg
    lib.rt_clear_error()
    assert last_error(lib) == ""


def test_render_views_argument_errors(lib):
    from raytracing_c_amd import ctypes_abi as abi
    scene = abi.Scene()                         # (never read: every case fails before the scene or the device is touched)
    views = _views(3)
    imgs, keep = _images([(16, 8)] * 3)
    P = C.byref

    def rv(scene_p, n, views_p, images_p, samples=4, bounces=2):
        return lambda: lib.rt_render_views(scene_p, n, views_p, images_p, samples, bounces, None, None)

    _fails(lib, rv(None, 3, views, imgs), "scene")
    _fails(lib, rv(P(scene), 3, None, imgs), "views")
    _fails(lib, rv(P(scene), 3, views, None), "images")
    _fails(lib, rv(P(scene), 0, views, imgs), "n_views")
    _fails(lib, rv(P(scene), -2, views, imgs), "n_views")
    mixed, keep2 = _images([(16, 8), (16, 8), (16, 9)])
    _fails(lib, rv(P(scene), 3, views, mixed), "image 2", "same size")
    two_comp, keep3 = _images([(16, 8)] * 3, components=2)
    _fails(lib, rv(P(scene), 3, views, two_comp), "components")
    narrow, keep4 = _images([(16, 8)] * 3, stride_minus=1)
    _fails(lib, rv(P(scene), 3, views, narrow), "stride")
    _fails(lib, rv(P(scene), 3, views, imgs, samples=0), "samples")
    _fails(lib, rv(P(scene), 3, views, imgs, bounces=-1), "max_bounces")
    # 5 x 8192^2 > 2^28 pixels: each view alone is within the one-frame bound
    big, keep5 = _images([(1, 1)])
    big[0].width, big[0].stride, big[0].height, big[0].pixels.data = 8192, 8192, 8192, None
    _fails(lib, rv(P(scene), 5, _views(5), big), "too many pixels")
    # 2^27 views of 1x1: 2^27 pixels, but 16 tiles per view (one 32x32 chunk) make 2^31 tile indices.  The sizes are checked
    # before views[1 ..] or images[1 ..] are read, so one-element arrays do.
    tiny, keep6 = _images([(1, 1)])
    _fails(lib, rv(P(scene), 1 << 27, _views(1), tiny), "too many tiles")
    assert lib.rt_render_views(P(scene), (1 << 27) - 1, _views(1), tiny, 0, 2, None, None) == -1   # (samples: still checked first)


def test_render_accumulate_views_argument_errors(lib):
    from raytracing_c_amd import ctypes_abi as abi
    views = _views(2)
    accum = (C.c_uint64 * 16)()
    fake_scene = (C.c_uint8 * 4096)()           # (never read: every case fails before the scene is dereferenced)
    p = abi.RT_Render_Params(16, 8, 4, 2, 0, 0, 1, 0, 0, 0, 0)

    def av(scene_p, n, views_p, params=p, acc=accum):
        return lambda: lib.rt_render_accumulate_views(scene_p, C.byref(params), n, views_p, acc, None)

    _fails(lib, av(None, 2, views), "NULL scene")
    _fails(lib, av(C.addressof(fake_scene), 2, views, acc=None), "accumulation buffer")
    _fails(lib, av(C.addressof(fake_scene), 0, views), "n_views")
    _fails(lib, av(C.addressof(fake_scene), 2, None), "views")
    bad = abi.RT_Render_Params(16, 8, 4, 2, 0, 0, 1, 0, 0, 3, 2)      # samples [3, 5) of 4
    _fails(lib, av(C.addressof(fake_scene), 2, views, params=bad), "sample range")
    big = abi.RT_Render_Params(8192, 8192, 4, 2, 0, 0, 1, 0, 0, 0, 0)
    _fails(lib, av(C.addressof(fake_scene), 5, views, params=big), "too many pixels")
    tiny = abi.RT_Render_Params(1, 1, 4, 2, 0, 0, 1, 0, 0, 0, 0)
    _fails(lib, av(C.addressof(fake_scene), 1 << 27, views, params=tiny), "too many tiles")
