"""What the host side holds on the device over a process's life (csrc/rt_mem.h): buffers that grow, shrink back to a smaller
request and grow again give the oracle's results every time and allocate nothing once warm; dropping a scene copy gives back
exactly what it held, also under a frame in flight; a process that used every kind of state ends cleanly.  The byte counts are
rt_diag_device_bytes_live() of the diagnostic library -- the library's own count, exact whatever else runs on the card."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, B = 2, 2                                                    # samples, bounces of every case
FRAMES = [(16, 16), (96, 64), (16, 16), (33, 17)]              # grow, shrink, grow (ragged: no multiple of the 8-pixel tile)
VIEW_COUNTS = [1, 3, 2]
VIEW_SEEDS = [5, 0xBEEF, 77]
RAY_COUNTS = [64, 5000, 64]
FEATURES = [(8, 8), (40, 24), (8, 8)]


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def hs():
    from raytracing_c_amd.configs import load_config
    return load_config("spheres")[0]


_expected = {}


def _once(key, make):
    """the oracle's answer, computed once and shared by the passes and tests that need it"""
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def _want_frame(hs, w, h, seed=0x1234ABCD):
    from tests import _oracle
    return _once(("frame", w, h, seed), lambda: _oracle.render(hs, w, h, S, B, seed=seed)["image"])


def _cameras(hs):
    from tests.test_gpu_views import _five_views
    return _once("cameras", lambda: _five_views(hs)[:3])


def _want_view(hs, v):
    from tests import _oracle
    from tests.test_gpu_views import _copy

    def make():
        saved = _copy(hs.scene.camera)
        hs.scene.camera = _cameras(hs)[v]
        try:
            return _oracle.render(hs, 32, 32, S, B, seed=VIEW_SEEDS[v])["image"]
        finally:
            hs.scene.camera = saved
    return _once(("view", v), make)


def _want_rays(oracle, hs, n):
    from tests.test_gpu_query import _oracle_trace, _rays

    def make():
        rays = _rays(hs, n, np.random.default_rng(n))
        return rays, _oracle_trace(oracle, hs, rays)[0]
    return _once(("rays", n), make)


def _want_features(hs, w, h):
    from tests import _features as F
    return F.expected_cached("lifecycle-spheres", hs, w, h, S, B)["sums"]


def _zero_counters(c):
    return (c.paths, c.rays, c.node_visits, c.leaf_visits, c.shades, c.backgrounds, c.textured) == (0,) * 7


def _frames(rt, lib, hs):
    for w, h in FRAMES:
        assert np.array_equal(rt.render_frame(hs, w, h, S, B, lib=lib)["image"], _want_frame(hs, w, h)), (w, h)


def _views(rt, lib, hs):
    for k in VIEW_COUNTS:
        got = rt.render_views(hs, _cameras(hs)[:k], 32, 32, S, B, seeds=VIEW_SEEDS[:k], lib=lib)
        for v in range(k):
            assert np.array_equal(got[v]["image"], _want_view(hs, v)), (k, v)


def _queries(rt, lib, oracle, hs):
    from tests.test_gpu_query import _same_hits
    for n in RAY_COUNTS:
        rays, want = _want_rays(oracle, hs, n)
        _same_hits(want, rt.closest_hits(hs, rays, lib=lib))
    for n in RAY_COUNTS:
        rays, want = _want_rays(oracle, hs, n)
        assert np.array_equal(rt.occluded(hs, rays, lib=lib), (want["triangle"] >= 0).astype(np.uint8)), n


def _features(rt, lib, hs):
    for w, h in FEATURES:
        assert np.array_equal(rt.render_features(hs, w, h, S, B, lib=lib)["sums"], _want_features(hs, w, h)), (w, h)


def _lanes(rt, lib, hs, w=96, h=64):
    a = rt.frame_begin(hs, w, h, S, B, lib=lib)
    b = rt.frame_begin(hs, w, h, S, B, seed=7, lib=lib)
    rt.frame_end(a[0], lib=lib)
    rt.frame_end(b[0], lib=lib)
    assert np.array_equal(a[1], _want_frame(hs, w, h)) and np.array_equal(b[1], _want_frame(hs, w, h, seed=7))


def test_grow_shrink_grow_allocates_nothing_once_warm(rt, diag, oracle, hs):
    """Every result of both passes equals the oracle's; after the first pass of the whole sequence the second leaves the count
    of device bytes exactly where it was (buffers never shrink; what is sized for ONE launch -- the schedule feedback -- ends the
    pass as it ended the one before)."""
    live = []
    for _ in range(2):
        _frames(rt, diag, hs)
        _views(rt, diag, hs)
        _queries(rt, diag, oracle, hs)
        _features(rt, diag, hs)
        live.append(diag.rt_diag_device_bytes_live())
    assert live[0] > 0 and live[1] == live[0], live


def test_dropping_a_scene_copy_gives_back_exactly_what_it_held(rt, diag, oracle, hs):
    def everything():
        first = rt.render_frame(hs, 96, 64, S, B, lib=diag)["image"]
        _views(rt, diag, hs)
        _lanes(rt, diag, hs)
        _queries(rt, diag, oracle, hs)
        _features(rt, diag, hs)
        return first

    everything()                                               # what is NOT the scene's -- workspaces, lanes, staging -- exists now
    diag.rt_scene_invalidate(C.byref(hs.scene))
    before = diag.rt_diag_device_bytes_live()
    first = everything()                                       # uploads: the copy, then its launch states as they are first used
    assert np.array_equal(first, _want_frame(hs, 96, 64))
    held = diag.rt_diag_device_bytes_live() - before
    n_tri = int(hs.scene.triangles.len)
    assert held > n_tri * (28 + 9) * 4, (held, n_tri)          # at least the shading records and the leaf tiles
    diag.rt_scene_invalidate(C.byref(hs.scene))
    assert diag.rt_diag_device_bytes_live() == before          # the copy and every launch state of it, to the byte
    assert _zero_counters(rt.render.get_counters(lib=diag))    # the counters of the last launch went with the copy: zeros
    again = rt.render_frame(hs, 96, 64, S, B, lib=diag)
    assert np.array_equal(again["image"], first) and not _zero_counters(again["counters"])


def test_a_copy_dropped_under_a_frame_in_flight_is_not_kept(rt, diag, oracle, hs):
    """tests/test_gpu_frames_in_flight.py's in-place edit, with the byte count: rt_frame_end() drops the stale copy and renders
    from a fresh one -- afterwards the device holds ONE copy of the scene."""
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _oracle
    w, h = 64, 40

    def lane_frame():
        t, out, keep = rt.frame_begin(hs, w, h, S, B, lib=diag)
        rt.frame_end(t, lib=diag)
        return out

    diag.rt_scene_invalidate(C.byref(hs.scene))                # (a copy that rendered larger frames keeps their larger buffers)
    rt.render_frame(hs, w, h, S, B, lib=diag)                  # the copy is resident, launch state 0 sized for this frame ...
    lane_frame()                                               # ... and lane 0's
    one_copy = diag.rt_diag_device_bytes_live()
    T = hs.scene.triangles
    i = int(T.len) // 2 + 37
    x0 = T.x[0][i]
    t, out, keep = rt.frame_begin(hs, w, h, S, B, lib=diag)    # in flight, from the copy made before the edit
    T.x[0][i] = x0 + 0.25                                      # edited in place, not reported
    try:
        want = _oracle.render(hs, w, h, S, B)["image"]
        rt.frame_end(t, lib=diag)                              # rendered again from a fresh copy:
        tm = abi.RT_Frame_Timing()
        assert diag.rt_get_frame_timing(C.byref(tm)) == 0 and tm.upload_ms > 0.0      # ... the frame's timing has an upload
        assert np.array_equal(out, want)
        assert diag.rt_diag_device_bytes_live() <= one_copy    # (the fresh copy has no launch state of lane 0 yet)
        assert np.array_equal(lane_frame(), want)              # unchanged now: the fresh copy serves, lane 0's state is made
        assert diag.rt_diag_device_bytes_live() == one_copy    # one copy with the launch states it had before, not two
    finally:
        T.x[0][i] = x0
        diag.rt_scene_invalidate(C.byref(hs.scene))


def test_a_process_that_used_everything_exits_cleanly(rt):
    """A fresh process renders a frame, a view batch, frames in flight, queries and a feature pass, then a frame over two
    rehearsed device slots (their worker threads stay parked), and returns from main: exit status 0, nothing on stderr --
    nothing of the library runs into the HIP runtime at exit.  (One line is not the process's: libdrm tells every process that
    opens the GPU when its table of marketing names, amdgpu.ids, is not installed.)"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "_lifecycle_worker.py")],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    stderr = [l for l in r.stderr.splitlines() if not l.endswith("amdgpu.ids: No such file or directory")]
    assert stderr == [], r.stderr
    assert r.stdout.strip().endswith("lifecycle ok"), r.stdout
