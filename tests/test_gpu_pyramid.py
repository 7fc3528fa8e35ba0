"""The pyramid culls of the path kernel (tile_pyramid, pyramid_cull_mask / node_enter_few, leafless_walk, pyramid_cull_tris /
leaf_test_uniform) at the scales where their margin arguments are weakest -- the scene and camera lists of tests/_pyramid.py,
whose aim tests/test_pyramid_cpu.py checks on the CPU: triangles that are large compared with their distance from the camera, with
the reference's fattened edge band reaching into a tile whose pyramid the three vertices are clear of; camera matrices that are no
rotations, focal lengths down to 0, extreme aspect ratios, a camera 1e5 units from the origin.

Everything is bit-exact against the CPU oracle, no tolerance: the u64 radiance sums, the image and all seven counters of a frame
(node_visits and leaf_visits are the sensitive ones: a wrongly culled box or triangle loses the visits behind it), the ten feature
sums per pixel, and per ray t, the triangle, the bits of (u, v) and both visit totals of rt_test_trace_stream() called with the
tile's own pyramid.  The same frames with RT_PYRAMID=0 (the diagnostic library, a process of its own) show whether a difference
belongs to the culls."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _pyramid as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "raytracing_c_amd", "librt_hip_diag.so")
LARGE_NEAR = [s.name for s in P.large_near_scenes()]


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _check_frame(name, hs, got, want, width, height, what):
    cam = hs.scene.camera
    msg = P.describe_difference(name, hs, cam, width, height, want["accum"], got["accum"])
    assert not msg, f"{what}, radiance sums: {msg}; counters (oracle, GPU) {P.counters_differ(want['counters'], got['counters'])}"
    msg = P.describe_difference(name, hs, cam, width, height, want["image"], got["image"])
    assert not msg, f"{what}, image: {msg}"
    bad = P.counters_differ(want["counters"], got["counters"])
    assert not bad, f"{name}, {what}: counters (name, oracle, GPU) {bad}"


# ---- (a) large-near triangles with a free edge ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", LARGE_NEAR)
def test_large_near_frames(rt, oracle, name):
    """64 samples: whole waves of camera rays sit on one leaf group and take the culled leaf block; 3 samples: mixed blocks"""
    hs = P.large_near_scene(name)
    for s, b in P.FRAME_SHAPES:
        want = P.large_near_oracle(name, s, b)
        got = rt.render_frame(hs, P.WIDTH, P.HEIGHT, s, b, want_accum=True)
        _check_frame(name, hs, got, want, P.WIDTH, P.HEIGHT, f"{s} samples")


@pytest.fixture(scope="module")
def unculled_results(oracle, tmp_path_factory):
    """the frames of (a) through the diagnostic library with RT_PYRAMID=0, in one process of its own; the worker leaves the sums of
    a frame whose digest is not the oracle's in a file, for the message"""
    if not os.path.exists(DIAG):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "raytracing_c_amd", "csrc"), "diag"], stdout=subprocess.DEVNULL)
    out = tmp_path_factory.mktemp("unculled")
    jobs = [dict(config="pyramid:" + name, w=P.WIDTH, h=P.HEIGHT, s=s, b=b, env={"RT_PYRAMID": "0"}, slabs=[0],
                 expect=hashlib.sha256(P.large_near_oracle(name, s, b)["accum"].tobytes()).hexdigest(), save=str(out / f"{i}_{s}.npy"))
            for i, name in enumerate(LARGE_NEAR) for s, b in P.FRAME_SHAPES]
    env = dict(os.environ, RT_LIB_PATH=DIAG)
    for k in list(env):
        if k.startswith("RT_") and k != "RT_LIB_PATH":
            del env[k]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_diag_worker.py")], input=json.dumps(jobs), text=True,
                       capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == len(jobs), (r.stdout[-1000:], r.stderr[-1000:])
    return {(j["config"], j["s"]): (j, l) for j, l in zip(jobs, lines)}


@pytest.mark.parametrize("name", LARGE_NEAR)
def test_large_near_frames_without_the_culls(oracle, unculled_results, name):
    """the control: with the culls switched off the same frames equal the oracle's, so a failure above belongs to the culls"""
    hs = P.large_near_scene(name)
    for s, b in P.FRAME_SHAPES:
        job, got = unculled_results[("pyramid:" + name, s)]
        assert got["error"] is None, got["error"]
        want = P.large_near_oracle(name, s, b)
        if got["digests"] != [job["expect"]]:
            sums = np.load(job["save"]).astype(np.uint64)
            pytest.fail(f"RT_PYRAMID=0, {s} samples, radiance sums: "
                        + P.describe_difference(name, hs, hs.scene.camera, P.WIDTH, P.HEIGHT, want["accum"], sums))
        counters = dict(zip(("rays", "node_visits", "leaf_visits", "shades"), got["counters"]))
        bad = [(k, want["counters"][k], v) for k, v in counters.items() if want["counters"][k] != v]
        assert not bad, f"{name}, RT_PYRAMID=0, {s} samples: counters (name, oracle, GPU) {bad}"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _trace_stream(rt, d, rays, pyr, exit_lanes, mode):
    n = len(rays)
    t, tri, uv = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
    visits = (C.c_uint64 * 2)()
    pyr = np.ascontiguousarray(pyr, np.float32)
    rc = rt.diag.rt_test_trace_stream(d, n, rays.ctypes.data, pyr.ctypes.data, exit_lanes, mode, t.ctypes.data, tri.ctypes.data,
                                     uv.ctypes.data, visits)
    assert rc == 0, rt.last_error(rt.diag)
    return t, tri, uv, (int(visits[0]), int(visits[1]))


def _check_bundle(name, tile, want, got, what):
    wt, wtri, wuv, wv = want
    gt, gtri, guv, gv = got
    bad = np.flatnonzero((wtri != gtri) | (_bits(wt) != _bits(gt)) | np.any(_bits(wuv) != _bits(guv), axis=1))
    if len(bad):
        i = int(bad[0])
        pytest.fail(f"{name}, tile {tile}, {what}: {len(bad)} of {len(wt)} rays differ, the first is ray {i} (pixel {i // 64} of the tile, "
                    f"sample {i % 64}): oracle triangle slot {int(wtri[i])} at u = {float(wuv[i, 0])!r}, v = {float(wuv[i, 1])!r}, "
                    f"t = {float(wt[i])!r}; GPU triangle slot {int(gtri[i])}, t = {float(gt[i])!r}; visits (oracle, GPU) {wv} {gv}")
    assert wv == gv, f"{name}, tile {tile}, {what}: (node, leaf) visits, oracle {wv}, GPU {gv}"


@pytest.mark.parametrize("name", [s.name for s in P.large_near_scenes() if s.ratio >= 100])
def test_large_near_bundles_with_the_tiles_own_pyramid(rt, oracle, diag, name):
    """The 4096 camera rays of the tile the band reaches deepest into (64 pixels x 64 samples), through traversal_blocks() with the 19
    floats tile_pyramid() computes for that tile."""
    hs = P.large_near_scene(name)
    cam = hs.scene.camera
    tile = P.band_tile(name)
    rays = np.ascontiguousarray(P.primary_rays(cam, P.WIDTH, P.HEIGHT, P.tile_pixels(P.WIDTH, P.HEIGHT, *tile), range(64)).reshape(-1, 6))
    assert len(rays) == 4096
    want = P.trace(hs, rays, counted=True)
    pyr = P.tile_pyramid_f32(cam, P.WIDTH, P.HEIGHT, *tile)
    d = rt.diag.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error(rt.diag)
    try:
        _check_bundle(name, tile, want, _trace_stream(rt, d, rays, pyr, 48, 0), "exit_lanes 48, mode 0")
        _check_bundle(name, tile, want, _trace_stream(rt, d, rays, pyr, 1, 1), "exit_lanes 1, mode 1")
    finally:
        rt.diag.rt_scene_release(d)


@pytest.mark.parametrize("name", LARGE_NEAR)
def test_large_near_features(rt, oracle, name):
    """The first-hit feature pass (its own kernel, no culls, the same traversal blocks): all ten sums of every pixel equal the
    oracle's.  A lost floor shows up as lost coverage."""
    from tests import _features as Fe
    w, h, s, b = P.WIDTH, P.HEIGHT, 4, 3
    hs = P.large_near_scene(name)
    want = Fe.expected_cached("pyramid:" + name, hs, w, h, s, b)
    assert want["hits"] > 0 and want["misses"] > 0, name
    got = rt.render_features(hs, w, h, s, b)
    diff = np.argwhere(np.any(got["sums"] != want["sums"], axis=2))
    if len(diff):
        y, x = (int(v) for v in diff[0])
        ray = P.primary_rays(hs.scene.camera, w, h, [(x, y)], [0]).reshape(1, 6)
        t, tri, uv = P.trace(hs, ray)
        pytest.fail(f"{name}: the feature sums of {len(diff)} pixels differ, the first at (x {x}, y {y}) in tile ({x & ~7}, {y & ~7}): "
                    f"coverage sum oracle {int(want['sums'][y, x, 0])}, GPU {int(got['sums'][y, x, 0])}; the oracle's camera ray of sample 0 "
                    f"hits triangle slot {int(tri[0])} at u = {float(uv[0, 0])!r}, v = {float(uv[0, 1])!r}")


def test_large_near_frame_through_the_wavefront_pipeline(oracle, diag):
    """the trace kernel of the wavefront pipeline shares traversal_blocks() and the tile's pyramid"""
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    name = "r1000-v<0-right-reference"
    hs = P.large_near_scene(name)
    assert rt.diag.rt_set_pipeline(1) == 0
    try:
        for s, b in P.FRAME_SHAPES:
            got = rt.render_frame(hs, P.WIDTH, P.HEIGHT, s, b, want_accum=True, lib=rt.diag)
            _check_frame(name, hs, got, P.large_near_oracle(name, s, b), P.WIDTH, P.HEIGHT, f"wavefront pipeline, {s} samples")
    finally:
        rt.diag.rt_set_pipeline(0)


# ---- (b) the same floor under a real asset --------------------------------------------------------------------------------

@pytest.mark.parametrize("builder", P.BUILDERS)
def test_floor_under_spheres_frames(rt, oracle, builder):
    hs = P.floor_under_spheres(builder)
    for s, b in P.FRAME_SHAPES:
        got = rt.render_frame(hs, *P.FLOOR_SHAPE, s, b, want_accum=True)
        _check_frame("floor-spheres-" + builder, hs, got, P.floor_oracle(builder, s, b), *P.FLOOR_SHAPE, f"{s} samples")


# ---- (c) camera classes for all culls -------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", P.CAMERA_SCENES)
@pytest.mark.parametrize("matrix", P.MATRICES)
def test_camera_classes(rt, oracle, scene, matrix):
    """every focal length in every frame shape, each at 64 and at 3 samples: 24 frames of at most 2 623 pixels"""
    from tests import _oracle
    hs = P.camera_scene(scene, matrix == "far")
    saved = P.copy_camera(hs.scene.camera)
    try:
        for case, s, b in P.camera_frames(scene, matrix):
            hs.scene.camera = P.copy_camera(case.camera)
            want = _oracle.render(hs, case.width, case.height, s, b)
            got = rt.render_frame(hs, case.width, case.height, s, b, want_accum=True)
            _check_frame(case.name, hs, got, want, case.width, case.height, f"{s} samples")
    finally:
        hs.scene.camera = saved
