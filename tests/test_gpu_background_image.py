"""The background as a padded float image (rt_device.h: RT_KParams.bg_image; background_lookup_image(), rt_dev.hip.h), which the
path kernel's batch loop reads in place of the RGBA8 texel pool: the lookup on it equals background_lookup() BIT FOR BIT -- NaN
patterns included -- and the oracle's; rows patched by rt_scene_touch land in it with their pad column and, for the last row, the
pad row; frames under small backgrounds equal the oracle's in full.  No tolerance anywhere."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import _bg_image as B

pytestmark = pytest.mark.gpu

RT_TEST_BG_IMAGE = 8
COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")
# rt_get_skipped_root_visits / rt_get_leafless_paths of the frames below, recorded from the commit before the float image
PARENT_COUNTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bg_image_frames.json")


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _lookup(rt, diag, d, mode, dirs):
    got = np.full((len(dirs), 3), -7.0, np.float32)
    assert diag.rt_test_background(d, mode, len(dirs), dirs.ctypes.data, got.ctypes.data) == 0, rt.last_error(diag)
    return got


def _assert_same_bits(a, b, dirs, what):
    bad = np.flatnonzero(np.any(a.view(np.uint32) != b.view(np.uint32), axis=1))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(dirs)} directions differ; first: item {bad[0]}, direction {dirs[bad[0]].tolist()}\n"
                           f"{a[bad[0]].tolist()} ({a[bad[0]].view(np.uint32).tolist()})\n{b[bad[0]].tolist()} ({b[bad[0]].view(np.uint32).tolist()})")


def _assert_oracle(want, got, dirs, what):
    from tests._shade_inputs import same_bits
    bad = np.flatnonzero(~np.all(same_bits(want, got), axis=1))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(dirs)} directions differ from the oracle; first: item {bad[0]}, direction "
                           f"{dirs[bad[0]].tolist()}\noracle {want[bad[0]].tolist()}\ndevice {got[bad[0]].tolist()}")


@pytest.mark.parametrize("w,h", B.SIZES, ids=[f"{w}x{h}" for w, h in B.SIZES])
def test_image_lookup_equals_texel_lookup_and_the_oracle(rt, oracle, diag, w, h):
    hs = B.quad_scene(w, h)
    d = diag.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error(diag)
    try:
        finite, odd = B.directions(w, h)
        want = B.oracle_lookup(hs.background_image, finite)
        for lds in (0, 1):
            for dirs, name in ((finite, "finite"), (odd, "non-finite")):
                old, new = _lookup(rt, diag, d, lds, dirs), _lookup(rt, diag, d, lds | RT_TEST_BG_IMAGE, dirs)
                _assert_same_bits(old, new, dirs, f"{w}x{h}, mode {lds} against {lds | RT_TEST_BG_IMAGE}, {name} directions")
                if dirs is finite:
                    _assert_oracle(want, old, dirs, f"{w}x{h}, mode {lds}")
                    _assert_oracle(want, new, dirs, f"{w}x{h}, mode {lds | RT_TEST_BG_IMAGE}")
        assert diag.rt_test_background(d, 2, 1, finite.ctypes.data, np.zeros(3, np.float32).ctypes.data) != 0
        assert diag.rt_test_background(d, 2 | RT_TEST_BG_IMAGE, 1, finite.ctypes.data, np.zeros(3, np.float32).ctypes.data) != 0
    finally:
        diag.rt_scene_release(d)


def _both_forms(rt, diag, d, dirs):
    return [_lookup(rt, diag, d, m, dirs) for m in (1, 1 | RT_TEST_BG_IMAGE)]


@pytest.mark.parametrize("w,h", [(7, 9), (64, 32)], ids=["7x9", "64x32"])
def test_touched_rows_reach_the_image_with_their_pads(rt, oracle, diag, w, h):
    """rows 0, h - 2 and h - 1 in turn, then a block that ends in the last column of several rows: after rt_scene_touch the cached
    copy answers like a fresh upload of the edited scene, in both forms -- a stale pad row shows below row h - 1, a stale pad column
    right of column w - 1, where every direction of the last row / column has its second tap."""
    hs = B.quad_scene(w, h)
    sc = C.byref(hs.scene)
    rt.render_frame(hs, 16, 16, 1, 1, lib=diag)                      # (the copy rt_scene_touch patches is the frame path's)
    d = diag.rt_diag_cached_scene(sc)
    assert d
    dirs, _ = B.directions(w, h)
    arr = hs._bg_array
    assert arr.shape == (h, w, 3) and arr.flags["C_CONTIGUOUS"]
    before = _both_forms(rt, diag, d, dirs)
    rng = np.random.default_rng(7300)
    edits = [("row 0", (0, 0), (0, w - 1)), (f"row {h - 2}", (h - 2, 0), (h - 2, w - 1)), (f"row {h - 1}", (h - 1, 0), (h - 1, w - 1)),
             ("the last two columns of rows 1 .. 3", (1, w - 2), (3, w - 1)), ("the last texel", (h - 1, w - 1), (h - 1, w - 1))]
    for name, (y0, x0), (y1, x1) in edits:
        flat = arr.reshape(-1, 3)
        i0, i1 = y0 * w + x0, y1 * w + x1 + 1
        flat[i0:i1] = 255 - flat[i0:i1] if name == "the last texel" else rng.integers(0, 256, (i1 - i0, 3), dtype=np.uint8)
        assert diag.rt_scene_touch(sc, flat[i0:].ctypes.data, (i1 - i0) * 3) == 0, (name, rt.last_error(diag))
        assert diag.rt_diag_cached_scene(sc) == d, "patched in place"
        got = _both_forms(rt, diag, d, dirs)
        fresh = diag.rt_scene_upload(sc)
        assert fresh, rt.last_error(diag)
        try:
            want = _both_forms(rt, diag, fresh, dirs)
        finally:
            diag.rt_scene_release(fresh)
        for g, wnt, form in zip(got, want, ("texel pool", "float image")):
            _assert_same_bits(wnt, g, dirs, f"{w}x{h}, {name} touched, {form}: fresh upload against patched copy")
        _assert_same_bits(got[0], got[1], dirs, f"{w}x{h}, {name} touched: texel pool against float image")
        _assert_oracle(B.oracle_lookup(hs.background_image, dirs), got[1], dirs, f"{w}x{h}, {name} touched, float image")
        assert not np.array_equal(got[1].view(np.uint32), before[1].view(np.uint32)), f"{name}: the edit is visible to these directions"
        before = got


def _u64(rt, fn):
    v = C.c_uint64()
    assert getattr(rt.lib, fn)(C.byref(v)) == 0, rt.last_error()
    return int(v.value)


@pytest.fixture(scope="module")
def frame_scenes():
    from raytracing_c_amd.configs import ASSETS, load_config
    from raytracing_c_amd.loaders import load_model
    scenes = {f"spheres-{w}x{h}": load_model(os.path.join(ASSETS, "spheres.glb"), background=B.background(w, h)) for w, h in ((5, 3), (7, 9))}
    scenes["helmet"] = load_config("helmet")[0]
    return scenes


FRAMES = [("spheres-5x3", 64, 64, 4, 4), ("spheres-5x3", 64, 64, 64, 4), ("spheres-7x9", 64, 64, 4, 4), ("spheres-7x9", 64, 64, 64, 4),
          ("helmet", 128, 128, 8, 3)]


@pytest.mark.parametrize("name,w,h,s,b", FRAMES, ids=[f"{f[0]}-{f[3]}spp" for f in FRAMES])
def test_frames_equal_the_oracle_in_full(rt, oracle, frame_scenes, name, w, h, s, b):
    """sums, image and all seven counters; the batch loop serves the paths it served before the float image (the two counts of
    the parent commit's frames, tests/golden/bg_image_frames.json)"""
    from tests import _oracle
    hs = frame_scenes[name]
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    skipped, leafless = _u64(rt, "rt_get_skipped_root_visits"), _u64(rt, "rt_get_leafless_paths")
    want = _oracle.render(hs, w, h, s, b)
    assert np.array_equal(got["accum"], want["accum"]), "radiance sums"
    assert np.array_equal(got["image"], want["image"]), "image"
    assert tuple(getattr(got["counters"], k) for k in COUNTERS) == tuple(want["counters"][k] for k in COUNTERS)
    with open(PARENT_COUNTS) as f:
        parent = json.load(f)[f"{name}-{w}x{h}-{s}spp-{b}b"]
    print(f"{name} {s} spp: skipped root visits {skipped} (parent {parent['skipped_root_visits']}), leafless paths {leafless} "
          f"(parent {parent['leafless_paths']})")
    assert skipped + leafless > 0, "the frame has batches of the loop under test"
    assert (skipped, leafless) == (parent["skipped_root_visits"], parent["leafless_paths"])
