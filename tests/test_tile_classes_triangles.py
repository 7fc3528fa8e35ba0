"""The host model of triangle-less tiles (raytracing_c_amd/tile_classes.py: cull_tris, classify_tiles with a triangle block): tiles
whose pyramid reaches leaf groups but no triangle of them.  CPU only."""
import numpy as np
import pytest

from raytracing_c_amd import tile_classes as tc
from tests import _triangleless as tl

FRAMES = [("helmet", 256, 256), ("helmet", 192, 108), ("spheres", 256, 256)]


@pytest.fixture(scope="module")
def scenes():
    from raytracing_c_amd.configs import load_config
    held = {}

    def get(name):
        if name not in held:
            held[name] = load_config(name)[0]
        return held[name]
    yield get
    for hs in held.values():
        hs.free()


@pytest.mark.parametrize("name,w,h", FRAMES)
def test_stricter_model_is_inside_the_float64_pyramid_model(scenes, name, w, h):
    """With the margin tightened tenfold the fp32 model culls less than the kernel.  Every tile it still calls triangle-less is one
    whose float64, margin-free pyramid (tests/_pyramid.py) is separated from EVERY triangle of the scene by one of its planes: a
    triangle below a culled box lies outside the plane that culled the box, a culled triangle outside the plane that culled it."""
    hs = scenes(name)
    strict = tc.classify_scene(hs, w, h, 1e-2, triangles=True)
    assert int(strict["triangleless"].sum()) >= 8
    assert not (strict["triangleless"] & strict["leafless"]).any()
    assert tl.unseparated(hs, w, h, strict["triangleless"]) == []
    # the kernel's own margin: the same statement holds (1e-3 is a thousand roundings of the plane test)
    model = tc.classify_scene(hs, w, h, 1e-3, triangles=True)
    assert tl.unseparated(hs, w, h, model["triangleless"]) == []
    assert (model["n_entries"] == model["n_listed"] - 1 + model["n_groups"]).all()
    assert (model["n_groups"][model["leafless"]] == 0).all()


@pytest.mark.parametrize("name,w,h", FRAMES)
def test_sizes_of_the_gpu_tests_have_enough_certain_tiles(scenes, name, w, h):
    assert int(tl.certainly_triangleless(scenes(name), w, h).sum()) >= 8


def test_all_zero_slots_never_keep_a_tile_out():
    hs = tl.zero_padded_scene()
    w, h = tl.ZERO_SHAPE
    soa = hs.soa_array()
    filled = np.any(soa != 0, axis=0).reshape(-1, 8).sum(axis=1)
    assert ((filled > 0) & (filled < 8)).any(), "a partly filled leaf group"
    with_rule = tc.classify_scene(hs, w, h, 1e-3, triangles=True)["triangleless"]
    without = tc.classify_scene(hs, w, h, 1e-3, triangles=True, zero_culled=False)["triangleless"]
    assert not (without & ~with_rule).any()                  # the rule only adds tiles ...
    assert int((with_rule & ~without).sum()) >= 1            # ... and here it does: the padding alone kept this tile out
    assert int(tl.needs_zero_rule(hs, w, h).sum()) >= 1
    # the tiles it adds meet no triangle either
    assert tl.unseparated(hs, w, h, with_rule) == []


def test_an_all_zero_group_is_culled_whatever_the_planes_say():
    """the camera looks at the world's origin: the four planes keep the point (0, 0, 0), the rule does not"""
    cam = np.eye(4, dtype=np.float32)
    cam[2, 3] = 5.0
    pn, origin = tc.tile_pyramids(cam, 2.0, 64, 64)
    centre = pn[4, 4][None]                                  # a tile next to the image centre ...
    soa = np.zeros((9, 16), np.float32)
    soa[:, 8:] = np.random.default_rng(1).normal(size=(9, 8)).astype(np.float32) * 0.01      # ... group 1: specks around the origin
    zero_group = np.array([0])
    assert not tc.cull_tris(soa, zero_group, pn[3, 3][None], origin, zero_culled=False).all() or \
        not tc.cull_tris(soa, zero_group, centre, origin, zero_culled=False).all()
    assert tc.cull_tris(soa, zero_group, centre, origin).all()
    assert tc.cull_tris(soa, np.array([7]), centre, origin).all()          # a group past the block: nothing there
    assert not tc.cull_tris(soa, np.array([1]), centre, origin).all() or not tc.cull_tris(soa, np.array([1]), pn[3, 3][None], origin).all()


@pytest.mark.parametrize("name", tl.LARGE_DEEP)
def test_large_triangle_scenes_have_certain_tiles(name):
    hs = tl.large_near_deep(name)
    assert hs.depth >= 2
    w, h = tl.LARGE_SHAPE
    strict = tc.classify_scene(hs, w, h, 1e-2, triangles=True)["triangleless"]
    assert int(strict.sum()) >= 1
    assert tl.unseparated(hs, w, h, strict) == []
