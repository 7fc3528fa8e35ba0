"""Triangle-less tiles (rt_tile.hip.h: leafless_walk; rt_kernels.hip): an 8x8 tile whose pixel pyramid, pruned through the tree,
reaches leaf groups but no triangle of them is served by the batch loop of the sky and leafless tiles -- its rays' node and leaf
visits counted from the few boxes the pyramid can touch.  Every frame here equals the CPU oracle's: the whole u64 accumulator
and all seven counters."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _triangleless as tl

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")
FRAMES = [("helmet", 256, 256), ("helmet", 192, 108), ("spheres", 256, 256)]      # (the odd size: partial tiles)
SPP = [4, 64]                                                                     # (64: the grouped adds of the batch loop)
BOUNCES = 2


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _u64(rt, fn):
    v = C.c_uint64()
    assert getattr(rt.lib, fn)(C.byref(v)) == 0, rt.last_error()
    return int(v.value)


def _render(rt, hs, w, h, s, b):
    """the GPU frame, its triangle-less, leafless and sky counts, and what differs from the oracle's frame ('' when nothing does)"""
    from tests import _oracle
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    served = dict(triangleless=_u64(rt, "rt_get_triangleless_paths"), leafless=_u64(rt, "rt_get_leafless_paths"),
                  skipped=_u64(rt, "rt_get_skipped_root_visits"))
    want = _oracle.render(hs, w, h, s, b)
    diff = []
    if not np.array_equal(got["accum"], want["accum"]):
        bad = np.argwhere(np.any((got["accum"] != want["accum"]).reshape(h, w, -1), axis=2))
        diff.append(f"radiance sums differ at {len(bad)} pixels, the first (x {int(bad[0][1])}, y {int(bad[0][0])})")
    for k in COUNTERS:
        if getattr(got["counters"], k) != want["counters"][k]:
            diff.append(f"{k}: oracle {want['counters'][k]}, GPU {getattr(got['counters'], k)}")
    print(f"{w}x{h} {s} spp: {served}")
    assert served["triangleless"] <= served["leafless"]
    return got, served, "; ".join(diff)


@functools.lru_cache(maxsize=None)
def _scene(name):
    from raytracing_c_amd.configs import load_config
    return load_config(name)[0]


@functools.lru_cache(maxsize=None)
def _frame(rt, name, w, h, s):
    """one render per frame of FRAMES x SPP, shared by the tests below (they leave it unchanged)"""
    return _render(rt, _scene(name), w, h, s, BOUNCES)


@pytest.mark.parametrize("s", SPP)
@pytest.mark.parametrize("name,w,h", FRAMES)
def test_frames_equal_the_oracle(rt, oracle, name, w, h, s):
    _, _, diff = _frame(rt, name, w, h, s)
    assert diff == ""


@pytest.mark.parametrize("s", SPP)
@pytest.mark.parametrize("name,w,h", FRAMES)
def test_triangleless_tiles_are_served(rt, oracle, name, w, h, s):
    t = tl.certainly_triangleless(_scene(name), w, h)
    n_t = int(t.sum())
    assert n_t >= 8
    _, served, _ = _frame(rt, name, w, h, s)
    print(f"{name} {w}x{h}: |T| = {n_t}, triangle-less paths {served['triangleless']}, bound {0.9 * 64 * s * n_t:.0f}")
    assert served["triangleless"] >= 0.9 * 64 * s * n_t
    # no more than the tiles that can be served hold, and no path of a tile that reaches no leaf box among the triangle-less ones
    assert served["leafless"] <= s * int(tl.tile_pixels(w, h)[tl.possibly_served(_scene(name), w, h)].sum())
    assert served["triangleless"] <= s * int(tl.tile_pixels(w, h)[tl.possibly_triangleless(_scene(name), w, h)].sum())


def test_tiles_over_the_entry_cap_are_ordinary_tiles(rt, oracle):
    hs, w, h, s = _scene("helmet"), 512, 512, 4
    over, possible = tl.over_the_cap(hs, w, h), tl.possibly_served(hs, w, h)
    assert int(over.sum()) >= 1 and not (over & possible).any()
    _, served, diff = _render(rt, hs, w, h, s, BOUNCES)
    assert diff == ""
    assert served["leafless"] <= s * int(tl.tile_pixels(w, h)[possible].sum())        # (the tiles over the cap are not among them)
    assert served["triangleless"] <= s * int(tl.tile_pixels(w, h)[tl.possibly_triangleless(hs, w, h)].sum())
    assert served["triangleless"] >= 0.9 * 64 * s * int(tl.certainly_triangleless(hs, w, h).sum())


@pytest.mark.parametrize("name", tl.LARGE_DEEP)
def test_large_triangles_where_the_margin_argument_is_weakest(rt, oracle, name):
    """one triangle up to 1e4 times larger than its distance (the ratio 1000 ones: a 1000-unit floor triangle seen from one unit
    above it), its free edge next to a tile boundary: the triangle cull decides whole tiles of the frame"""
    hs = tl.large_near_deep(name)
    w, h = tl.LARGE_SHAPE
    _, served, diff = _render(rt, hs, w, h, 8, BOUNCES)
    assert diff == ""
    assert served["triangleless"] >= 64 * 8 * int(tl.certainly_triangleless(hs, w, h).sum()) > 0


@pytest.mark.parametrize("builder", ["reference", "sah"])
def test_floor_under_spheres(rt, oracle, builder):
    from tests import _pyramid as py
    hs = py.floor_under_spheres(builder)
    _, served, diff = _render(rt, hs, 128, 128, 8, BOUNCES)
    assert diff == ""
    assert served["triangleless"] >= 64 * 8 * int(tl.certainly_triangleless(hs, 128, 128).sum()) > 0


def test_large_near_scenes_of_depth_one_keep_no_list(rt, oracle):
    """the scenes of tests/_pyramid.py as they are: their root's children are leaf groups, the walk needs a level of nodes"""
    from tests import _pyramid as py
    for name in ("r1000-v<0-above-reference", "r10000-u+v>1-right-reference"):
        _, served, diff = _render(rt, py.large_near_scene(name), 128, 128, 8, BOUNCES)
        assert diff == "", name
        assert served["triangleless"] == 0


def test_hand_over_outside_the_fused_slab_domain(rt, oracle):
    """a scene 1e5 units from the origin: no camera ray is NaN-free in the sense of rt_slab_fast (include/rt_math.h), every batch
    of a leafless or triangle-less tile hands over to the general loop"""
    from tests._far_scene import translated_spheres
    for w, h in ((64, 64), (256, 256)):
        _, served, diff = _render(rt, translated_spheres(1e5), w, h, 2, BOUNCES)
        assert diff == ""
        assert served["triangleless"] == 0 and served["leafless"] == 0 and served["skipped"] == 0


def test_zero_padded_groups(rt, oracle):
    """the padding of a partly filled leaf group, all-zero triangles at the world's origin, inside a tile's pyramid: the tile is
    served all the same, and nothing is accepted there"""
    hs = tl.zero_padded_scene()
    w, h = tl.ZERO_SHAPE
    t, rule = tl.certainly_triangleless(hs, w, h), tl.needs_zero_rule(hs, w, h)
    assert int(rule.sum()) >= 1 and int(t.sum()) >= 8
    for s in (4, 64):
        _, served, diff = _render(rt, hs, w, h, s, BOUNCES)
        assert diff == ""
        assert served["triangleless"] >= 0.9 * 64 * s * int(t.sum())
        # every path of every certain tile whose rays are all NaN-free (whole tiles, no hand-over), the one the padding would keep
        # out among them
        clean = tl.nan_free(hs, w, h, t, s)
        assert (rule & clean).any() and int(clean.sum()) >= int(t.sum()) - 2
        assert served["triangleless"] >= 64 * s * int(clean.sum())
        # ... which only holds with that tile served: the other tiles that can list a group at all are as many as the bound's, and
        # one of them hands a batch over to the general loop
        possible = tl.possibly_triangleless(hs, w, h)
        assert served["triangleless"] <= 64 * s * int(possible.sum())
        assert int(possible.sum()) - 1 == int(clean.sum()) and (possible & ~clean & ~rule).any()
