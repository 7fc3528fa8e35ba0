"""Leafless tiles (rt_kernels.hip): an 8x8 tile whose pixel pyramid, pruned through the tree from the root with the node blocks'
own plane test, reaches no leaf group is served by the batch loop of the sky tiles -- no traversal state machine, only the node
visits of its rays counted from the few boxes the pyramid can touch.  Every frame here equals the CPU oracle's: the whole u64
accumulator and all seven counters."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _u64(rt, fn):
    v = C.c_uint64()
    assert getattr(rt.lib, fn)(C.byref(v)) == 0, rt.last_error()
    return int(v.value)


def _frame_and_oracle(rt, hs, w, h, s, b):
    """(GPU frame, its leafless paths, its skipped root visits), checked against the oracle's frame"""
    from tests import _oracle
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    leafless, skipped = _u64(rt, "rt_get_leafless_paths"), _u64(rt, "rt_get_skipped_root_visits")
    want = _oracle.render(hs, w, h, s, b)
    assert np.array_equal(got["accum"], want["accum"]), "radiance sums"
    assert tuple(getattr(got["counters"], k) for k in COUNTERS) == tuple(want["counters"][k] for k in COUNTERS)
    return got, leafless, skipped


def _certainly_leafless(hs, w, h):
    """Tiles that are leafless for the kernel whatever the rounding of its plane test: leafless, and within the kernel's caps, when
    the host model (raytracing_c_amd/tile_classes.py) prunes with a margin ten times stricter than the kernel's (1e-2: fewer boxes
    culled, so the kernel's pruned tree is a part of this one), and NOT root-miss even under a margin ten times looser (1e-4) --
    a root-miss tile is a sky tile, counted by rt_get_skipped_root_visits instead."""
    from raytracing_c_amd import tile_classes as tc
    n_lds = tc.lds_nodes(hs.n_nodes, hs.depth)               # (16-wave workgroups: the fewest LDS nodes of the three sizes)
    assert n_lds == hs.n_nodes, "the model below assumes the whole tree in LDS"
    strict, loose = tc.classify_scene(hs, w, h, 1e-2), tc.classify_scene(hs, w, h, 1e-4)
    return strict["leafless"] & ~loose["root_miss"] & (strict["n_listed"] <= 8) & (strict["max_surv"] <= 4)


@pytest.mark.parametrize("name,w,h,s,b", [("helmet", 256, 144, 4, 2), ("spheres", 256, 256, 4, 4)])
def test_leafless_tiles_are_served_and_exact(rt, oracle, name, w, h, s, b):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config(name)
    t = _certainly_leafless(hs, w, h)
    n_t = int(t.sum())
    assert n_t >= 8
    got, leafless, skipped = _frame_and_oracle(rt, hs, w, h, s, b)
    print(f"{name}: |T| = {n_t}, leafless paths {leafless}, bound {0.9 * 64 * s * n_t:.0f}, skipped root visits {skipped}")
    assert leafless >= 0.9 * 64 * s * n_t
    if name == "spheres":
        # skipped root visits keep their meaning: whole pixels of sky tiles; a leafless path is a background path of another tile
        assert skipped % s == 0
        assert skipped + leafless <= got["counters"].backgrounds


def test_no_shortcut_for_rays_outside_the_fused_slab_domain(rt, oracle):
    """a scene 1e5 units from the origin: no camera ray is NaN-free in the sense of rt_slab_fast (include/rt_math.h,
    RT_SLAB_FUSED_MAX_ORIGIN), every batch of a leafless tile hands over to the general loop"""
    from tests._far_scene import translated_spheres
    _, leafless, skipped = _frame_and_oracle(rt, translated_spheres(1e5), 64, 64, 2, 2)
    assert leafless == 0 and skipped == 0


def test_tiles_over_the_caps_are_ordinary_tiles(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("tower")
    _frame_and_oracle(rt, hs, 256, 144, 4, 2)


def test_two_views_in_one_launch(rt, oracle):
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    from tests.test_gpu_views import _copy, _five_views
    hs, _ = load_config("spheres")
    w, h, s, b = 64, 64, 4, 3
    cams = [_five_views(hs)[0], _five_views(hs)[2]]
    seeds = [5, 0xBEEF]
    got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_accum=True)
    assert _u64(rt, "rt_get_leafless_paths") > 0
    saved = _copy(hs.scene.camera)
    try:
        total = dict.fromkeys(COUNTERS, 0)
        for v, (cam, sd) in enumerate(zip(cams, seeds)):
            hs.scene.camera = cam
            want = _oracle.render(hs, w, h, s, b, seed=sd)
            assert np.array_equal(got[v]["accum"], want["accum"]), f"view {v}"
            assert np.array_equal(got[v]["image"], want["image"]), f"view {v}"
            for k in COUNTERS:
                total[k] += want["counters"][k]
        assert tuple(getattr(got[0]["counters"], k) for k in COUNTERS) == tuple(total[k] for k in COUNTERS)      # (of the whole batch)
    finally:
        hs.scene.camera = saved


@pytest.mark.parametrize("w,h,s", [(256, 144, 16), (640, 360, 16)])
def test_workgroup_sizes(rt, oracle, w, h, s):
    """8- and 12-wave workgroups (tests/test_gpu_edge_cases.py: the launch geometry by paths per wave slot) carry the same loop"""
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    _, leafless, _ = _frame_and_oracle(rt, hs, w, h, s, 4)
    assert leafless > 0
