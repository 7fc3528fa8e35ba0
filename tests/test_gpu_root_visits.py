"""Root visits in front of the traversal call (rt_kernels.hip): when the root has at most four populated children, every NaN-free
ray that the S block starts takes its root visit before the first traversal round -- node_enter_few() over the populated children,
camera and bounce rays in one block -- instead of a node block of its own.  rt_get_fused_root_visits() counts the rays served
this way.  Every frame here equals the CPU oracle's: the whole u64 accumulator and all seven counters."""
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


def _root_children(hs):
    """populated children of the root: an all-zero box counts as empty, as in the kernel"""
    nodes = hs.nodes_array()
    if len(nodes) == 0:
        return 0
    return int(np.any(nodes[0] != 0.0, axis=0).sum())


def _frame(rt, hs, w, h, s, b, seed=0x1234ABCD):
    """(GPU frame, fused root visits, skipped root visits, leafless paths); the frame is checked against the oracle's"""
    from tests import _oracle
    got = rt.render_frame(hs, w, h, s, b, seed=seed, want_accum=True)
    fused, skipped, leafless = (_u64(rt, "rt_get_fused_root_visits"), _u64(rt, "rt_get_skipped_root_visits"),
                                _u64(rt, "rt_get_leafless_paths"))
    want = _oracle.render(hs, w, h, s, b, seed=seed)
    assert np.array_equal(got["accum"], want["accum"]), "radiance sums"
    assert tuple(getattr(got["counters"], k) for k in COUNTERS) == tuple(want["counters"][k] for k in COUNTERS)
    print(f"rays {got['counters'].rays}, fused {fused}, skipped {skipped}, leafless {leafless}")
    return got, fused, skipped, leafless


def _every_started_ray_is_fused(got, fused, skipped, leafless, not_nan_free=0):
    """every ray that the sky / leafless loop does not serve starts in an S block, and its root visit runs at the top of the traversal
    call behind that block -- unless the ray is not NaN-free (rt_slab_fast, include/rt_math.h: a direction component that is exactly
    zero or not finite): such a ray keeps the node blocks by design.  `not_nan_free`: the number of those rays in the frame; the
    count does not depend on scheduling, so the equality is exact."""
    started = got["counters"].rays - skipped - leafless
    print(f"started {started}, fused {fused}, not fused {started - fused}")
    assert fused == started - not_nan_free
    assert fused > 0


@pytest.mark.parametrize("name,w,h,s,b,root", [("spheres", 256, 256, 4, 4, 2), ("tower", 256, 144, 4, 2, 2),
                                               ("helmet", 256, 144, 4, 2, 4)])
def test_each_arm_at_the_root_of_the_assets(rt, oracle, name, w, h, s, b, root):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config(name)
    assert _root_children(hs) == root
    # tower: axis-aligned walls, and exactly one of the 35 907 rays this frame starts has a direction component that is exactly zero:
    # it is not NaN-free and takes the exact node block (a ledger build counts those blocks in this frame).  The frame is
    # deterministic, so the count is pinned: fused == rays - skipped - leafless - 1.  Everywhere else no such ray occurs.
    _every_started_ray_is_fused(*_frame(rt, hs, w, h, s, b), not_nan_free=1 if name == "tower" else 0)


SOUP_SEED, SOUP_TRIS = 11, 10000


def test_a_root_with_three_populated_children(rt, oracle):
    from tests.test_gpu_random_scenes import make_scene
    hs = make_scene(SOUP_SEED, SOUP_TRIS)
    assert hs.depth == 4 and _root_children(hs) == 3
    _every_started_ray_is_fused(*_frame(rt, hs, 72, 56, 6, 7, seed=SOUP_SEED))


def test_a_full_root_is_left_to_the_node_blocks(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres", builder="sah")
    assert _root_children(hs) == 8
    _, fused, _, _ = _frame(rt, hs, 256, 256, 4, 4)
    assert fused == 0


def test_a_tree_of_depth_0_has_no_root_visit(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("quad")
    assert hs.depth == 0
    _, fused, _, _ = _frame(rt, hs, 128, 128, 4, 4)
    assert fused == 0


def test_rays_outside_the_fused_slab_domain_take_the_node_blocks(rt, oracle):
    """a scene 1e5 units from the origin: no ray is NaN-free in the sense of rt_slab_fast (include/rt_math.h)"""
    from tests._far_scene import translated_spheres
    hs = translated_spheres(1e5)
    assert _root_children(hs) == 2
    _, fused, skipped, leafless = _frame(rt, hs, 64, 64, 2, 2)
    assert fused == 0 and skipped == 0 and leafless == 0


@pytest.mark.parametrize("w,h,s", [(256, 144, 16), (640, 360, 16)])
def test_mixed_blocks_and_workgroup_sizes(rt, oracle, w, h, s):
    """8- and 12-wave workgroups (the launch geometry by paths per wave slot, tests/test_gpu_edge_cases.py); with 16 samples a unit is
    two pixels of 16 paths, so an S block starts camera and bounce rays together"""
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    _every_started_ray_is_fused(*_frame(rt, hs, w, h, s, 4))


def test_two_views_in_one_launch(rt, oracle):
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    from tests.test_gpu_views import _copy, _five_views
    hs, _ = load_config("spheres")
    w, h, s, b = 64, 64, 4, 3
    cams = [_five_views(hs)[0], _five_views(hs)[2]]
    seeds = [5, 0xBEEF]
    got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_accum=True)
    fused, skipped, leafless = (_u64(rt, "rt_get_fused_root_visits"), _u64(rt, "rt_get_skipped_root_visits"),
                                _u64(rt, "rt_get_leafless_paths"))
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
    _every_started_ray_is_fused(got[0], fused, skipped, leafless)


def test_a_frame_after_a_gpu_refit(rt, oracle):
    """a GPU refit moves the root's populated child boxes in place: the frame after it equals the oracle's on the refitted scene and
    every started ray is still served.  (A refit keeps the topology, so it cannot change WHICH children are populated: this does not
    tell a mask derived in the kernel from one cached on the host.)"""
    from tests import _refit
    sp = _refit.soup(513)
    hs = sp.build("reference")
    w, h, s, b = 72, 40, 8, 4
    root = _root_children(hs)
    assert 1 <= root <= 4
    first = _frame(rt, hs, w, h, s, b, seed=9)
    _every_started_ray_is_fused(*first)
    P, N, UV = sp.moved(amount=0.08)
    before = hs.nodes_array()[0].copy()
    hs.refit(positions=P, normals=N, uvs=UV, device="gpu")
    assert not np.array_equal(before, hs.nodes_array()[0]), "the deformation must move the root's child boxes"
    second = _frame(rt, hs, w, h, s, b, seed=9)
    _every_started_ray_is_fused(*second)
    assert not np.array_equal(first[0]["accum"], second[0]["accum"]), "the deformation must be visible"


def test_one_bounce(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    got, fused, skipped, leafless = _frame(rt, hs, 64, 64, 4, 1)
    assert got["counters"].rays == got["counters"].paths            # camera rays only
    _every_started_ray_is_fused(got, fused, skipped, leafless)


def test_no_bounce_starts_no_ray(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    got, fused, _, _ = _frame(rt, hs, 64, 64, 4, 0)
    assert got["counters"].rays == 0 and fused == 0
