"""The LDS split on both sides of "the tree fits" (lds_split, rt_launch.cpp): a depth-4 tree has 585 nodes and fits beside the
waves of every launch geometry (590 nodes of room under the path kernel's 16 waves, 708 under the query and feature kernels'),
a depth-5 tree has 4 681 and fits none (777 is the largest room of any geometry), so its leading nodes come from LDS and the
rest from memory.  Frame, batch query with 16 and with 8 waves per workgroup, feature pass: each equals the oracle bit for bit.
(The depth-5 frame is tests/test_gpu_random_scenes.py's 40 000-triangle case.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOUPS = {4: (21, 5000), 5: (9, 40000)}      # depth -> (seed, triangles) of tests.test_gpu_random_scenes.make_scene
NODES = {4: 585, 5: 4681}
ROOM_MIN, ROOM_MAX = 590, 777               # nodes of room: the smallest (16 waves with accumulator tiles) and the largest of any geometry


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def soups():
    from tests.test_gpu_random_scenes import make_scene
    out = {}
    for depth, (seed, n_tris) in SOUPS.items():
        hs = make_scene(seed, n_tris)
        assert hs.depth == depth and hs.n_nodes == NODES[depth], (hs.depth, hs.n_nodes)
        out[depth] = hs
    assert NODES[4] <= ROOM_MIN and NODES[5] > ROOM_MAX
    return out


def test_frame_of_a_tree_that_fits(rt, oracle, soups):
    from tests import _oracle
    hs = soups[4]
    w, h, s, b = 64, 64, 4, 4
    want = _oracle.render(hs, w, h, s, b, seed=3)
    assert want["counters"]["shades"] > 200 and want["counters"]["backgrounds"] > 200
    got = rt.render_frame(hs, w, h, s, b, seed=3, want_accum=True)
    assert np.array_equal(want["accum"], got["accum"]) and np.array_equal(want["image"], got["image"])
    for k in ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured"):
        assert want["counters"][k] == getattr(got["counters"], k), k


@pytest.mark.parametrize("depth", [4, 5])
def test_batch_queries_with_16_and_8_waves(rt, oracle, soups, diag, depth):
    import torch
    from tests.test_gpu_query import _Dev, _oracle_trace, _rays, _same_hits
    hs = soups[depth]
    rays = _rays(hs, 20000, np.random.default_rng(depth))
    want, visits = _oracle_trace(oracle, hs, rays)
    assert int((want["triangle"] >= 0).sum()) > len(rays) // 10
    # (a batch of at most num_cus * 512 rays is the one the product traces with 8 waves per workgroup)
    assert len(rays) <= torch.cuda.get_device_properties(0).multi_processor_count * 512
    _same_hits(want, rt.closest_hits(hs, rays))
    c = rt.get_query_counters()
    assert (c.node_visits, c.leaf_visits) == visits
    for waves in ("16", "8"):
        os.environ["RT_QUERY_WG_WAVES"] = waves
        try:
            dd = _Dev(rt, hs, lib=diag)
            try:
                _same_hits(want, dd.closest(rays))
                c = rt.get_query_counters(lib=diag)
                assert (c.node_visits, c.leaf_visits) == visits, waves
            finally:
                dd.close()
        finally:
            del os.environ["RT_QUERY_WG_WAVES"]


@pytest.mark.parametrize("depth", [4, 5])
def test_feature_pass(rt, oracle, soups, depth):
    from tests import _features as F
    from tests.test_gpu_features import _same
    hs = soups[depth]
    w, h, s, b = 64, 64, 4, 4
    want = F.expected_cached("soup-depth-%d" % depth, hs, w, h, s, b)
    assert want["hits"] > 1000 and want["misses"] + want["exhausted"] > 100      # (the camera sits inside the soup: no sky, but back faces)
    _same(rt.render_features(hs, w, h, s, b), want["sums"], s)
