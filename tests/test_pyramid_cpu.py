"""The scene and camera lists of tests/_pyramid.py through the ORACLE ALONE: they reach what tests/test_gpu_pyramid.py is meant to
carry to the device, so that test cannot pass vacuously.  The counts are conditions on the lists, not measurements: a list that
misses one is a reason to change the list.

What is counted for the scenes of (a) and (b): oracle hits that lie outside the triangle proper (fattened_only: the reference's
1e-4 band beyond an edge) and come from pixels whose tile pyramid -- float64, no margin -- has all three vertices of the hit
triangle outside one plane by more than 1e-3 of their distance.  Those are the hits a cull by vertices would lose."""
import numpy as np
import pytest

from tests import _pyramid as P


def _by_class(hits):
    """per EDGES index: (such hits, tiles that have some)"""
    return [(sum(h["classes"][i] for h in hits), sum(1 for h in hits if h["classes"][i] > 0)) for i in range(3)]


def test_the_model_on_the_case_of_the_issue(oracle):
    """identity camera at the origin, focal length 2, 96 x 96, the triangle (0, -1, -1), (1000, -1, -2), (0, -1, -3): the tiles at
    (40, 80) and (40, 88) are clear of its vertices, yet hundreds of their camera rays hit it under the reference's test (through
    a plain traversal: the scene is this one triangle, its leaf group's box is left out of the count as in the restatement)"""
    cam = P.make_camera(np.eye(4, dtype=np.float32), focal_length=2.0)
    tri = np.array([[0, -1, -1], [1000, -1, -2], [0, -1, -3]], np.float64)
    for tile in ((40, 80), (40, 88)):
        pyr = P.tile_pyramid_f64(cam, 96, 96, *tile)
        assert P.separated(pyr, tri, 1e-3), tile
        assert P.separated(pyr, tri, 0.0), tile
        assert len(pyr[0]) == 4
    assert not P.separated(P.tile_pyramid_f64(cam, 96, 96, 48, 80), tri, 0.0)
    # the float32 pyramid the kernel computes is the float64 one up to rounding, with the same orientation
    for tile in ((40, 80), (0, 0), (88, 88)):
        p32 = P.tile_pyramid_f32(cam, 96, 96, *tile)
        p64 = P.tile_pyramid_f64(cam, 96, 96, *tile)[0]
        for q in range(4):
            a, b = p32[4 * q:4 * q + 3].astype(np.float64), p64[q]
            assert np.allclose(a / np.linalg.norm(a), b / np.linalg.norm(b), atol=1e-5), (tile, q)
    assert P.fattened_only(-1e-5, 0.5) and P.fattened_only(0.5, -1e-5) and P.fattened_only(0.6, 0.40001)
    assert not P.fattened_only(0.0, 0.0) and not P.fattened_only(0.5, 0.5)
    assert P.edge_class(np.array([-1e-5, 0.5, 0.6, 0.2]), np.array([0.5, -1e-5, 0.40001, 0.2])).tolist() == [0, 1, 2, -1]


def test_degenerate_and_mirrored_pyramids():
    """focal length 0: all rays in one plane, the model lists both orientations of it (and the wedge within it); a mirrored
    matrix: the planes still point outward"""
    flat = P.make_camera(np.eye(4, dtype=np.float32), focal_length=0.0)
    planes, origin = P.tile_pyramid_f64(flat, 96, 96, 80, 16)
    assert len(planes) >= 2 and np.allclose(np.abs(planes[0] / np.linalg.norm(planes[0])), [0, 0, 1])
    assert P.separated((planes, origin), np.array([[5, 1, 1], [6, 1, 2], [5, 2, 1.5]]), 1e-3)            # off the plane of the rays
    assert P.separated((planes, origin), np.array([[-5, -1, 0], [-6, -1, 0], [-5, -2, 0]]), 1e-3)        # in it, on the other side
    assert not P.separated((planes, origin), np.array([[5, 3.5, -1], [6, 5, 1], [5, 4.5, 1]]), 0.0)       # across it, in the wedge
    mirror = np.eye(4, dtype=np.float32)
    mirror[0, 0] = -1.0
    cam = P.make_camera(mirror, focal_length=2.0)
    planes, origin = P.tile_pyramid_f64(cam, 96, 96, 80, 40)          # right of the centre on the screen: x < 0 in the mirrored world
    inside = np.array([-0.375, 0.05, -1.0])
    assert np.all(planes @ inside < 0)
    p32 = P.tile_pyramid_f32(cam, 96, 96, 80, 40)
    assert all(p32[4 * q:4 * q + 3] @ inside < 0 for q in range(4))


def test_large_near_list_is_what_it_says(oracle):
    scenes = P.large_near_scenes()
    assert len(scenes) == 60 and len({s.name for s in scenes}) == 60
    for key in ("ratio", "edge", "side"):
        for value in {getattr(s, key) for s in scenes}:
            assert {s.builder for s in scenes if getattr(s, key) == value} == set(P.BUILDERS), (key, value)
    for sc in scenes:
        hs = P.large_near_scene(sc.name)
        assert hs.n_input_triangles >= 9 and hs.depth >= 1, sc.name
        sm = hs.slot_map()
        assert sm[sc.big] // 8 == sm[sc.mate] // 8, f"{sc.name}: the large triangle and its mate must share a leaf group"
        tri = P.slot_triangle(hs, sm[sc.big])
        eye = P.camera_rows(hs.scene.camera)[:, 3].astype(np.float64)
        edges = [np.linalg.norm(tri[i] - tri[(i + 1) % 3]) for i in range(3)]
        nearest = min(np.linalg.norm(v - eye) for v in tri)
        assert abs(max(edges) / nearest / sc.ratio - 1.0) < 0.01, (sc.name, max(edges) / nearest)


@pytest.mark.parametrize("edge", P.EDGES)
def test_large_near_scenes_reach_the_band(oracle, edge):
    """Per free edge: every scene of ratio 100 and more has at least 100 hits in the band from tiles that are clear of the
    triangle's vertices, over at least 2 tiles, all beyond the edge the scene is named after; ratio 1 -- the control -- has none,
    in the tiles next to the edge or anywhere else.  Ratio 10 is the turning point and has none either, in all twelve scenes:
    its band is at most 1e-4 x 10 = 1e-3 radians wide, the very clearance that is asked of the vertices, and the footprint's
    0.05 px lie between the band and the nearest ray on top of that."""
    i = P.EDGES.index(edge)
    total = tiles = 0
    for sc in (s for s in P.large_near_scenes() if s.edge == edge):
        hits = P.large_near_band(sc.name)
        per_class = _by_class(hits)
        print(sc.name, "boundary", sc.boundary, "offset", sc.offset, per_class)
        total += per_class[i][0]
        tiles += per_class[i][1]
        if sc.ratio >= 100:
            assert per_class[i][0] >= 100 and per_class[i][1] >= 2, (sc.name, per_class)
            assert per_class[i][0] >= 0.99 * sum(n for n, _ in per_class), (sc.name, per_class)
        if sc.ratio == 10:
            assert not hits, (sc.name, hits)
        if sc.ratio == 1:
            assert not hits, (sc.name, hits)
            hs = P.large_near_scene(sc.name)
            cam, slot = hs.scene.camera, int(hs.slot_map()[sc.big])
            near = P.neighbour_tiles(hs, cam, P.WIDTH, P.HEIGHT, slot)
            assert near, sc.name
            for tile in near:                                     # also where the band_hits() did not look
                rays = P.primary_rays(cam, P.WIDTH, P.HEIGHT, P.tile_pixels(P.WIDTH, P.HEIGHT, *tile), range(16)).reshape(-1, 6)
                t, tri, uv = P.trace(hs, rays)
                assert not (tri == slot).any(), (sc.name, tile)
    assert total >= 100 and tiles >= 2, (edge, total, tiles)


@pytest.mark.parametrize("builder", P.BUILDERS)
def test_floor_under_spheres_reaches_the_band(oracle, builder):
    hs = P.floor_under_spheres(builder)
    assert hs.depth >= 3
    hits = P.floor_band(builder)
    per_class = _by_class(hits)
    print(builder, per_class, [(h["tile"], h["n"]) for h in hits])
    assert per_class[0][0] >= 100 and per_class[0][1] >= 2, per_class           # the free edge of the first floor triangle is u < 0
    # the spheres are part of the frame: some camera rays hit them
    cam = hs.scene.camera
    rays = P.primary_rays(cam, *P.FLOOR_SHAPE, [(x, y) for y in range(0, 96, 4) for x in range(0, 96, 4)], [0]).reshape(-1, 6)
    tri = P.trace(hs, rays)[1]
    floor = [int(s) for s in hs.slot_map()[list(range(hs.n_input_triangles - 4, hs.n_input_triangles))]]
    assert ((tri >= 0) & ~np.isin(tri, floor)).sum() >= 20


@pytest.mark.parametrize("scene", P.CAMERA_SCENES)
@pytest.mark.parametrize("matrix", P.MATRICES)
def test_every_camera_has_sky_leaves_and_a_near_miss(oracle, scene, matrix):
    cases = P.camera_cases(scene, matrix)
    assert len(cases) == 12
    lin = P.camera_rows(cases[0].camera)[:, :3].astype(np.float64)
    det = np.linalg.det(lin)
    if matrix == "mirrored":
        assert det < 0
    if matrix.startswith("scaled"):
        assert abs(abs(det) ** (1 / 3) / float(matrix[7:]) - 1) < 1e-3
    if matrix == "far":
        assert np.all(np.abs(P.camera_rows(cases[0].camera)[:, 3]) > 9e4)
    for case in cases:
        assert np.all(np.isfinite(P.camera_rows(case.camera))) and np.isfinite(case.camera.focal_length), case.name
        assert (case.camera.focal_length == 0.0) == (case.focal == "focal0"), case.name
        for what in ("sky", "leaf", "near"):
            assert case.stats[what] >= 1, (case.name, case.stats)
    frames = P.camera_frames(scene, matrix)
    assert len(frames) == 24 and {(c.name, s) for c, s, b in frames} == {(c.name, s) for c in cases for s in (64, 3)}
