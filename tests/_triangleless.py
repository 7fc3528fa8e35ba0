"""What the triangle-less tile tests share (tests/test_tile_classes_triangles.py, tests/test_gpu_triangleless_tiles.py): the tiles
that are certainly triangle-less for the kernel, from the host model (raytracing_c_amd/tile_classes.py), and the float64 statement
"the pyramid meets no triangle" of tests/_pyramid.py for whole tile sets.

TEST INFRASTRUCTURE: imports tests/_pyramid.py, so nothing under raytracing_c_amd/ may import it.
"""
import numpy as np

LIST_CAP = 32            # RT_LL_MAX (rt_tile.hip.h): entries of a tile's list, the root's included


def certainly_triangleless(hs, w, h, cap=LIST_CAP):
    """Tiles that are triangle-less for the kernel whatever the rounding of its plane tests.  Under a margin ten times stricter
    than the kernel's (1e-2) fewer boxes and fewer triangles are culled: the kernel's pruned tree and its surviving triangles are
    a part of that model's, so a tile that is triangle-less and within the caps there is so for the kernel, or leafless.  Under a
    margin ten times looser (1e-4) more is culled: a tile that still reaches a leaf box there reaches one in the kernel, so it is
    not a leafless (or sky) tile, whose paths rt_get_triangleless_paths() does not count."""
    from raytracing_c_amd import tile_classes as tc
    n_lds = tc.lds_nodes(hs.n_nodes, hs.depth)               # (16-wave workgroups: the fewest LDS nodes of the three sizes)
    assert n_lds == hs.n_nodes, "the model below assumes the whole tree in LDS"
    strict = tc.classify_scene(hs, w, h, 1e-2, triangles=True)
    loose = tc.classify_scene(hs, w, h, 1e-4, triangles=True)
    return strict["triangleless"] & ~loose["leafless"] & (strict["n_entries"] < cap) & (strict["max_surv"] <= 4)


def _bracket(hs, w, h):
    """The host model under margins a tenth above and a tenth below the kernel's 1e-3.  The rounding of the kernel's plane tests
    is four orders of magnitude below that tenth, so the kernel culls no more than the lower margin's model and no less than the
    higher one's: its pruned tree lies between the two."""
    from raytracing_c_amd import tile_classes as tc
    return tc.classify_scene(hs, w, h, 1.1e-3, triangles=True), tc.classify_scene(hs, w, h, 0.9e-3, triangles=True)


def over_the_cap(hs, w, h, cap=LIST_CAP):
    """Tiles that reach no triangle but whose list is certainly too long for the kernel: no triangle even in the larger pruned
    tree, `cap` entries or more even in the smaller one"""
    more, fewer = _bracket(hs, w, h)
    return (more["triangleless"] | (more["leafless"] & ~more["root_miss"])) & (fewer["n_entries"] >= cap)


def possibly_served(hs, w, h, cap=LIST_CAP):
    """Every tile the kernel's batch loop can serve as leafless or triangle-less: no triangle in the smaller pruned tree, which is
    within the cap there, and not a sky tile even in the larger one.  Disjoint from over_the_cap()."""
    more, fewer = _bracket(hs, w, h)
    return (fewer["triangleless"] | fewer["leafless"]) & ~more["root_miss"] & (fewer["n_entries"] < cap)


def possibly_triangleless(hs, w, h, cap=LIST_CAP):
    """the tiles of possibly_served() that can list a leaf group: the larger pruned tree reaches a leaf box"""
    more, _ = _bracket(hs, w, h)
    return possibly_served(hs, w, h, cap) & ~more["leafless"]


def nan_free(hs, w, h, tile_mask, samples):
    """the tiles of `tile_mask` all of whose camera rays of samples 0 .. samples - 1 have a finite reciprocal direction: no batch
    of such a tile hands over to the general loop (an axis-parallel ray is not NaN-free in the slab test, rt_slab_fast)"""
    from tests import _pyramid as py
    out = np.zeros_like(tile_mask)
    for ty, tx in np.argwhere(tile_mask):
        rays = py.primary_rays(hs.scene.camera, w, h, py.tile_pixels(w, h, 8 * int(tx), 8 * int(ty)), range(samples)).reshape(-1, 6)
        out[ty, tx] = bool(np.all(rays[:, 3:] != 0))
    return out


def tile_pixels(w, h):
    """(tiles_y, tiles_x) pixels of each tile that lie inside the frame"""
    ty, tx = (h + 7) // 8, (w + 7) // 8
    return np.minimum(8, w - 8 * np.arange(tx))[None, :] * np.minimum(8, h - 8 * np.arange(ty))[:, None]


def triangles_f64(hs):
    """(n, 3, 3) float64 vertices of the scene's triangles; the all-zero slots that pad a leaf group are left out"""
    soa = np.array(hs.soa_array(), np.float64)               # x0 x1 x2 y0 y1 y2 z0 z1 z2
    soa = soa[:, np.any(soa != 0, axis=0)]
    return soa.T.reshape(-1, 3, 3).transpose(0, 2, 1)


def unseparated(hs, w, h, tile_mask):
    """[(tile_x0, tile_y0, triangles)] for the tiles of `tile_mask` whose float64, margin-free pyramid (tests/_pyramid.py) is NOT
    separated from some triangle of the scene by one of its planes (_pyramid.separated with rel = 0, here for all triangles at
    once): tiles whose pyramid may meet a triangle"""
    from tests import _pyramid as py
    tris = triangles_f64(hs)
    out = []
    for ty, tx in np.argwhere(tile_mask):
        planes, origin = py.tile_pyramid_f64(hs.scene.camera, w, h, 8 * int(tx), 8 * int(ty))
        d = (tris - origin) @ np.asarray(planes).T          # (n, 3 vertices, planes)
        sep = np.any(np.all(d > 0, axis=1), axis=1)
        if not sep.all():
            out.append((8 * int(tx), 8 * int(ty), int((~sep).sum())))
    return out


ZERO_SHAPE = (128, 128)


def zero_padded_scene():
    """A hundred small triangles on a ring around the view axis, built by the reference's builder, whose last populated leaf group is
    partly empty: all-zero slots.  World and camera are moved together so that the world's origin -- where an all-zero triangle
    lies -- is inside the pyramid of a tile that reaches that group and none of its triangles: the planes alone do not cull the
    padding there (tests/_pyramid.py, EYE, avoids exactly this)."""
    from tests import _pyramid as py
    n, shift = 100, np.array([1.189, 1.551, 0.327])
    rng = np.random.default_rng(n)
    ang = rng.uniform(0, 2 * np.pi, n)
    c = np.stack([1.5 * np.cos(ang), 1.5 * np.sin(ang), rng.uniform(-0.3, 0.3, n)], axis=1)[:, None, :]
    pos = c + rng.normal(size=(n, 3, 3)) * 0.08 - shift
    cam = np.eye(4, dtype=np.float32)
    cam[:3, 3] = np.array([0.0, 0.0, 6.0]) - shift
    return py._plain_scene(pos.astype(np.float32), cam, "reference")


def needs_zero_rule(hs, w, h):
    """the tiles of certainly_triangleless() that are not triangle-less when an all-zero slot is left to the plane test"""
    from raytracing_c_amd import tile_classes as tc
    plain = tc.classify_scene(hs, w, h, 1e-2, triangles=True, zero_culled=False)["triangleless"]
    return certainly_triangleless(hs, w, h) & ~plain


LARGE_DEEP = ["r1-u<0-right-reference", "r10-u+v>1-left-reference", "r100-v<0-right-sah", "r1000-v<0-above-reference",
              "r10000-u+v>1-right-reference"]
LARGE_SHAPE = (128, 128)


def large_near_deep(name):
    """A large-near scene of tests/_pyramid.py (one triangle up to 1e4 times larger than its distance, a free edge next to a tile
    boundary) with 120 more small triangles where its other leaf group lies, far to the left above the horizon: the tree gets a
    level of nodes above the groups, which the walk of the tile set-up needs (a tree of depth 1 keeps no list)."""
    from tests import _pyramid as py
    sc = py.large_near(name)
    eye = np.array(py.EYE)
    pos = py._large_near_geometry(sc.ratio, sc.edge, sc.side, sc.boundary, sc.offset).astype(np.float64) + eye
    rng = np.random.default_rng(77)
    fill = np.stack([rng.uniform(-30, -8, 120), rng.uniform(1, 20, 120), rng.uniform(-45, -35, 120)], axis=1)[:, None, :]
    fill = fill + rng.normal(size=(120, 3, 3)) * 0.5 + eye
    cam = np.eye(4, dtype=np.float32)
    cam[:3, 3] = py.EYE
    hs = py._plain_scene(np.concatenate([pos, fill]).astype(np.float32), cam, sc.builder)
    hs.scene.camera.focal_length = py.FOCAL
    return hs
