"""A CPU model of the tile pyramid and the scene and camera lists of the pyramid-cull tests (tests/test_pyramid_cpu.py,
tests/test_gpu_pyramid.py).

The path kernel culls node and leaf blocks of camera rays against the four side planes of the tile's pixel pyramid
(rt_tile.hip.h: tile_pyramid, leafless_walk; rt_dev.hip.h: pyramid_cull_mask, pyramid_cull_tris).  Each cull rests on a margin
argument.  The model here knows NOTHING of the kernel's margin rule: it is the pyramid in float64 without any margin, the plain
statement "all three vertices lie outside one plane" and the plain statement "this hit lies outside the triangle proper", so that
it stays valid whatever the kernel does about its margins.

The lists are aimed at the scales where the margin argument is weakest:
  (a) large_near_scenes(): ONE triangle that is large compared with its distance from the camera, one edge of it free and a
      fraction of a pixel to a few pixels beyond a tile boundary.  The reference accepts hits up to 1e-4 of the triangle's own SIZE
      beyond an edge (raytracer.c:137-149: u >= -1e-4, v >= -1e-4, u + v <= 1 + 1e-4); that band reaches into the tile next door,
      whose pyramid the three vertices are clear of.
  (b) floor_under_spheres(): the same floor under a real asset.
  (c) camera_cases(): camera matrices that are no rotations, focal lengths down to 0, extreme aspect ratios, 1e5 units from the
      origin.

TEST INFRASTRUCTURE: imports tests/_oracle.py, so nothing under raytracing_c_amd/ may import it.
"""
import ctypes as C
import functools
import os
from fractions import Fraction

import numpy as np

from raytracing_c_amd import ctypes_abi as abi

F = np.float32
EPS = 1e-4                                   # EPSILON of the reference's triangle test (common.h:8)
COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


# ---------------------------------------------------------------------------------------------------------------------
# the pyramid

def camera_rows(cam):
    """(3, 4) float32: the rows of the view matrix the kernels read"""
    return np.array([[cam.view_matrix.rows[i][j] for j in range(4)] for i in range(3)], F)


def make_camera(matrix, fov=0.9, focal_length=None):
    """abi.Camera of a 4 x 4 matrix and a field of view, or a focal length given directly (0 included)"""
    from raytracing_c_amd.scene import set_camera
    cam = abi.Camera()
    set_camera(cam, matrix, fov)
    if focal_length is not None:
        cam.focal_length = float(F(focal_length))
    return cam


def copy_camera(cam):
    out = abi.Camera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(abi.Camera))
    return out


def tiles_of(width, height):
    """[(tile_x0, tile_y0)] of every 8 x 8 tile that holds a pixel of the frame"""
    return [(x0, y0) for y0 in range(0, height, 8) for x0 in range(0, width, 8)]


def _fma32(a, b, c):
    """float32 fused multiply-add, correctly rounded: the exact a * b + c, then ONE rounding (ties to even)"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    f = F(float(exact))                                   # a double rounding can be off by one float32 step: look at both neighbours
    best = None
    for cand in (np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - exact)
        even = (int(np.array(cand, F).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, cand, even)
    return F(best[1])


def _diff2(a, b, c, d):
    return _fma32(a, b, -(F(c) * F(d)))                   # rt_diff2: a * b - c * d


def _dot3(a, b):
    return _fma32(a[2], b[2], _fma32(a[1], b[1], F(a[0]) * F(b[0])))      # rt_dot3: left to right


def _cross(a, b):
    return np.array([_diff2(a[1], b[2], a[2], b[1]), _diff2(a[2], b[0], a[0], b[2]), _diff2(a[0], b[1], a[1], b[0])], F)


def _footprint(width, height, tile_x0, tile_y0, dtype):
    """u coordinates of the tile's pixel footprint with tile_pyramid's 0.05 px margin, in the kernel's order of operations"""
    T = dtype
    m = T(0.05)
    if dtype is F:
        inv_w, inv_h, asp = F(1.0) / F(width), F(1.0) / F(height), F(width) / F(height)
    else:
        inv_w, inv_h, asp = 1.0 / width, 1.0 / height, float(F(width) / F(height))      # (the aspect the rays are made with)
    ux0 = (T(tile_x0) - T(0.5) - m) * T(2.0) * inv_w - T(1.0)
    ux1 = (T(tile_x0) + T(7.5) + m) * T(2.0) * inv_w - T(1.0)
    uy0 = (T(tile_y0) - T(0.5) - m) * T(2.0) * inv_h - T(1.0)
    uy1 = (T(tile_y0) + T(7.5) + m) * T(2.0) * inv_h - T(1.0)
    return ux0, ux1, uy0, uy1, asp


def tile_pyramid_f32(cam, width, height, tile_x0, tile_y0):
    """The 19 floats tile_pyramid() writes for this tile -- plane normal q at [4 q .. 4 q + 2], the ray origin at [16 .. 18] --
    computed in float32 operation for operation: plain products and sums for the corners, rt_diff2 / rt_dot3 (fused) for the
    cross products and the orientation test.
    KEEP IN STEP with tile_pyramid() (csrc/rt_tile.hip.h) and rt_dot3 / rt_diff2 (include/rt_math.h): no entry point reads the
    kernel's pyramid back, so nothing but reading the two side by side shows that they agree to the bit; the CPU test only holds
    this against the float64 model (direction within 1e-5, same orientation).  A pyramid that drifted by an ulp would still lie
    around the bundle's rays, and the bundle test would still pass, with masks computed from slightly different planes."""
    m = camera_rows(cam)
    fl = F(cam.focal_length)
    ux0, ux1, uy0, uy1, asp = _footprint(width, height, tile_x0, tile_y0, F)
    c = []
    for q in range(4):
        cx, cy, cz = (ux1 if q in (1, 2) else ux0) * asp, -(uy1 if q >= 2 else uy0), -fl
        c.append(np.array([m[i, 0] * cx + m[i, 1] * cy + m[i, 2] * cz for i in range(3)], F))
    pyr = np.zeros(19, F)
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(4):
            n = _cross(c[q], c[(q + 1) & 3])
            if _dot3(n, c[(q + 2) & 3]) > 0:
                n = n * F(-1.0)
            pyr[4 * q:4 * q + 3] = n
    pyr[16:19] = m[:, 3]
    return pyr


def tile_pyramid_f64(cam, width, height, tile_x0, tile_y0):
    """(planes (k, 3), origin (3,)) in float64, NO margin but the 0.05 px of the footprint: outward normals of the planes
    through the camera position and two neighbouring corners of the footprint.  Outward = the middle of the footprint is inside.
    With focal_length 0 the four corners and every ray lie in ONE plane through the camera and the four cross products are all
    normal to it: the planes are then both orientations of that plane (a point off it meets no ray) and, within it, the sides
    of the wedge the footprint spans seen from the camera (none when the footprint surrounds the image centre)."""
    m = camera_rows(cam).astype(np.float64)
    fl = float(cam.focal_length)
    ux0, ux1, uy0, uy1, asp = _footprint(width, height, tile_x0, tile_y0, np.float64)
    c = [m[:, :3] @ np.array([(ux1 if q in (1, 2) else ux0) * asp, -(uy1 if q >= 2 else uy0), -fl]) for q in range(4)]
    origin = m[:, 3].copy()
    mid = c[0] + c[1] + c[2] + c[3]
    normals = [np.cross(c[q], c[(q + 1) & 3]) for q in range(4)]
    inward = [float(n @ mid) for n in normals]
    if all(abs(s) > 1e-9 * np.linalg.norm(n) * np.linalg.norm(mid) for s, n in zip(inward, normals)):
        return np.array([-n if s > 0 else n for s, n in zip(inward, normals)]), origin
    flat = max(normals, key=np.linalg.norm)
    flat = flat / np.linalg.norm(flat)
    planes = [flat, -flat]
    for i in range(4):
        n = np.cross(c[i], flat)
        side = [float(n @ c[j]) for j in range(4) if j != i]
        tol = 1e-12 * np.linalg.norm(n) * max(np.linalg.norm(v) for v in c)
        if all(v <= tol for v in side):
            planes.append(n)
        elif all(v >= -tol for v in side):
            planes.append(-n)
    return np.array(planes), origin


def separated(tile, triangle, rel):
    """tile = (planes, origin) of tile_pyramid_f64; triangle (3, 3).  True when all three vertices lie outside ONE plane by more
    than rel * |n| * |v - o|."""
    planes, origin = tile
    d = np.asarray(triangle, np.float64) - origin                          # (3, 3)
    dist = np.linalg.norm(d, axis=1)
    for n in planes:
        ln = np.linalg.norm(n)
        if ln > 0 and np.all(d @ n > rel * ln * dist):
            return True
    return False


def fattened_only(u, v):
    """a hit the reference accepts (u >= -1e-4, v >= -1e-4, u + v <= 1 + 1e-4) that lies outside the triangle proper"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return (u < 0) | (v < 0) | (u + v > 1)


def edge_class(u, v):
    """index into EDGES of the edge a fattened-only hit lies beyond (the most violated one), -1 for a hit inside the triangle"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    viol = np.stack([-u, -v, u + v - 1.0], axis=-1)
    return np.where(viol.max(axis=-1) > 0, viol.argmax(axis=-1), -1)


def box_clearance(tile, lo, hi):
    """The largest, over the planes, of (smallest n . (p - o) over the box) / (largest |n . (p - o)| term sum over the box): > 0
    when the box lies outside a plane, and by what fraction of its own extent.  |clearance| <= 0.01: the pyramid passes
    within 1 % of the box."""
    planes, origin = tile
    lo, hi = np.asarray(lo, np.float64) - origin, np.asarray(hi, np.float64) - origin
    best = -np.inf
    for n in planes:
        a, b = n * lo, n * hi
        nearest = np.minimum(a, b).sum()
        extent = np.maximum(np.abs(a), np.abs(b)).sum()
        if extent > 0:
            best = max(best, nearest / extent)
    return best


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's primary rays and their hits

def primary_rays(cam, width, height, pixels, samples):
    """oracle_primary_ray for every (x, y) of `pixels` and every sample of `samples`: (len(pixels), len(samples), 6) float32"""
    from tests import _oracle
    orc = _oracle.load()
    rays = np.zeros((len(pixels), len(samples), 6), F)
    ref = C.byref(cam)
    for i, (x, y) in enumerate(pixels):
        for j, s in enumerate(samples):
            orc.oracle_primary_ray(ref, width, height, int(x), int(y), int(s), rays[i, j].ctypes.data)
    return rays


def tile_pixels(width, height, tile_x0, tile_y0):
    return [(x, y) for y in range(tile_y0, min(tile_y0 + 8, height)) for x in range(tile_x0, min(tile_x0 + 8, width))]


def trace(hs, rays, counted=False):
    """oracle_trace_rays over (n, 6) rays: t, triangle slot (-1: none), uv (n, 2) [, (node visits, leaf visits)]"""
    from tests import _oracle
    orc = _oracle.load()
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    n = len(rays)
    t, tri, uv = np.zeros(n, F), np.zeros(n, np.int32), np.zeros((n, 2), F)
    if counted:
        visits = (C.c_uint64 * 2)()
        orc.oracle_trace_rays_counted(C.byref(hs.scene), n, rays.ctypes.data, t.ctypes.data, tri.ctypes.data, uv.ctypes.data, visits)
        return t, tri, uv, (int(visits[0]), int(visits[1]))
    orc.oracle_trace_rays(C.byref(hs.scene), n, rays.ctypes.data, t.ctypes.data, tri.ctypes.data, uv.ctypes.data)
    return t, tri, uv


def slot_triangle(hs, slot):
    """(3, 3) vertices of the triangle in `slot` of the scene's triangle block"""
    soa = hs.soa_array()[:, slot]                     # x0 x1 x2 y0 y1 y2 z0 z1 z2
    return np.array(soa, np.float64).reshape(3, 3).T


# ---------------------------------------------------------------------------------------------------------------------
# (a) large-near triangles with a free edge

WIDTH = HEIGHT = 96
FOCAL = 2.0
RATIOS = [1, 10, 100, 1000, 10000]                        # (longest edge) / (distance of the nearest vertex)
EDGES = ["u<0", "v<0", "u+v>1"]                           # the free edge, by the barycentric bound it is
SIDES = ["right", "left", "above", "below"]               # where the triangle lies, seen from the tile boundary its edge is near
BUILDERS = ["reference", "sah"]
BOUNDARIES = [47.5, 39.5, 55.5]                           # footprint coordinate of the tile boundary (between pixels 47 | 48, ...)
# How far beyond the boundary the edge lies, in pixels.  The band is 1e-4 * ratio radians wide, a pixel 0.0104 radians: 0.1, 1, 10,
# 100 pixels for ratios 10 .. 1e4, so the offsets of a ratio stay inside its band.
OFFSETS = {1: [0.2, 0.35], 10: [0.2, 0.35], 100: [0.2, 0.35], 1000: [0.2, 0.6, 1.5, 3.5], 10000: [0.2, 0.6, 1.5, 3.5]}
_ROT = {"right": ((1, 0), (0, 1)), "above": ((0, -1), (1, 0)), "left": ((-1, 0), (0, -1)), "below": ((0, 1), (-1, 0))}


class LargeNear:
    """name, ratio, edge, side, builder, boundary, offset; build() -> HostScene; big / mate: source indices of the large triangle
    and of the small one that shares its leaf group; triangle: (3, 3) float32 vertices of the large one in its stored order"""

    def build(self):
        return _build_large_near(self.name)


def _large_near_geometry(ratio, edge, side, boundary, offset):
    """(positions (16, 3, 3) float32; 0 = the large triangle, 1 = its mate) relative to a camera with the identity matrix.
    Canonical form: the triangle to the RIGHT of the boundary, on the floor y = -1, its free edge a-c on a vertical line of the
    screen from depth 2 to depth 3; the other sides are this one turned about the view axis."""
    sign = 1.0 if side in ("right", "below") else -1.0
    s_e = boundary + sign * offset                                  # footprint coordinate of the edge
    xe = (s_e * 2.0 / WIDTH - 1.0) / FOCAL                          # tan of its angle from the view axis ...
    if side in ("left", "above"):
        xe = -xe                                                    # ... along the canonical +x
    a = np.array([2.0 * xe, -1.0, -2.0])
    c = np.array([3.0 * xe, -1.0, -3.0])
    along = np.array([1.0, 0.0, -0.25])
    along /= np.linalg.norm(along)
    length = ratio * np.linalg.norm(a)
    for _ in range(8):                                              # longest edge = ratio x distance of the nearest vertex
        b = a + along * length
        length *= ratio * min(np.linalg.norm(v) for v in (a, b, c)) / max(np.linalg.norm(p - q) for p, q in ((a, b), (b, c), (c, a)))
    b = a + along * length
    e = (c - a) / np.linalg.norm(c - a)
    out = -((b - a) - e * ((b - a) @ e))                            # in the floor, away from the triangle, across the edge
    hb = np.linalg.norm(out)                                        # height of b over the edge: the band is EPS * hb wide
    out /= hb
    reach = 1.3 * EPS * hb + 0.002
    # the mate: a copy of the triangle a little below the floor, moved across the edge to the far side of the band.  The leaf group's
    # box is the union of its triangles, so with the mate in the group the box covers the band and the reference reaches the
    # triangle test there.  (A mate as large as the triangle itself: the surface-area builder separates a small one from it.)
    shift = out * reach + [0, -0.05, 0]
    mate = np.array([a + shift, b + shift, c + shift])
    # six specks under the body of the large triangle, hidden by it: they fill the leaf group to its eight, so that both builders
    # must cut between this group and the other one; seen from the tiles the band reaches into they lie far beyond the edge
    specks = []
    for i in range(6):
        q = a + (c - a) * ((i + 0.5) / 6.0) - out * (0.3 + 0.04 * i) + [0, -0.2, 0]
        specks.append([q, q + [0.05, 0, 0], q + [0, 0, -0.05]])
    tri = {"u<0": (a, b, c), "v<0": (a, c, b), "u+v>1": (b, a, c)}[edge]
    rng = np.random.default_rng(5150)
    # eight small triangles far to the left of everything, above the horizon: the other leaf group, and something to hit
    fill = np.stack([rng.uniform(-30, -8, 8), rng.uniform(1, 20, 8), rng.uniform(-45, -35, 8)], axis=1)[:, None, :] + rng.normal(size=(8, 3, 3)) * 1.5
    pos = np.concatenate([np.array([tri, mate]), np.array(specks), fill])
    (r00, r01), (r10, r11) = _ROT[side]
    x, y = pos[..., 0].copy(), pos[..., 1].copy()
    pos[..., 0], pos[..., 1] = r00 * x + r01 * y, r10 * x + r11 * y
    return pos.astype(F)


@functools.lru_cache(maxsize=None)
def large_near_scenes():
    """60 scenes: every ratio x free edge x side; the builder, the boundary and the offset go round by the indices so that both
    builders, every boundary and every offset meet every ratio, every edge and every side"""
    out = []
    for ir, ratio in enumerate(RATIOS):
        for ie, edge in enumerate(EDGES):
            for js, side in enumerate(SIDES):
                sc = LargeNear()
                sc.ratio, sc.edge, sc.side = ratio, edge, side
                sc.builder = BUILDERS[(ir + ie + js) % 2]
                sc.boundary = BOUNDARIES[(ie + js) % len(BOUNDARIES)]
                sc.offset = OFFSETS[ratio][(ie + 2 * js + ir) % len(OFFSETS[ratio])]
                sc.big, sc.mate = 0, 1
                sc.name = f"r{ratio}-{edge}-{side}-{sc.builder}"
                out.append(sc)
    return out


def large_near(name):
    return next(s for s in large_near_scenes() if s.name == name)


def _identity_camera():
    return np.eye(4, dtype=F)


def _plain_scene(pos, cam_matrix, builder, fov=0.9):
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import Material, build_scene
    pos = np.ascontiguousarray(pos, F)
    e1, e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    fn = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-30)
    nrm = np.repeat(fn[:, None, :], 3, axis=1).astype(F)
    uv = np.tile(np.array([[0, 0], [1, 0], [0, 1]], F), (len(pos), 1, 1))
    mats = [Material(base_color=(0.8, 0.7, 0.5), roughness=0.6), Material(base_color=(0.3, 0.5, 0.9), roughness=0.2, metalness=0.5)]
    ids = np.arange(len(pos)) % 2
    return build_scene(pos, nrm, uv, ids, mats, [], cam_matrix, fov, procedural_background(64, 32), builder=builder)


# Where the camera of (a) stands.  NOT the origin: the unused slots of a leaf group are all-zero triangles, which pyramid_cull_tris
# keeps when the camera stands on them; a group with five unused slots then never takes the culled leaf block.
EYE = (3.0, 2.0, 10.0)


def _build_large_near(name):
    sc = large_near(name)
    cam = _identity_camera()
    cam[:3, 3] = EYE
    pos = _large_near_geometry(sc.ratio, sc.edge, sc.side, sc.boundary, sc.offset).astype(np.float64) + np.array(EYE)
    hs = _plain_scene(pos, cam, sc.builder)
    hs.scene.camera.focal_length = FOCAL
    return hs


@functools.lru_cache(maxsize=None)
def large_near_scene(name):
    """the HostScene of a scene of (a), shared by the tests that need it (they leave it unchanged)"""
    return _build_large_near(name)


# ---------------------------------------------------------------------------------------------------------------------
# which hits the culls could lose

# the three bands of a triangle in (u, v), twice as wide as the reference's: beyond u = 0, beyond v = 0, beyond u + v = 1
_BANDS = (((0, 0), (0, 1), (-2 * EPS, 1 + 4 * EPS), (-2 * EPS, -2 * EPS)),
          ((0, 0), (1, 0), (1 + 4 * EPS, -2 * EPS), (-2 * EPS, -2 * EPS)),
          ((1, 0), (0, 1), (-2 * EPS, 1 + 4 * EPS), (1 + 4 * EPS, -2 * EPS)))


def band_hits(hs, cam, width, height, slots, samples, max_tiles=24, rel=1e-3):
    """Oracle hits on the triangles in `slots` that are fattened_only and come from pixels whose tile is separated(..., rel) from
    the triangle hit.  Looks at the tiles that are separated from a triangle of `slots` while one of its three bands is not,
    `max_tiles` at the most.  Returns a list of dicts: tile, slot, n (such hits), n_rays,
    classes (count per EDGES index), u_range."""
    slots = [int(s) for s in slots]
    tris = {s: slot_triangle(hs, s) for s in slots}
    cand = []
    for tile in tiles_of(width, height):
        pyr = tile_pyramid_f64(cam, width, height, *tile)
        for s, tri in tris.items():
            if not separated(pyr, tri, rel):
                continue
            a, e1, e2 = tri[0], tri[1] - tri[0], tri[2] - tri[0]
            if any(not separated(pyr, np.array([a + e1 * u + e2 * v for u, v in band]), 0.0) for band in _BANDS):
                cand.append(tile)
                break
    if len(cand) > max_tiles:                         # a first look with two samples per pixel: the tiles with the most such hits
        samples = list(samples)
        first = []
        for tile in cand:
            rays = primary_rays(cam, width, height, tile_pixels(width, height, *tile), samples[:2]).reshape(-1, 6)
            t, tri, uv = trace(hs, rays)
            first.append(-int((np.isin(tri, slots) & fattened_only(uv[:, 0], uv[:, 1])).sum()))
        cand = [cand[i] for i in np.argsort(first, kind="stable")]
    out = []
    for tile in cand[:max_tiles]:
        px = tile_pixels(width, height, *tile)
        rays = primary_rays(cam, width, height, px, samples).reshape(-1, 6)
        t, tri, uv = trace(hs, rays)
        pyr = tile_pyramid_f64(cam, width, height, *tile)
        for s in slots:
            if not separated(pyr, tris[s], rel):
                continue
            k = (tri == s) & fattened_only(uv[:, 0], uv[:, 1])
            if k.any():
                cls = edge_class(uv[k, 0], uv[k, 1])
                out.append(dict(tile=tile, slot=s, n=int(k.sum()), n_rays=len(rays), classes=[int((cls == i).sum()) for i in range(3)],
                                u_range=(float(uv[k].min()), float(uv[k].max()))))
    return out


@functools.lru_cache(maxsize=None)
def large_near_band(name):
    """band_hits() of the large triangle of a scene of (a), 16 samples per pixel"""
    hs = large_near_scene(name)
    slot = int(hs.slot_map()[large_near(name).big])
    return band_hits(hs, hs.scene.camera, WIDTH, HEIGHT, [slot], range(16))


def band_tile(name):
    """the tile of a scene of (a) with the most hits of large_near_band()"""
    hits = large_near_band(name)
    assert hits, name
    return max(hits, key=lambda h: h["n"])["tile"]


def neighbour_tiles(hs, cam, width, height, slot, rel=1e-3):
    """tiles separated from the triangle in `slot` that touch a tile which is not: where a band would be if there were one"""
    tri = slot_triangle(hs, slot)
    sep = {t: separated(tile_pyramid_f64(cam, width, height, *t), tri, rel) for t in tiles_of(width, height)}
    out = []
    for (x0, y0), s in sep.items():
        if s and any(sep.get((x0 + dx, y0 + dy)) is False for dx in (-8, 0, 8) for dy in (-8, 0, 8)):
            out.append((x0, y0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# frames: the oracle's, once per (scene, shape), and what to say when a GPU frame differs

FRAME_SHAPES = ((64, 3), (3, 3))          # (samples, max_bounces): whole waves of camera rays on one leaf group | mixed blocks


@functools.lru_cache(maxsize=None)
def large_near_oracle(name, samples, max_bounces):
    from tests import _oracle
    return _oracle.render(large_near_scene(name), WIDTH, HEIGHT, samples, max_bounces)


def describe_difference(name, hs, cam, width, height, want, got):
    """'' when the (h, w, ...) arrays are equal, else: the scene, the number of differing pixels, the first one, its tile and what
    the oracle's camera rays hit there"""
    diff = np.argwhere(np.any((want != got).reshape(height, width, -1), axis=2))
    if len(diff) == 0:
        return ""
    y, x = (int(v) for v in diff[0])
    rays = primary_rays(cam, width, height, [(x, y)], range(64)).reshape(-1, 6)
    t, tri, uv = trace(hs, rays)
    band = np.flatnonzero((tri >= 0) & fattened_only(uv[:, 0], uv[:, 1]))
    k = int(band[0]) if len(band) else 0           # a sample in a fattened band, if the pixel has one
    return (f"{name}: {len(diff)} pixels differ, the first at (x {x}, y {y}) in tile ({x & ~7}, {y & ~7}); {len(band)} of the oracle's camera "
            f"rays of samples 0 .. 63 there end in a fattened band; that of sample {k} hits triangle slot {int(tri[k])} at "
            f"u = {float(uv[k, 0])!r}, v = {float(uv[k, 1])!r}, t = {float(t[k])!r}")


def counters_differ(want, got):
    """[(name, oracle's, GPU's)] of the seven counters that differ; `got`: render.Counters"""
    return [(k, want[k], getattr(got, k)) for k in COUNTERS if want[k] != getattr(got, k)]


def scene_by_name(name):
    """a scene of the lists here by its name: a scene of (a), or "floor-spheres-<builder>" of (b)"""
    if name.startswith("floor-spheres-"):
        return floor_under_spheres(name[len("floor-spheres-"):])
    return large_near_scene(name)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the same floor under a real asset

FLOOR_SHAPE = (96, 96)
FLOOR_Y, FLOOR_X0, FLOOR_Z1, FLOOR_SIZE = -1.02, -4.5, 8.0, 2000.0
FLOOR_EDGE_COLUMN = 47.8                                        # footprint coordinate of the floor's free edge: 0.3 px right of 47 | 48


def _asset(name):
    from raytracing_c_amd.loaders import load_model_data
    return load_model_data(os.path.join(ASSETS, {"spheres": "spheres.glb", "tower": "tower.obj"}[name]))


@functools.lru_cache(maxsize=None)
def floor_under_spheres(builder="reference"):
    """spheres.glb on a floor quad of 2000 x 2000 units whose edge x = -4.5 is free, a copy of the quad a little lower and 0.3 units
    further out (the group-mate that carries the box over the band, as in (a)).  The camera stands 0.5 above the floor over that
    edge, 0.3 units behind the floor's corner, and looks along the edge, level: the edge is a vertical line of the frame from the
    horizon down, 0.3 px right of the tile boundary 47 | 48, the band to its left up to 19 px wide, the spheres to its right.
    hs.floor: source indices of the two floor triangles (the first has the free edge, u < 0)."""
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import build_scene
    from tests._shade_inputs import _look_at
    d = _asset("spheres")
    x0, x1, z0, z1, y = FLOOR_X0, FLOOR_X0 + FLOOR_SIZE, FLOOR_Z1 - FLOOR_SIZE, FLOOR_Z1, FLOOR_Y
    quad = np.array([[(x0, y, z1), (x1, y, z1), (x0, y, z0)], [(x1, y, z0), (x0, y, z0), (x1, y, z1)]], np.float64)
    pos = np.concatenate([d["positions"], quad, quad + [-0.3, -0.05, 0.0]]).astype(F)
    n0 = len(d["positions"])
    nrm = np.concatenate([d["normals"], np.tile(np.array([0, 1, 0], F), (4, 3, 1))])
    uvs = np.concatenate([d["uvs"], np.zeros((4, 3, 2), F)])
    ids = np.concatenate([d["material_ids"], np.zeros(4, np.int64)])
    fl = float(F(1.0) / np.tan(F(0.9) * F(0.5), dtype=F))
    yaw = np.arctan(-(FLOOR_EDGE_COLUMN * 2.0 / FLOOR_SHAPE[0] - 1.0) / fl)          # to the right: the edge appears left of the centre
    eye = np.array([FLOOR_X0, FLOOR_Y + 0.5, FLOOR_Z1 + 0.3])
    cam = _look_at(eye, eye + [np.sin(yaw), 0.0, -np.cos(yaw)])
    hs = build_scene(pos, nrm, uvs, ids, d["materials"], d["images"], cam, 0.9, procedural_background(64, 32), builder=builder)
    hs.floor = (n0, n0 + 1)
    return hs


@functools.lru_cache(maxsize=None)
def floor_band(builder):
    hs = floor_under_spheres(builder)
    sm = hs.slot_map()
    return band_hits(hs, hs.scene.camera, *FLOOR_SHAPE, [int(sm[i]) for i in hs.floor], range(16))


@functools.lru_cache(maxsize=None)
def floor_oracle(builder, samples, max_bounces):
    from tests import _oracle
    return _oracle.render(floor_under_spheres(builder), *FLOOR_SHAPE, samples, max_bounces)


# ---------------------------------------------------------------------------------------------------------------------
# (c) camera classes for all culls

CAMERA_SCENES = ["spheres", "tower", "soup700"]
CAMERA_SHAPES = [(256, 8), (8, 256), (61, 43)]
FOCALS = ["fov0.05", "fov0.9", "fov3.0", "focal0"]             # the FOVS of tests/_shade_inputs.py
MATRICES = ["identity", "look-z", "look-oblique", "look-down", "sheared", "far", "mirrored", "scaled-1e-3", "scaled-1e3"]
FAR = 1e5                                                       # the "far" matrix: camera AND scene moved by (1e5, 1e5, 1e5)


def _linear_part(kind):
    """the 3 x 3 linear part of camera matrix class `kind`: the six of _shade_inputs.camera_matrices(), a mirrored one and two with
    scaled columns.  The translation is chosen per scene (camera_case): these matrices are aimed at a scene, not at the origin."""
    from tests._shade_inputs import camera_matrices
    six = camera_matrices()
    if kind in MATRICES[:6]:
        return six[MATRICES.index(kind)][:3, :3].astype(np.float64)
    rot = six[2][:3, :3].astype(np.float64)
    if kind == "mirrored":
        return rot @ np.diag([-1.0, 1.0, 1.0])                  # determinant -1
    return rot * (1e-3 if kind == "scaled-1e-3" else 1e3)


@functools.lru_cache(maxsize=None)
def camera_scene(scene, far=False, builder="reference"):
    """the HostScene of a scene of (c), moved by (1e5, 1e5, 1e5) for the far camera; hs.centre, hs.radius: of its bounds"""
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import build_scene
    shift = F(FAR) if far else F(0)
    if scene == "soup700":
        rng = np.random.default_rng(700)
        c = rng.uniform(-1, 1, (700, 1, 3))
        pos = (c + rng.normal(size=(700, 3, 3)) * rng.choice([0.03, 0.1, 0.3], (700, 1, 1))).astype(F)
        hs = _plain_scene(pos + shift, _identity_camera(), builder)
    else:
        d = _asset(scene)
        pos = d["positions"].astype(F)
        hs = build_scene(pos + shift, d["normals"], d["uvs"], d["material_ids"], d["materials"], d["images"], _identity_camera(), 0.9,
                         procedural_background(64, 32), builder=builder)
    lo, hi = pos.reshape(-1, 3).min(axis=0).astype(np.float64), pos.reshape(-1, 3).max(axis=0).astype(np.float64)
    hs.centre, hs.radius = (lo + hi) / 2 + float(shift), float(np.linalg.norm(hi - lo)) / 2
    return hs


def _focal_length(focal):
    if focal == "focal0":
        return 0.0
    return float(F(1.0) / np.tan(F(focal[3:]) * F(0.5), dtype=F))                # set_camera's


def _stand(lin, focal_length, width, height, hs):
    """(point the camera aims at, unit step away from it, the distance at which the scene's bounding sphere fills 40 % of the
    frame's larger side)"""
    m0, m1, m2 = lin[:, 0], lin[:, 1], lin[:, 2]
    asp = width / height
    if focal_length > 0:                                        # the view axis -m2 through the scene's centre
        base = 2.5 * hs.radius * focal_length * np.linalg.norm(m2) / max(np.linalg.norm(m0) * asp, np.linalg.norm(m1))
        return hs.centre, m2 / np.linalg.norm(m2), base
    # focal length 0: every ray lies in the plane of the camera's x and y axes; the scene stands in the direction of the image
    # point half way to the frame's right and upper edge
    along = m0 * (0.5 * asp) + m1 * 0.5
    return hs.centre, -along / np.linalg.norm(along), 3.0 * hs.radius


class CameraCase:
    """scene, matrix, focal, width, height, name; camera: abi.Camera; far; stats: dict(sky, leaf, near) tile counts"""


def _root_boxes(hs):
    root = hs.nodes_array()[0].astype(np.float64)               # (6, 8)
    return [(root[0:3, k], root[3:6, k]) for k in range(8) if np.any(root[:, k] != 0)]


def tile_clearance(hs, cam, width, height, tile):
    """the smallest box_clearance() of the tile over the populated child boxes of the root: > 0 when the pyramid clears them all"""
    pyr = tile_pyramid_f64(cam, width, height, *tile)
    return min(box_clearance(pyr, lo, hi) for lo, hi in _root_boxes(hs))


def tile_stats(hs, cam, width, height):
    """How many tiles of the frame are SKY (the float64 pyramid clears every populated child box of the root by more than 0.2 % of
    the box's extent: twice the margin the kernel asks for, so it is a sky tile for the kernel too), pass NEAR a populated root
    child box (within 1 %: |tile_clearance| <= 0.01), reach a LEAF (one of the oracle's camera rays of samples 0 .. 15 of the
    tile's pixels hits a triangle; looked for in the four tiles deepest inside the boxes, and only until one is found: 0 or 1)."""
    tiles = tiles_of(width, height)
    cl = np.array([tile_clearance(hs, cam, width, height, t) for t in tiles])
    leaf = 0
    for i in np.argsort(cl, kind="stable")[:4]:
        if cl[i] > 0:
            break
        rays = primary_rays(cam, width, height, tile_pixels(width, height, *tiles[i]), range(16)).reshape(-1, 6)
        if (trace(hs, rays)[1] >= 0).any():
            leaf = 1
            break
    return dict(sky=int((cl > 0.002).sum()), leaf=leaf, near=int((np.abs(cl) <= 0.01).sum()))


@functools.lru_cache(maxsize=None)
def camera_case(scene, matrix, focal, width, height):
    """The camera of a class, aimed at the scene from the distance at which the pyramid of one tile just touches a child box of
    the root: between a near stand and a far one some tile changes from touching the boxes to clearing them, and the distance is
    bisected on that tile's clearance.  Other tiles are then sky, the middle of the scene reaches leaves."""
    lin = _linear_part(matrix)
    far = matrix == "far"
    hs = camera_scene(scene, far)
    fl = _focal_length(focal)
    case = CameraCase()
    case.scene, case.matrix, case.focal, case.width, case.height, case.far = scene, matrix, focal, width, height, far
    case.name = f"{scene}-{matrix}-{focal}-{width}x{height}"
    aim, step, base = _stand(lin, fl, width, height, hs)

    def camera_at(dist):
        m = np.eye(4, dtype=F)
        m[:3, :3] = lin
        m[:3, 3] = aim + step * dist
        return make_camera(m, 0.9, fl)

    tiles = tiles_of(width, height)
    near, away = 0.2 * base, max(6.0 * base, 4.0 * hs.radius)
    g_near = [tile_clearance(hs, camera_at(near), width, height, t) for t in tiles]
    g_away = [tile_clearance(hs, camera_at(away), width, height, t) for t in tiles]
    flips = sorted((i for i in range(len(tiles)) if g_near[i] < 0 < g_away[i]), key=lambda i: g_away[i])

    def touching(i):
        """the distance at which tile i passes within 0.3 % of the boxes"""
        lo, hi = near, away
        for _ in range(60):
            dist = 0.5 * (lo + hi)
            g = tile_clearance(hs, camera_at(dist), width, height, tiles[i])
            if abs(g) <= 0.003:
                break
            lo, hi = (dist, hi) if g < 0 else (lo, dist)
        return dist

    def settle(distances):
        for dist in distances:
            stats = tile_stats(hs, camera_at(dist), width, height)
            if case.stats is None or min(stats.values()) > 0:
                case.camera, case.stats = camera_at(dist), stats
            if min(stats.values()) > 0:
                return True
        return False

    case.camera, case.stats = camera_at(base), None
    # the tiles that clear the boxes last (by their clearance at the far stand) first: the others are sky by then; where that guess
    # fails (tiles that look almost the same way), every tile's distance, the largest first
    if not settle(touching(i) for i in flips[:4]):
        if not settle(sorted((touching(i) for i in flips), reverse=True)[:12]):
            settle([base])
    assert np.all(np.isfinite(camera_rows(case.camera)))
    return case


def camera_cases(scene, matrix):
    """the twelve cameras of a scene and a matrix class: every focal length in every frame shape"""
    return [camera_case(scene, matrix, focal, w, h) for focal in FOCALS for w, h in CAMERA_SHAPES]


def camera_frames(scene, matrix):
    """[(case, samples, max_bounces)]: every one of the twelve cameras of camera_cases() at both FRAME_SHAPES, 64 samples (whole waves
    of camera rays on one leaf group: the culled leaf block) and 3 (mixed blocks)"""
    return [(case, s, b) for case in camera_cases(scene, matrix) for s, b in FRAME_SHAPES]
