"""Hand-aimed inputs for the unit-level parity tests of ONE PATH STEP -- shade_hit() of raytracing_c_amd/csrc/rt_dev.hip.h and
feature_hit() of rt_features.hip -- and the oracle's answers to them (tests/test_step_inputs_cpu.py, tests/test_gpu_shade_hit.py).

A frame reaches the step only with the hits its assets produce: unit vertex normals that agree with the face, points near the
origin, tints between 0 and 1.  The list here is aimed at the rest: face-test dots that are exactly +0 or -0, dots whose
rt_v3_dot chain is not zero where their real value is, NaN dots, shading normals on the other side of the face, interpolated
normals of length 0, 1e-25 .. 3e19, corners, edges and the barycentrics the leaf test still accepts outside the triangle,
points at 1e5 and 2^20 where RT_EPS is below one ulp, infinite points, the last bounce on every arm, carried tints with 0,
denormals, values above 1 and infinity.

THE SCENE is one of its own (the lists of tests/_shade_inputs.py keep their items); it reuses that module's materials, images
and debug-proc patching.  A few dozen triangles, every one chosen for the record it produces: see GEOMETRIES, NORMAL_CLASSES and
_triangle_table().  Neither scene_init nor rt_scene_upload looks at vertex normals, so none of the classes below was refused.

AN ITEM is a hit the test names -- triangle slot, (t, u, v) -- with the ray, the carried tint and emission, the RNG state and
whether it is the path's last bounce.  shade_hit() computes the point from the ray and t, so an item need not be a true
intersection; most are (the origin is the point moved back along the direction), so that the magnitudes are a frame's.

Everything is generated from fixed seeds; the oracle's answers are computed once per process (functools.lru_cache) and shared.

TEST INFRASTRUCTURE: imports tests/_oracle.py, so nothing under raytracing_c_amd/ may import it.
"""
import ctypes as C
import functools

import numpy as np

from raytracing_c_amd import ctypes_abi as abi
from tests import _shade_inputs as S

F = np.float32
RT_EPS = F(0.0001)
MAX_BOUNCES = (1, 4)
RADIANCE_UNSET = np.array([-1.0, -2.0, -3.0], F)          # what both sides hold where the step did not end the path

bits, same_bits = S.bits, S.same_bits


# ---------------------------------------------------------------------------------------------------------------------
# float32 arithmetic of rt_math.h, exactly: rt_madd is one fused multiply-add, rt_dot3(a, b) = madd(a2, b2, madd(a1, b1, a0 * b0))

def fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd there
    (TwoSum gives the error), and 53 bits rounded to odd round to 24 bits as the exact value does"""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        up = (err > 0) == (s > 0)                                   # the exact value is larger in magnitude than s
        sb = s.view(np.int64) + np.where(fix, np.where(up, 1, -1), 0)
        return sb.view(np.float64).astype(F)


def dot32(a, b):
    """rt_v3_dot of (n, 3) float32 arrays"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        return fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))


# rt_pcg (rt_math.h) and its inverse: the state that makes the k-th draw of a shade() a chosen number
_M32 = 0xFFFFFFFF


def pcg(v):
    state = (v * 747796405 + 2891336453) & _M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & _M32
    return (word >> 22) ^ word


def pcg_inverse(r):
    word = r ^ (r >> 22)                                            # (x >> 22) ^ x: the top 22 bits are x's own
    x = (word * pow(277803737, -1, 1 << 32)) & _M32
    shift = (x >> 28) + 4                                           # the top four bits of the state survive the xorshift
    state = x
    for _ in range(8):
        state = x ^ (state >> shift)
    return ((state - 2891336453) * pow(747796405, -1, 1 << 32)) & _M32


def seed_for_zero_draw(k):
    """the RNG state whose k-th draw (1-based) is 0.0, the only u32 that rt_rand_f32 maps to 0"""
    s = 0
    for _ in range(k):
        s = pcg_inverse(s)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the scene

def _rot(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


_Z = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)        # edges (1, 0, 0), (0, 1, 0): the face normal is exactly +z
_X = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
_Y = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0]], np.float64)
_FLIP = [0, 2, 1]
# name -> (positions (3, 3), magnitude class of its points).  The axis faces and `diag` have small integer coordinates: edges,
# cross product and the normalisation of (0, 0, 1) are exact, so n_geo is EXACTLY the axis; diag's is (a, a, 0) with equal a.
GEOMETRIES = {
    "+z": (_Z + [0, 0, 0], "1"), "-z": (_Z[_FLIP] + [3, 0, 0], "1"), "+x": (_X + [6, 0, 0], "1"), "-x": (_X[_FLIP] + [9, 0, 0], "1"),
    "+y": (_Y + [12, 0, 0], "1"), "-y": (_Y[_FLIP] + [15, 0, 0], "1"),
    "diag": (np.array([[0, 0, 0], [0, 0, 1], [1, -1, 0]], np.float64) + [18, 4, 0], "1"),
    "tilt_a": (_Z @ _rot(7101).T * 1.7 + [0.3, 5.1, -2.2], "1"), "tilt_b": (_Z @ _rot(7102).T * 0.6 + [-4.4, 2.5, 1.9], "1"),
    "far_1e5": (_Z + [1e5, -1e5, 1e5], "1e5"), "far_1e5_tilt": (_Z @ _rot(7103).T * 3.0 + [-1e5, 1e5, 9e4], "1e5"),
    "far_2^20": (_Z * 2.0 + [2.0 ** 20, 2.0 ** 20, -2.0 ** 20], "2^20"), "far_2^20_tilt": (_Z @ _rot(7104).T * 5.0 + [-2.0 ** 20, 2.0 ** 20, 2.0 ** 20], "2^20"),
}
AXIS = ["+z", "-z", "+x", "-x", "+y", "-y"]
TILTED = ["tilt_a", "tilt_b"]
FAR = ["far_1e5", "far_2^20", "far_1e5_tilt", "far_2^20_tilt"]
LENGTHS = {"len_1e-25": 1e-25, "len_1e-20": 1e-20, "len_1e-15": 1e-15, "len_1e-10": 1e-10, "len_1e10": 1e10, "len_1e19": 1e19, "len_3e19": 3e19}
NORMAL_CLASSES = (["unit", "tilt30", "tilt80", "tilt90", "tilt120"] + list(LENGTHS) + ["cancel", "zero_vertex", "all_zero", "diag_int"])
# (material of _shade_inputs._materials(), behind the debug proc?): as shade_scene(), 13 is debug only and 12 is both
VARIANTS = [(m, False) for m in range(15) if m != 13] + [(12, True), (13, True)]
PLAIN_SCATTER = 0                                                   # variant 0: no texture, scatters


def _vertex_normals(name, pos):
    """(3, 3) float64 vertex normals of class `name` for the triangle `pos`"""
    e1, e2 = pos[1] - pos[0], pos[2] - pos[0]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n)
    p = e1 / np.linalg.norm(e1)
    if name == "unit":
        return np.tile(n, (3, 1))
    if name.startswith("tilt"):
        a = np.radians(float(name[4:]))
        return np.tile(np.cos(a) * n + np.sin(a) * p if name != "tilt90" else p, (3, 1))
    if name in LENGTHS:
        return np.tile(n * LENGTHS[name], (3, 1))
    if name == "cancel":                                            # a and b cancel at the middle of their edge
        return np.stack([p, -p, n])
    if name == "zero_vertex":
        return np.stack([np.zeros(3), n, n])
    if name == "all_zero":
        return np.zeros((3, 3))
    assert name == "diag_int"                                       # (a, a, 0) at every vertex, whatever the face
    return np.tile(np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), (3, 1))


def _triangle_table():
    """[(geometry, normal class, variant)]"""
    geoms = list(GEOMETRIES)
    tab = [(geoms[k % len(geoms)], "unit", k) for k in range(len(VARIANTS))]                 # every material on a plain triangle
    tab += [(g, "unit", PLAIN_SCATTER) for g in geoms]                                           # every geometry scatters
    textured = [2, 5, 11, 9]                                                                     # variants: normal map, all four, ..., plain
    for j, nc in enumerate(NORMAL_CLASSES[1:-1]):
        tab.append((AXIS[j % 6], nc, PLAIN_SCATTER))
        tab.append((TILTED[j % 2], nc, textured[j % 4]))
        tab.append((FAR[j % 4], nc, [8, len(VARIANTS) - 1][j % 2]))                              # a mirror, or the debug material
    tab += [("diag", "tilt90", PLAIN_SCATTER), ("+z", "diag_int", PLAIN_SCATTER), ("-y", "tilt90", 3), ("+z", "tilt90", PLAIN_SCATTER)]
    return tab


class StepScene:
    """hs: the HostScene.  Per triangle of _triangle_table(), in its order: slot, geometry, nclass, variant, magnitude; pos (3, 3)
    float32; n_geo (3,) float32 as the builder computed it; material / debug of the variant"""


@functools.lru_cache(maxsize=None)
def step_scene():
    from raytracing_c_amd.native import symbol_address
    from raytracing_c_amd.scene import build_scene
    src = S.shade_scene().hs                                        # its images and its background
    tab = _triangle_table()
    n = len(tab)
    pos = np.stack([GEOMETRIES[g][0] for g, _, _ in tab]).astype(F)
    nrm = np.stack([_vertex_normals(nc, GEOMETRIES[g][0]) for g, nc, _ in tab]).astype(F)
    rng = np.random.default_rng(7100)
    uv = (np.array([[0, 0], [1, 0], [0, 1]], np.float64) * rng.uniform(0.5, 3.0, (n, 1, 1)) + rng.uniform(-2, 2, (n, 1, 2))).astype(F)
    mats = S._materials()
    hs = build_scene(pos, nrm, uv, [VARIANTS[v][0] for _, _, v in tab], mats, src._image_arrays, np.eye(4, dtype=F), 0.9, src._bg_array)
    slots = hs.slot_map().copy()
    aos = hs.scene.triangles.aos
    debug_proc = symbol_address("debug_shader_proc")
    for k, (_, _, v) in enumerate(tab):
        if VARIANTS[v][1]:
            aos[int(slots[k])].shader.proc = debug_proc
    sc = StepScene()
    sc.hs, sc.table, sc.slot, sc.pos = hs, tab, slots.astype(np.int32), pos
    sc.geometry, sc.nclass = [g for g, _, _ in tab], [nc for _, nc, _ in tab]
    sc.variant = np.array([v for _, _, v in tab])
    sc.magnitude = [GEOMETRIES[g][1] for g in sc.geometry]
    sc.n_geo = np.array([[aos[int(s)].normal.x, aos[int(s)].normal.y, aos[int(s)].normal.z] for s in slots], F)
    sc.vertex_normals = nrm
    sc.materials = mats
    sc.debug = np.array([VARIANTS[v][1] for v in sc.variant])
    for k, g in enumerate(sc.geometry):                             # what the aimed directions below rely on
        if g in AXIS:
            want = np.zeros(3, F)
            want["xyz".index(g[1])] = 1.0 if g[0] == "+" else -1.0
            assert np.array_equal(sc.n_geo[k], want) and not np.any(np.signbit(sc.n_geo[k]) & (sc.n_geo[k] == 0)), (g, sc.n_geo[k])
        if g == "diag":
            assert sc.n_geo[k][0] == sc.n_geo[k][1] > 0 and sc.n_geo[k][2] == 0, sc.n_geo[k]
    return sc


def _triangles(sc, geometry=None, nclass=None, variant=None, scatter=None):
    """indices into the triangle table"""
    def one(x):
        return x if isinstance(x, (list, tuple, set)) else [x]
    keep = [k for k in range(len(sc.table))
            if (geometry is None or sc.geometry[k] in one(geometry)) and (nclass is None or sc.nclass[k] in one(nclass))
            and (variant is None or sc.variant[k] in one(variant)) and (scatter is None or (not sc.debug[k]) == scatter)]
    assert keep, (geometry, nclass, variant)
    return np.array(keep)


# ---------------------------------------------------------------------------------------------------------------------
# the items

GROUPS = ["face", "zero_geo", "zero_int", "zero_both", "chain_geo", "chain_int", "chain_both", "nan_dir", "bary", "normal_length", "origin",
          "far_t", "accounting", "carry", "below_zero"]
SPECIAL_TINT = [0.0, -0.0, 1e-40, 1e-45, 1.5, 64.0, 3e38, np.inf, 1.0, 0.25]
SPECIAL_EMISSION = [0.0, 0.0, 1e-40, 2.0, 1e30, np.inf, 0.5]
ORIGIN_KINDS = ["hit point", "point only", "free"]


def _facing(rng, sc, tri, cos_lo=0.05, cos_hi=1.0):
    """unit directions against BOTH the face and the vertex normals' mean where that can be done, else against the face"""
    n = sc.n_geo[tri].astype(np.float64)
    m = sc.vertex_normals[tri].astype(np.float64).mean(axis=1)
    ln = np.linalg.norm(m, axis=1, keepdims=True)
    m = np.where(ln > 0, m / np.where(ln > 0, ln, 1), n)
    axis = n + m
    la = np.linalg.norm(axis, axis=1, keepdims=True)
    axis = np.where(la > 0.7, axis / np.where(la > 0, la, 1), n)
    return -S._tilted(rng, axis, cos_lo, cos_hi)


@functools.lru_cache(maxsize=None)
def step_items():
    """dict of arrays over the items: tri (index into the triangle table), slot, hit (n, 3) = t, u, v; ray (n, 6) = origin,
    direction; carry (n, 6) = tint, emission; seed; last (bool: bounce_in = max_bounces - 1, else 0); group (index into GROUPS)"""
    sc = step_scene()
    rng = np.random.default_rng(7110)
    parts = []

    def add(group, tri, d, u=None, v=None, t=None, origin="hit point", seed=None):
        n = len(tri)
        u = rng.uniform(0.02, 0.96, n) * 0.5 if u is None else u
        v = rng.uniform(0.02, 0.96, n) * 0.5 if v is None else v
        t = 10.0 ** rng.uniform(-2, 1.5, n) if t is None else t
        parts.append(dict(group=np.full(n, GROUPS.index(group)), tri=np.asarray(tri), d=np.asarray(d, np.float64), u=np.asarray(u, np.float64),
                          v=np.asarray(v, np.float64), t=np.asarray(t, np.float64), origin=np.full(n, ORIGIN_KINDS.index(origin)),
                          seed=rng.integers(0, 2 ** 32, n, dtype=np.uint32) if seed is None else np.full(n, seed, np.uint32)))

    def pick(tris, n):
        return tris[rng.integers(0, len(tris), n)]

    def zero_along(d, axis_vec, zero):
        """d with its component along the axis vector replaced by the signed zero `zero`"""
        d = d.copy()
        k = np.argmax(np.abs(axis_vec), axis=1)
        d[np.arange(len(d)), k] = zero
        return d

    axis_tris = lambda nc: _triangles(sc, geometry=AXIS, nclass=nc)          # noqa: E731

    # face test: any direction against triangles whose shading normal agrees with the face, leans, or lies on its other side
    tri = pick(_triangles(sc, nclass=["unit", "tilt30", "tilt80", "tilt120"]), 4200)
    add("face", tri, S._unit(rng, len(tri)))
    # a dot that is exactly +0 or -0: the direction has a signed zero along an axis normal (the other products are zeros of
    # the other components' signs; the sum is -0 only when all three are)
    for group, nc, n in (("zero_both", "unit", 700), ("zero_geo", ["tilt30", "tilt80", "tilt120"], 900)):
        tri = pick(axis_tris(nc), n)
        d = S._unit(rng, n)
        d[: n // 3] = -np.abs(d[: n // 3])                                     # every component negative: with -0, the dot is -0 on a + face
        d[n // 3: 2 * n // 3] = np.abs(d[n // 3: 2 * n // 3])
        add(group, tri, zero_along(d, sc.n_geo[tri], rng.choice([0.0, -0.0], n)))
    tri = pick(axis_tris("tilt90"), 500)                                       # the shading normal is an axis in the face: zero along IT,
    d = zero_along(_facing(rng, sc, tri), sc.vertex_normals[tri][:, 0], rng.choice([0.0, -0.0], 500))      # against the face
    add("zero_int", tri, d)
    # a dot whose chain is not zero where its value is: normal (a, a, 0), direction (b, -b, z) -- a * b is rounded, the fused
    # second product returns the rounding error alone
    for group, tris, zsign, n in (("chain_both", _triangles(sc, geometry="diag", nclass="unit"), 0.0, 400),
                                  ("chain_geo", _triangles(sc, geometry="diag", nclass="tilt90"), -1.0, 400),      # n_int = +z: dz < 0 faces it
                                  ("chain_int", _triangles(sc, geometry="+z", nclass="diag_int"), -1.0, 400)):
        b = rng.uniform(0.1, 0.7, n) * rng.choice([-1.0, 1.0], n)
        add(group, pick(tris, n), np.stack([b, -b, zsign * rng.uniform(0.1, 0.7, n)], axis=1))
    # a NaN dot
    tri = pick(np.arange(len(sc.table)), 160)
    d = _facing(rng, sc, tri)
    d[np.arange(160), rng.integers(0, 3, 160)] = np.nan
    add("nan_dir", tri, d)
    # barycentrics: corners, edges, and what the leaf test still accepts outside the triangle
    tri = np.tile(np.arange(len(sc.table)), 36)
    n = len(tri)
    kind = np.repeat(np.arange(9), n // 9 + 1)[:n]
    r = rng.uniform(0.0, 1.0, n)
    eps = rng.uniform(0.0, 1.0, n) * float(RT_EPS) * 0.999
    u = np.choose(kind, [0 * r, 1 + 0 * r, 0 * r, r, 0 * r, r, -eps - 1e-12, r * 0.9, r])
    v = np.choose(kind, [0 * r, 0 * r, 1 + 0 * r, 0 * r, r, 1 - r, r * 0.9, -eps - 1e-12, 1 - r + eps + 1e-9])
    add("bary", tri, _facing(rng, sc, tri), u=u, v=v)
    # the length of the interpolated normal: zero at the cancelling edge's middle and at the zero corner, everything between
    tri = pick(_triangles(sc, nclass=list(LENGTHS) + ["all_zero"]), 1500)
    add("normal_length", tri, _facing(rng, sc, tri))
    tri = pick(_triangles(sc, nclass="cancel"), 150)
    add("normal_length", tri, _facing(rng, sc, tri), u=np.full(150, 0.5), v=np.zeros(150))
    tri = pick(_triangles(sc, nclass="zero_vertex"), 150)
    add("normal_length", tri, _facing(rng, sc, tri), u=np.zeros(150), v=np.zeros(150))
    # the next origin at |point| about 1, 1e5 and 2^20, on materials that scatter and shading normals that lean (the outgoing
    # direction then goes below the face as well as above it)
    tri = pick(_triangles(sc, nclass=["unit", "tilt30", "tilt80", "len_1e10"], scatter=True), 2400)
    add("origin", tri, _facing(rng, sc, tri), origin="point only", t=np.zeros(len(tri)))
    tri = pick(_triangles(sc, nclass=["unit", "tilt30", "tilt80"]), 900)
    add("origin", tri, S._unit(rng, 900))
    # distances up to 1e30, directions that are not unit vectors: the point overflows
    tri = pick(_triangles(sc, nclass=["unit", "tilt30"]), 400)
    sure = (np.arange(400) >= 200)[:, None]                                    # the second half overflows for certain
    d = _facing(rng, sc, tri) * (10.0 ** np.where(sure, rng.uniform(10, 12, (400, 1)), rng.uniform(0, 12, (400, 1))))
    add("far_t", tri, d, t=10.0 ** np.where(sure[:, 0], rng.uniform(29, 30, 400), rng.uniform(20, 30, 400)), origin="free")
    # accounting: every material on both faces (`last` is dealt out below)
    tri = pick(_triangles(sc, nclass=["unit", "tilt30", "tilt80"]), 2600)
    d = _facing(rng, sc, tri, 0.0005, 1.0)
    back = rng.random(len(tri)) < 0.3
    d[back] = -d[back]
    add("accounting", tri, d)
    # carried values
    tri = pick(_triangles(sc, nclass=["unit", "tilt30"]), 1000)
    d = _facing(rng, sc, tri)
    back = rng.random(len(tri)) < 0.25
    d[back] = -d[back]
    add("carry", tri, d)
    # dot(n_geo, outgoing direction) exactly 0: face +z, shading normal +x, direction (-, y, -0): the tangent is +-z, the
    # bitangent +-y; the diffuse lobe's angle is the 4th draw, and with 0 there the sample has no tangent component
    tri = pick(_triangles(sc, geometry="+z", nclass="tilt90"), 96)
    d = S._unit(rng, 96)
    d[:, 0] = -np.abs(d[:, 0]) - 0.1
    d[:, 2] = -0.0
    add("below_zero", tri, d, seed=seed_for_zero_draw(4))

    it = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    n = len(it["tri"])
    tri, t = it["tri"], it["t"]
    P = sc.pos[tri].astype(np.float64)
    point = P[:, 0] + it["u"][:, None] * (P[:, 1] - P[:, 0]) + it["v"][:, None] * (P[:, 2] - P[:, 0])
    d32 = it["d"].astype(F)
    with np.errstate(all="ignore"):
        org = np.where((it["origin"] == 0)[:, None], point - np.nan_to_num(it["d"]) * t[:, None], point)
    free = it["origin"] == 2
    org[free] = rng.uniform(-3, 3, (int(free.sum()), 3))
    hit = np.stack([t, it["u"], it["v"]], axis=1).astype(F)
    ray = np.concatenate([org.astype(F), d32], axis=1)
    # carry: tint in [0, 1.5), emission zero for half the items; the carry group draws from the special values
    tint = rng.uniform(0.0, 1.5, (n, 3)).astype(F)
    tint[rng.random(n) < 0.2] = 1.0
    emis = (rng.uniform(0.0, 2.0, (n, 3)) * (rng.random((n, 1)) < 0.5)).astype(F)
    k = np.flatnonzero(it["group"] == GROUPS.index("carry"))
    sp = rng.random((len(k), 3)) < 0.6
    tint[k] = np.where(sp, rng.choice(np.array(SPECIAL_TINT, F), (len(k), 3)), tint[k])
    emis[k] = np.where(sp[:, ::-1], rng.choice(np.array(SPECIAL_EMISSION, F), (len(k), 3)), emis[k])
    seed = it["seed"].copy()
    seed[::991] = 0
    seed[it["group"] == GROUPS.index("below_zero")] = seed_for_zero_draw(4)
    out = dict(tri=tri.astype(np.int32), slot=sc.slot[tri], hit=np.ascontiguousarray(hit), ray=np.ascontiguousarray(ray),
               carry=np.ascontiguousarray(np.concatenate([tint, emis], axis=1)), seed=seed, last=rng.random(n) < 0.5,
               group=it["group"].astype(np.int32))
    assert 10000 <= n <= 20000, n
    for a in out.values():
        a.setflags(write=False)
    return out


def bounce_in(max_bounces):
    return np.where(step_items()["last"], max_bounces - 1, 0).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's answers

@functools.lru_cache(maxsize=None)
def filled_hits():
    """oracle_fill_hit of every item: a HIT_DTYPE array"""
    from tests import _oracle
    orc = _oracle.load()
    sc, it = step_scene(), step_items()
    n = len(it["slot"])
    hits = np.zeros(n, abi.HIT_DTYPE)
    chits = (abi.Hit * n).from_buffer(hits)
    rays = (abi.Ray * n).from_buffer_copy(it["ray"])
    scene = C.byref(sc.hs.scene)
    hit = it["hit"]
    for i in range(n):
        orc.oracle_fill_hit(scene, C.byref(rays[i]), float(hit[i, 0]), int(it["slot"][i]), float(hit[i, 1]), float(hit[i, 2]), C.byref(chits[i]))
    del chits
    hits.setflags(write=False)
    return hits


@functools.lru_cache(maxsize=None)
def step_reference(max_bounces):
    """oracle_path_step of every item: out (n, 15) = origin, direction, tint, emission, radiance; words (n, 5) = rng, bounce, done,
    shades, textured -- the layout of rt_test_shade_hit"""
    from tests import _oracle
    orc = _oracle.load()
    sc, it, hits = step_scene(), step_items(), filled_hits()
    n = len(it["slot"])
    chits = (abi.Hit * n).from_buffer_copy(hits)
    out = np.zeros((n, 15), F)
    out[:, 0:6], out[:, 6:12], out[:, 12:15] = it["ray"], it["carry"], RADIANCE_UNSET
    words = np.zeros((n, 5), np.uint32)
    cfg = _oracle.config_for(sc.hs, n_threads=1)
    scene, pcfg = C.byref(sc.hs.scene), C.byref(cfg)
    b_in = bounce_in(max_bounces)
    state, bounce, done = C.c_uint32(), C.c_int32(), C.c_int32()
    cnt = np.zeros(2, np.uint64)
    p0 = out.ctypes.data
    for i in range(n):
        state.value, bounce.value, done.value = int(it["seed"][i]), int(b_in[i]), -1
        row = p0 + i * 60
        orc.oracle_path_step(scene, pcfg, C.cast(C.c_void_p(row), C.POINTER(abi.Ray)), C.byref(chits[i]), row + 24, row + 36, C.byref(state),
                             C.byref(bounce), max_bounces, C.byref(done), row + 48, cnt.ctypes.data)
        words[i] = (state.value, bounce.value & _M32, done.value, int(cnt[0]), int(cnt[1]))
    out.setflags(write=False)
    words.setflags(write=False)
    return dict(out=out, words=words)


@functools.lru_cache(maxsize=None)
def shader_inputs():
    """What the step hands to shade() for every item: (n, 20) float32 in Shader_Input's layout, from the filled hit; the normal is
    rt_v3_normalize(hit.normal) = v * (1 / sqrt(v . v)) through the oracle's own square root and quotient"""
    from tests import _oracle
    it, hits = step_items(), filled_hits()
    nn = dot32(hits["normal"], hits["normal"])
    inv = _oracle.math(10, _oracle.math(9, nn))
    with np.errstate(all="ignore"):
        normal = hits["normal"] * inv[:, None]
    sin = np.concatenate([it["ray"][:, 3:6], normal, hits["normal_geo"], hits["tangent"], hits["bitangent"], hits["point"], hits["tex_coords"]],
                         axis=1).astype(F)
    return dict(sin=np.ascontiguousarray(sin), nn=nn)


@functools.lru_cache(maxsize=None)
def feature_reference():
    """out (n, 12) = origin afterwards, albedo, normal, position; flag (n,): the layout of rt_test_feature_hit.  Flag and origin
    are the path step's (a step that shaded is a feature hit), position is the filled hit's point, normal the debug proc's
    emission on the step's shader input, albedo tests/_features.albedo_of."""
    from tests import _features, _oracle
    orc = _oracle.load()
    it, hits, ref = step_items(), filled_hits(), step_reference(MAX_BOUNCES[1])
    sin = shader_inputs()["sin"]
    n = len(it["slot"])
    flag = (ref["words"][:, 3] != 0).astype(np.int32)
    out = np.zeros((n, 12), F)
    out[:, 0:3] = np.where(flag[:, None] != 0, it["ray"][:, 0:3], ref["out"][:, 0:3])
    ins = (abi.Shader_Input * n).from_buffer_copy(sin)
    so = abi.Shader_Output()
    for i in np.flatnonzero(flag):
        data = int(hits["shader_data"][i])
        orc.oracle_debug_shade(C.cast(data, C.POINTER(abi.PBR_Shader_Data)), C.byref(ins[i]), C.byref(so))
        out[i, 6:9] = (so.emission.x, so.emission.y, so.emission.z)
        out[i, 3:6] = _features.albedo_of(orc, data, hits["tex_coords"][i])[0]
        out[i, 9:12] = hits["point"][i]
    out.setflags(write=False)
    return dict(out=out, flag=flag)


# ---------------------------------------------------------------------------------------------------------------------
# classes: what the oracle did with the items, not what the generator meant

@functools.lru_cache(maxsize=None)
def _draws(max_bounces):
    from tests import _oracle
    return S.draws_after(_oracle.load(), step_items()["seed"], step_reference(max_bounces)["words"][:, 0])


@functools.lru_cache(maxsize=None)
def step_classes(max_bounces):
    """class name -> boolean mask over the items, from the filled hits, exact float32 dots of them, and oracle_path_step's outputs"""
    sc, it, hits, ref = step_scene(), step_items(), filled_hits(), step_reference(max_bounces)
    out, words = ref["out"], ref["words"]
    d = it["ray"][:, 3:6]
    geo, nint = dot32(hits["normal_geo"], d), dot32(hits["normal"], d)
    with np.errstate(all="ignore"):
        geo64 = np.sum(hits["normal_geo"].astype(np.float64) * d.astype(np.float64), axis=1)
        int64 = np.sum(hits["normal"].astype(np.float64) * d.astype(np.float64), axis=1)
        agree = np.sum(hits["normal"].astype(np.float64) * hits["normal_geo"].astype(np.float64), axis=1)
    shaded = words[:, 3] == 1
    passed = ~shaded
    done = words[:, 2] == 1
    moved_dir = ~np.all(same_bits(out[:, 3:6], d), axis=1)
    scattered = shaded & (words[:, 1].astype(np.int32) == bounce_in(max_bounces) + 1)
    terminated = shaded & ~scattered
    debug = sc.debug[it["tri"]]
    draws = _draws(max_bounces)
    last = it["last"] | (max_bounces == 1)
    u, v = it["hit"][:, 1].astype(np.float64), it["hit"][:, 2].astype(np.float64)
    nn = shader_inputs()["nn"]
    point, org = hits["point"], out[:, 0:3]
    with np.errstate(all="ignore"):
        pmag = np.max(np.abs(point), axis=1)
        below = dot32(hits["normal_geo"], out[:, 3:6])
        stuck = np.all(org == point, axis=1)                           # RT_EPS was below half an ulp on every axis
    tint, emis = it["carry"][:, 0:3], it["carry"][:, 3:6]
    zero = lambda x, neg: (x == 0) & (np.signbit(x) == neg)             # noqa: E731
    fin = np.isfinite
    cls = {
        "face: both dots negative": shaded & (geo < 0) & (nint < 0),
        "face: only n_geo positive": passed & (geo > 0) & ~(nint > 0),
        "face: only n_int positive": passed & ~(geo > 0) & (nint > 0),
        "face: both positive": passed & (geo > 0) & (nint > 0),
        "face: n_geo dot +0, shaded": shaded & zero(geo, False), "face: n_geo dot -0, shaded": shaded & zero(geo, True),
        "face: n_int dot +0, shaded": shaded & zero(nint, False), "face: n_int dot -0, shaded": shaded & zero(nint, True),
        "face: n_geo chain > 0 where the float64 dot is 0, passed": passed & (geo > 0) & (geo64 == 0) & ~(nint > 0),
        "face: n_geo chain < 0 where the float64 dot is 0, shaded": shaded & (geo < 0) & (geo64 == 0),
        "face: n_int chain > 0 where the float64 dot is 0, passed": passed & (nint > 0) & (int64 == 0) & ~(geo > 0),
        "face: n_int chain < 0 where the float64 dot is 0, shaded": shaded & (nint < 0) & (int64 == 0),
        "face: NaN dot, shaded": shaded & np.isnan(geo) & np.isnan(nint),
        "face: shading normal on the other side of the face": (agree < 0) & fin(geo) & fin(nint),
        "bary: corner": ((u == 0) & (v == 0)) | ((u == 1) & (v == 0)) | ((u == 0) & (v == 1)),
        "bary: edge": ((u == 0) ^ (v == 0)) & (u + v < 1) | ((u + v == 1) & (u > 0) & (v > 0)),
        "bary: u or v in [-RT_EPS, 0)": ((u < 0) & (u >= -float(RT_EPS))) | ((v < 0) & (v >= -float(RT_EPS))),
        "bary: u + v in (1, 1 + RT_EPS]": (it["hit"][:, 1] + it["hit"][:, 2] > 1) & (it["hit"][:, 1] + it["hit"][:, 2] <= F(1) + RT_EPS),
        "normal: dot(n_int, n_int) exactly 0, shaded": shaded & (nn == 0),
        "normal: dot(n_int, n_int) below 2^-96, shaded": shaded & (nn > 0) & (nn < 2.0 ** -96) & (nn >= 2.0 ** -126),
        "normal: dot(n_int, n_int) denormal, shaded": shaded & (nn > 0) & (nn < 2.0 ** -126),
        "normal: dot(n_int, n_int) infinite, shaded": shaded & np.isinf(nn),
        "normal: NaN shading normal, shaded": shaded & np.any(np.isnan(shader_inputs()["sin"][:, 3:6]), axis=1),
        "origin: |point| about 1, scattered": scattered & (pmag < 64),
        "origin: |point| about 1e5, scattered": scattered & (pmag > 5e4) & (pmag < 2e5),
        "origin: |point| about 2^20, scattered": scattered & (pmag > 2.0 ** 19) & (pmag < 2.0 ** 21),
        "origin: |point| about 1e5, passed": passed & (pmag > 5e4) & (pmag < 2e5),
        "origin: |point| about 2^20, passed": passed & (pmag > 2.0 ** 19) & (pmag < 2.0 ** 21),
        "origin: the bias is below half an ulp, origin = point": (scattered | passed) & stuck & fin(pmag),
        "origin: infinite point": ~np.all(fin(point), axis=1) & np.all(fin(it["ray"]), axis=1),
        "origin: next direction above the face": scattered & (below > 0),
        "origin: next direction below the face": scattered & (below < 0),
        "origin: dot(n_geo, next direction) exactly 0": scattered & (below == 0),
        "origin: bias along a shading normal that is not the face's": scattered & ~np.all(same_bits(shader_inputs()["sin"][:, 3:6], hits["normal_geo"]), axis=1)
                                                                     & np.all(fin(shader_inputs()["sin"][:, 3:6]), axis=1),
        "accounting: first bounce, back face": passed & ~last, "accounting: last bounce, back face": passed & last,
        "accounting: first bounce, scatter": scattered & ~last, "accounting: last bounce, scatter": scattered & last,
        "accounting: first bounce, debug material": terminated & debug & ~last, "accounting: last bounce, debug material": terminated & debug & last,
        "accounting: first bounce, diffuse lobe ends the path": terminated & ~debug & (draws == 5) & ~last,
        "accounting: last bounce, diffuse lobe ends the path": terminated & ~debug & (draws == 5) & last,
        "accounting: first bounce, specular lobe ends the path": terminated & ~debug & (draws == 3) & ~last,
        "accounting: last bounce, specular lobe ends the path": terminated & ~debug & (draws == 3) & last,
        "accounting: the path goes on": ~done,
        "accounting: emission gathered at a terminating hit": terminated & ~np.all(same_bits(out[:, 9:12], emis), axis=1),
        "carry: a tint component 0": np.any(tint == 0, axis=1), "carry: a tint component denormal": np.any((tint > 0) & (tint < 2.0 ** -126), axis=1),
        "carry: a tint component above 1": np.any((tint > 1) & fin(tint), axis=1), "carry: a tint component infinite": np.any(np.isinf(tint), axis=1),
        "carry: emission 0": np.all(emis == 0, axis=1), "carry: emission not 0": np.any(emis != 0, axis=1),
        "carry: infinity x 0 in tint x shader tint or emission x tint": shaded & np.any(np.isinf(it["carry"]), axis=1)
                                                                       & (np.any(np.isnan(out[:, 6:12]), axis=1)),
        "carry: tint not (1, 1, 1), scattered": scattered & ~np.all(tint == 1, axis=1),
        "direction unchanged by a back face": passed & ~moved_dir,
    }
    if max_bounces == 1:
        cls = {k: m for k, m in cls.items() if "first bounce" not in k and k != "accounting: the path goes on"}
    return cls


# classes that must hold at least this many items (every other class: 32)
CLASS_MINIMUM = {"origin: next direction below the face": 100, "face: only n_geo positive": 100, "face: only n_int positive": 100}
DEFAULT_MINIMUM = 32


def describe_step_item(i, max_bounces=MAX_BOUNCES[1]):
    sc, it, hits = step_scene(), step_items(), filled_hits()
    k = int(it["tri"][i])
    names = [name for name, m in step_classes(max_bounces).items() if m[i]]
    m, dbg = VARIANTS[sc.variant[k]]
    return (f"item {i}: group {GROUPS[it['group'][i]]}, classes {names}\n"
            f"  triangle {k} (slot {it['slot'][i]}): geometry {sc.geometry[k]}, vertex normals {sc.nclass[k]}, material {m} (debug={dbg}) = {sc.materials[m]}\n"
            f"  hit (t, u, v) {it['hit'][i].tolist()}, origin {it['ray'][i, 0:3].tolist()}, direction {it['ray'][i, 3:6].tolist()}\n"
            f"  tint {it['carry'][i, 0:3].tolist()}, emission {it['carry'][i, 3:6].tolist()}, seed {it['seed'][i]:#x}, "
            f"bounce_in {int(bounce_in(max_bounces)[i])} of {max_bounces}\n"
            f"  filled hit: point {hits['point'][i].tolist()}, n_geo {hits['normal_geo'][i].tolist()}, n_int {hits['normal'][i].tolist()}")
