"""Helpers of tests/test_reference_pin.py, tests/test_gpu_reference_pin.py and tools/make_reference_pin_fixtures.py: ctypes
access to oracle/_ref/libref.so (the reference's OWN hot-path sources compiled against the codin stand-in, oracle/Makefile
target `ref`), scenes that libref.so and liboracle_v1.so can share in memory, seeded rays with the hard cases, and the
conditions that keep a comparison from being blind.  TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C
import os

import numpy as np

from raytracing_c_amd import ctypes_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
REFERENCE_DIR = os.environ.get("RT_REFERENCE_DIR", "/root/reference")
LIBREF = os.path.join(ROOT, "oracle", "_ref", "libref.so")
LIBORACLE_V1 = os.path.join(ROOT, "oracle", "liboracle_v1.so")
FIXTURE_DIR = os.path.join(ROOT, "tests", "golden", "ref")
F = np.float32
EPSILON = F(0.0001)
SKIP_REASON = "the reference tree is not on this machine, so there is no oracle/_ref/libref.so to compare with"

_ref = None


def reference_state():
    """'ready' (libref.so is built), 'unbuilt' (the reference tree is here but libref.so is not: a FAILURE) or 'absent'."""
    if os.path.exists(LIBREF):
        return "ready"
    return "unbuilt" if os.path.isdir(REFERENCE_DIR) else "absent"


def load_ref():
    global _ref
    if _ref is not None:
        return _ref
    d = C.CDLL(LIBREF)
    P, vp, f, i32 = C.POINTER, C.c_void_p, C.c_float, C.c_int32
    d.ref_last_panic.restype = C.c_char_p
    d.ref_min_f32x8.argtypes = [vp, f, P(i32)]
    d.ref_min_f32x8.restype = f
    d.ref_ray_aabbs_hit_8.argtypes = [P(abi.Ray), f, f, vp, vp]
    d.ref_ray_aabbs_hit_8.restype = None
    d.ref_ray_triangles_hit_8.argtypes = [P(abi.Ray), P(abi.Triangles), abi.isize, P(abi.Hit)]
    d.ref_ray_scene_hit.argtypes = [P(abi.Ray), P(abi.Scene), P(abi.Hit)]
    d.ref_trace_rays.argtypes = [P(abi.Scene), i32, vp, vp, vp, vp]
    d.ref_rand_f32_seq.argtypes = [C.c_uint32, i32, vp]
    d.ref_rand_f32_seq.restype = None
    d.ref_cast_ray.argtypes = [P(abi.Scene), P(abi.Ray), abi.isize, P(C.c_uint32), vp]
    d.ref_hash12x8.argtypes = [vp, vp, vp]
    d.ref_hash12x8.restype = None
    d.ref_encode_u8.argtypes = [f]
    d.ref_encode_u8.restype = C.c_uint8
    d.ref_render.argtypes = [P(abi.Scene), P(abi.Image), abi.isize, abi.isize, C.c_uint32]
    d.ref_lightmap_bake.argtypes = [P(abi.Image), P(abi.Scene), abi.isize, C.c_uint32]
    d.ref_denoise_image.argtypes = [P(abi.Image), P(abi.Image)]
    d.ref_scene_init.argtypes = [P(abi.Scene), vp, abi.isize]
    d.ref_scene_free.argtypes = [P(abi.Scene)]
    d.ref_scene_free.restype = None
    d.ref_sample_texture_bilinear.argtypes = [P(abi.Image), f, f, vp]
    d.ref_sample_texture_bilinear.restype = None
    d.ref_sample_background.argtypes = [P(abi.Image), vp, vp]
    d.ref_sample_background.restype = None
    d.ref_proc_address.argtypes = [i32]
    d.ref_proc_address.restype = vp
    d.ref_sample_disney_brdf.argtypes = [f] * 5 + [vp, vp, P(C.c_uint32), vp, vp]
    d.ref_sample_disney_brdf.restype = None
    d.ref_shade.argtypes = [i32, P(abi.PBR_Shader_Data), P(abi.Shader_Input), P(C.c_uint32), P(abi.Shader_Output)]
    d.ref_shade.restype = None
    _ref = d
    return d


def load_oracle_v1():
    from tests import _oracle
    d = _oracle.load(LIBORACLE_V1)
    P = C.POINTER
    d.oracle_set_literal.argtypes = [C.c_int]
    d.oracle_set_literal.restype = C.c_int
    d.oracle_cast_ray.argtypes = [P(abi.Scene), P(_oracle.Oracle_Config), P(abi.Ray), abi.isize, P(C.c_uint32), C.c_void_p]
    d.oracle_cast_ray.restype = None
    d.oracle_debug_shade.argtypes = [P(abi.PBR_Shader_Data), P(abi.Shader_Input), P(abi.Shader_Output)]
    d.oracle_debug_shade.restype = None
    return d


def bits(a):
    """raw uint32 view of an fp32 array: what every comparison here is made on"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def plus_zero(a):
    """-0.0 -> +0.0, everything else bit for bit (ref_trace_rays reads u and v out of a sum that loses the sign of a zero)"""
    a = np.array(a, np.float32)
    a[a == 0] = 0.0
    return a


# ---- scenes -----------------------------------------------------------------------------------------------------------

def soup_data(seed, n_tris):
    """Random triangle soup with exact duplicates (equal `t`, equal sort keys), a degenerate triangle and axis-aligned
    triangles through the origin; one material without textures."""
    from raytracing_c_amd.scene import Material
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n_tris, 1, 3))
    P = (c + rng.normal(size=(n_tris, 3, 3)) * rng.choice([0.05, 0.3, 0.8], (n_tris, 1, 1))).astype(F)
    if n_tris >= 8:
        k = max(2, n_tris // 10)
        P[-k:] = P[:k]
        P[k] = P[k][[0, 0, 0]]
    if n_tris > 12:
        P[k + 1] = [[0, -1, -1], [0, 1, -1], [0, 1, 1]]
        P[k + 2] = [[-1, 0, -1], [1, 0, -1], [1, 0, 1]]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    fn = np.cross(e1, e2)
    fn = fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    N = (fn[:, None, :] + rng.normal(size=(n_tris, 3, 3)) * 0.2).astype(F)
    UV = rng.uniform(-1.5, 2.5, (n_tris, 3, 2)).astype(F)
    mats = [Material(base_color=(0.7, 0.6, 0.5), roughness=0.4, metalness=0.3, sheen=0.5, sheen_tint=0.5),
            Material(base_color=(0.9, 0.2, 0.2), emission=(2.0, 1.0, 0.5), roughness=0.9)]
    return dict(positions=P, normals=N, uvs=UV, material_ids=(np.arange(n_tris) % 2).astype(np.int32), materials=mats,
                images=[], camera=None)


def model_data(name):
    """'quad' | 'spheres' | 'tower' (the small assets) or 'soup<N>' (seeded by N)."""
    from raytracing_c_amd.configs import CONFIGS
    from raytracing_c_amd.loaders import default_camera, load_model_data, camera_from_trs
    if name.startswith("soup"):
        n = int(name[4:])
        d = soup_data(1000 + n, n)
        d["camera"] = (camera_from_trs((0, 0, 4)), 1.0)
        return d
    asset, _w, _h, _s, _b, cam = CONFIGS[name]
    d = load_model_data(os.path.join(ASSETS, asset))
    d["camera"] = cam or d["camera"] or default_camera()
    return d


class PinScene:
    """One set of triangles, built by the library's scene_init (`hs`, always) and by the reference's (`rs`, or None with
    `panic` = the assertion of the reference that stopped it).  Both Scenes carry libref.so's procs as material tokens, so
    libref.so CALLS them and the oracle recognises them by address (oracle_config)."""

    def __init__(self, name, ref=None, data=None):
        from raytracing_c_amd.background import procedural_background
        from raytracing_c_amd.scene import build_scene
        import raytracing_c_amd as rt
        self.name = name
        d = self.data = data or model_data(name)
        self.ref = ref
        n = len(d["positions"])
        self.hs = build_scene(d["positions"], d["normals"], d["uvs"], d["material_ids"], d["materials"], d["images"],
                              d["camera"][0], d["camera"][1], procedural_background(64, 32))
        self.tokens = (rt.native.symbol_address("disney_shader_proc"), rt.native.symbol_address("debug_shader_proc"),
                       rt.native.symbol_address("sample_background"))
        self.tri = np.zeros(n, abi.TRIANGLE_DTYPE)
        self.tri["positions"] = np.ascontiguousarray(d["positions"], F)
        self.tri["normals"] = np.ascontiguousarray(d["normals"], F).reshape(n, 3, 3)
        self.tri["tex_coords"] = np.ascontiguousarray(d["uvs"], F).reshape(n, 3, 2)
        self.tri["shader_data"] = C.addressof(self.hs.materials) + np.asarray(d["material_ids"]).astype(np.uint64) * 80
        self.tri["shader_proc"] = self.tokens[0]
        self.rs, self.panic = None, None
        if ref is not None:
            self.tokens = tuple(ref.ref_proc_address(k) for k in range(3))
            self.tri["shader_proc"] = self.tokens[0]
            aos = np.ctypeslib.as_array(C.cast(self.hs.scene.triangles.aos, C.POINTER(C.c_uint64)), (self.hs.n_slots, 14))
            aos[:, 13][aos[:, 13] != 0] = self.tokens[0]
            self.hs.scene.background.proc = self.tokens[2]
            rs = abi.Scene()
            rs.camera, rs.background = self.hs.scene.camera, self.hs.scene.background
            rc = ref.ref_scene_init(C.byref(rs), self.tri.ctypes.data, n)
            if rc == 0:
                self.rs = rs
            else:
                self.panic = ref.ref_last_panic().decode()

    def use_debug_shader(self):
        for sc in (self.hs.scene, self.rs):
            if sc is not None:
                aos = np.ctypeslib.as_array(C.cast(sc.triangles.aos, C.POINTER(C.c_uint64)), (int(sc.triangles.len), 14))
                aos[:, 13][aos[:, 13] != 0] = self.tokens[1]

    def oracle_config(self, seed=0, literal=True):
        from tests import _oracle
        cfg = _oracle.Oracle_Config()
        cfg.disney_proc, cfg.debug_proc, cfg.background_proc = self.tokens
        cfg.seed, cfg.n_threads, cfg.literal = seed, 1, 1 if literal else 0
        return cfg

    def free(self):
        if self.rs is not None:
            self.ref.ref_scene_free(C.byref(self.rs))
            self.rs = None
        if self.ref is not None:                 # give the library its own tokens back before it releases the scene
            self.hs.scene.background.proc = 0
        self.hs.free()


def scene_bytes(scene, materials_base):
    """(depth, last_row_offset, n_nodes, slots), node bytes (n, 48) u32, triangle block (slots, 9 + 24) u32 with the Shader
    of every record replaced by (material index or -1, proc != 0): the Shader holds host pointers."""
    n_nodes = int(scene.bvh.nodes.len)
    nodes = np.zeros((0, 48), np.uint32)
    if n_nodes:
        nodes = np.ctypeslib.as_array(C.cast(scene.bvh.nodes.data, C.POINTER(C.c_uint32)), (n_nodes, 48)).copy()
    n = int(scene.triangles.len)
    soa = np.ctypeslib.as_array(C.cast(scene.triangles.x[0], C.POINTER(C.c_uint32)), (9, n)).copy()
    aos = np.ctypeslib.as_array(C.cast(scene.triangles.aos, C.POINTER(C.c_uint32)), (n, 28)).copy()
    ptr = aos[:, 24:28].copy().view(np.uint64)
    mat = np.where(ptr[:, 0] != 0, (ptr[:, 0].astype(np.int64) - materials_base) // 80, -1).astype(np.int32)
    has_proc = (ptr[:, 1] != 0)
    head = (int(scene.bvh.depth), int(scene.bvh.last_row_offset), n_nodes, n)
    return head, nodes, soa, aos[:, :24].copy(), mat, has_proc


# ---- rays -------------------------------------------------------------------------------------------------------------

def seeded_rays(scene, n, seed):
    """n rays (n, 6) against the populated part of a Scene: rays aimed at points of triangles from outside and from inside
    the scene, rays along the axes (zero direction components, infinite reciprocals), rays that start ON a box plane,
    rays that start on a triangle (t = 0 < EPSILON), rays in a triangle's plane, rays through a triangle's edge and
    vertex, and directions with an infinite or NaN component."""
    rng = np.random.default_rng(seed)
    slots = int(scene.triangles.len)
    soa = np.ctypeslib.as_array(scene.triangles.x[0], (9, slots))
    P = soa.reshape(3, 3, slots).transpose(2, 1, 0)              # (slot, vertex, xyz)
    used = np.flatnonzero(np.any(P.reshape(slots, 9) != 0, axis=1))
    assert len(used) > 0
    lo, hi = P[used].reshape(-1, 3).min(0), P[used].reshape(-1, 3).max(0)
    ext = np.maximum(hi - lo, 1e-3)
    pick = rng.choice(used, n)
    w = rng.dirichlet((1, 1, 1), n).astype(F)
    kind = rng.integers(0, 12, n)
    w[kind == 8] = [0.5, 0.5, 0.0]                                # through an edge
    w[kind == 9] = [1.0, 0.0, 0.0]                                # through a vertex
    target = np.einsum("nk,nkc->nc", w, P[pick]).astype(F)
    origin = (lo + ext * rng.uniform(-1.5, 2.5, (n, 3))).astype(F)
    inside = kind == 1
    origin[inside] = (lo + ext * rng.uniform(0, 1, (n, 3)))[inside].astype(F)
    direction = target - origin
    direction /= np.maximum(np.linalg.norm(direction, axis=1, keepdims=True), 1e-20)
    direction = direction.astype(F)
    ax = kind == 2                                                # axis-parallel: two zero components
    direction[ax] = np.eye(3, dtype=F)[rng.integers(0, 3, n)][ax] * rng.choice([-1, 1], (n, 1))[ax]
    origin[ax] = (target - direction * F(3.0))[ax]
    onp = kind == 3                                               # the origin lies on a plane of the scene's bounding box
    a = rng.integers(0, 3, n)
    origin[onp, a[onp]] = np.where(rng.integers(0, 2, n) == 0, lo[a], hi[a])[onp]
    direction[onp] = (target - origin)[onp]
    ont = kind == 4                                               # starts on the triangle itself
    origin[ont] = target[ont]
    direction[ont] = rng.normal(size=(n, 3)).astype(F)[ont]
    inp = kind == 5                                               # lies in the triangle's plane: det ~ 0
    origin[inp] = (P[pick][:, 0] + (P[pick][:, 0] - P[pick][:, 1]) * F(2.0))[inp]
    direction[inp] = (target - origin)[inp]
    direction[kind == 6, 0] = np.inf
    direction[kind == 7, 1] = np.nan
    return np.ascontiguousarray(np.concatenate([origin, direction], axis=1), F)


# ---- recorded results (tests/golden/ref/*.npz, tools/make_reference_pin_fixtures.py) --------------------------------------

def fixture_triangles(g, materials_base, proc):
    """the input Triangle[] of a fixture, with shader = (materials_base + 80 * material, proc)"""
    n = len(g["triangles"])
    tri = np.zeros(n, abi.TRIANGLE_DTYPE)
    tri.view(np.uint8).reshape(n, 112)[:, :96] = np.ascontiguousarray(g["triangles"]).view(np.uint8).reshape(n, 96)
    tri["shader_data"] = materials_base + g["material"].astype(np.uint64) * 80
    tri["shader_proc"] = proc
    return tri


def expand_fixture(g):
    """(head, nodes (n, 48), coordinates (9, slots), records (slots, 24), material (slots,), populated (slots,)) of the BUILT
    scene a fixture records: the same tuple scene_bytes() returns for a Scene in memory."""
    depth, last_row, n_nodes, slots = (int(v) for v in g["head"])
    nodes = np.zeros((n_nodes, 48), np.uint32)
    nodes[g["node_rows"]] = g["node_bits"]
    words = np.ascontiguousarray(g["triangles"])[g["slot_input"]]             # (populated, 24): positions, normals, tex_coords
    soa = np.zeros((9, slots), np.uint32)
    soa[:, g["slot_index"]] = words[:, :9].reshape(-1, 3, 3).transpose(2, 1, 0).reshape(9, -1)
    aos = np.zeros((slots, 24), np.uint32)
    aos[g["slot_index"], 0:3] = g["frames"][:, 0:3]
    aos[g["slot_index"], 3:12] = words[:, 9:18]
    aos[g["slot_index"], 12:18] = g["frames"][:, 3:9]
    aos[g["slot_index"], 18:24] = words[:, 18:24]
    mat = np.full(slots, -1, np.int32)
    mat[g["slot_index"]] = g["material"][g["slot_input"]]
    populated = np.zeros(slots, bool)
    populated[g["slot_index"]] = True
    return (depth, last_row, n_nodes, slots), nodes, soa, aos, mat, populated
