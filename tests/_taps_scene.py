"""The scene of tests/test_gpu_shade_taps.py: six unit quads in a row, one material each, with the texture sets at which the
shared-taps form of the shade block (SharedTaps, raytracing_c_amd/csrc/rt_dev.hip.h) can differ from the general one, and the
shade-level items aimed at tex_taps()' wrap, tile and clamp rules.  The oracle's answers are computed once per process.

  material 0   four 8 x 8 textures (two 4 x 4 tiles a row)
  material 1   four 5 x 3 textures: ragged, two tiles a row for 5 texels, one row of tiles for 3
  material 2   normal + emission alone, 4 x 4
  material 3   no texture
  material 4   a normal map (4 x 4) behind the debug material
  material 5   an albedo alone, 4 wide and 8 high: it keeps that image in the texture pool, so that an in-place edit can give
               material 0 a normal map of another size than its albedo

mixed=True builds the same scene with material 0's normal map 4 x 8 from the start.

TEST INFRASTRUCTURE: imports tests/_oracle.py, so nothing under raytracing_c_amd/ may import it."""
import ctypes as C
import functools

import numpy as np

from raytracing_c_amd import ctypes_abi as abi

F = np.float32
IMAGE_SIZES = [(8, 8)] * 4 + [(5, 3)] * 4 + [(4, 4)] * 2 + [(4, 8)]          # (width, height) of images 0 .. 10
MIXED_IMAGE = 10
N_MATERIALS = 6
DEBUG_MATERIAL = 4
# 0, 1 - 1 ulp, a tile boundary of the 8-wide and the 5-wide textures from either side (texel 4.0 and just below), the last texel
# (right / bottom clamp) of 8, 5, 4 and 3 texels, a texel centre, a negative coordinate, one beyond 1
COORDS = [0.0, 0.99999994, 0.5, 0.49999997, 0.8, 0.79999995, 0.9375, 0.9, 0.875, 0.84, 0.375, -0.3, 5.75]


def _materials(mixed):
    from raytracing_c_amd.scene import Material as M
    return [
        M(base_color=(0.9, 0.8, 0.7), emission=(0.5, 1.0, 2.0), roughness=1.0, metalness=1.0, normal_map_strength=0.8,
          texture_albedo=0, texture_normal=MIXED_IMAGE if mixed else 1, texture_metal_roughness=2, texture_emission=3),
        M(base_color=(0.7, 0.9, 0.6), emission=(1.0, 0.5, 0.25), roughness=0.9, metalness=0.8, normal_map_strength=1.0, sheen=0.5,
          sheen_tint=0.5, texture_albedo=4, texture_normal=5, texture_metal_roughness=6, texture_emission=7),
        M(base_color=(0.5, 0.6, 0.9), emission=(2.0, 2.0, 1.0), roughness=0.3, metalness=0.2, normal_map_strength=0.6,
          texture_normal=8, texture_emission=9),
        M(base_color=(0.8, 0.3, 0.2), roughness=0.4, metalness=0.1),
        M(base_color=(0.4, 0.4, 0.8), normal_map_strength=1.0, texture_normal=8),
        M(base_color=(0.9, 0.9, 0.9), roughness=0.7, metalness=0.0, texture_albedo=MIXED_IMAGE),
    ]


class TapsScene:
    """hs: the HostScene; slots[m]: the populated triangle slots of material m; materials: the Material list"""


def build(mixed=False):
    from raytracing_c_amd.native import symbol_address
    from raytracing_c_amd.scene import build_scene
    from tests._shade_inputs import _look_at
    rng = np.random.default_rng(1401)
    images = [rng.integers(0, 256, (h, w, 3 + (k & 1)), dtype=np.uint8) for k, (w, h) in enumerate(IMAGE_SIZES)]
    background = rng.integers(0, 256, (16, 32, 3), dtype=np.uint8)
    pos, uv, ids = [], [], []
    corner_uv = np.array([[-0.25, -0.25], [1.25, -0.25], [1.25, 1.25], [-0.25, 1.25]], F)      # the wrap on every edge
    for m in range(N_MATERIALS):
        c = np.array([[m, 0, 0], [m + 1, 0, 0], [m + 1, 1, 0], [m, 1, 0]], F)
        for a, b, d in ((0, 1, 2), (0, 2, 3)):
            pos.append(c[[a, b, d]])
            uv.append(corner_uv[[a, b, d]])
            ids.append(m)
    n = len(pos)
    nrm = np.tile(np.array([0, 0, 1], F), (n, 3, 1))
    mats = _materials(mixed)
    hs = build_scene(np.array(pos), nrm, np.array(uv), ids, mats, images, _look_at((3.0, 0.5, 1.5), (3.0, 0.5, 0.0)), 1.2, background)
    base, size = C.addressof(hs.materials), C.sizeof(abi.PBR_Shader_Data)
    aos = hs.scene.triangles.aos
    sc = TapsScene()
    sc.hs, sc.materials, sc.slots = hs, mats, [[] for _ in mats]
    for s in range(hs.n_slots):
        if aos[s].shader.proc:
            sc.slots[(aos[s].shader.data - base) // size].append(s)
    assert all(len(v) == 2 for v in sc.slots)
    for s in sc.slots[DEBUG_MATERIAL]:
        aos[s].shader.proc = symbol_address("debug_shader_proc")
    return sc


@functools.lru_cache(maxsize=None)
def scene():
    return build(False)


@functools.lru_cache(maxsize=None)
def items():
    """every pair of COORDS on every material: inp (n, 14) f32 = direction, normal, tangent, bitangent, uv; tri (n,) i32;
    seed (n,) u32; material (n,)"""
    from tests._shade_inputs import _perp, _unit
    sc = scene()
    rng = np.random.default_rng(1402)
    uv = np.array([(u, v) for u in COORDS for v in COORDS], F)
    material = np.repeat(np.arange(N_MATERIALS), len(uv))
    n = len(material)
    nrm, d = _unit(rng, n), _unit(rng, n)
    d *= -np.sign(np.sum(nrm * d, axis=1))[:, None]                       # the view above the surface
    tan = _perp(rng, nrm)
    inp = np.concatenate([d, nrm, tan, np.cross(nrm, tan), np.tile(uv, (N_MATERIALS, 1))], axis=1).astype(F)
    tri = np.array([sc.slots[m][j & 1] for j, m in enumerate(material)], np.int32)
    return dict(inp=np.ascontiguousarray(inp), tri=tri, seed=rng.integers(0, 2 ** 32, n, dtype=np.uint32), material=material)


@functools.lru_cache(maxsize=None)
def reference():
    """the oracle's shaders on items(): out (n, 9) f32 = out_dir, tint, emission; terminate, state, textured (n,)"""
    from tests import _oracle
    orc = _oracle.load()
    sc, it = scene(), items()
    n = len(it["tri"])
    sin = np.zeros((n, 20), F)                      # Shader_Input: direction, normal, normal_geo, tangent, bitangent, position, uv
    inp = it["inp"]
    sin[:, 0:3], sin[:, 3:6], sin[:, 6:9], sin[:, 9:12], sin[:, 12:15], sin[:, 18:20] = (inp[:, 0:3], inp[:, 3:6], inp[:, 3:6], inp[:, 6:9],
                                                                                           inp[:, 9:12], inp[:, 12:14])
    ins = (abi.Shader_Input * n).from_buffer(sin)
    outs = (abi.Shader_Output * n)()
    state = np.zeros(n, np.uint32)
    st = C.c_uint32()
    for i in range(n):
        m = int(it["material"][i])
        data = C.pointer(sc.hs.materials[m])
        st.value = int(it["seed"][i])
        if m == DEBUG_MATERIAL:
            orc.oracle_debug_shade(data, C.byref(ins[i]), C.byref(outs[i]))
        else:
            orc.oracle_disney_shade(data, C.byref(ins[i]), C.byref(st), C.byref(outs[i]))
        state[i] = st.value
    raw = np.frombuffer(outs, np.dtype([("f", "<f4", (9,)), ("terminate", "u1"), ("pad", "u1", (3,))]))
    has_tex = np.array([m not in (3, DEBUG_MATERIAL) for m in range(N_MATERIALS)])
    return dict(out=raw["f"].copy(), terminate=raw["terminate"].astype(np.int32), state=state,
                textured=has_tex[it["material"]].astype(np.int32))


def uniform_order():
    """whole waves of one material: every material's items padded with its own first ones to a multiple of 64"""
    m = items()["material"]
    out = []
    for k in range(N_MATERIALS):
        idx = np.flatnonzero(m == k)
        out.append(np.concatenate([idx, idx[:(-len(idx)) % 64]]))
    return np.concatenate(out)


def mixed_order():
    """every wave holds two materials or more"""
    m = items()["material"]
    order = np.random.default_rng(1403).permutation(len(m))
    assert all(len(np.unique(m[order[j:j + 64]])) >= 2 for j in range(0, len(order), 64))
    return order


def material_table(rows):
    """packed material rows (36 words each, rt_device.h) for rt_materials_share_taps: rows = per material a list of four entries,
    None or (width, height, stride), in the order albedo, normal, metal-roughness, emission; offsets differ from slot to slot"""
    t = np.zeros((len(rows), 36), np.int32)
    for r, slots in enumerate(rows):
        for k, s in enumerate(slots):
            t[r, 12 + k] = -1 if s is None else 4 * r + k
            if s is not None:
                t[r, 20 + 4 * k:24 + 4 * k] = (1000 * (4 * r + k), *s)
    return t
