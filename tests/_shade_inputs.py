"""Hand-aimed inputs for the unit-level parity tests of the shade block, the background lookup and the camera rays
(tests/test_shade_inputs_cpu.py, tests/test_gpu_shade.py), and the oracle's answers to them.

A frame draws whatever shading inputs its scene and its RNG produce; the lists here are aimed at the arms a frame reaches rarely
or never: the second and third arm of basis(), in_dir == (0, 0, 1) in the VNDF sampler, both material-load arms of shade(), the
clamps of roughness and metalness, sheen on a black base colour, NaN normals, the poles and the seam of the environment map,
one-pixel and 16384-wide frames, camera matrices that are no rotations.  Everything is generated from fixed seeds; the oracle's
answers are computed once per process (functools.lru_cache) and shared by the tests that need them.

TEST INFRASTRUCTURE: imports tests/_oracle.py, so nothing under raytracing_c_amd/ may import it.
"""
import ctypes as C
import functools

import numpy as np

from raytracing_c_amd import ctypes_abi as abi

F = np.float32

IMAGE_SIZES = [(1, 1), (5, 7), (37, 23), (16, 16)]        # (width, height) of images 0 .. 3
IMAGE_COMPONENTS = [3, 4, 3, 4]
BACKGROUND_SIZE = (67, 33)                                 # no multiple of the 4 x 4 texel tile in either direction

GROUPS = ["generic", "head_on", "head_on_axis", "near_y_hi", "near_y_lo", "near_hi", "near_lo", "on_threshold", "grazing", "below",
          "degenerate"]
GROUP_SIZES = [6000, 600, 360, 150, 150, 500, 500, 300, 600, 600, 200]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(want, got):
    """per element: equal bit patterns, or both NaN"""
    want, got = np.ascontiguousarray(want, F), np.ascontiguousarray(got, F)
    return (bits(want) == bits(got)) | (np.isnan(want) & np.isnan(got))


# ---------------------------------------------------------------------------------------------------------------------
# the scene: two dozen triangles (geometry is irrelevant), 15 material records, two of them behind the debug material too

def _materials():
    from raytracing_c_amd.scene import Material as M
    return [
        M(base_color=(0.8, 0.6, 0.4), roughness=0.2, metalness=0.0),                                                   # 0 no texture
        M(base_color=(0.9, 0.9, 0.9), roughness=1.0, metalness=0.5, texture_albedo=1),                                # 1 albedo alone
        M(base_color=(0.5, 0.7, 0.2), roughness=0.2, metalness=0.0, normal_map_strength=0.5, texture_normal=2),       # 2 normal alone
        M(base_color=(0.7, 0.7, 0.9), roughness=1.5, metalness=1.5, texture_metal_roughness=3),                       # 3 metal-roughness alone: both clamps by texel
        M(base_color=(0.3, 0.3, 0.3), emission=(2.0, 1.0, 0.5), roughness=0.001, metalness=0.0, texture_emission=0),  # 4 emission alone (1 x 1 image)
        M(base_color=(0.9, 0.5, 0.3), emission=(0.5, 0.5, 2.0), roughness=1.0, metalness=1.0, normal_map_strength=1.0, sheen=0.6,
          sheen_tint=0.5, anisotropic_strength=0.7, texture_albedo=2, texture_normal=3, texture_metal_roughness=1,
          texture_emission=0),                                                                                         # 5 all four
        M(base_color=(0.0, 0.0, 0.0), roughness=0.2, metalness=0.0, sheen=0.6, sheen_tint=0.5),                        # 6 sheen on black
        M(base_color=(0.9, 0.8, 0.1), roughness=0.0, metalness=0.95, anisotropic_strength=1.0),                       # 7 above the 0.9 clamp: dw = 0
        M(base_color=(0.6, 0.6, 0.6), roughness=0.001, metalness=1.0),                                                 # 8
        M(base_color=(0.2, 0.9, 0.6), roughness=1.5, metalness=1.5),                                                   # 9 both clamps without a texture
        M(base_color=(0.7, 0.2, 0.2), emission=(1.0, 1.0, 1.0), roughness=1.0, metalness=0.5, anisotropic_strength=0.7),   # 10 emission, no texture
        M(base_color=(1.0, 1.0, 1.0), emission=(1.0, 2.0, 3.0), roughness=1.5, metalness=1.5, normal_map_strength=0.0, sheen=0.6,
          sheen_tint=1.0, anisotropic_strength=1.0, texture_albedo=3, texture_normal=1, texture_metal_roughness=2,
          texture_emission=3),                                                                                         # 11 all four, strength 0
        M(base_color=(0.4, 0.4, 0.8), roughness=0.2, metalness=0.0, normal_map_strength=1.0, texture_normal=3),       # 12 disney AND debug with a normal texture
        M(base_color=(0.1, 0.2, 0.3), roughness=0.5, metalness=0.0),                                                   # 13 debug without a texture
        M(base_color=(0.2, 0.5, 0.9), roughness=0.2, metalness=0.0, sheen=0.6, sheen_tint=1.0),                        # 14 sheen on a colour
    ]


TRIANGLE_MATERIALS = list(range(15)) + [12] + list(range(8))          # 24 triangles; the second triangle of 12 becomes debug
SHEEN_ON_BLACK = 6


class ShadeScene:
    """hs: the HostScene.  A VARIANT is one device material: a material record behind one of the two shader procs.
    variant_slots[v]: triangle slots of variant v; variant_material[v]: index into _materials(); variant_debug[v];
    variant_textured[v] (the increment of the `textured` counter); variant_plain[v]: no normal texture, the shading normal is
    the input normal; slot_variant: variant of a populated slot, -1 otherwise."""


@functools.lru_cache(maxsize=None)
def shade_scene():
    from raytracing_c_amd.native import symbol_address
    from raytracing_c_amd.scene import build_scene
    rng = np.random.default_rng(7001)
    images = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for (w, h), c in zip(IMAGE_SIZES, IMAGE_COMPONENTS)]
    background = rng.integers(0, 256, (BACKGROUND_SIZE[1], BACKGROUND_SIZE[0], 3), dtype=np.uint8)
    n = len(TRIANGLE_MATERIALS)
    pos = np.zeros((n, 3, 3), F)
    pos[:, :, 0] = 3.0 * np.arange(n)[:, None]
    pos[:, 1, 0] += 1.0
    pos[:, 2, 1] = 1.0
    nrm = np.tile(np.array([0, 0, 1], F), (n, 3, 1))
    uv = np.tile(np.array([[0, 0], [1, 0], [0, 1]], F), (n, 1, 1))
    mats = _materials()
    hs = build_scene(pos, nrm, uv, TRIANGLE_MATERIALS, mats, images, np.eye(4, dtype=F), 0.9, background)
    debug_proc = symbol_address("debug_shader_proc")
    base, size = C.addressof(hs.materials), C.sizeof(abi.PBR_Shader_Data)
    aos = hs.scene.triangles.aos
    slots_of = {}
    for s in range(hs.n_slots):
        if aos[s].shader.proc:
            slots_of.setdefault((aos[s].shader.data - base) // size, []).append(s)
    assert sorted(slots_of) == list(range(len(mats))) and sum(len(v) for v in slots_of.values()) == n
    for s in slots_of[12][1:] + slots_of[13]:
        aos[s].shader.proc = debug_proc
    sc = ShadeScene()
    sc.hs = hs
    sc.variant_slots, sc.variant_material, sc.variant_debug = [], [], []
    for m in range(len(mats)):
        if m != 13:
            sc.variant_slots.append(slots_of[m][:1] if m == 12 else slots_of[m])
            sc.variant_material.append(m)
            sc.variant_debug.append(False)
    for m in (12, 13):
        sc.variant_slots.append(slots_of[m][1:] if m == 12 else slots_of[m])
        sc.variant_material.append(m)
        sc.variant_debug.append(True)
    has_tex = [any(t is not None for t in (m.texture_albedo, m.texture_normal, m.texture_metal_roughness, m.texture_emission)) for m in mats]
    sc.variant_textured = np.array([int(has_tex[m] and not d) for m, d in zip(sc.variant_material, sc.variant_debug)], np.int32)
    sc.variant_plain = np.array([mats[m].texture_normal is None for m in sc.variant_material])
    sc.variant_debug = np.array(sc.variant_debug)
    sc.slot_variant = np.full(hs.n_slots, -1, np.int32)
    for v, slots in enumerate(sc.variant_slots):
        sc.slot_variant[slots] = v
    sc.materials = mats
    return sc


# ---------------------------------------------------------------------------------------------------------------------
# shade-level inputs

def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, nrm):
    """a random unit vector perpendicular to every row of nrm"""
    t = np.cross(nrm, _unit(rng, len(nrm)))
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def _tilted(rng, axis, cos_lo, cos_hi):
    """unit vectors at an angle acos(c), c uniform in [cos_lo, cos_hi], from every row of `axis`"""
    c = rng.uniform(cos_lo, cos_hi, len(axis))[:, None]
    return axis * c + _perp(rng, axis) * np.sqrt(1.0 - c * c)


def _ulps(x, k):
    """float32 x moved by k units in the last place (towards larger magnitude for k > 0)"""
    return (np.ascontiguousarray(x, F).view(np.int32) + k.astype(np.int32)).view(F)


SPECIAL_UV = [0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 7.0, -0.0, -1e-9, 0.99999994, 65536.5, -65536.25, 1048576.0, -1048576.0, 0.5, 0.25]


def _tex_coords(rng, n):
    uv = rng.uniform(-2, 3, (n, 2)).astype(F)
    special = rng.random((n, 2)) < 0.3
    uv[special] = rng.choice(np.array(SPECIAL_UV, F), int(special.sum()))
    return uv


@functools.lru_cache(maxsize=None)
def shade_items():
    """dict: inp (n, 14) f32 = direction, normal, tangent, bitangent, uv; tri (n,) i32 triangle slot; seed (n,) u32;
    variant (n,); group (n,) index into GROUPS; finite (n,) bool; nd (n,) f64 = normal . direction of the f32 inputs"""
    sc = shade_scene()
    rng = np.random.default_rng(7002)
    group = np.repeat(np.arange(len(GROUPS)), GROUP_SIZES)
    n = len(group)
    nrm, d = _unit(rng, n), _unit(rng, n)
    nrm32 = None
    g = lambda name: group == GROUPS.index(name)        # noqa: E731
    k = g("generic")
    d[k] *= -np.sign(np.sum(nrm[k] * d[k], axis=1))[:, None]                      # facing hemisphere: n . d < 0
    k = g("head_on_axis")
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    nrm[k] = axes[np.arange(k.sum()) % 6]
    k = g("near_y_hi")                                                             # head-on, third arm of basis(): |n.y| clearly above 0.9999
    nrm[k] = _tilted(rng, np.tile([0.0, 1.0, 0.0], (k.sum(), 1)) * rng.choice([-1.0, 1.0], (k.sum(), 1)), 0.99996, 1.0)
    k = g("near_y_lo")                                                             # ... second arm: |n.y| clearly below
    nrm[k] = _tilted(rng, np.tile([0.0, 1.0, 0.0], (k.sum(), 1)) * rng.choice([-1.0, 1.0], (k.sum(), 1)), 0.9990, 0.99975)
    k = g("near_hi")
    d[k] = -_tilted(rng, nrm[k], 0.99996, 0.999999)
    k = g("near_lo")
    d[k] = -_tilted(rng, nrm[k], 0.9990, 0.99975)
    k = g("on_threshold")
    d[k] = -_tilted(rng, nrm[k], 0.9999, 0.9999)
    k = g("grazing")
    c = (10.0 ** rng.uniform(-7, -3, k.sum()))[:, None]
    d[k] = _perp(rng, nrm[k]) * np.sqrt(1 - c * c) - nrm[k] * c
    k = g("below")
    c = rng.uniform(0.01, 1.0, k.sum())[:, None]
    d[k] = _perp(rng, nrm[k]) * np.sqrt(1 - c * c) + nrm[k] * c
    nrm32, d32 = nrm.astype(F), d.astype(F)
    for name in ("head_on", "head_on_axis", "near_y_hi", "near_y_lo"):
        d32[g(name)] = -nrm32[g(name)]                                             # exactly: d = -n in float32
    k = np.flatnonzero(g("on_threshold"))                                          # a few float32 ulps either side of acos(0.9999)
    big = np.argmax(np.abs(d32[k]), axis=1)
    d32[k, big] = _ulps(d32[k, big], rng.integers(-3, 4, len(k)))
    tan = _perp(rng, nrm)
    tan32, bit32 = tan.astype(F), np.cross(nrm, tan).astype(F)
    k = np.flatnonzero(g("degenerate"))
    kind = np.arange(len(k)) % 5
    nrm32[k[kind == 0]] = np.nan                                                   # a zero-length normal, normalised
    d32[k[kind == 1], 0] = np.nan
    nrm32[k[kind == 2]] = np.array([1e-40, 1.0, -1e-42], F)                        # denormal components, head-on along y
    d32[k[kind == 2]] = -nrm32[k[kind == 2]]
    nrm32[k[kind == 3]] = np.array([0.0, 0.0, 1.0], F)
    d32[k[kind == 3]] = np.array([1e-39, -1e-41, -1.0], F)
    nrm32[k[kind == 4]] = np.array([1e-40, 1e-40, 1e-40], F)                       # a normal nobody normalised
    uv = _tex_coords(rng, n)
    assert np.all(np.isfinite(uv)) and np.abs(uv).max() <= 2.0 ** 20
    variant = rng.integers(0, len(sc.variant_slots), n)
    tri = np.array([sc.variant_slots[v][j % len(sc.variant_slots[v])] for j, v in enumerate(variant)], np.int32)
    seed = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    seed[::997] = 0
    inp = np.concatenate([d32, nrm32, tan32, bit32, uv], axis=1).astype(F)
    nd = np.sum(nrm32.astype(np.float64) * d32.astype(np.float64), axis=1)
    # the groups are what their names say, in float64 on the float32 values
    assert np.all(np.abs(nd[g("near_hi")]) >= 0.99995) and np.all(np.abs(nd[g("near_lo")]) <= 0.9998)
    assert np.all(np.abs(nd[g("head_on")]) >= 0.99995) and np.all(nd[g("below")] > 0) and np.all(nd[g("generic")] < 0)
    assert np.all(np.abs(nrm32[g("near_y_hi"), 1]) >= 0.99995) and np.all(np.abs(nrm32[g("near_y_lo"), 1]) <= 0.9998)
    return dict(inp=inp, tri=tri, seed=seed, variant=variant, group=group, finite=np.all(np.isfinite(inp), axis=1), nd=nd)


def draws_after(orc, seed, state_out):
    """how many random numbers lie between seed and state_out: 0, 3 (specular lobe), 5 (diffuse lobe); -1 = none of them"""
    seq = np.zeros(5, np.uint32)
    out = np.full(len(seed), -1, np.int32)
    for i in range(len(seed)):
        orc.oracle_rand_u32_seq(int(seed[i]), 5, seq.ctypes.data)
        s = state_out[i]
        out[i] = 0 if s == seed[i] else 5 if s == seq[4] else 3 if s == seq[2] else -1
    return out


@functools.lru_cache(maxsize=None)
def shade_reference():
    """The oracle on shade_items(): out (n, 9) f32 = out_dir, tint, emission; terminate (n,) i32; state (n,) u32; textured (n,) i32;
    draws (n,) i32.  The material of an item is the host Shader of its triangle's AoS record."""
    from tests import _oracle
    orc = _oracle.load()
    sc, it = shade_scene(), shade_items()
    n = len(it["tri"])
    sin = np.zeros((n, 20), F)                      # Shader_Input: direction, normal, normal_geo, tangent, bitangent, position, uv
    inp = it["inp"]
    sin[:, 0:3], sin[:, 3:6], sin[:, 6:9], sin[:, 9:12], sin[:, 12:15], sin[:, 18:20] = (inp[:, 0:3], inp[:, 3:6], inp[:, 3:6], inp[:, 6:9],
                                                                                           inp[:, 9:12], inp[:, 12:14])
    assert C.sizeof(abi.Shader_Input) == 80 and C.sizeof(abi.Shader_Output) == 40
    ins = (abi.Shader_Input * n).from_buffer(sin)
    outs = (abi.Shader_Output * n)()
    state = np.zeros(n, np.uint32)
    aos = sc.hs.scene.triangles.aos
    from raytracing_c_amd.native import symbol_address
    debug_proc = symbol_address("debug_shader_proc")
    shader = {int(s): (C.cast(aos[int(s)].shader.data, C.POINTER(abi.PBR_Shader_Data)), aos[int(s)].shader.proc == debug_proc)
              for s in np.unique(it["tri"])}
    st = C.c_uint32()
    for i in range(n):
        data, debug = shader[int(it["tri"][i])]
        st.value = int(it["seed"][i])
        if debug:
            orc.oracle_debug_shade(data, C.byref(ins[i]), C.byref(outs[i]))
        else:
            orc.oracle_disney_shade(data, C.byref(ins[i]), C.byref(st), C.byref(outs[i]))
        state[i] = st.value
    raw = np.frombuffer(outs, np.dtype([("f", "<f4", (9,)), ("terminate", "u1"), ("pad", "u1", (3,))]))
    return dict(out=raw["f"].copy(), terminate=raw["terminate"].astype(np.int32), state=state,
                textured=sc.variant_textured[it["variant"]], draws=draws_after(orc, it["seed"], state))


def shade_classes():
    """class name -> boolean mask over shade_items(), from the inputs, the material records and the oracle's outputs alone"""
    sc, it, ref = shade_scene(), shade_items(), shade_reference()
    v = it["variant"]
    debug, plain = sc.variant_debug[v], sc.variant_plain[v] & ~sc.variant_debug[v] & it["finite"]
    nd, ny = it["nd"], np.abs(it["inp"][:, 4].astype(np.float64))
    counted = it["group"] != GROUPS.index("on_threshold")
    term = ref["terminate"] != 0
    cls = {
        "basis arm 2": plain & counted & (np.abs(nd) >= 0.99995) & (ny <= 0.9998),
        "basis arm 3": plain & counted & (np.abs(nd) >= 0.99995) & (ny >= 0.99995),
        "continued": ~term,
        "terminated, view below the surface": term & ~debug & it["finite"] & (nd > 0),
        "terminated, view above the surface": term & plain & (nd < 0),
        "diffuse lobe": ~debug & (ref["draws"] == 5),
        "specular lobe": ~debug & (ref["draws"] == 3),
        "debug material": debug,
        "sheen on black, diffuse, continued": (np.array(sc.variant_material)[v] == SHEEN_ON_BLACK) & ~term & (ref["draws"] == 5),
        "NaN output": np.any(np.isnan(ref["out"]), axis=1),
    }
    for k in range(len(sc.variant_slots)):
        cls[f"variant {k}"] = v == k
    return cls


SHADE_CLASS_MINIMUM = {"basis arm 2": 200, "basis arm 3": 50, "continued": 5000, "terminated, view below the surface": 200,
                       "terminated, view above the surface": 50, "diffuse lobe": 1000, "specular lobe": 1000, "debug material": 200,
                       "sheen on black, diffuse, continued": 30, "NaN output": 20}


def describe_shade_item(i):
    sc, it = shade_scene(), shade_items()
    v = int(it["variant"][i])
    names = [k for k, m in shade_classes().items() if m[i]]
    return (f"item {i}: group {GROUPS[it['group'][i]]}, classes {names}, variant {v} (debug={bool(sc.variant_debug[v])}) = "
            f"{sc.materials[sc.variant_material[v]]}, triangle slot {it['tri'][i]}, seed {it['seed'][i]:#x}, "
            f"direction {it['inp'][i, 0:3].tolist()}, normal {it['inp'][i, 3:6].tolist()}, tangent {it['inp'][i, 6:9].tolist()}, "
            f"bitangent {it['inp'][i, 9:12].tolist()}, uv {it['inp'][i, 12:14].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# BRDF-level inputs: the shade-level list carried into tangent space with its materials' constant parameters, plus the exact
# corners no basis produces

@functools.lru_cache(maxsize=None)
def brdf_items():
    """dict: params (n, 8) f32 = roughness, metalness, sheen, sheen_tint, aniso2, base colour; in_dir (n, 3) f32; seed (n,) u32"""
    sc, it = shade_scene(), shade_items()
    rng = np.random.default_rng(7003)
    keep = np.flatnonzero(~sc.variant_debug[it["variant"]])
    inp = it["inp"][keep].astype(np.float64)
    d, nrm, tan, bit = inp[:, 0:3], inp[:, 3:6], inp[:, 6:9], inp[:, 9:12]
    with np.errstate(invalid="ignore"):
        in_dir = np.stack([-np.sum(tan * d, axis=1), -np.sum(bit * d, axis=1), -np.sum(nrm * d, axis=1)], axis=1).astype(F)
    par = np.zeros((len(keep), 8), F)
    for j, i in enumerate(keep):
        m = sc.materials[sc.variant_material[it["variant"][i]]]
        rough = min(max(F(m.roughness), F(0.001)), F(1.0))
        metal = min(F(m.metalness), F(0.9)) / F(0.9)
        par[j] = [rough, metal, m.sheen, m.sheen_tint, F(m.anisotropic_strength) * F(m.anisotropic_strength), *m.base_color]
    extra_par, extra_dir = [], []
    for metal in (0.0, 1.0):
        for rough in (0.001, 1.0):
            for aniso2 in (0.0, 0.49, 1.0):
                for sheen, base in ((0.0, (0.8, 0.6, 0.4)), (0.6, (0.0, 0.0, 0.0)), (0.6, (0.2, 0.5, 0.9))):
                    dirs = np.zeros((14, 3))
                    dirs[0:4] = [0.0, 0.0, 1.0]                                    # the lensq > 0 arm of the VNDF sampler fails
                    dirs[4:7] = _unit(rng, 3) * [1, 1, 0]                          # in_dir.z == 0
                    dirs[4:7] /= np.linalg.norm(dirs[4:7], axis=1, keepdims=True)
                    dirs[7:10] = _unit(rng, 3)
                    dirs[7:10, 2] = -np.abs(dirs[7:10, 2])                         # in_dir.z < 0
                    dirs[10:14] = _unit(rng, 4)
                    dirs[10:14, 2] = np.abs(dirs[10:14, 2])
                    extra_dir.append(dirs)
                    extra_par.append(np.tile([rough, metal, sheen, 0.5, aniso2, *base], (14, 1)))
    par = np.concatenate([par, np.concatenate(extra_par).astype(F)])
    in_dir = np.concatenate([in_dir, np.concatenate(extra_dir).astype(F)])
    seed = np.concatenate([it["seed"][keep], rng.integers(0, 2 ** 32, len(par) - len(keep), dtype=np.uint32)])
    return dict(params=np.ascontiguousarray(par), in_dir=np.ascontiguousarray(in_dir), seed=seed)


@functools.lru_cache(maxsize=None)
def brdf_reference():
    """oracle_sample_disney_brdf on brdf_items(): out_dir (n, 3), brdf (n, 4), state (n,), draws (n,)"""
    from tests import _oracle
    orc = _oracle.load()
    it = brdf_items()
    n = len(it["seed"])
    out_dir, brdf, state = np.zeros((n, 3), F), np.zeros((n, 4), F), np.zeros(n, np.uint32)
    st = C.c_uint32()
    par, in_dir = it["params"], it["in_dir"]
    for i in range(n):
        st.value = int(it["seed"][i])
        p = par[i]
        orc.oracle_sample_disney_brdf(p[0], p[1], p[2], p[3], p[4], par[i, 5:].ctypes.data, in_dir[i].ctypes.data, C.byref(st),
                                      out_dir[i].ctypes.data, brdf[i].ctypes.data)
        state[i] = st.value
    return dict(out_dir=out_dir, brdf=brdf, state=state, draws=draws_after(orc, it["seed"], state))


# ---------------------------------------------------------------------------------------------------------------------
# background directions

@functools.lru_cache(maxsize=None)
def background_dirs():
    rng = np.random.default_rng(7004)
    parts = [_unit(rng, 6000)]
    zeros = [(a, b) for a in (0.0, -0.0) for b in (0.0, -0.0)]
    for axis in range(3):                                                          # the six axes, both signs of zero elsewhere
        for s in (1.0, -1.0):
            for a, b in zeros:
                v = [a, b]
                v.insert(axis, s)
                parts.append(np.array([v]))
    tiny = np.concatenate([[0.0, -0.0], 10.0 ** rng.uniform(-30, -8, 49), -(10.0 ** rng.uniform(-30, -8, 49))])
    for x in (-1.0, 1.0):                                                          # the seam (u = 0 or 1) and its opposite (u = 0.5)
        for y in (0.0, -0.0, 0.3, -0.7):
            parts.append(np.stack([np.full(100, x), np.full(100, y), tiny], axis=1))
    for y in (1.0, -1.0, 1.5, -2.0, 5.0, -5.0):                                    # the poles, |y| > 1: rt_asinf clamps
        parts.append(np.stack([np.concatenate([[0.0, -0.0], rng.uniform(-1e-3, 1e-3, 18)]),
                               np.full(20, y), np.concatenate([[0.0, -0.0], rng.uniform(-1e-3, 1e-3, 18)])], axis=1))
    parts.append(_unit(rng, 1000) * (10.0 ** rng.uniform(-20, 20, (1000, 1))))      # unnormalised, lengths 1e-20 .. 1e20
    parts.append(_unit(rng, 500) * np.array([1.0, 1.0, 1.0]) * np.stack([np.ones(500), rng.uniform(1, 5, 500), np.ones(500)], axis=1))
    dirs = np.ascontiguousarray(np.concatenate(parts), F)
    assert np.all(np.isfinite(dirs))
    return dirs


def background_uv(dirs):
    """(u, v) of driver.c:95-104 for each direction, through the oracle's own atan2 and asin"""
    from tests import _oracle
    at = _oracle.math(5, dirs[:, 2], dirs[:, 0]).astype(np.float64)
    asn = _oracle.math(6, dirs[:, 1]).astype(np.float64)
    pi = F(3.14159265358979323846)
    inv_pi, inv_two_pi = F(1.0) / pi, F(1.0) / (F(2.0) * pi)
    return (at * np.float64(inv_two_pi) + 0.5).astype(F), (-asn * np.float64(inv_pi) + 0.5).astype(F)


@functools.lru_cache(maxsize=None)
def background_reference():
    from tests import _oracle
    orc = _oracle.load()
    sc, dirs = shade_scene(), background_dirs()
    want = np.zeros((len(dirs), 3), F)
    img = C.byref(sc.hs.background_image)
    for i in range(len(dirs)):
        orc.oracle_sample_background(img, dirs[i].ctypes.data, want[i].ctypes.data)
    return want


# ---------------------------------------------------------------------------------------------------------------------
# camera rays

FRAME_SIZES = [(1, 1), (3, 2), (65, 31), (1920, 1080), (3840, 2160), (16384, 1), (1, 16384)]
SAMPLES = [0, 1, 63, 1023, 65535]
FOVS = [0.05, 0.9, 3.0, None]                               # None: focal_length = 0
PIXELS_PER_CALL, CALLS = 167, 12                            # 12 x 167 = 2 004 random pixels per frame size


def _look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """view_matrix of driver.c:765 convention (as tests/test_gpu_random_scenes.py): columns = camera x, y, z axes in world space"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    if np.linalg.norm(r) < 1e-6:
        r = np.cross(f, (1.0, 0.0, 0.0))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    m = np.eye(4, dtype=F)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, -f, eye
    return m


def camera_matrices():
    sheared = np.array([[2.5, 0.75, -0.125, 1.0], [0.0, 0.5, 0.25, -2.0], [-0.375, 0.0, 3.0, 0.5], [0, 0, 0, 1]], F)
    far = _look_at((0.3, 0.2, 4.0), (0.0, 0.1, 0.0))
    far[:3, 3] += F(1e5)
    return [np.eye(4, dtype=F), _look_at((0, 0, 5), (0, 0, 0)), _look_at((3, 4, -2), (0.5, 0, 0.25)), _look_at((0, 7, 0), (0, 0, 0)),
            sheared, far]


def camera_for(call):
    """the Camera of call k of a frame size: every matrix twice, every focal length three times over the 12 calls"""
    from raytracing_c_amd.scene import set_camera
    cam = abi.Camera()
    fov = FOVS[call % len(FOVS)]
    set_camera(cam, camera_matrices()[call % 6], fov if fov is not None else 0.9)
    if fov is None:
        cam.focal_length = 0.0
    return cam


@functools.lru_cache(maxsize=None)
def primary_items(width, height):
    """per call k: (Camera, xys (n, 3) i32 = x, y, sample): the four corners, the edge mid-points and PIXELS_PER_CALL random
    pixels, each with every sample of SAMPLES"""
    rng = np.random.default_rng(7005 + width * 31 + height)
    w1, h1, wm, hm = width - 1, height - 1, width // 2, height // 2
    fixed = [(0, 0), (w1, 0), (0, h1), (w1, h1), (wm, 0), (wm, h1), (0, hm), (w1, hm)]
    calls = []
    for k in range(CALLS):
        px = np.concatenate([np.array(fixed), np.stack([rng.integers(0, width, PIXELS_PER_CALL), rng.integers(0, height, PIXELS_PER_CALL)], axis=1)])
        xys = np.concatenate([np.concatenate([px, np.full((len(px), 1), s)], axis=1) for s in SAMPLES]).astype(np.int32)
        calls.append((camera_for(k), np.ascontiguousarray(xys)))
    return calls


@functools.lru_cache(maxsize=None)
def primary_reference(width, height):
    from tests import _oracle
    orc = _oracle.load()
    out = []
    for cam, xys in primary_items(width, height):
        rays = np.zeros((len(xys), 6), F)
        for i in range(len(xys)):
            orc.oracle_primary_ray(C.byref(cam), width, height, int(xys[i, 0]), int(xys[i, 1]), int(xys[i, 2]), rays[i].ctypes.data)
        out.append(rays)
    return out
