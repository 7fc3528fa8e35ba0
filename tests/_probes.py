"""What the light-probe calls must return (include/rt_hip.h, "light probes"), from the CPU oracle and rt_math.h alone.
TEST INFRASTRUCTURE ONLY.

A record is built the way the contract reads: tests/c/probe_math.c (gcc -O2 -ffp-contract=off over include/rt_math.h) gives the
direction of (seed, probe, sample), the RNG state behind it and the nine basis values; oracle_cast_ray traces the reference's
cast_ray from that ray and state; oracle_ray_scene_hit with entry distance infinity gives t.  Sums are Python integers mod 2^64 of
_features.quantize_signed(one numpy f32 multiply), coefficients the numpy restatement of rt_accum_resolve_signed times one numpy
f32 multiply by 4 pi.

Classes.  Every sample is also WALKED: oracle_ray_scene_hit and oracle_path_step -- the very function cast_ray calls per hit -- one
iteration at a time, which tells how the path ended and what it met on the way; a walk that ends in a shader or by exhaustion
carries the path's radiance, which must be oracle_cast_ray's bit for bit.  (The callback shader of tests/_features.py ends the path
it records, so it cannot say whether the real path went on to the background; the step function can.  What the callback DOES see
-- whether a path is shaded at all, and with what material first -- the walk must agree with: first_shade_by_callback.)
  miss       the first segment left the scene (t = +inf)
  background the path ended on the background after at least one hit
  ended      the path was exhausted or ended by a shader
  backface   the path passed at least one back face
  textured   the path shaded at least one textured material
The first three partition the samples with max_bounces > 0; the last two overlap them.
"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from raytracing_c_amd import ctypes_abi as abi
from tests import _features as F
from tests import _oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234ABCD
FOUR_PI = np.float32(12.566371)
CLASSES = ("miss", "background", "ended", "backface", "textured")
# (n, sample_count, sample_first, samples): a single path; a probe boundary and the end of the list inside one wave; more probes than
# two waves have lanes; several refills and grabs
SHAPES = [(1, 1, 0, 1), (3, 70, 0, 70), (130, 1, 0, 1), (2, 600, 40, 700)]
BOUNCES = (0, 1, 8)

_exe = None


def probe_math(*args):
    """tests/c/probe_math.c, built once per process; returns its output split into words."""
    global _exe
    if _exe is None:
        cc = shutil.which("gcc") or shutil.which("cc")
        assert cc is not None, "no C compiler on this machine"
        exe = os.path.join(tempfile.mkdtemp(prefix="probe_math_"), "probe_math")
        subprocess.run([cc, "-std=gnu11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c", "probe_math.c"), "-o", exe, "-lm"], check=True)
        _exe = exe
    out = []
    args = [str(a) for a in args]
    for k in range(0, len(args), 4096 * 12):                         # (both forms' argument counts divide 12)
        out += subprocess.run([_exe, *args[k:k + 4096 * 12]], capture_output=True, text=True, check=True).stdout.split()
    return out


def sampler(seed, pairs):
    """For (global probe index, sample) pairs: directions (m, 3) float32, states after (m,) uint32, basis values (m, 9) float32."""
    args = []
    for g, s in pairs:
        args += ["s", f"{seed:08x}", int(g), int(s)]
    words = np.array([int(w, 16) for w in probe_math(*args)], np.uint32).reshape(len(pairs), 13)
    return words[:, :3].copy().view(np.float32), words[:, 3].copy(), words[:, 4:].copy().view(np.float32)


def products_by_c(a, b):
    """rt_accum_quantize_signed(a * b) of float32 arrays, by probe_math."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    args = []
    for x, y in zip(a.view(np.uint32), b.view(np.uint32)):
        args += ["p", f"{int(x):08x}", f"{int(y):08x}"]
    return [int(w, 16) for w in probe_math(*args)]


def resolve(sums, samples):
    """rt_accum_resolve_signed of uint64 sums -> float32, then the one f32 multiply by 4 pi."""
    sums = np.ascontiguousarray(sums, np.uint64)
    mean = (sums.view(np.int64).astype(np.float64) / (float(samples) * 4294967296.0)).astype(np.float32)
    return mean * FOUR_PI


def walk(oracle, hs, cfg, origin, direction, state, max_bounces):
    """One sample's path, iteration by iteration -> (set of classes, radiance or None when it ended on the background)."""
    ray = abi.Ray(abi.Vec3(*[float(v) for v in origin]), abi.Vec3(*[float(v) for v in direction]))
    st, bounce, done = C.c_uint32(int(state)), C.c_int32(0), C.c_int32(0)
    tint, emis, rad = np.ones(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    cnt = (C.c_uint64 * 2)()
    got = set()
    first = True
    while True:
        hit = abi.Hit()
        hit.distance = np.inf
        tri = C.c_int32(-1)
        oracle.oracle_ray_scene_hit(C.byref(ray), C.byref(hs.scene), C.byref(hit), C.byref(tri))
        if tri.value < 0:
            got.add("miss" if first else "background")
            return got, None
        first = False
        oracle.oracle_path_step(C.byref(hs.scene), C.byref(cfg), C.byref(ray), C.byref(hit), tint.ctypes.data, emis.ctypes.data,
                                C.byref(st), C.byref(bounce), max_bounces, C.byref(done), rad.ctypes.data, cnt)
        got.add("shaded" if cnt[0] else "backface")                 # ("shaded": not a class of its own, see first_shade_by_callback)
        if cnt[1]:
            got.add("textured")
        if done.value:
            got.add("ended")
            return got, rad


def first_shade_by_callback(hs, positions, samples, max_bounces, seed=SEED):
    """The callback-proc technique of tests/_features.py on the same samples: the scene's shaders replaced by a recording callback
    that ends the path, so it sees the FIRST hit the reference hands to a shader and nothing behind it.  Per sample: (the callback
    fired, its material has an albedo or normal texture, the walk's classes) -- what the two techniques must agree on."""
    oracle = _oracle.load()
    rec = F.Recorder()
    cb, cfg = F.with_procs(hs, rec)
    cfg.seed = seed
    positions = np.ascontiguousarray(positions, np.float32)
    pairs = [(i, k) for i in range(len(positions)) for k in range(samples)]
    dirs, states, _ = sampler(seed, pairs)
    rgb = np.zeros(3, np.float32)
    out = []
    for j, (i, k) in enumerate(pairs):
        o = positions[i]
        ray = abi.Ray(abi.Vec3(float(o[0]), float(o[1]), float(o[2])), abi.Vec3(*[float(v) for v in dirs[j]]))
        st = C.c_uint32(int(states[j]))
        rec.hit = None
        oracle.oracle_cast_ray(C.byref(cb.scene), C.byref(cfg), C.byref(ray), max_bounces, C.byref(st), rgb.ctypes.data)
        tex = False
        if rec.hit is not None:
            d = abi.PBR_Shader_Data.from_address(rec.hit[0])
            tex = bool(d.texture_albedo) or bool(d.texture_normal) or bool(d.texture_metal_roughness) or bool(d.texture_emission)
        got, _ = walk(oracle, hs, _oracle.config_for(hs, seed=seed, n_threads=1), o, dirs[j], states[j], max_bounces)
        out.append((rec.hit is not None, tex, got))
    return out


def expected(hs, positions, samples, max_bounces, seed=SEED, probe_first=0, sample_range=None, classes=True, pick=None):
    """dict(records (n, count) PROBE_SAMPLE_DTYPE, sums (n, 9, 3) uint64, coeffs (n, 9, 3) float32, paths, classes {name: count})
    of the probes at `positions` over the sample range (default: all).  pick: only these (probe, sample-of-the-range) pairs are
    traced -- records is then (len(pick),) and there are no sums."""
    oracle = _oracle.load()
    cfg = _oracle.config_for(hs, seed=seed, n_threads=1)
    positions = np.ascontiguousarray(positions, np.float32)
    n = len(positions)
    first, count = sample_range if sample_range else (0, samples)
    pairs = [(i, k) for i in range(n) for k in range(count)] if pick is None else [(int(i), int(k)) for i, k in pick]
    dirs, states, basis = sampler(seed, [(probe_first + i, first + k) for i, k in pairs])
    rec = np.zeros(len(pairs), abi.PROBE_SAMPLE_DTYPE)
    counts = dict.fromkeys(CLASSES, 0)
    rgb = np.zeros(3, np.float32)
    for j, (i, k) in enumerate(pairs):
        o = positions[i]
        ray = abi.Ray(abi.Vec3(float(o[0]), float(o[1]), float(o[2])), abi.Vec3(*[float(v) for v in dirs[j]]))
        st = C.c_uint32(int(states[j]))
        oracle.oracle_cast_ray(C.byref(hs.scene), C.byref(cfg), C.byref(ray), max_bounces, C.byref(st), rgb.ctypes.data)
        t = np.float32(np.inf)
        if max_bounces > 0:
            hit = abi.Hit()
            hit.distance = np.inf
            oracle.oracle_ray_scene_hit(C.byref(ray), C.byref(hs.scene), C.byref(hit), None)
            t = np.float32(hit.distance)
        rec[j]["radiance"], rec[j]["t"], rec[j]["direction"] = rgb, t, dirs[j]
        if classes and max_bounces > 0:
            got, rad = walk(oracle, hs, cfg, o, dirs[j], states[j], max_bounces)
            assert ("miss" in got) == bool(np.isinf(t))
            assert rad is None or rad.tobytes() == rgb.tobytes(), "the walk is not cast_ray's path"
            for c in got & set(CLASSES):
                counts[c] += 1
    if pick is not None:
        return dict(records=rec, classes=counts)
    rec = rec.reshape(n, count)
    basis = basis.reshape(n, count, 9)
    # sums: one numpy f32 multiply per (sample, k, c), quantised and added as Python integers mod 2^64
    prod = rec["radiance"][:, :, None, :] * basis[:, :, :, None]                  # (n, count, 9, 3) float32
    assert prod.dtype == np.float32
    sums = np.zeros((n, 9, 3), np.uint64)
    for i in range(n):
        acc = [0] * 27
        for row in prod[i].reshape(count, 27).tolist():
            for q, v in enumerate(row):
                acc[q] += F.quantize_signed(v)
        sums[i] = np.array([v & 0xFFFFFFFFFFFFFFFF for v in acc], np.uint64).reshape(9, 3)
    if count:                                                                    # the multiply and the quantisation against the C text
        few = min(count, 4)
        want = products_by_c(np.broadcast_to(rec["radiance"][0, :few, None, :], (few, 9, 3)),
                             np.broadcast_to(basis[0, :few, :, None], (few, 9, 3)))
        assert want == [F.quantize_signed(v) for v in prod[0, :few].ravel().tolist()]
    return dict(records=rec, sums=sums, coeffs=resolve(sums, samples), paths=n * count, classes=counts)


# ---- the inputs of the GPU tests (tests/test_gpu_probes.py); tests/test_probes_cpu.py counts the classes they reach ----------------
def _vertices(hs):
    T = hs.scene.triangles
    n = int(T.len)
    return np.stack([np.stack([np.ctypeslib.as_array(getattr(T, ax)[k], (n,)) for ax in "xyz"], 1) for k in range(3)], 1)   # (n, 3 vertices, xyz)


def _populated(hs):
    """Indices of the triangle slots that hold a triangle (the builder's empty slots have no shader)."""
    n = int(hs.scene.triangles.len)
    rows = np.zeros(n, F._AOS_DTYPE)
    C.memmove(rows.ctypes.data, hs.scene.triangles.aos, n * 112)
    return np.flatnonzero(rows["shader_proc"] != 0)


def bbox(hs):
    v = _vertices(hs)[_populated(hs)].reshape(-1, 3).astype(np.float64)
    return v.min(axis=0), v.max(axis=0)


def spheres_placements(hs):
    """Outside the geometry; inside a closed sphere (just behind a vertex of it, along the inward normal); on a vertex of a
    triangle; at distance 1e4; one with a NaN coordinate."""
    V = _vertices(hs)
    lo, hi = bbox(hs)
    c, e = (lo + hi) / 2, hi - lo
    aos = hs.scene.triangles.aos
    populated = _populated(hs)
    k = int(populated[len(populated) // 3])
    na = aos[k].normal_a
    inward = -np.array([na.x, na.y, na.z], np.float64)
    inside = V[k, 0].astype(np.float64) + inward * 0.02 * float(e.max())
    return np.array([c + e * (0.05, 0.75, 0.1), inside, V[k, 1], c + (1e4, 0.0, 0.0), (np.nan, c[1], c[2])], np.float32)


def passthrough_placements():
    """Between the two back-facing quads of the middle column; between the left column's front face and its back face; in front of
    everything; beside the quads, level with them."""
    return np.array([(0.1, 0.0, 1.25), (-1.0, 0.1, 0.5), (0.0, 0.0, 3.5), (1.5, 0.2, 0.7)], np.float32)


def helmet_placements(hs):
    lo, hi = bbox(hs)
    c, e = (lo + hi) / 2, hi - lo
    return np.array([c + e * (0.0, 0.1, 0.9), c, c + e * (0.7, 0.3, 0.2)], np.float32)


def tiled(placements, n):
    return np.ascontiguousarray(placements[np.arange(n) % len(placements)])


_scenes = {}


def scene(name):
    """(HostScene, placements) of "spheres", "passthrough" or "helmet", built once."""
    if name not in _scenes:
        from raytracing_c_amd.configs import load_config
        if name == "passthrough":
            hs = F.passthrough_scene()
            _scenes[name] = (hs, passthrough_placements())
        else:
            hs, _ = load_config(name)
            _scenes[name] = (hs, spheres_placements(hs) if name == "spheres" else helmet_placements(hs))
    return _scenes[name]


def gpu_cases():
    """(scene name, shape, max_bounces) of every bit-exact GPU case: spheres and the pass-through scene in every shape at every
    bounce count, the helmet once."""
    cases = [(s, shape, b) for s in ("spheres", "passthrough") for shape in SHAPES for b in BOUNCES]
    return cases + [("helmet", SHAPES[1], 8)]


_cache = {}


def expected_case(name, shape, max_bounces):
    """expected() of one GPU case, once: the tests that share it read it and leave it unchanged."""
    key = (name, shape, max_bounces)
    if key not in _cache:
        hs, placements = scene(name)
        n, count, first, samples = shape
        e = expected(hs, tiled(placements, n), samples, max_bounces, sample_range=(first, count))
        for k in ("records", "sums", "coeffs"):
            e[k].setflags(write=False)
        _cache[key] = e
    return _cache[key]
