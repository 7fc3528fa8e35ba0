"""The aimed path-step inputs of tests/_step_inputs.py, with the oracle alone: that the list reaches the arms it aims at -- counted on
what the oracle computed for the items, not on what the generator meant -- and that oracle_fill_hit / oracle_path_step, which give
tests/test_gpu_shade_hit.py its expected values, are the code a frame runs: chained in Python they return oracle_cast_ray's radiance
and RNG state bit for bit."""
import ctypes as C

import numpy as np
import pytest

from raytracing_c_amd import ctypes_abi as abi
from tests import _step_inputs as T

F = np.float32


@pytest.mark.parametrize("max_bounces", T.MAX_BOUNCES)
def test_every_class_is_reached(oracle, max_bounces):
    """every class by at least 32 items; the below-the-face bias and each "only one dot positive" class by at least 100"""
    cls = T.step_classes(max_bounces)
    n = len(T.step_items()["slot"])
    assert 10000 <= n <= 20000
    counts = {name: int(m.sum()) for name, m in cls.items()}
    low = {name: (c, T.CLASS_MINIMUM.get(name, T.DEFAULT_MINIMUM)) for name, c in counts.items() if c < T.CLASS_MINIMUM.get(name, T.DEFAULT_MINIMUM)}
    assert not low, f"classes below their minimum (count, minimum): {low}"
    for name in T.CLASS_MINIMUM:
        assert name in cls


def test_the_face_test_is_the_two_float32_dots(oracle):
    """the arm oracle_path_step took is the one the exact float32 dots of the filled hit name: the classes rest on those dots"""
    it, hits, ref = T.step_items(), T.filled_hits(), T.step_reference(T.MAX_BOUNCES[1])
    d = it["ray"][:, 3:6]
    geo, nint = T.dot32(hits["normal_geo"], d), T.dot32(hits["normal"], d)
    passed = ref["words"][:, 3] == 0
    bad = np.flatnonzero(passed != ((geo > 0) | (nint > 0)))
    assert len(bad) == 0, T.describe_step_item(int(bad[0]))
    # ... and a float64 dot would have chosen otherwise for the items aimed at that
    with np.errstate(all="ignore"):
        geo64 = np.sum(hits["normal_geo"].astype(np.float64) * d.astype(np.float64), axis=1)
        int64 = np.sum(hits["normal"].astype(np.float64) * d.astype(np.float64), axis=1)
    assert int(np.sum(passed & ~((geo64 > 0) | (int64 > 0)))) >= 200


def test_what_the_oracle_did_with_the_arms(oracle):
    """spot checks of the step's outputs on the classes: the pass-through arm leaves everything but the origin alone, a zero-length
    normal reaches the shader as NaN or infinity, the bias has the sign of the outgoing direction, exhaustion returns the emission"""
    mb = T.MAX_BOUNCES[1]
    it, hits, ref, cls = T.step_items(), T.filled_hits(), T.step_reference(mb), T.step_classes(mb)
    out, words = ref["out"], ref["words"]
    passed = words[:, 3] == 0
    # pass-through: direction, tint, emission and the RNG untouched, one bounce counted, origin = madd(direction, RT_EPS, point)
    k = np.flatnonzero(passed)
    assert np.all(T.same_bits(out[k, 3:12], np.concatenate([it["ray"][k, 3:6], it["carry"][k]], axis=1)))
    assert np.array_equal(words[k, 0], it["seed"][k]) and np.array_equal(words[k, 1].astype(np.int32), T.bounce_in(mb)[k] + 1)
    want = np.stack([T.fma32(it["ray"][k, 3 + c], np.full(len(k), T.RT_EPS), hits["point"][k, c]) for c in range(3)], axis=1)
    assert np.all(T.same_bits(want, out[k, 0:3]))
    # a normal whose square is 0 is not finite in the shader input; a square in the denormals or below 2^-96 still normalises to
    # length 1
    sin = T.shader_inputs()["sin"]
    zero_len = sin[cls["normal: dot(n_int, n_int) exactly 0, shaded"], 3:6]                # 0 x infinity, or 1e-25 x infinity
    assert np.all(np.any(~np.isfinite(zero_len), axis=1)) and np.sum(np.all(np.isnan(zero_len), axis=1)) >= T.DEFAULT_MINIMUM
    for name in ("normal: dot(n_int, n_int) below 2^-96, shaded", "normal: dot(n_int, n_int) denormal, shaded"):
        ln = np.linalg.norm(sin[cls[name], 3:6].astype(np.float64), axis=1)
        assert np.all(np.abs(ln - 1) < 1e-3), (name, ln.min(), ln.max())
    # scatter: origin = madd(n_geo, +-2 RT_EPS / 2, point), the sign is that of dot(n_geo, new direction)
    for name, sign in (("origin: next direction above the face", 1.0), ("origin: next direction below the face", -1.0),
                       ("origin: dot(n_geo, next direction) exactly 0", 1.0)):
        k = np.flatnonzero(cls[name])
        bias = F(sign) * (F(0.5) * F(2.0) * T.RT_EPS)
        want = np.stack([T.fma32(hits["normal_geo"][k, c], np.full(len(k), bias), hits["point"][k, c]) for c in range(3)], axis=1)
        assert np.all(T.same_bits(want, out[k, 0:3])), name
    # the path's value: emission when the step ended it, untouched otherwise
    done = words[:, 2] == 1
    assert np.all(T.same_bits(out[done, 12:15], out[done, 9:12])) and np.all(out[~done, 12:15] == T.RADIANCE_UNSET)
    assert np.all(done[T.bounce_in(mb) == mb - 1]) and np.all(T.step_reference(1)["words"][:, 2] == 1)


def test_the_inverse_generator_step():
    for v in (0, 1, 0x1234ABCD, 0xFFFFFFFF, 2891336453):
        assert T.pcg_inverse(T.pcg(v)) == v and T.pcg(T.pcg_inverse(v)) == v
    s = T.seed_for_zero_draw(4)
    for _ in range(4):
        s = T.pcg(s)
    assert s == 0


def test_fma32_is_the_fused_multiply_add():
    """against exact rational arithmetic, on values whose float64 sum lands on a float32 tie"""
    from fractions import Fraction
    rng = np.random.default_rng(7120)
    a = rng.normal(size=4000).astype(F)
    b = rng.normal(size=4000).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(F)                       # cancels the product's leading bits
    c[2000:] = (rng.normal(size=2000) * 10.0 ** rng.uniform(-8, 8, 2000)).astype(F)
    a[:3], b[:3], c[:3] = [1 + 2.0 ** -12, 1.0, 3.0], [1 + 2.0 ** -12, 2.0 ** -24, 2.0 ** -25], [2.0 ** -60, 1.0, 1.0]   # ties but for a sticky bit
    got = T.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = float(got[i])
        lo, hi = float(np.nextafter(got[i], F(-np.inf))), float(np.nextafter(got[i], F(np.inf)))
        err = abs(Fraction(g) - exact)
        assert err <= abs(Fraction(lo) - exact) and err <= abs(Fraction(hi) - exact), (i, a[i], b[i], c[i], g)
        if err == abs(Fraction(lo) - exact) or err == abs(Fraction(hi) - exact):
            assert (int(got[i:i + 1].view(np.uint32)[0]) & 1) == 0, (i, a[i], b[i], c[i], g)      # a true tie goes to even


def test_the_chained_steps_are_cast_ray(oracle):
    """2 000 camera rays of the helmet, 8 bounces: oracle_ray_scene_hit -> oracle_fill_hit -> oracle_path_step (-> oracle_sample_background)
    in a Python loop give oracle_cast_ray's three floats and its final RNG state, bit for bit; on the way oracle_fill_hit rebuilds the
    Hit that the traversal filled."""
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    hs, _ = load_config("helmet")
    cfg = _oracle.config_for(hs, n_threads=1)
    scene, pcfg = C.byref(hs.scene), C.byref(cfg)
    rng = np.random.default_rng(7121)
    n, w, h, mb = 2000, 640, 360, 8
    # 1 700 camera rays that meet the helmet and 300 that see the sky at once, out of 30 000 drawn over the frame
    cand = np.stack([rng.integers(0, w, 30000), rng.integers(0, h, 30000), rng.integers(0, 64, 30000)], axis=1)
    rays = np.zeros((len(cand), 6), F)
    for i in range(len(cand)):
        oracle.oracle_primary_ray(C.byref(hs.scene.camera), w, h, int(cand[i, 0]), int(cand[i, 1]), int(cand[i, 2]), rays[i].ctypes.data)
    ct, ctri, cuv = np.zeros(len(cand), F), np.zeros(len(cand), np.int32), np.zeros((len(cand), 2), F)
    oracle.oracle_trace_rays(scene, len(cand), rays.ctypes.data, ct.ctypes.data, ctri.ctypes.data, cuv.ctypes.data)
    xys = np.concatenate([cand[ctri >= 0][:1700], cand[ctri < 0][:300]])
    assert len(xys) == n
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    r6, rgb, t1, uv1, bg = np.zeros(6, F), np.zeros(3, F), np.zeros(1, F), np.zeros(2, F), np.zeros(3, F)
    tri1 = np.zeros(1, np.int32)
    carry, radiance, cnt = np.zeros(6, F), np.zeros(3, F), np.zeros(2, np.uint64)
    state, bounce, done, tri = C.c_uint32(), C.c_int32(), C.c_int32(), C.c_int32()
    hit, filled, ray = abi.Hit(), abi.Hit(), abi.Ray()
    steps = hits_seen = grounded = 0
    for i in range(n):
        oracle.oracle_primary_ray(C.byref(hs.scene.camera), w, h, int(xys[i, 0]), int(xys[i, 1]), int(xys[i, 2]), r6.ctypes.data)
        C.memmove(C.byref(ray), r6.ctypes.data, 24)
        state.value = int(seeds[i])
        oracle.oracle_cast_ray(scene, pcfg, C.byref(ray), mb, C.byref(state), rgb.ctypes.data)
        want_state = state.value
        state.value, bounce.value = int(seeds[i]), 0
        carry[:] = (1, 1, 1, 0, 0, 0)
        got = None
        while got is None:
            assert bounce.value < mb
            C.memset(C.byref(hit), 0, C.sizeof(hit))
            hit.distance = np.inf
            oracle.oracle_ray_scene_hit(C.byref(ray), scene, C.byref(hit), C.byref(tri))
            if tri.value < 0:
                d = np.array([ray.direction.x, ray.direction.y, ray.direction.z], F)
                oracle.oracle_sample_background(C.byref(hs.background_image), d.ctypes.data, bg.ctypes.data)
                got = T.fma32(bg, carry[0:3], carry[3:6])                            # rt_v3_mul_add(bg, tint, emission)
                break
            C.memmove(r6.ctypes.data, C.byref(ray), 24)
            oracle.oracle_trace_rays(scene, 1, r6.ctypes.data, t1.ctypes.data, tri1.ctypes.data, uv1.ctypes.data)
            assert tri1[0] == tri.value and T.bits(t1)[0] == T.bits(np.array([hit.distance], F))[0]
            oracle.oracle_fill_hit(scene, C.byref(ray), float(t1[0]), tri.value, float(uv1[0]), float(uv1[1]), C.byref(filled))
            assert bytes(filled) == bytes(hit), f"ray {i}, bounce {bounce.value}: oracle_fill_hit differs from the traversal's Hit"
            hits_seen += 1
            oracle.oracle_path_step(scene, pcfg, C.byref(ray), C.byref(filled), carry.ctypes.data, carry.ctypes.data + 12, C.byref(state),
                                    C.byref(bounce), mb, C.byref(done), radiance.ctypes.data, cnt.ctypes.data)
            steps += 1
            if done.value:
                got = radiance.copy()
                grounded += 1
        assert np.all(T.same_bits(rgb, got)) and state.value == want_state, (i, xys[i].tolist(), rgb.tolist(), np.asarray(got).tolist())
    # every ray that met the helmet took a step, some took several, and some paths ended on a step instead of in the sky
    assert steps == hits_seen > 1700 and grounded >= 1, (steps, grounded)
    hs.free()
