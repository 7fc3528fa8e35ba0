"""The short forms of the environment lookup and of the normalisations (raytracing_c_amd/csrc/rt_dev.hip.h: atan_pos_dev, asin_dev,
atan2_dev, inv_sqrt_exact, sqrt_dev, the background's coordinates without tex_taps' negative wrap) against the functions of
include/rt_math.h they stand for.

Bar: EQUALITY.  Each form of one float is compared on the device with the unmodified rt_math.h function over all 2^32 bit
patterns (rt_test_env_sweep); atan2_dev, of two floats, on special pairs, on the directions of a frame and on 2^26 random pairs;
samples of all of them with the CPU's rt_math.h (the oracle library); the whole lookup and small frames with the oracle bit for
bit.  A NaN equals any NaN, as in the reciprocal's sweep (tests/test_gpu_parity.py); everything else is compared by its bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _shade_inputs as S

pytestmark = pytest.mark.gpu

F = np.float32
ALL = 1 << 32


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(want, got):
    return (_bits(want) == _bits(got)) | (np.isnan(want) & np.isnan(got))


def _sweep(rt, diag, which, what, seed=0):
    """(compared, differing, first differing pattern or pair as text, differing when a NaN keeps its bits); prints them"""
    out = (C.c_uint64 * 4)()
    assert diag.rt_test_env_sweep(which, seed, out) == 0, rt.last_error(diag)
    n, bad, first, strict = (int(v) for v in out)
    first = "none" if first == 0 else (f"{first - 1:#010x}" if which < 6 else f"pair {first - 1}")
    print(f"{what}: {n} compared, {bad} differ (first: {first}), {strict} differ when a NaN must keep its bits")
    return n, bad, first, strict


def _device(rt, diag, op, x, y=None):
    x = np.ascontiguousarray(x, F)
    y = np.ascontiguousarray(y, F) if y is not None else None
    got = np.zeros_like(x)
    assert diag.rt_test_math(op, x.size, x.ctypes.data, y.ctypes.data if y is not None else None, got.ctypes.data) == 0, rt.last_error(diag)
    return got


def _sample_bits(seed, n=200000):
    """random bit patterns, and the patterns where a form's ranges and special cases begin"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, ALL, n, dtype=np.uint64).astype(np.uint32)
    edges = np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x00800000, 0x807FFFFF, 0x0F800000, 0x0F7FFFFF, 0x7F7FFFFF, 0x7F800000,
                      0xFF800000, 0x7FC00000, 0xFFC00000, 0x3F800000, 0x3F7FFFFF, 0x3F800001, 0x3F000000, 0x3F000001, 0x3EFFFFFF,
                      0xBF800000, 0xBF000001, 0x3ED413CD, 0x3ED413CC, 0x3ED413CE, 0x401A827A, 0x401A8279, 0x401A827B,
                      0x71800000, 0x717FFFFF, 0x7E800000], np.uint32)
    bits[:edges.size] = edges
    bits[edges.size:edges.size + n // 8] &= np.uint32(0x807FFFFF)                   # denormals of both signs
    bits[n // 2:] = (bits[n // 2:] & np.uint32(0x807FFFFF)) | (rng.integers(118, 132, n - n // 2).astype(np.uint32) << 23)   # around 1
    return bits.view(F)


# ---------------------------------------------------------------------------------------------------------------------
# one float in, one float out: all 2^32 bit patterns

ONE_FLOAT_FORMS = [(0, "atan_pos_dev", 15), (1, "asin_dev", 16), (2, "inv_sqrt_exact", 17), (5, "sqrt_dev", 18)]


@pytest.mark.parametrize("which,name,op", ONE_FLOAT_FORMS, ids=[f[1] for f in ONE_FLOAT_FORMS])
def test_form_equals_rt_math_for_every_float(rt, oracle, diag, which, name, op):
    """atan_pos_dev / rt_atanf_pos, asin_dev / rt_asinf, inv_sqrt_exact / rcp_exact(rt_sqrtf()) and the division 1 / rt_sqrtf(),
    sqrt_dev / rt_sqrtf: no bit pattern differs on the device, and a sample has the CPU's bits."""
    from tests import _oracle
    n, bad, first, strict = _sweep(rt, diag, which, name)
    assert n == ALL
    assert bad == 0, f"{name}: {bad} patterns differ, first {first}"
    x = _sample_bits(1300 + which)
    if which == 0:                                     # rt_atan2f(a, 1) = rt_atanf_pos(a / 1) for a > 0 (rt_math.h)
        x = np.abs(x)
        x[x == 0] = F(0.75)
    got = _device(rt, diag, op, x)
    if which == 0:
        want = _oracle.math(5, x, np.ones_like(x))
    elif which == 1:
        want = _oracle.math(6, x)
    elif which == 2:
        want = _oracle.math(10, _oracle.math(9, x))
    else:
        want = _oracle.math(9, x)
    same = _same(want, got)
    assert same.all(), f"{name}: x = {x[~same][:4]!r} (bits {_bits(x[~same][:4])}), CPU {want[~same][:4]!r}, device {got[~same][:4]!r}"


@pytest.mark.parametrize("which,name,limit", [(3, "u", F(3.14159265358979323846)), (4, "v", F(1.5707963267948966192))], ids=["u", "v"])
def test_background_coordinate_never_takes_the_negative_wrap(rt, diag, which, name, limit):
    """u = fma(t, 1 / 2 pi, 0.5) over every float the arctangent can return (|t| <= RT_PI, NaN) and v = fma(-t, 1 / pi, 0.5) over
    every float the arcsine can (|t| <= pi / 2, NaN): wrap + fract of tex_taps and the fract alone that background_lookup() ships
    give the same coordinate, bit for bit."""
    n, bad, first, strict = _sweep(rt, diag, which, name)
    in_range = 2 * (int(_bits(np.array([limit]))[0]) + 1)                        # +-0 .. +-limit
    nans = 2 * ((1 << 23) - 1)
    assert n == in_range + nans
    assert bad == 0 and strict == 0, f"{name}: the wrap changes {bad} angles, first {first}"


# ---------------------------------------------------------------------------------------------------------------------
# atan2_dev: pairs

SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, 2.0 ** 127, -2.0 ** 127, np.inf, -np.inf, np.nan], F)


def _check_pairs(rt, diag, y, x, what, cpu=True):
    from tests import _oracle
    got, dev = _device(rt, diag, 14, y, x), _device(rt, diag, 5, y, x)
    same = _same(dev, got)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} pairs differ from rt_atan2f on the device, first (y, x) = ({y[~same][0]!r}, {x[~same][0]!r})"
    if cpu:
        want = _oracle.math(5, y, x)
        same = _same(want, got)
        assert same.all(), f"{what}: {np.count_nonzero(~same)} pairs differ from the CPU's rt_atan2f, first (y, x) = ({y[~same][0]!r}, {x[~same][0]!r})"


def test_atan2_special_pairs(rt, oracle, diag):
    y, x = (a.ravel().copy() for a in np.meshgrid(SPECIAL, SPECIAL, indexing="ij"))
    assert y.size == 13 * 13
    _check_pairs(rt, diag, y, x, "special values")


def test_atan2_on_the_directions_of_a_frame(rt, oracle, diag):
    """every ordered pair of components of every primary direction (sample 0) of a 64 x 64 frame"""
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.scene import set_camera
    cam = abi.Camera()
    set_camera(cam, S._look_at((3, 4, -2), (0.5, 0, 0.25)), 0.9)
    xs, ys = np.meshgrid(np.arange(64), np.arange(64))
    xys = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel(), np.zeros(64 * 64, np.int64)], axis=1).astype(np.int32))
    rays = np.zeros((len(xys), 6), F)
    assert diag.rt_test_primary_ray(C.byref(cam), 64, 64, len(xys), xys.ctypes.data, rays.ctypes.data) == 0, rt.last_error(diag)
    d = rays[:, 3:6]
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    y = np.concatenate([d[:, i] for i in range(3) for j in range(3)])
    x = np.concatenate([d[:, j] for i in range(3) for j in range(3)])
    _check_pairs(rt, diag, y, x, "frame directions")


def test_atan2_random_pairs(rt, oracle, diag):
    """2^26 seeded pairs on the device (half of them random bit patterns, half of them of ordinary size), 2^18 more against the CPU"""
    n, bad, first, strict = _sweep(rt, diag, 6, "atan2_dev", seed=0x13E5F0A1)
    assert n == 1 << 26
    assert bad == 0, f"{bad} pairs differ, first: {first}"
    y, x = _sample_bits(1311, 1 << 18), _sample_bits(1312, 1 << 18)
    x = x[np.random.default_rng(1313).permutation(x.size)]
    _check_pairs(rt, diag, y, x, "random pairs")


# ---------------------------------------------------------------------------------------------------------------------
# the whole lookup

def _next(x, k):
    return (_bits(np.array([x], F)).astype(np.int64) + k).astype(np.uint32).view(F)[0]


@functools.lru_cache(maxsize=None)
def _lookup_dirs():
    rng = np.random.default_rng(1320)
    axes = [v for a in range(3) for s in (1.0, -1.0) for v in [np.roll([s, 0.0, 0.0], a)]]
    zero_ish = [0.0, -0.0, 1e-45, -1e-45, 2.0 ** -126, -(2.0 ** -126)]             # 0 exactly and its neighbours
    one_ish = [s * float(_next(1.0, k)) for s in (1.0, -1.0) for k in (-1, 0, 1)]    # |y| = 1 exactly and its neighbours
    edge = []
    for z in zero_ish:
        for o in (0.6, -0.6, 1.0, -1.0, 1e-30):
            for yy in (0.0, 0.8, -0.8):
                edge.append([z, yy, o])                                             # dir.x = 0
                edge.append([o, yy, z])                                             # dir.z = 0
        edge += [[z, 0.3, w] for w in zero_ish]                                     # both
    for yy in one_ish:
        for a in zero_ish + [1e-4, -1e-4]:
            edge += [[a, yy, 0.0], [0.0, yy, a], [a, yy, -a]]
    v = rng.normal(size=(1 << 20, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    dirs = np.ascontiguousarray(np.concatenate([np.array(axes), np.array(edge), v]), F)
    assert np.all(np.isfinite(dirs))
    return dirs


@functools.lru_cache(maxsize=None)
def _lookup_reference():
    from tests import _oracle
    orc = _oracle.load()
    dirs = _lookup_dirs()
    want = np.zeros((len(dirs), 3), F)
    img, f, pd, pw = C.byref(S.shade_scene().hs.background_image), orc.oracle_sample_background, dirs.ctypes.data, want.ctypes.data
    for i in range(len(dirs)):
        f(img, pd + 12 * i, pw + 12 * i)
    return want


@pytest.fixture(scope="module")
def dscene(rt, diag):
    d = diag.rt_scene_upload(C.byref(S.shade_scene().hs.scene))
    assert d, rt.last_error(diag)
    yield d
    diag.rt_scene_release(d)


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
def test_lookup_equals_the_oracle(rt, oracle, diag, dscene, mode):
    """background_lookup() through its unit kernel: the six axes, directions with dir.x = 0, dir.z = 0 or |dir.y| = 1 exactly and
    their one-ulp neighbours, and 2^20 random unit directions, each with the oracle's bits"""
    dirs, want = _lookup_dirs(), _lookup_reference()
    got = np.zeros_like(want)
    assert diag.rt_test_background(dscene, mode, len(dirs), dirs.ctypes.data, got.ctypes.data) == 0, rt.last_error(diag)
    ok = np.all(S.same_bits(want, got), axis=1)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"mode {mode}: {bad.size} of {len(dirs)} directions differ; first: item {bad[0]}, direction {dirs[bad[0]].tolist()} "
                           f"(bits {S.bits(dirs[bad[0]]).tolist()})\noracle {want[bad[0]].tolist()}\ndevice {got[bad[0]].tolist()}")
    assert len(np.unique(_bits(want), axis=0)) > 1000, "the lookup must see the image, not one texel"


# ---------------------------------------------------------------------------------------------------------------------
# small frames: sky tiles, leafless tiles and general tiles through the lookup's zero and sign branches, shade()'s normalisations

LOOKS = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+z": (0, 0, 1), "-z": (0, 0, -1), "up": (0, 1, 0), "down": (0, -1, 0)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    from raytracing_c_amd.configs import load_config
    return load_config(name)[0]


@pytest.mark.parametrize("spp", [4, 64])
@pytest.mark.parametrize("name", ["quad", "spheres"])
def test_small_frames_equal_the_oracle(rt, oracle, name, spp):
    """32 x 32, 2 bounces, the camera three units from the origin looking along each axis at it: image, radiance sums, counters"""
    from tests import _oracle
    hs = _scene(name)
    seen = 0
    for look, axis in LOOKS.items():
        eye = -3.0 * np.array(axis, np.float64)
        hs.set_camera(S._look_at(eye, (0.0, 0.0, 0.0)), 1.2)
        want = _oracle.render(hs, 32, 32, spp, 2)
        got = rt.render_frame(hs, 32, 32, spp, 2, want_linear=True, want_accum=True)
        assert np.array_equal(want["accum"], got["accum"]), f"{name} {look}: fixed-point radiance sums differ"
        assert np.array_equal(_bits(want["linear"]), _bits(got["linear"])), f"{name} {look}"
        assert np.array_equal(want["image"], got["image"]), f"{name} {look}"
        for k in ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured"):
            assert want["counters"][k] == getattr(got["counters"], k), f"{name} {look}: {k}"
        assert want["counters"]["backgrounds"] > 0, f"{name} {look}: no path reached the environment"
        seen += want["counters"]["shades"]
    assert seen > 0, "no camera saw the scene: shade() never ran"
