"""First-hit feature buffers (include/rt_hip.h: rt_render_features, rt_render_accumulate_features, rt_resolve_features) without a
GPU: the signed fixed-point pair of rt_math.h against Python integers, the CPU helper the GPU tests compare with (tests/_features.py)
against the oracle's own counters, and every argument error reported before the device is touched."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_render_accumulate_features", "rt_resolve_features", "rt_render_features"]
MAX = 1048576.0


def _bits(v):
    return int(np.float32(v).view(np.uint32))


@pytest.fixture(scope="module")
def features_math(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    exe = str(tmp_path_factory.mktemp("features") / "features_math")
    subprocess.run([cc, "-std=gnu11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "features_math.c"), "-o", exe], check=True)

    def run(*args):
        return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, check=True).stdout.split()
    return run


def _exact_q(v):
    """The definition, in exact arithmetic: NaN -> 0, clamp to +-2^20, times 2^32, truncate towards zero, mod 2^64."""
    v = np.float32(v)
    if v != v:
        return 0
    f = max(Fraction(-(1 << 20)), min(Fraction(1 << 20), Fraction(float(v)))) if np.isfinite(v) else Fraction((1 << 20) if v > 0 else -(1 << 20))
    n = f * (1 << 32)
    return (int(n) if n >= 0 else -int(-n)) & 0xFFFFFFFFFFFFFFFF


VALUES = [0.0, -0.0, 1e-12, -1e-12, 2.0 ** -32, -(2.0 ** -32), 2.0 ** -33, -(2.0 ** -33), 1.5 * 2.0 ** -32, -1.5 * 2.0 ** -32,
          1.0, -1.0, 0.1, -0.1, 3.4567, -3.4567, 12345.678, -12345.678, MAX, -MAX, np.nextafter(np.float32(MAX), np.float32(0)),
          -np.nextafter(np.float32(MAX), np.float32(0)), 2e6, -2e6, 3e38, -3e38, np.inf, -np.inf, np.nan, 1e-45, -1e-45]


def test_signed_quantize_matches_python_integers(features_math):
    from tests import _features as F
    args = []
    for v in VALUES:
        args += ["q", f"{_bits(v):08x}"]
    got = [int(x, 16) for x in features_math(*args)]
    assert len(got) == len(VALUES)
    for v, g in zip(VALUES, got):
        assert g == _exact_q(v) == F.quantize_signed(v), (v, hex(g))
    # beyond the clamp = at the clamp; tiny = 0; symmetric about zero
    q = dict(zip([_bits(v) for v in VALUES], got))
    assert q[_bits(2e6)] == q[_bits(MAX)] == q[_bits(np.inf)] == 1 << 52
    assert q[_bits(-2e6)] == q[_bits(-MAX)] == q[_bits(-np.inf)] == (1 << 64) - (1 << 52)
    assert q[_bits(1e-12)] == q[_bits(-1e-12)] == q[_bits(-0.0)] == q[_bits(np.nan)] == 0
    assert q[_bits(2.0 ** -32)] == 1 and q[_bits(-(2.0 ** -32))] == (1 << 64) - 1
    # non-negative values quantise like the unsigned rt_accum_quantize (restated in the helper)
    for v in VALUES:
        if np.float32(v) >= 0:
            assert F.quantize_signed(v) == F.quantize(v), v


def test_signed_resolve_of_sums_whose_sign_flips(features_math):
    from tests import _features as F
    M = 1 << 64
    cases = []
    for vals, samples in (((2.5, -4.0), 3), ((-4.0, 2.5, 1.5), 3), ((-0.1, 0.1), 2), ((-MAX,) * 7, 7), ((MAX,) * 5, 8),
                          ((-3.4567, -12345.678, 1.0), 4), ((2.0 ** -32, -(2.0 ** -32), -(2.0 ** -32)), 1), ((0.0,), 1)):
        total = 0
        for k, v in enumerate(vals):
            total = (total + F.quantize_signed(v)) % M                    # the running sum wraps mod 2^64 ...
            cases.append((total, samples))                                # ... and every prefix is resolved too
    args = []
    for total, samples in cases:
        args += ["r", f"{total:016x}", samples]
    got = [int(x, 16) for x in features_math(*args)]
    flips = 0
    prev = 0
    for (total, samples), g in zip(cases, got):
        signed = total - M if total >= 1 << 63 else total
        want = np.float32(float(Fraction(signed, samples << 32)))         # exact mean, rounded once to double, once to float
        assert g == _bits(want), (hex(total), samples)
        res = F.resolve(np.full((1, 1, 10), total, np.uint64), samples)
        assert _bits(res["position"][0, 0, 0]) == g
        flips += (signed < 0) != (prev < 0)
        prev = signed
    assert flips >= 4


def test_helper_agrees_with_the_oracles_counters():
    """The helper classifies every sample as feature hit / miss / exhausted by itself; an oracle_render of the same scene with the
    same procs counts shades and backgrounds: coverage = samples - backgrounds - exhausted paths."""
    from tests import _features as F, _oracle
    oracle = _oracle.load()
    hs = F.passthrough_scene()
    w, h, s = 16, 16, 2
    seen = {}
    for b in (1, 2, 3):
        e = F.expected_cached("passthrough", hs, w, h, s, b)
        rec = F.Recorder()
        cb, cfg = F.with_procs(hs, rec)
        img = np.zeros((h, w, 3), np.uint8)
        image = _oracle.abi.Image()
        image.components, image.pixel_type, image.width, image.stride, image.height = 3, 0, w, w, h
        image.pixels.data, image.pixels.len = img.ctypes.data, img.size
        cnt = _oracle.Oracle_Counters()
        assert oracle.oracle_render(C.byref(cb.scene), C.byref(image), s, b, C.byref(cfg), None, None, C.byref(cnt)) == 0
        paths = w * h * s
        assert cnt.paths == paths == e["hits"] + e["misses"] + e["exhausted"]
        assert cnt.shades == e["hits"] and cnt.backgrounds == e["misses"]
        coverage = int((e["sums"][..., 0] >> np.uint64(32)).sum())
        assert coverage == paths - cnt.backgrounds - e["exhausted"] == e["hits"]
        assert (e["sums"][..., 0] & np.uint64(0xFFFFFFFF) == 0).all()
        # every shader terminates, so the surplus of rays over paths counts the pass-throughs (none fits into one iteration)
        assert (cnt.rays - cnt.paths > 0) == (b > 1)
        seen[b] = e
    assert seen[1]["hits"] == 0 and seen[1]["exhausted"] > 0
    assert seen[2]["hits"] > 0 and seen[2]["exhausted"] > 0 and seen[3]["exhausted"] == 0 and seen[3]["hits"] > seen[2]["hits"]
    assert seen[3]["textured"] > 0 and seen[3]["untextured"] > 0


def _fails(lib, call, *words):
    from raytracing_c_amd.native import last_error
    lib.rt_clear_error()
    assert call() == -1
    msg = last_error(lib)
    for w in words:
        assert w in msg, msg
    lib.rt_clear_error()


def test_symbols_and_python_entry_point():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    for n in NAMES:
        assert n in abi.EXPORTED_SYMBOLS
        assert getattr(rt.lib, n) is not None and getattr(rt.diag, n) is not None
    assert abi.RT_FEATURE_CHANNELS == 10 and C.sizeof(abi.RT_Features) == 32
    assert callable(rt.render_features)


def test_argument_errors_before_the_device_is_touched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    scene = abi.Scene()                             # (never read: every case fails before the scene or the device is touched)
    s = C.byref(scene)
    planes = np.full(4 * 4 * 10, 7.0, np.float32)
    sums = np.full(4 * 4 * 10, 0x55, np.uint64)
    fp = C.POINTER(C.c_float)
    out = abi.RT_Features(planes.ctypes.data_as(fp), None, None, None)
    o, q = C.byref(out), sums.ctypes.data
    who = "rt_render_features"
    _fails(lib, lambda: lib.rt_render_features(None, 4, 4, 2, 2, o, q), who, "scene is NULL")
    _fails(lib, lambda: lib.rt_render_features(s, 0, 4, 2, 2, o, q), who, "image size")
    _fails(lib, lambda: lib.rt_render_features(s, 4, -1, 2, 2, o, q), who, "image size")
    _fails(lib, lambda: lib.rt_render_features(s, 1 << 15, (1 << 13) + 1, 2, 2, o, q), who, "too large")
    _fails(lib, lambda: lib.rt_render_features(s, 4, 4, 0, 2, o, q), who, "samples must be positive")
    _fails(lib, lambda: lib.rt_render_features(s, 4, 4, -3, 2, o, q), who, "samples must be positive")
    _fails(lib, lambda: lib.rt_render_features(s, 4, 4, 2, -1, o, q), who, "max_bounces")
    _fails(lib, lambda: lib.rt_render_features(s, 4, 4, 1 << 40, 2, o, q), who, "32 bits")
    _fails(lib, lambda: lib.rt_render_features(s, 4, 4, 2, 2, None, None), who, "no output")
    _fails(lib, lambda: lib.rt_render_features(s, 4, 4, 2, 2, C.byref(abi.RT_Features()), None), who, "no output")
    # device level
    fake = (C.c_uint8 * 4096)()                     # (never read: every case fails before the scene is dereferenced)
    d = C.addressof(fake)

    def params(**kw):
        p = abi.RT_Render_Params(width=4, height=4, samples=2, max_bounces=2, world=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    who = "rt_render_accumulate_features"
    _fails(lib, lambda: lib.rt_render_accumulate_features(None, params(), q, None), who, "scene is NULL")
    _fails(lib, lambda: lib.rt_render_accumulate_features(d, None, q, None), who, "params are NULL")
    _fails(lib, lambda: lib.rt_render_accumulate_features(d, params(), None, None), who, "d_sums is NULL")
    _fails(lib, lambda: lib.rt_render_accumulate_features(d, params(width=0), q, None), who, "image size")
    _fails(lib, lambda: lib.rt_render_accumulate_features(d, params(samples=0), q, None), who, "samples must be positive")
    _fails(lib, lambda: lib.rt_render_accumulate_features(d, params(rank=1, world=2), q, None), who, "rank 1 / world 2")
    _fails(lib, lambda: lib.rt_render_accumulate_features(d, params(world=0), q, None), who, "world 0")
    _fails(lib, lambda: lib.rt_render_accumulate_features(d, params(sample_first=1, sample_count=2), q, None), who, "sample range")
    who = "rt_resolve_features"
    p0 = planes.ctypes.data
    _fails(lib, lambda: lib.rt_resolve_features(None, q, p0, None, None, None, None), who, "params are NULL")
    _fails(lib, lambda: lib.rt_resolve_features(params(), None, p0, None, None, None, None), who, "d_sums is NULL")
    _fails(lib, lambda: lib.rt_resolve_features(params(), q, None, None, None, None, None), who, "no output")
    _fails(lib, lambda: lib.rt_resolve_features(params(height=0), q, p0, None, None, None, None), who, "image size")
    assert (planes == 7.0).all() and (sums == 0x55).all()


def test_fails_loudly_without_a_device_and_touches_nothing():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("quad")
    planes = np.full((8, 8, 3), 7.0, np.float32)
    sums = np.full((8, 8, 10), 0x55, np.uint64)
    out = abi.RT_Features(None, planes.ctypes.data_as(C.POINTER(C.c_float)), None, None)
    rt.lib.rt_clear_error()
    assert rt.lib.rt_render_features(C.byref(hs.scene), 8, 8, 2, 2, C.byref(out), sums.ctypes.data) == -1
    assert "no HIP device" in rt.last_error()
    assert (planes == 7.0).all() and (sums == 0x55).all()
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.render_features(hs, 8, 8, 2, 2)
    rt.lib.rt_clear_error()
