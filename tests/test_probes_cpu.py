"""Light probes (include/rt_hip.h, "light probes") without a GPU: the sampler and the SH basis of rt_math.h against float64
restatements, the irradiance helper against closed forms, a furnace through the oracle, the classes the GPU tests' inputs reach,
every refusal before a device is touched, and the layout of the two structs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_probe_trace", "rt_probe_project", "rt_probe_resolve", "rt_scene_probes", "rt_get_probe_counters"]
M32 = 0xFFFFFFFF


def _ulp(x):
    return np.spacing(np.abs(np.float32(x))).astype(np.float64)


def test_sampler_is_the_rejection_of_common_h_on_the_path_seed_stream(oracle):
    """4 096 (probe, sample) pairs, probe indices at both ends of 32 bits.  The rejection is restated in float64 on the draws the
    oracle's generator gives: r * 2 + -1 as the two f32 operations the text has (the product is exact; the sum is exact from
    r >= 1/4 on and rounded below), the length test and the normalisation in float64."""
    from tests import _probes as P
    probes = list(range(32)) + list(range((1 << 32) - 32, 1 << 32))
    pairs = [(g, s) for g in probes for s in range(64)]
    assert len(pairs) == 4096
    dirs, after, _ = P.sampler(P.SEED, pairs)
    one = np.zeros(1, np.uint32)
    tries_seen = set()
    MAX = 3 * 64
    u, f = np.zeros(MAX, np.uint32), np.zeros(MAX, np.float32)
    for j, (g, s) in enumerate(pairs):
        oracle.oracle_rand_u32_seq((P.SEED ^ g) & M32, 1, one.ctypes.data)               # rt_path_seed: pcg(pcg(seed ^ g) + s)
        oracle.oracle_rand_u32_seq((int(one[0]) + s) & M32, 1, one.ctypes.data)
        state = int(one[0])
        oracle.oracle_rand_u32_seq(state, MAX, u.ctypes.data)
        oracle.oracle_rand_f32_seq(state, MAX, f.ctypes.data)
        p32 = f * np.float32(2.0) + np.float32(-1.0)
        assert p32.dtype == np.float32
        p = p32.astype(np.float64).reshape(-1, 3)
        lensq = (p * p).sum(axis=1)
        ok = np.flatnonzero((float(np.float32(0.0001)) < lensq) & (lensq <= 1.0))
        tries = int(ok[0]) + 1
        tries_seen.add(tries)
        assert int(after[j]) == int(u[3 * tries - 1]), (g, s, tries)
        want = p[tries - 1] / np.sqrt(lensq[tries - 1])
        assert (np.abs(dirs[j].astype(np.float64) - want) <= 4 * _ulp(want)).all(), (g, s, dirs[j], want)
    assert {1, 2, 3} <= tries_seen                       # (the cube's corners are rejected 48 % of the time)
    # the direction is uniform enough for its first moment to vanish: |mean| <= 6 / sqrt(3 n) per axis
    assert (np.abs(dirs.astype(np.float64).mean(axis=0)) <= 6.0 / np.sqrt(3 * len(pairs))).all()


def _quadrature():
    """Gauss-Legendre (16 nodes in z) x 32 uniform phi: exact for the degree-4 products of two basis functions; weights sum to 1."""
    z, wz = np.polynomial.legendre.leggauss(16)
    phi = (np.arange(32) + 0.5) * (2.0 * np.pi / 32)
    r = np.sqrt(1.0 - z * z)
    d = np.stack([np.outer(r, np.cos(phi)), np.outer(r, np.sin(phi)), np.outer(z, np.ones(32))], -1).reshape(-1, 3)
    w = np.outer(wz / 2.0, np.full(32, 1.0 / 32)).ravel()
    return d, w


def test_sh9_basis_is_orthonormal():
    from raytracing_c_amd.probes import sh9_basis
    from tests import _probes as P
    d, w = _quadrature()
    d32 = d.astype(np.float32)
    args = []
    for v in d32.view(np.uint32):
        args += ["y"] + [f"{int(b):08x}" for b in v]
    Y = np.array([int(x, 16) for x in P.probe_math(*args)], np.uint32).view(np.float32).reshape(len(d), 9).astype(np.float64)
    G = 4.0 * np.pi * np.einsum("n,ni,nj->ij", w, Y, Y)
    assert np.abs(G - np.eye(9)).max() <= 1e-4, G
    # the float64 restatement of the Python side is the same nine functions
    assert np.abs(sh9_basis(d32.astype(np.float64)) - Y).max() <= 1e-6


def test_sh9_irradiance_against_closed_forms():
    from raytracing_c_amd.probes import sh9_basis, sh9_irradiance, sh9_radiance
    rng = np.random.default_rng(11)
    normals = rng.normal(size=(100, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    d, w = _quadrature()
    Y = sh9_basis(d)
    # a constant radiance L: only c0 = L * integral of Y0; the irradiance is pi L whatever the normal
    L = np.array([0.7, 1.3, 0.02])
    const = 4.0 * np.pi * np.einsum("n,nk,c->kc", w, Y, L)
    assert np.abs(const[1:]).max() <= 1e-12
    for n in normals:
        assert np.abs(sh9_irradiance(const, n) - np.pi * L).max() <= 1e-5 * np.pi * L.max()
        assert np.abs(sh9_radiance(const, n) - L).max() <= 1e-5 * L.max()
    # L(d) = 1 + 0.5 d_z, projected with the same quadrature: pi + (pi / 3) n_z
    rad = 1.0 + 0.5 * d[:, 2]
    c = 4.0 * np.pi * np.einsum("n,nk,n->k", w, Y, rad)[:, None] * np.ones(3)
    for n in normals:
        assert np.abs(sh9_irradiance(c, n) - (np.pi + np.pi / 3.0 * n[2])).max() <= 1e-4
        assert np.abs(sh9_radiance(c, n) - (1.0 + 0.5 * n[2])).max() <= 1e-4


def test_probe_grid_and_visibility():
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.probes import probe_grid, probe_visibility
    g = probe_grid((0, 10, -1), (3, 12, 1), (4, 3, 2))
    assert g.dtype == np.float32 and g.shape == (24, 3)
    assert g[0].tolist() == [0, 10, -1] and g[1].tolist() == [1, 10, -1] and g[4].tolist() == [0, 11, -1]      # x fastest
    assert g[12].tolist() == [0, 10, 1] and g[-1].tolist() == [3, 12, 1]                                       # end points included
    rec = np.zeros((2, 4), abi.PROBE_SAMPLE_DTYPE)
    rec["t"] = [[1.0, np.inf, 3.0, np.inf], [np.inf] * 4]
    frac, mean = probe_visibility(rec)
    assert frac.tolist() == [0.5, 0.0] and mean[0] == 2.0 and np.isnan(mean[1])


def test_furnace_through_the_oracle():
    """One small triangle far from the probe under a background of one texel value: every sample's radiance is the same L, so c0
    is resolve(samples * q(L * Y0)) * 4 pi exactly and the other coefficients are noise around zero: the second moment of Y_k
    over the sphere is 1 / 4 pi, so 6 L sqrt(4 pi / samples) is six standard deviations of the estimator."""
    from raytracing_c_amd.loaders import camera_from_trs
    from raytracing_c_amd.scene import Material, build_scene
    from tests import _features as F, _probes as P
    tri = np.array([[(1000.0, 1000.0, 1000.0), (1000.001, 1000.0, 1000.0), (1000.0, 1000.001, 1000.0)]], np.float32)
    hs = build_scene(tri, np.array([[(0.0, 0.0, 1.0)] * 3], np.float32), np.zeros((1, 3, 2), np.float32), [0],
                     [Material(base_color=(0.5, 0.5, 0.5))], [], camera_from_trs((0.0, 0.0, 3.0)), 0.9,
                     np.zeros((4, 8, 3), np.uint8))      # (texel value 0: a bilinear lerp of equal texels is exact for 0 alone)
    samples = 4096
    e = P.expected(hs, np.zeros((1, 3), np.float32), samples, 4)
    rec = e["records"][0]
    assert e["classes"]["miss"] == samples and np.isinf(rec["t"]).all()
    L = rec["radiance"][0]
    assert (rec["radiance"].view(np.uint32) == L.view(np.uint32)).all(), "the furnace is not constant"
    assert (L > 0).all()                             # ((0 + 0.055) / 1.055) ^ 2.4: the decode has no linear toe
    for c in range(3):
        q = F.quantize_signed(L[c] * np.float32(0.282095))
        want = P.resolve(np.array([(samples * q) & 0xFFFFFFFFFFFFFFFF], np.uint64), samples)[0]
        assert e["coeffs"][0, 0, c].tobytes() == want.tobytes()
        assert int(e["sums"][0, 0, c]) == samples * q
        bound = 6.0 * float(L[c]) * np.sqrt(4.0 * np.pi / samples)
        assert (np.abs(e["coeffs"][0, 1:, c].astype(np.float64)) <= bound).all(), (c, e["coeffs"][0, :, c], bound)
    assert np.abs(e["coeffs"][0, 1:]).max() > 0


def test_the_gpu_tests_inputs_reach_every_class():
    """Counted by the oracle alone over the inputs of tests/test_gpu_probes.py together: at least 20 samples of each class."""
    from tests import _probes as P
    total = dict.fromkeys(P.CLASSES, 0)
    per_scene = {}
    for name, shape, b in P.gpu_cases():
        e = P.expected_case(name, shape, b)
        assert e["paths"] == shape[0] * shape[1]
        if b == 0:
            assert not e["sums"].any() and not e["records"]["radiance"].any() and np.isinf(e["records"]["t"]).all()
            assert not e["coeffs"].any()
        for k, v in e["classes"].items():
            total[k] += v
            per_scene.setdefault(name, dict.fromkeys(P.CLASSES, 0))[k] += v
    for k in P.CLASSES:
        assert total[k] >= 20, total
    # the placements do what they are for: inside the closed sphere every first hit is a back face; between the back-facing quads
    # paths pass back faces and shade the textured material; the helmet shades textured Disney materials
    hs, pl = P.scene("spheres")
    inside = P.expected(hs, pl[1:2], 64, 8)
    assert inside["classes"]["backface"] == 64 and inside["classes"]["miss"] == 0
    assert per_scene["passthrough"]["backface"] >= 20 and per_scene["passthrough"]["textured"] >= 20
    assert per_scene["helmet"]["textured"] >= 20
    assert np.isnan(pl[4][0]) and np.abs(pl[3]).max() >= 1e4


def test_the_walk_and_the_callback_shader_agree_on_what_a_path_shades_first():
    """The classes come from walking a path with oracle_path_step.  The callback shader of tests/_features.py, which ends the path
    it records, sees the same paths up to their first shaded hit: it fires exactly where the walk shades at all, and where its
    material is textured the walk counts a textured shade."""
    from tests import _probes as P
    hs, pl = P.scene("passthrough")
    rows = P.first_shade_by_callback(hs, pl, 40, 8)
    fired = sum(1 for f, _, _ in rows if f)
    assert 20 <= fired <= len(rows) - 20
    for f, tex, got in rows:
        assert f == ("shaded" in got), got
        if tex:
            assert "textured" in got, got
    assert sum(1 for f, tex, got in rows if tex) >= 10 and sum(1 for f, tex, got in rows if f and not tex) >= 10
    assert any(tex and "backface" in got for f, tex, got in rows)                  # the textured quad behind a back face


def _fails(lib, call, *words):
    from raytracing_c_amd.native import last_error
    lib.rt_clear_error()
    assert call() == -1
    msg = last_error(lib)
    for w in words:
        assert w in msg, msg
    lib.rt_clear_error()


def test_symbols_and_python_entry_points():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    for n in NAMES:
        assert n in abi.EXPORTED_SYMBOLS
        assert getattr(rt.lib, n) is not None and getattr(rt.diag, n) is not None
    for f in ("bake_probes", "bake_probes_device", "probe_grid", "sh9_basis", "sh9_radiance", "sh9_irradiance", "probe_visibility",
              "get_probe_counters"):
        assert callable(getattr(rt, f)), f


def test_struct_layouts_match_the_c_header(tmp_path):
    from raytracing_c_amd import ctypes_abi as abi
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    exe = str(tmp_path / "probe_layout")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "probe_layout.c"), "-o", exe], check=True)
    got = {k: int(v) for k, v in (line.split() for line in
                                  subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["sizeof.RT_Probe_Sample"] == 32 == C.sizeof(abi.RT_Probe_Sample) == abi.PROBE_SAMPLE_DTYPE.itemsize
    assert got["sizeof.RT_Probe_Params"] == 24 == C.sizeof(abi.RT_Probe_Params)
    for T in (abi.RT_Probe_Sample, abi.RT_Probe_Params):
        for f, *_ in T._fields_:
            assert got[f"{T.__name__}.{f}"] == getattr(T, f).offset, (T.__name__, f)
    for f in ("radiance", "t", "direction", "pad"):
        assert abi.PROBE_SAMPLE_DTYPE.fields[f][1] == got["RT_Probe_Sample." + f]
    assert got["RT_PROBE_COEFFS"] == abi.RT_PROBE_COEFFS == 9
    assert got["RT_PROBE_MAX_PATHS"] == abi.RT_PROBE_MAX_PATHS == 1 << 30
    assert got["RT_PROBE_SLICE"] == abi.RT_PROBE_SLICE == 1 << 21


def test_refusals_before_a_device_is_touched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    scene = abi.Scene()                             # (never read: every case fails before the scene or the device is touched)
    s = C.byref(scene)
    fake = (C.c_uint8 * 4096)()                     # (never read: every case fails before the device scene is dereferenced)
    d = C.addressof(fake)
    pos = np.full((4, 3), 7.0, np.float32)
    coeffs = np.full((4, 9, 3), 7.0, np.float32)
    sums = np.full((4, 9, 3), 0x55, np.uint64)
    rec = np.full(4 * 2 * 8 + 8, 7.0, np.float32)
    rp = rec.ctypes.data + (-rec.ctypes.data) % 16  # a 16-byte aligned record array inside `rec`
    pp, cp, qp = pos.ctypes.data, coeffs.ctypes.data, sums.ctypes.data

    def params(**kw):
        p = abi.RT_Probe_Params(samples=2, sample_first=0, sample_count=0, max_bounces=2, seed=1, probe_first=0)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    # what every call shares: the parameter block and n
    shared = [(dict(samples=0), "samples must be positive"), (dict(samples=-3), "samples must be positive"),
              (dict(sample_first=-1), "sample range"), (dict(sample_first=1, sample_count=2), "sample range"),
              (dict(sample_count=-1), "sample range"), (dict(sample_first=3), "sample range"),
              (dict(max_bounces=-1), "max_bounces"), (dict(probe_first=M32 - 2), "32-bit probe index")]
    calls = {
        "rt_probe_trace": lambda p, n=4: lib.rt_probe_trace(d, p, n, pp, rp, None),
        "rt_probe_project": lambda p, n=4: lib.rt_probe_project(p, n, rp, qp, None),
        "rt_probe_resolve": lambda p, n=4: lib.rt_probe_resolve(p, n, qp, cp, None),
        "rt_scene_probes": lambda p, n=4: lib.rt_scene_probes(s, p, n, pp, cp, qp, rp),
    }
    for who, call in calls.items():
        _fails(lib, lambda: call(None), who, "params are NULL")
        _fails(lib, lambda: call(params(), 0), who, "n must be positive")
        _fails(lib, lambda: call(params(), -5), who, "n must be positive")
        for kw, text in shared:
            _fails(lib, lambda: call(params(**kw)), who, text)
    # one launch holds at most 2^30 paths (device level only)
    big = params(samples=1 << 20)
    _fails(lib, lambda: lib.rt_probe_trace(d, big, (1 << 10) + 1, pp, rp, None), "rt_probe_trace", "too many paths")
    _fails(lib, lambda: lib.rt_probe_project(big, (1 << 10) + 1, rp, qp, None), "rt_probe_project", "too many paths")
    _fails(lib, lambda: lib.rt_probe_resolve(params(), (1 << 30) + 1, qp, cp, None), "rt_probe_resolve", "too many probes")
    # NULL pointers, each with its own text
    _fails(lib, lambda: lib.rt_probe_trace(None, params(), 4, pp, rp, None), "rt_probe_trace", "device scene is NULL")
    _fails(lib, lambda: lib.rt_probe_trace(d, params(), 4, None, rp, None), "rt_probe_trace", "d_positions is NULL")
    _fails(lib, lambda: lib.rt_probe_trace(d, params(), 4, pp, None, None), "rt_probe_trace", "d_samples is NULL")
    _fails(lib, lambda: lib.rt_probe_project(params(), 4, None, qp, None), "rt_probe_project", "d_samples is NULL")
    _fails(lib, lambda: lib.rt_probe_project(params(), 4, rp, None, None), "rt_probe_project", "d_sums is NULL")
    _fails(lib, lambda: lib.rt_probe_resolve(params(), 4, None, cp, None), "rt_probe_resolve", "d_sums is NULL")
    _fails(lib, lambda: lib.rt_probe_resolve(params(), 4, qp, None, None), "rt_probe_resolve", "d_coeffs is NULL")
    _fails(lib, lambda: lib.rt_scene_probes(None, params(), 4, pp, cp, qp, rp), "rt_scene_probes", "scene is NULL")
    _fails(lib, lambda: lib.rt_scene_probes(s, params(), 4, None, cp, qp, rp), "rt_scene_probes", "positions is NULL")
    _fails(lib, lambda: lib.rt_scene_probes(s, params(), 4, pp, None, None, None), "rt_scene_probes", "no output is wanted")
    # a misaligned record array
    _fails(lib, lambda: lib.rt_probe_trace(d, params(), 4, pp, rp + 4, None), "rt_probe_trace", "not 16-byte aligned")
    _fails(lib, lambda: lib.rt_probe_project(params(), 4, rp + 8, qp, None), "rt_probe_project", "not 16-byte aligned")
    _fails(lib, lambda: lib.rt_get_probe_counters(None), "rt_get_probe_counters", "NULL")
    assert (pos == 7.0).all() and (coeffs == 7.0).all() and (sums == 0x55).all() and (rec == 7.0).all()


def test_fails_loudly_without_a_device_and_touches_nothing():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import raytracing_c_amd as rt
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("quad")
    pos = np.zeros((2, 3), np.float32)
    coeffs = np.full((2, 9, 3), 7.0, np.float32)
    p = rt.abi.RT_Probe_Params(samples=4, max_bounces=2, seed=1)
    rt.lib.rt_clear_error()
    assert rt.lib.rt_scene_probes(C.byref(hs.scene), C.byref(p), 2, pos.ctypes.data, coeffs.ctypes.data, None, None) == -1
    assert "no HIP device" in rt.last_error()
    assert (coeffs == 7.0).all()
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.bake_probes(hs, pos, 4, 2)
    rt.lib.rt_clear_error()
