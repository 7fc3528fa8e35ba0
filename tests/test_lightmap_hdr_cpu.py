"""HDR lightmaps without a GPU: the texel list against the oracle's bake, the sampler against a float64 rejection, what the GPU
tests' inputs reach, the estimator against the reference's in expectation, wrong kernels the inputs would expose, the dilation's
numpy form, every refusal and every struct layout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


def test_a_texel_is_listed_exactly_when_the_oracle_writes_it(oracle):
    from tests import _lightmap as LM
    from tests import _lightmap_hdr as L
    hs = L.scene("soup")
    tex, owner, count = L.texel_list(hs, 40, 48)
    mask, _, _ = LM.written_mask(oracle, hs, 48, 40)
    listed = np.zeros(48 * 40, bool)
    listed[tex["texel"]] = True
    assert np.array_equal(listed.reshape(48, 40), mask)
    assert (np.diff(tex["texel"].astype(np.int64)) > 0).all()        # row-major, each texel once
    assert np.array_equal(tex["triangle"], owner.ravel()[tex["texel"]])


def test_sampler_is_a_rejection_on_the_path_seed_stream(oracle):
    """2 048 (texel, sample, normal) triples.  The loop is restated in float64 on the draws the oracle's generator gives: the unit
    direction as tests/test_probes_cpu.py restates it, the cosine as a float64 dot product; a cosine within 1e-6 of zero decides
    nothing (none of these is)."""
    from tests import _lightmap_hdr as L
    rng = np.random.default_rng(5)
    texels = np.concatenate([np.arange(1024), np.arange((1 << 32) - 1024, 1 << 32)])
    samples = rng.integers(0, 1 << 20, len(texels))
    normals = rng.normal(size=(len(texels), 3)).astype(np.float32)
    normals[::7] *= 1e-3                                              # (not normalised: short normals accept the same directions)
    dirs, cosv, after, tries, ok = L.sampler(L.SEED, texels, samples, normals)
    assert ok.all()
    one = np.zeros(1, np.uint32)
    MAX = 3 * 64 * 8
    u, f = np.zeros(MAX, np.uint32), np.zeros(MAX, np.float32)
    seen = set()
    for j in range(len(texels)):
        oracle.oracle_rand_u32_seq((L.SEED ^ int(texels[j])) & M32, 1, one.ctypes.data)      # rt_path_seed: pcg(pcg(seed ^ p) + s)
        oracle.oracle_rand_u32_seq((int(one[0]) + int(samples[j])) & M32, 1, one.ctypes.data)
        state = int(one[0])
        oracle.oracle_rand_u32_seq(state, MAX, u.ctypes.data)
        oracle.oracle_rand_f32_seq(state, MAX, f.ctypes.data)
        p = (f * np.float32(2.0) + np.float32(-1.0)).astype(np.float64).reshape(-1, 3)
        lensq = (p * p).sum(axis=1)
        unit = np.flatnonzero((float(np.float32(0.0001)) < lensq) & (lensq <= 1.0))          # the draws that end a rt_rand_unit_vec3
        n64 = normals[j].astype(np.float64)
        t = 0
        for t, k in enumerate(unit, 1):
            c = float((p[k] / np.sqrt(lensq[k])) @ n64)
            assert abs(c) > 1e-6 * float(np.linalg.norm(n64))
            if c > 0:
                break
        assert t == int(tries[j]), (j, t, tries[j])
        assert int(after[j]) == int(u[3 * k + 2])
        want = p[k] / np.sqrt(lensq[k])
        assert np.abs(dirs[j].astype(np.float64) - want).max() <= 1e-6
        assert abs(float(cosv[j]) - float(want @ n64)) <= 1e-6 * float(np.linalg.norm(n64))
        seen.add(t)
    assert {1, 2, 3} <= seen
    # a zero normal and a NaN normal accept nothing: 64 tries, given up
    _, _, _, tries, ok = L.sampler(L.SEED, [5, 6], [0, 1], np.array([(0, 0, 0), (np.nan, 1, 0)], np.float32))
    assert not ok.any() and (tries == 64).all()


def test_the_gpu_tests_inputs_reach_every_class(oracle):
    """Counted by the oracle alone over the cases of tests/test_gpu_lightmap_hdr.py."""
    from tests import _lightmap_hdr as L
    total = dict.fromkeys(L.CLASSES, 0)
    for case in L.CASES:
        name, W, H, samples, b = case
        e = L.expected_case(case)
        for k, v in e["classes"].items():
            total[k] += v
        if (W, H) in ((40, 48), (16, 16)) and b == 8 and name != "nan":
            owned, overlap = float((e["owner"] >= 0).mean()), float((e["count"] >= 2).mean())
            dark = float((e["sums"] == 0).all(axis=1).mean())
            print(f"\nlightmap_hdr[{name} {W}x{H} s{samples}]: owned {owned:.3f} overlap {overlap:.3f} all-zero {dark:.3f}")
            if name != "quad":                                       # (quad.obj is ONE chart over the whole map: all owned, little
                assert 0.15 <= owned <= 0.95, owned                  #  overlap -- the case the issue names for a full list)
                assert overlap >= 0.10, overlap
            else:
                assert owned == 1.0
            assert dark < 0.5, dark
    print("classes", total)
    for k, v in total.items():
        assert v >= 20, (k, total)


def test_the_estimator_and_the_reference_agree_in_expectation(oracle):
    """A SANITY LINK, not a bit-exact one: lightmap_bake seeds a texel once and runs its samples on one stream, the HDR bake seeds
    every (texel, sample); both estimate the same integral.  Per owned texel of a 24 x 24 map at 256 samples: the new mean (scale 1)
    lies within 6 standard errors + 1 of the oracle's byte at 256 samples (the byte is a truncation: up to 1 below its mean).  The
    standard error comes from the samples themselves.  Saturated bytes and the zero-normal triangle are excluded."""
    from tests import _lightmap as LM
    from tests import _lightmap_hdr as L
    hs = L.scene("soup")
    W = H = 24
    e = L.expected(hs, W, H, 256, 8, counters=False)
    ref = LM.oracle_bake(oracle, hs, H, W, samples=256, seed=L.SEED)[:, :W, :3].reshape(-1, 3)[e["texels"]["texel"]].astype(np.float64)
    with np.errstate(all="ignore"):
        v = (e["radiance"] * e["cosine"][:, :, None]).astype(np.float64)      # (given-up samples: radiance 0)
    v = np.where(v > 0, v, 0.0)
    mean, se = v.mean(axis=1), v.std(axis=1, ddof=1) / np.sqrt(256.0)
    keep = (ref < 255).all(axis=1) & (e["texels"]["triangle"] != LM.special_slots(hs)["zero_normal"])
    print(f"\nexpectation link: {int(keep.sum())} of {len(keep)} owned texels kept")
    assert keep.mean() >= 0.95, keep.mean()
    dev = np.abs(mean - ref)[keep]
    bound = (6.0 * se + 1.0)[keep]
    assert (dev <= bound).all(), (int((dev > bound).sum()), float((dev - bound).max()))
    assert (ref[keep] > 0).mean() > 0.5                               # the link sees light


def test_wrong_kernels_change_what_the_gpu_inputs_expect(oracle):
    from tests import _lightmap_hdr as L
    case = ("soup", 40, 48, 5, 8)
    e = L.expected_case(case)
    hs = L.scene("soup")
    for wrong in L.WRONG:
        w = L.expected(hs, 40, 48, 5, 8, wrong=wrong, counters=True)
        if wrong == "cast_after_giving_up":                          # (its products are L x c with c <= 0 or NaN: the sums stay, the rays do not)
            assert w["rays"] > e["rays"] and w["rays"] - e["rays"] >= e["classes"]["given_up"]
        else:
            assert (w["sums"] != e["sums"]).any(axis=1).mean() > 0.5, wrong
    img = L.dilation_masks(19, 70)["random"]
    assert L.dilate(img, 2, in_place=True).tobytes() != L.dilate(img, 2).tobytes()


def test_the_dilation_fills_texels_in_each_of_eight_passes():
    from tests import _lightmap_hdr as L
    for H, W in L.DILATE_SIZES:
        masks = L.dilation_masks(H, W)
        assert L.dilate(masks["empty"], 8).tobytes() == masks["empty"].tobytes()
        assert L.dilate(masks["owned"], 8).tobytes() == masks["owned"].tobytes()
        assert L.dilate(masks["random"], 0).tobytes() == masks["random"].tobytes()
    out = L.dilate(L.dilation_masks(19, 70)["islands"], 8)
    for k in range(1, 9):
        assert (out[..., 3] == k + 1).any(), k
    out = L.dilate(L.dilation_masks(300, 5)["islands"], 8)
    for k in range(1, 9):
        assert (out[..., 3] == k + 1).any(), k
    # a filled texel is the f32 mean of its usable neighbours in visiting order
    img = np.zeros((3, 3, 4), np.float32)
    img[0, 0], img[0, 2], img[2, 1] = (0.1, 1, 2, 1), (0.2, 3, 4, 1), (0.7, 5, 6, 1)
    want = (np.float32(0.1) + np.float32(0.2) + np.float32(0.7)) / np.float32(3)
    got = L.dilate(img, 1)
    assert got[1, 1, 0] == want and got[1, 1, 3] == 2.0 and got[0, 0].tolist() == img[0, 0].tolist()


def test_symbols_and_python_entry_points():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    for name in ("rt_lightmap_texels", "rt_lightmap_trace", "rt_lightmap_resolve", "rt_lightmap_work_bytes", "rt_lightmap_dilate",
                 "rt_scene_lightmap", "rt_get_lightmap_counters"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(rt.lib, name)
    for name in ("bake_lightmap", "bake_lightmap_device", "lightmap_texels", "dilate_lightmap", "get_lightmap_counters"):
        assert callable(getattr(rt, name))
    assert rt.lib.rt_lightmap_work_bytes(70, 19) == 70 * 19 * 16


def test_struct_layouts_match_the_c_header(tmp_path):
    from raytracing_c_amd import ctypes_abi as abi
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None
    exe = str(tmp_path / "lightmap_layout")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "lightmap_layout.c"), "-o", exe], check=True)
    got = {k: int(v) for k, v in (line.split() for line in
                                  subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())}
    for T in (abi.RT_Lightmap_Texel, abi.RT_Lightmap_Params):
        assert got["sizeof." + T.__name__] == C.sizeof(T)
        for name, _ in T._fields_:
            assert got[f"{T.__name__}.{name}"] == getattr(T, name).offset, (T.__name__, name)
    for name in abi.LIGHTMAP_TEXEL_DTYPE.names:
        assert abi.LIGHTMAP_TEXEL_DTYPE.fields[name][1] == getattr(abi.RT_Lightmap_Texel, name).offset
    assert got["RT_LIGHTMAP_MAX_TEXELS"] == abi.RT_LIGHTMAP_MAX_TEXELS == 1 << 28
    assert got["RT_LIGHTMAP_MAX_PATHS"] == abi.RT_LIGHTMAP_MAX_PATHS == 1 << 30
    assert got["RT_LIGHTMAP_MAX_PASSES"] == abi.RT_LIGHTMAP_MAX_PASSES == 254
    assert got["RT_LIGHTMAP_SLICE"] == abi.RT_LIGHTMAP_SLICE == 1 << 21


def _refused(lib, call, *words):
    from raytracing_c_amd.native import last_error
    lib.rt_clear_error()
    assert call() == -1
    msg = last_error(lib)
    for w in words:
        assert w in msg, msg
    lib.rt_clear_error()


def test_refusals_before_a_device_is_touched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    scene = abi.Scene()                             # (never read: every case fails before the scene or the device is touched)
    s = C.byref(scene)
    fake = (C.c_uint8 * 4096)()                     # (never read: every case fails before the device scene is dereferenced)
    d = C.addressof(fake)
    buf = np.full(4096, 7.0, np.float32)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned pointer inside `buf`
    sums = np.full((16, 3), 0x55, np.uint64)
    n_out = C.c_int64(-9)

    def params(**kw):
        p = abi.RT_Lightmap_Params(width=4, height=4, samples=2, sample_first=0, sample_count=0, max_bounces=2, seed=1, scale=1.0)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    shared = [(dict(width=0), "width and height"), (dict(height=-2), "width and height"),
              (dict(width=1 << 15, height=(1 << 13) + 1), "too large"), (dict(samples=0), "samples must be positive"),
              (dict(sample_first=-1), "sample range"), (dict(sample_first=1, sample_count=2), "sample range"),
              (dict(sample_count=-1), "sample range"), (dict(sample_first=3), "sample range"), (dict(max_bounces=-1), "max_bounces")]
    calls = {
        "rt_lightmap_trace": lambda p: lib.rt_lightmap_trace(d, p, a, 0, 4, sums.ctypes.data, None),
        "rt_lightmap_resolve": lambda p: lib.rt_lightmap_resolve(p, 4, a, sums.ctypes.data, a + 1024, None),
        "rt_scene_lightmap": lambda p: lib.rt_scene_lightmap(s, p, 0, a, sums.ctypes.data, a + 1024, C.byref(n_out)),
    }
    for who, call in calls.items():
        _refused(lib, lambda: call(None), who, "params are NULL")
        for kw, text in shared:
            _refused(lib, lambda: call(params(**kw)), who, text)
    # rt_lightmap_texels
    tx = lambda **kw: lib.rt_lightmap_texels(*[kw.get(k, v) for k, v in (("d", d), ("v", a), ("w", 4), ("h", 4), ("o", a + 256), ("t", a + 512), ("c", a + 2048), ("s", None))])
    _refused(lib, lambda: tx(d=None), "rt_lightmap_texels", "device scene is NULL")
    _refused(lib, lambda: tx(v=None), "d_vertices is NULL")
    _refused(lib, lambda: tx(o=None), "d_owner is NULL")
    _refused(lib, lambda: tx(t=None), "d_texels is NULL")
    _refused(lib, lambda: tx(c=None), "d_count is NULL")
    _refused(lib, lambda: tx(t=a + 516), "not 16-byte aligned")
    _refused(lib, lambda: tx(w=0), "width and height")
    _refused(lib, lambda: tx(w=1 << 14, h=(1 << 14) + 1), "too large")
    # rt_lightmap_trace
    tr = lambda p=None, **kw: lib.rt_lightmap_trace(kw.get("d", d), p or params(), kw.get("t", a), kw.get("j0", 0), kw.get("m", 4),
                                                    kw.get("q", sums.ctypes.data), None)
    _refused(lib, lambda: tr(d=None), "rt_lightmap_trace", "device scene is NULL")
    _refused(lib, lambda: tr(t=None), "d_texels is NULL")
    _refused(lib, lambda: tr(q=None), "d_sums is NULL")
    _refused(lib, lambda: tr(t=a + 4), "not 16-byte aligned")
    _refused(lib, lambda: tr(j0=-1), "texel range")
    _refused(lib, lambda: tr(m=0), "texel range")
    _refused(lib, lambda: tr(j0=13, m=4), "texel range")
    _refused(lib, lambda: tr(params(width=1 << 14, height=1 << 14, samples=8), m=(1 << 27) + 1), "too many paths")
    # rt_lightmap_resolve
    rs = lambda p=None, **kw: lib.rt_lightmap_resolve(p or params(), kw.get("n", 4), kw.get("t", a), kw.get("q", sums.ctypes.data),
                                                      kw.get("i", a + 1024), None)
    _refused(lib, lambda: rs(n=-1), "rt_lightmap_resolve", "n_texels")
    _refused(lib, lambda: rs(n=17), "n_texels")
    _refused(lib, lambda: rs(i=None), "d_image is NULL")
    _refused(lib, lambda: rs(t=None), "d_texels is NULL")
    _refused(lib, lambda: rs(q=None), "d_sums is NULL")
    _refused(lib, lambda: rs(i=a + 1028), "not 16-byte aligned")
    # rt_lightmap_dilate, rt_lightmap_work_bytes
    dl = lambda **kw: lib.rt_lightmap_dilate(kw.get("w", 4), kw.get("h", 4), kw.get("k", 1), kw.get("i", a), kw.get("x", a + 1024), None)
    _refused(lib, lambda: dl(w=0), "rt_lightmap_dilate", "width and height")
    _refused(lib, lambda: dl(w=1 << 14, h=(1 << 14) + 1), "too large")
    _refused(lib, lambda: dl(k=-1), "passes")
    _refused(lib, lambda: dl(k=255), "passes")
    _refused(lib, lambda: dl(i=None), "d_image is NULL")
    _refused(lib, lambda: dl(x=None), "d_work is NULL")
    _refused(lib, lambda: dl(x=a), "must differ")
    _refused(lib, lambda: dl(x=a + 1028), "not 16-byte aligned")
    _refused(lib, lambda: int(lib.rt_lightmap_work_bytes(0, 4)), "rt_lightmap_work_bytes", "width and height")
    # rt_scene_lightmap, rt_get_lightmap_counters
    sl = lambda p=None, **kw: lib.rt_scene_lightmap(kw.get("s", s), p or params(), kw.get("k", 0), kw.get("i", a), None, None, None)
    _refused(lib, lambda: sl(s=None), "rt_scene_lightmap", "scene is NULL")
    _refused(lib, lambda: sl(i=None), "image is NULL")
    _refused(lib, lambda: sl(k=255), "passes")
    _refused(lib, lambda: sl(k=-1), "passes")
    _refused(lib, lambda: lib.rt_get_lightmap_counters(None), "rt_get_lightmap_counters")
    # nothing was written
    assert (buf == 7.0).all() and (sums == 0x55).all() and n_out.value == -9


def test_fails_loudly_without_a_device_and_touches_nothing():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a device: tests/test_gpu_lightmap_hdr.py runs the calls")
    import raytracing_c_amd as rt
    from tests import _lightmap_hdr as L
    hs = L.scene("quad")
    p = rt.abi.RT_Lightmap_Params(width=4, height=4, samples=2, max_bounces=2, seed=1, scale=1.0)
    image = np.full((4, 4, 4), 7.0, np.float32)
    rt.lib.rt_clear_error()
    assert rt.lib.rt_scene_lightmap(C.byref(hs.scene), C.byref(p), 0, image.ctypes.data, None, None, None) == -1
    assert "no HIP device" in rt.last_error()
    assert (image == 7.0).all()
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.bake_lightmap(hs, 4, 4, 2, 2, seed=1)
    rt.lib.rt_clear_error()
