"""The sky loop's sample adds (rt_kernels.hip, tile_add_samples_grouped in rt_dev.hip.h): where the lanes of an aligned group of
G = RT_SKY_ADD_GROUP lanes share a pixel (G <= samples per unit), their quantised samples are summed in registers and one lane
adds the sum to the LDS tile; with fewer samples per pixel every lane adds its own.  Sums mod 2^64 are order-free, so every
frame here equals the CPU oracle's: the whole u64 accumulator and all seven counters."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")
SPP = (1, 2, 4, 16, 64, 100, 128)          # samples per unit 1, 2, 4, 16, 64, 64 (the second block ends at lane 36), 64 (two full blocks)


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def spheres():
    from raytracing_c_amd.configs import load_config
    return load_config("spheres")[0]


def _u64(rt, fn):
    v = C.c_uint64()
    assert getattr(rt.lib, fn)(C.byref(v)) == 0, rt.last_error()
    return int(v.value)


def _same_as_oracle(got_accum, got_counters, want):
    assert np.array_equal(got_accum, want["accum"]), "radiance sums"
    assert tuple(getattr(got_counters, k) for k in COUNTERS) == tuple(want["counters"][k] for k in COUNTERS)


def _frame_and_oracle(rt, hs, w, h, s, b):
    """the GPU frame's (leafless paths, skipped root visits); the frame is checked against the oracle's"""
    from tests import _oracle
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    leafless, skipped = _u64(rt, "rt_get_leafless_paths"), _u64(rt, "rt_get_skipped_root_visits")
    _same_as_oracle(got["accum"], got["counters"], _oracle.render(hs, w, h, s, b))
    return leafless, skipped


def _unit_shift(spp, slab=64):
    """chunk_shift of a launch (rt_launch.cpp): log2 of the samples per unit"""
    shift = 0
    while (1 << shift) < slab and (1 << shift) < spp:
        shift += 1
    return shift


def test_sample_counts_cover_both_forms(diag):
    g = diag.rt_test_sky_add_group()
    assert g in (4, 16, 64)
    shifts = [_unit_shift(s) for s in SPP]
    assert sorted(set(shifts)) == [0, 1, 2, 4, 6]
    assert any((1 << sh) < g for sh in shifts), "no sample count keeps the per-lane adds"
    assert any((1 << sh) >= g for sh in shifts), "no sample count takes the group sum"


@pytest.mark.parametrize("spp", SPP)
def test_sample_counts(rt, oracle, spheres, spp):
    leafless, skipped = _frame_and_oracle(rt, spheres, 64, 64, spp, 2)
    assert leafless + skipped > 0


@pytest.mark.parametrize("spp", [4, 64])
def test_odd_frame_size(rt, oracle, spheres, spp):
    """61 x 37: the second pixel of the last pair of a row is outside the image, and the last tiles are ragged"""
    leafless, skipped = _frame_and_oracle(rt, spheres, 61, 37, spp, 2)
    assert leafless + skipped > 0


@pytest.mark.parametrize("slab", [16, 256])
def test_slab_parameter(rt, oracle, spheres, slab):
    """units of 16 and of 256 samples (RT_Render_Params.slab) through rt_render_accumulate, as bench.py calls it"""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _oracle
    w, h, s, b = 32, 32, 256, 2
    assert _unit_shift(s, slab) == {16: 4, 256: 8}[slab]
    d = rt.lib.rt_scene_upload(C.byref(spheres.scene))
    assert d, rt.last_error()
    try:
        accum = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
        p = abi.RT_Render_Params(w, h, s, b, 0x1234ABCD, 0, 1, slab, 0)
        assert rt.lib.rt_render_accumulate(d, C.byref(p), accum.data_ptr(), None) == 0, rt.last_error()
        torch.cuda.synchronize()
        got = accum.cpu().numpy().view(np.uint64)
        counters = rt.render.get_counters()
        assert _u64(rt, "rt_get_leafless_paths") + _u64(rt, "rt_get_skipped_root_visits") > 0
    finally:
        rt.lib.rt_scene_release(d)
    _same_as_oracle(got, counters, _oracle.render(spheres, w, h, s, b))


@pytest.fixture(scope="module")
def helmet_frame(oracle):
    """(scene, width, height, the oracle's frame at 64 spp and 1 bounce) of the smallest helmet frame for which the CPU model names
    at least 8 certainly-leafless tiles"""
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    from tests.test_gpu_leafless_tiles import _certainly_leafless
    hs, _ = load_config("helmet")
    sizes = [(8 * k, (8 * k * 9 + 8) // 16) for k in range(4, 17)]          # 32 x 18 ... 128 x 72
    w, h = next((w, h) for w, h in sizes if int(_certainly_leafless(hs, w, h).sum()) >= 8)
    return hs, w, h, _oracle.render(hs, w, h, 64, 1)


def test_leafless_and_sky_tiles(rt, helmet_frame):
    """both kinds of tile of the loop in one frame"""
    hs, w, h, want = helmet_frame
    got = rt.render_frame(hs, w, h, 64, 1, want_accum=True)
    leafless, skipped = _u64(rt, "rt_get_leafless_paths"), _u64(rt, "rt_get_skipped_root_visits")
    print(f"helmet {w} x {h}: leafless paths {leafless}, skipped root visits {skipped}")
    _same_as_oracle(got["accum"], got["counters"], want)
    assert leafless > 0 and skipped > 0


def test_two_views_in_one_launch(rt, oracle, spheres):
    from tests import _oracle
    from tests.test_gpu_views import _copy, _five_views
    hs = spheres
    w, h, s, b = 64, 64, 64, 2
    cams = [_five_views(hs)[0], _five_views(hs)[2]]
    seeds = [5, 0xBEEF]
    got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_accum=True)
    assert _u64(rt, "rt_get_leafless_paths") + _u64(rt, "rt_get_skipped_root_visits") > 0
    saved = _copy(hs.scene.camera)
    try:
        total = dict.fromkeys(COUNTERS, 0)
        for v, (cam, sd) in enumerate(zip(cams, seeds)):
            hs.scene.camera = cam
            want = _oracle.render(hs, w, h, s, b, seed=sd)
            assert np.array_equal(got[v]["accum"], want["accum"]), f"view {v}"
            for k in COUNTERS:
                total[k] += want["counters"][k]
        assert tuple(getattr(got[0]["counters"], k) for k in COUNTERS) == tuple(total[k] for k in COUNTERS)      # (of the whole batch)
    finally:
        hs.scene.camera = saved


def test_hand_over_adds_nothing_twice(rt, oracle):
    """a scene 1e5 units from the origin: every batch hands over to the general loop, before anything of it was added"""
    from tests._far_scene import translated_spheres
    leafless, skipped = _frame_and_oracle(rt, translated_spheres(1e5), 64, 64, 64, 2)
    assert leafless == 0 and skipped == 0


def test_a_group_sum_carries_into_the_high_word(helmet_frame, diag):
    """On the oracle's data, for the helmet frame above: a pixel of a certain sky tile whose channel sum over the 64 samples
    reaches 2^32 -- and whose first G samples, one aligned group of lanes, already do while sample 0 alone does not: the carry out
    of the low words happens inside a group sum."""
    from raytracing_c_amd import tile_classes as tc
    from tests import _oracle
    hs, w, h, want = helmet_frame
    g = diag.rt_test_sky_add_group()
    sky = np.asarray(tc.classify_scene(hs, w, h, 1e-2)["root_miss"], bool)          # (the stricter margin culls less: sky for the kernel too)
    assert sky.any()
    mask = np.kron(sky, np.ones((8, 8), bool))[:h, :w, None]
    assert (want["accum"] * mask).max() >= 1 << 32
    group = _oracle.render(hs, w, h, g, 1)["accum"]
    one = _oracle.render(hs, w, h, 1, 1)["accum"]
    assert (mask & (group >= 1 << 32) & (one < 1 << 32)).any()


@pytest.mark.parametrize("group", [4, 16, 64])
def test_group_sum_unit(diag, group):
    """group_sum3_u64 on crafted lanes: low words of all ones, values up to the clamp 2^52, zeros, random validity masks"""
    rng = np.random.default_rng(group)
    n_waves = 64
    n = n_waves * 64
    v = rng.integers(0, (1 << 52) + 1, n, dtype=np.uint64)
    v[0:256] = 0xFFFFFFFF                                          # every step carries
    v[256:512] = 1 << 52                                           # RT_ACCUM_MAX, quantised
    v[512:768] = (rng.integers(0, 1 << 20, 256, dtype=np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
    v[768:1024] = 0
    v[1024:1280] = np.where(rng.random(256) < 0.5, 0, 0xFFFFFFFF).astype(np.uint64)
    valid = (rng.random(n) < 0.7).astype(np.uint8)
    valid[0:128] = 1
    valid[1280:1344] = 0                                           # a wave without a sample
    valid[1344:1408] = np.arange(64) < 36                          # a sample block that ends inside the wave
    # three channels at once, as the loop sums them: the values, the same a wave on, and large random ones that wrap mod 2^64
    chans = np.ascontiguousarray(np.stack([v, np.roll(v, 64), rng.integers(0, 1 << 64, n, dtype=np.uint64)]))
    out = np.zeros((3, n), np.uint64)
    assert diag.rt_test_group_sum(group, n_waves, chans.ctypes.data, valid.ctypes.data, out.ctypes.data) == 0
    for c in range(3):
        want = np.where(valid != 0, chans[c], np.uint64(0)).reshape(-1, group).sum(axis=1, dtype=np.uint64)      # (mod 2^64)
        assert np.array_equal(out[c].reshape(-1, group), np.repeat(want[:, None], group, axis=1)), f"channel {c}"
