"""The batch loop of the path kernel (rt_kernels.hip: sky, leafless and triangle-less tiles) takes several units of its tile per
atomic -- RT_KParams.grab_batch (rt_launch.cpp) while the tile has plenty left, then 2, then 1 -- where the other tiles take
grab_max.  Every unit is still handed out exactly once, whichever wave, loop or grab size consumes it: every frame here equals
the CPU oracle's, the whole u64 accumulator and all seven counters.  The frames run with the constant the library ships; the
knob test runs the other values the diagnostic library accepts, 16 among them."""
import hashlib
import json
import os
import subprocess
import sys
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")
SEED = 0x1234ABCD                             # the oracle's default


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


def _served(rt):
    return dict(triangleless=_u64(rt, "rt_get_triangleless_paths"), leafless=_u64(rt, "rt_get_leafless_paths"),
                skipped=_u64(rt, "rt_get_skipped_root_visits"))


def _same_as_oracle(got_accum, got_counters, want):
    assert np.array_equal(got_accum, want["accum"]), "radiance sums"
    assert tuple(getattr(got_counters, k) for k in COUNTERS) == tuple(want["counters"][k] for k in COUNTERS)


def _frame_and_oracle(rt, hs, w, h, s, b):
    from tests import _oracle
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    served = _served(rt)
    _same_as_oracle(got["accum"], got["counters"], _oracle.render(hs, w, h, s, b))
    return served


def _units(spp, slab=64):
    """(paths per unit, units per tile) of a launch of spp samples (rt_launch.cpp: chunk_shift, n_sample_blocks, n_chunks_tile)"""
    shift = 0
    while (1 << shift) < slab and (1 << shift) < spp:
        shift += 1
    return 2 << shift, 32 * ((spp + (1 << shift) - 1) >> shift)


def test_the_sample_counts_cover_the_unit_sizes():
    """of the cases below: units of 32 paths (half a batch), of 64 and of 128; tiles of 32, 64 and 256 units -- under the taper
    (8 g units left: g, 8 left: 2, else 1) a tile of 32 or 64 units never sees a grab of 8, one of 256 units does for most of it"""
    assert _units(16) == (32, 32) and _units(32) == (64, 32) and _units(64) == (128, 32)
    assert _units(100) == (128, 64) and _units(128) == (128, 64) and _units(512) == (128, 256)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "raytracing_c_amd", "librt_hip_diag.so")
# (spheres, samples): 256 units per tile, where every value is taken as it is, and 32, where the host puts the tile through the taper
KNOB_JOBS = [dict(config="spheres", w=32, h=32, s=512, b=2, env=({"RT_GRAB_BATCH": str(g)} if g else {}), slabs=[0]) for g in (0, 1, 2, 4, 16)] + \
            [dict(config="spheres", w=64, h=64, s=64, b=2, env={"RT_GRAB_BATCH": str(g)}, slabs=[0]) for g in (1, 16)]


@pytest.fixture(scope="module")
def knob_results():
    """the jobs in a process of their own: the diagnostic library reads RT_GRAB_BATCH at every launch (tests/_diag_worker.py)"""
    env = dict(os.environ, RT_LIB_PATH=DIAG)
    for k in list(env):
        if k.startswith("RT_") and k != "RT_LIB_PATH":
            del env[k]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_diag_worker.py")], input=json.dumps(KNOB_JOBS), text=True,
                       capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == len(KNOB_JOBS), (r.stdout[-1000:], r.stderr[-1000:])
    return lines


def test_units_per_atomic_do_not_change_the_frame(oracle, spheres, knob_results):
    """1, 2, 4 and 16 units per atomic and the shipped value: the oracle's radiance sums and counters, every time"""
    from tests import _oracle
    want = {}
    for job, got in zip(KNOB_JOBS, knob_results):
        assert got["error"] is None, got["error"]
        key = (job["w"], job["h"], job["s"])
        if key not in want:
            o = _oracle.render(spheres, job["w"], job["h"], job["s"], job["b"])
            want[key] = (hashlib.sha256(o["accum"].tobytes()).hexdigest(), [o["counters"][k] for k in ("rays", "node_visits", "leaf_visits", "shades")])
        assert got["digests"] == [want[key][0]], job["env"]
        assert got["counters"] == want[key][1], job["env"]


@pytest.mark.parametrize("spp", [32, 64, 100, 128])
def test_sample_counts(rt, oracle, spheres, spp):
    """units of 64 and of 128 paths; 100 spp: the last unit of a pixel ends inside the unit"""
    served = _frame_and_oracle(rt, spheres, 64, 64, spp, 2)
    assert served["leafless"] + served["skipped"] > 0


def test_units_smaller_than_a_batch(rt, oracle, spheres):
    """16 spp: 32 paths per unit, half a batch; a tile of 32 units, which the host puts through the taper (2 per atomic, then 1)"""
    assert _units(16)[0] < 64
    served = _frame_and_oracle(rt, spheres, 64, 64, 16, 2)
    assert served["leafless"] + served["skipped"] > 0


def test_a_tile_with_plenty_left(rt, oracle, spheres):
    """512 spp: 256 units per tile, the shipped units per atomic for most of the tile"""
    served = _frame_and_oracle(rt, spheres, 32, 32, 512, 2)
    assert served["leafless"] + served["skipped"] > 0


def test_odd_frame_size(rt, oracle, spheres):
    """61 x 37: tiles cut by the right and the bottom edge of the image, and chunks with tiles outside it"""
    served = _frame_and_oracle(rt, spheres, 61, 37, 64, 2)
    assert served["leafless"] + served["skipped"] > 0


@pytest.fixture(scope="module")
def helmet_frame(oracle):
    """the helmet frame of tests/test_gpu_sky_adds.py: (scene, width, height, the oracle's frame at 64 spp and 1 bounce)"""
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    from tests.test_gpu_leafless_tiles import _certainly_leafless
    hs, _ = load_config("helmet")
    sizes = [(8 * k, (8 * k * 9 + 8) // 16) for k in range(4, 17)]
    w, h = next((w, h) for w, h in sizes if int(_certainly_leafless(hs, w, h).sum()) >= 8)
    return hs, w, h, _oracle.render(hs, w, h, 64, 1)


def test_sky_leafless_and_triangleless_tiles(rt, helmet_frame):
    """all three kinds of batch tile in one frame, their served paths within the host model's bounds (tests/_triangleless.py)"""
    from tests import _triangleless as tl
    hs, w, h, want = helmet_frame
    assert (w, h) == (80, 45)
    s = 64
    got = rt.render_frame(hs, w, h, s, 1, want_accum=True)
    served = _served(rt)
    print(f"helmet {w} x {h}: {served}")
    _same_as_oracle(got["accum"], got["counters"], want)
    assert served["skipped"] > 0 and served["leafless"] > 0
    # (a sky pixel of this frame whose channel sum reaches 2^32: the accumulators compared above carry into the high word)
    from raytracing_c_amd import tile_classes as tc
    sky = np.asarray(tc.classify_scene(hs, w, h, 1e-2)["root_miss"], bool)
    assert (want["accum"] * np.kron(sky, np.ones((8, 8), bool))[:h, :w, None]).max() >= 1 << 32
    pixels = tl.tile_pixels(w, h)
    assert served["triangleless"] <= served["leafless"] <= s * int(pixels[tl.possibly_served(hs, w, h)].sum())
    assert served["triangleless"] <= s * int(pixels[tl.possibly_triangleless(hs, w, h)].sum())
    clean = tl.nan_free(hs, w, h, tl.certainly_triangleless(hs, w, h), s)          # (whole tiles, no hand-over)
    assert served["triangleless"] >= s * int(pixels[clean].sum())


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


def test_hand_over_with_units_in_hand(rt, oracle):
    """a scene 1e5 units from the origin: the first batch of every batch tile hands over to the general loop, which consumes the
    units the batch loop grabbed and every later one"""
    from tests._far_scene import translated_spheres
    served = _frame_and_oracle(rt, translated_spheres(1e5), 64, 64, 64, 2)
    assert served == dict(triangleless=0, leafless=0, skipped=0)


def test_sample_window(rt, oracle, spheres):
    """rt_render_accumulate on samples [3, 103) of 128: 64 samples per unit, the window ends inside the second sample block"""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _oracle
    w, h, s, b, first, count = 64, 64, 128, 2, 3, 100
    assert _units(count) == (128, 64)
    want = _oracle.render(spheres, w, h, s, b, sample_range=(first, count))
    d = rt.lib.rt_scene_upload(C.byref(spheres.scene))
    assert d, rt.last_error()
    try:
        accum = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
        p = abi.RT_Render_Params(width=w, height=h, samples=s, max_bounces=b, seed=SEED, rank=0, world=1, sample_first=first, sample_count=count)
        assert rt.lib.rt_render_accumulate(d, C.byref(p), accum.data_ptr(), None) == 0, rt.last_error()
        torch.cuda.synchronize()
        got = accum.cpu().numpy().view(np.uint64)
        counters = rt.render.get_counters()
        assert _u64(rt, "rt_get_leafless_paths") + _u64(rt, "rt_get_skipped_root_visits") > 0
    finally:
        rt.lib.rt_scene_release(d)
    assert counters.paths == w * h * count
    _same_as_oracle(got, counters, want)
