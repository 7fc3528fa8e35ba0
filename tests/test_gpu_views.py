"""rt_render_views / rt_render_accumulate_views (include/rt_hip.h): K views of one scene in ONE launch of the path kernel give
every view the pixels, linear values and radiance sums of rt_render_frame with that view's camera and seed, bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = [0x1234ABCD, 7, 0xDEADBEEF, 99, 12345, 0x51D3]


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _camera(matrix, yfov):
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.scene import set_camera
    cam = abi.Camera()
    set_camera(cam, matrix, yfov)
    return cam


def _copy(cam):
    from raytracing_c_amd import ctypes_abi as abi
    out = abi.Camera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(abi.Camera))
    return out


def _rot_y(deg):
    a = np.deg2rad(deg)
    r = np.eye(4, dtype=np.float32)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return r


def _matrix(cam):
    return np.array([[cam.view_matrix.rows[i][j] for j in range(4)] for i in range(4)], np.float32)


def _five_views(hs):
    """the file camera, two orbits about the world's y axis, one turned away from the model, one with another fov"""
    file_cam = hs.scene.camera
    m, fov = _matrix(file_cam), float(file_cam.fov)
    return [_copy(file_cam),
            _camera(_rot_y(35.0) @ m, fov),
            _camera(_rot_y(-70.0) @ m, fov),
            _camera(m @ _rot_y(180.0), fov),          # looks away from the model: sky tiles only
            _camera(m, fov * 0.6)]


def _frame_as(rt, hs, cam, w, h, s, b, seed, **kw):
    """rt_render_frame with scene->camera = cam and rt_set_seed(seed); the scene's camera is restored"""
    saved = _copy(hs.scene.camera)
    hs.scene.camera = cam
    try:
        r = rt.render_frame(hs, w, h, s, b, seed=seed, **kw)
        r["skipped"] = _skipped(rt)
        return r
    finally:
        hs.scene.camera = saved


def _skipped(rt):
    v = C.c_uint64()
    assert rt.lib.rt_get_skipped_root_visits(C.byref(v)) == 0, rt.last_error()
    return int(v.value)


def _ctuple(c):
    return (c.paths, c.rays, c.node_visits, c.leaf_visits, c.shades, c.backgrounds, c.textured)


@pytest.mark.parametrize("name", ["spheres", "helmet", "quad", "tower"])
@pytest.mark.parametrize("w,h", [(45, 31), (100, 70), (128, 96)])
def test_every_view_equals_its_own_frame(rt, name, w, h):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config(name)
    s, b = 4, 3
    cams = _five_views(hs)
    seeds = SEEDS[:5]
    got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_linear=True, want_accum=True)
    batch_counters, batch_skipped = _ctuple(got[0]["counters"]), _skipped(rt)
    want = [_frame_as(rt, hs, c, w, h, s, b, sd, want_linear=True, want_accum=True) for c, sd in zip(cams, seeds)]
    for v, (g, r) in enumerate(zip(got, want)):
        assert np.array_equal(g["accum"], r["accum"]), f"view {v}: radiance sums"
        assert np.array_equal(g["linear"], r["linear"]), f"view {v}: linear values"
        assert np.array_equal(g["image"], r["image"]), f"view {v}: image"
    assert batch_counters == tuple(map(sum, zip(*[_ctuple(r["counters"]) for r in want])))
    assert batch_skipped == sum(r["skipped"] for r in want)
    if hs.scene.bvh.depth > 0:                # (a one-leaf scene has no root node to skip)
        assert want[3]["skipped"] > 0, "the view turned away from the model has sky tiles"


def test_two_views_equal_the_oracle(rt, oracle):
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    hs, _ = load_config("spheres")
    w, h, s, b = 40, 36, 4, 3
    cams = _five_views(hs)[1:3]
    seeds = [5, 0xBEEF]
    got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_accum=True)
    saved = _copy(hs.scene.camera)
    try:
        for v, (cam, sd) in enumerate(zip(cams, seeds)):
            hs.scene.camera = cam
            want = _oracle.render(hs, w, h, s, b, seed=sd)
            assert np.array_equal(got[v]["accum"], want["accum"]), f"view {v}"
            assert np.array_equal(got[v]["image"], want["image"]), f"view {v}"
    finally:
        hs.scene.camera = saved


def test_a_batch_is_one_launch(rt):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    cams = _five_views(hs) + [_camera(_rot_y(120.0) @ _matrix(hs.scene.camera), float(hs.scene.camera.fov))]
    rt.lib.rt_kernel_timing_reset()
    rt.render_views(hs, cams, 64, 48, 4, 3, seeds=SEEDS)
    n = C.c_int32()
    ms = rt.lib.rt_kernel_timing_mean_ms(C.byref(n))
    assert n.value == 1 and ms > 0.0
    t = rt.abi.RT_Frame_Timing()
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0
    assert t.gpu_path_ms > 0.0 and t.total_ms > 0.0


def test_one_view_and_seeds(rt):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("helmet")
    w, h, s, b = 72, 40, 4, 4
    m, fov = _matrix(hs.scene.camera), float(hs.scene.camera.fov)
    one = rt.render_views(hs, [(m, fov)], w, h, s, b, seeds=[77], want_accum=True)[0]
    ref = _frame_as(rt, hs, _camera(m, fov), w, h, s, b, 77, want_accum=True)
    assert np.array_equal(one["accum"], ref["accum"]) and np.array_equal(one["image"], ref["image"])
    same = rt.render_views(hs, [(m, fov), (m, fov)], w, h, s, b, seeds=[77, 77])
    assert np.array_equal(same[0]["image"], same[1]["image"])
    assert np.array_equal(same[0]["image"], one["image"])
    diff = rt.render_views(hs, [(m, fov), (m, fov)], w, h, s, b, seeds=[77, 78])
    assert np.array_equal(diff[0]["image"], one["image"])
    assert not np.array_equal(diff[0]["image"], diff[1]["image"])


@pytest.mark.parametrize("name,w,h,k,s", [("spheres", 256, 256, 4, 6), ("helmet", 64, 48, 3, 96)])
def test_progressive_device_level_batches(rt, name, w, h, k, s):
    """rt_render_accumulate_views over two sample ranges (and over two ranks) sums to one call; rt_resolve per view gives the
    images of rt_render_views.  spheres 256^2 x 6 spp: units of 4 samples, 4096 tiles, units taken in pairs (grab_max = 2)."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.configs import load_config
    from raytracing_c_amd.render import make_views
    hs, _ = load_config(name)
    b = 4
    cams = _five_views(hs)[:k]
    seeds = SEEDS[:k]
    views = make_views(cams, seeds)
    d = rt.lib.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error()
    try:
        def run(ranges, world=1):
            acc = torch.zeros((k, h, w, 3), dtype=torch.int64, device="cuda")
            for rank in range(world):
                for first, count in ranges:
                    p = abi.RT_Render_Params(w, h, s, b, 0xFFFF, rank, world, 0, 0, first, count)
                    assert rt.lib.rt_render_accumulate_views(d, C.byref(p), k, views, acc.data_ptr(), None) == 0, rt.last_error()
            torch.cuda.synchronize()
            return acc

        whole = run([(0, 0)])
        halves = run([(0, s // 2), (s // 2, s - s // 2)])
        ranks = run([(0, 0)], world=2)
        assert torch.equal(whole, halves)
        assert torch.equal(whole, ranks)
        p = abi.RT_Render_Params(w, h, s, b, 0, 0, 1, 0, 0, 0, 0)
        want = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_accum=True)
        for v in range(k):
            assert np.array_equal(whole[v].cpu().numpy().view(np.uint64), want[v]["accum"]), f"view {v}"
            image = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            ptr = whole.data_ptr() + v * h * w * 3 * 8
            assert rt.lib.rt_resolve(C.byref(p), ptr, None, image.data_ptr(), None, None) == 0, rt.last_error()
            torch.cuda.synchronize()
            assert np.array_equal(image.cpu().numpy(), want[v]["image"]), f"view {v}"
    finally:
        rt.lib.rt_scene_release(d)


def test_frames_and_batches_interleaved(rt):
    """single frames, batches and a frame in flight of the same scene and shape: separate launch states and schedules"""
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    w, h, s, b = 96, 64, 4, 3
    cams = _five_views(hs)[:3]
    seeds = SEEDS[:3]
    ref_views = [_frame_as(rt, hs, c, w, h, s, b, sd)["image"] for c, sd in zip(cams, seeds)]
    ref_file = rt.render_frame(hs, w, h, s, b, seed=SEEDS[4])["image"]
    for _ in range(2):
        got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds)
        assert all(np.array_equal(g["image"], r) for g, r in zip(got, ref_views))
        assert np.array_equal(rt.render_frame(hs, w, h, s, b, seed=SEEDS[4])["image"], ref_file)
    ticket, out, keep = rt.frame_begin(hs, w, h, s, b, seed=SEEDS[4])
    got = rt.render_views(hs, cams[::-1], w, h, s, b, seeds=seeds[::-1])
    rt.frame_end(ticket)
    assert np.array_equal(out, ref_file)
    assert all(np.array_equal(g["image"], r) for g, r in zip(got, ref_views[::-1]))
    assert np.array_equal(rt.render_views(hs, cams[:1], w, h, s, b, seeds=seeds[:1])[0]["image"], ref_views[0])


def _textured_quad():
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import Material, build_scene
    pos = np.array([[[-1, -1, 0], [1, -1, 0], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0]]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (2, 3, 1))
    uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], np.float32)
    tex = (np.arange(4 * 4 * 3, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(4, 4, 3)
    cam = np.eye(4, dtype=np.float32)
    cam[2, 3] = 2.5
    mats = [Material(base_color=(0.9, 0.8, 0.7), roughness=0.6, texture_albedo=0)]
    return build_scene(pos, nrm, uv, np.zeros(2, np.int32), mats, [tex], cam, 1.0, procedural_background(64, 32))


def test_in_place_scene_edits_are_seen_by_the_next_batch(rt, oracle):
    from tests import _oracle
    hs = _textured_quad()
    w, h, s, b = 48, 32, 4, 3
    m = _matrix(hs.scene.camera)
    cams = [_copy(hs.scene.camera), _camera(_rot_y(25.0) @ m, 1.0)]
    seeds = [3, 4]

    def oracle_views():
        saved = _copy(hs.scene.camera)
        try:
            out = []
            for cam, sd in zip(cams, seeds):
                hs.scene.camera = cam
                out.append(_oracle.render(hs, w, h, s, b, seed=sd)["image"])
            return out
        finally:
            hs.scene.camera = saved

    first = [g["image"] for g in rt.render_views(hs, cams, w, h, s, b, seeds=seeds)]
    assert all(np.array_equal(g, r) for g, r in zip(first, oracle_views()))
    hs.materials[0].base_color.x = 0.1                      # material record edited in place
    hs.soa_array()[6:9, :2] -= 0.25                         # both triangles moved back (z)
    second = [g["image"] for g in rt.render_views(hs, cams, w, h, s, b, seeds=seeds)]
    assert all(np.array_equal(g, r) for g, r in zip(second, oracle_views()))
    assert not any(np.array_equal(a, c) for a, c in zip(first, second))


def test_multi_device_setting_is_refused(rt):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    cams = _five_views(hs)[:2]
    try:
        assert rt.lib.rt_set_devices(2, 1) == 0
        rt.lib.rt_clear_error()
        with pytest.raises(RuntimeError, match="one device"):
            rt.render_views(hs, cams, 64, 32, 2, 2)
    finally:
        assert rt.lib.rt_set_devices(1, 0) == 0
    got = rt.render_views(hs, cams, 64, 32, 2, 2, seeds=[1, 2])
    assert np.array_equal(got[0]["image"], _frame_as(rt, hs, cams[0], 64, 32, 2, 2, 1)["image"])


def test_full_size_helmet_six_views(rt):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("helmet")
    w = h = 512
    s, b = 16, 8
    m, fov = _matrix(hs.scene.camera), float(hs.scene.camera.fov)
    cams = [_camera(_rot_y(60.0 * k) @ m, fov) for k in range(6)]         # an orbit in six steps around the model
    seeds = SEEDS
    got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_accum=True)
    for v, (cam, sd) in enumerate(zip(cams, seeds)):
        want = _frame_as(rt, hs, cam, w, h, s, b, sd, want_accum=True)
        assert np.array_equal(got[v]["accum"], want["accum"]), f"view {v}"
        assert np.array_equal(got[v]["image"], want["image"]), f"view {v}"
