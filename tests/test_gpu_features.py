"""First-hit feature buffers on the GPU (rt_render_features, rt_render_accumulate_features, rt_resolve_features; rt_features.hip)
against the CPU oracle (tests/_features.py): all ten u64 sums of every pixel equal, the f32 planes equal to their resolve, bit
for bit -- textured random scene with ragged image and texture sizes, back faces passed through at the price of an iteration,
a depth-0 scene and a model, a buffer filled progressively, and no effect on frames, queries and their counters."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANES = ("coverage", "albedo", "normal", "position")


def _same(got, want_sums, samples):
    from tests import _features as F
    assert got["sums"].dtype == np.uint64 and got["sums"].shape == want_sums.shape
    diff = np.argwhere(got["sums"] != want_sums)
    assert len(diff) == 0, (len(diff), diff[:4].tolist())
    want = F.resolve(want_sums, samples)
    for k in PLANES:
        assert got[k].dtype == np.float32 and got[k].tobytes() == want[k].tobytes(), k


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def passthrough():
    from tests import _features as F
    return F.passthrough_scene()


def test_textured_random_scene(rt, oracle):
    """Albedo and normal textures of ragged sizes, six materials, duplicated and degenerate triangles; 40 x 24 is no multiple of
    the 8-pixel tile or the 32-pixel chunk; with 4 samples a unit is 16 pixels x 4 lanes."""
    from tests import _features as F
    from tests.test_gpu_random_scenes import make_scene
    hs = make_scene(6, 400)
    w, h, s, b = 40, 24, 4, 8
    want = F.expected_cached("random6", hs, w, h, s, b)
    cov = want["sums"][..., 0] >> np.uint64(32)
    assert int(((cov > 0) & (cov < s)).sum()) >= 20                  # edges: pixels whose samples disagree
    assert want["textured"] > 0 and want["untextured"] > 0 and want["misses"] > 0
    _same(rt.render_features(hs, w, h, s, b), want["sums"], s)


def test_back_faces_are_passed_through_at_the_price_of_an_iteration(rt, oracle, passthrough):
    from tests import _features as F, _oracle
    hs = passthrough
    w, h, s = 16, 16, 2
    want = {b: F.expected_cached("passthrough", hs, w, h, s, b) for b in (1, 2, 3)}
    cov = {b: want[b]["sums"][..., 0] >> np.uint64(32) for b in want}
    one_back = (cov[2] == s) & (cov[1] == 0)                         # behind one back face
    two_back = (cov[3] == s) & (cov[2] == 0)                         # behind two
    sky = cov[3] == 0
    assert one_back.sum() >= 20 and two_back.sum() >= 20 and sky.sum() >= 20
    assert (cov[1] == 0).all()                                       # at 1 nothing behind a back face is covered
    # on the oracle's side: with terminating shaders rays - paths counts the pass-throughs
    rec = F.Recorder()
    cb, cfg = F.with_procs(hs, rec)
    img = np.zeros((h, w, 3), np.uint8)
    image = _oracle.abi.Image()
    image.components, image.pixel_type, image.width, image.stride, image.height = 3, 0, w, w, h
    image.pixels.data, image.pixels.len = img.ctypes.data, img.size
    cnt = _oracle.Oracle_Counters()
    assert oracle.oracle_render(C.byref(cb.scene), C.byref(image), s, 3, C.byref(cfg), None, None, C.byref(cnt)) == 0
    assert cnt.rays - cnt.paths > 0
    for b in (1, 2, 3):
        got = rt.render_features(hs, w, h, s, b)
        _same(got, want[b]["sums"], s)
        assert (got["coverage"][one_back] == (1.0 if b >= 2 else 0.0)).all(), b
        assert (got["coverage"][two_back] == (1.0 if b >= 3 else 0.0)).all(), b
        assert (got["coverage"][sky] == 0.0).all() and (got["position"][sky] == 0.0).all()
    # max_bounces = 0: the loop of raytracer.c:512 runs zero times
    got = rt.render_features(hs, w, h, s, 0)
    assert not got["sums"].any() and not got["coverage"].any()


def test_depth_zero_scene_and_model(rt, oracle):
    from raytracing_c_amd.configs import load_config
    from tests import _features as F
    from tests.test_gpu_random_scenes import make_scene
    hs = make_scene(2, 8)
    assert hs.depth == 0 and hs.n_input_triangles <= 8               # one leaf group, no node (oracle.h D3)
    w, h, s, b = 32, 32, 2, 4
    want = F.expected_cached("random2", hs, w, h, s, b)
    assert want["hits"] > 0 and want["misses"] > 0
    _same(rt.render_features(hs, w, h, s, b), want["sums"], s)
    hs, _ = load_config("spheres")
    want = F.expected_cached("spheres", hs, w, h, s, b)
    assert want["hits"] > 100 and want["misses"] > 100
    got = rt.render_features(hs, w, h, s, b)
    _same(got, want["sums"], s)
    assert (got["position"] < 0).any() and (got["position"] > 0).any()      # the signed channel carries both signs


def test_progressive_fill_on_the_device_level(rt, oracle, passthrough):
    """sample_first / sample_count: (0, 3) + (3, 5) into one buffer = one call with 8 samples = the oracle's 8 samples; the
    samples of a pixel are then 4 + 8 lanes of a unit, 8 lanes of a unit."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _features as F
    hs = passthrough
    w, h, s, b = 16, 16, 8, 3
    want = F.expected_cached("passthrough", hs, w, h, s, b)
    d = rt.lib.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error()
    try:
        def run(ranges):
            sums = torch.zeros((h, w, 10), dtype=torch.int64, device="cuda")
            for first, count in ranges:
                p = abi.RT_Render_Params(width=w, height=h, samples=s, max_bounces=b, world=1, sample_first=first, sample_count=count)
                assert rt.lib.rt_render_accumulate_features(d, C.byref(p), sums.data_ptr(), None) == 0, rt.last_error()
            planes = [torch.full((h, w) if k == 0 else (h, w, 3), 7.0, dtype=torch.float32, device="cuda") for k in range(4)]
            p = abi.RT_Render_Params(width=w, height=h, samples=s, max_bounces=b, world=1)
            assert rt.lib.rt_resolve_features(C.byref(p), sums.data_ptr(), *[t.data_ptr() for t in planes], None) == 0, rt.last_error()
            torch.cuda.synchronize()
            out = dict(sums=sums.cpu().numpy().view(np.uint64))
            out.update({k: t.cpu().numpy() for k, t in zip(PLANES, planes)})
            return out
        whole = run([(0, 0)])
        parts = run([(0, 3), (3, 5)])
        _same(whole, want["sums"], s)
        _same(parts, want["sums"], s)
        part = run([(3, 5)])                                         # ... and a part alone is the oracle's part
        assert np.array_equal(part["sums"], F.expected_cached("passthrough", hs, w, h, s, b, (3, 5))["sums"])
    finally:
        rt.lib.rt_scene_release(d)


def _camera_rays(hs, n):
    rng = np.random.default_rng(3)
    rays = np.zeros((n, 6), np.float32)
    rays[:, :3] = (0.0, 0.0, 3.5)
    rays[:, 3:] = rng.normal(size=(n, 3)) * (0.4, 0.4, 0.1) + (0.0, 0.0, -1.0)
    return rays


def test_frames_and_queries_are_not_affected(rt, oracle, passthrough):
    from tests import _features as F
    hs = passthrough
    w, h, s, b = 16, 16, 2, 3
    want = F.expected_cached("passthrough", hs, w, h, s, b)
    rays = _camera_rays(hs, 500)

    def frame_and_query():
        f = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
        q = rt.closest_hits(hs, rays)
        return f["image"].tobytes(), f["accum"].tobytes(), f["counters"], q.tobytes(), rt.get_query_counters()
    before = frame_and_query()
    _same(rt.render_features(hs, w, h, s, b), want["sums"], s)
    assert rt.get_query_counters() == before[4]                      # (the pass borrows a slot of the query ring, not its counters)
    assert rt.render.get_counters() == before[2]
    assert frame_and_query() == before
    # a feature pass while a frame is in flight on a lane
    ticket, pixels, keep = rt.frame_begin(hs, 48, 40, 4, 4, seed=7)
    got = rt.render_features(hs, w, h, s, b)
    counters = rt.frame_end(ticket)
    _same(got, want["sums"], s)
    assert pixels.tobytes() == before[0] and counters == before[2]


def test_python_wrapper_equals_the_c_entry_point(rt, oracle, passthrough):
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _features as F
    hs = passthrough
    w, h, s, b = 16, 16, 2, 3
    want = F.expected_cached("passthrough", hs, w, h, s, b)
    py = rt.render_features(hs, w, h, s, b)
    fp = C.POINTER(C.c_float)
    # the C entry point, planes one at a time and without the sums, then the sums alone
    for k in PLANES:
        plane = np.full(py[k].shape, 7.0, np.float32)
        out = abi.RT_Features(**{k: plane.ctypes.data_as(fp)})
        assert rt.lib.rt_render_features(C.byref(hs.scene), w, h, s, b, C.byref(out), None) == 0, rt.last_error()
        assert plane.tobytes() == py[k].tobytes(), k
    sums = np.zeros((h, w, 10), np.uint64)
    assert rt.lib.rt_render_features(C.byref(hs.scene), w, h, s, b, None, sums.ctypes.data) == 0, rt.last_error()
    assert np.array_equal(sums, py["sums"]) and np.array_equal(sums, want["sums"])


def test_an_edit_nobody_reported_is_seen_by_the_next_pass(rt, oracle):
    """rt_render_features runs through the frame path's scene check: vertices moved in place without rt_scene_touch -- outside the
    few bytes the per-call stamp samples (8 runs of 512 bytes per block, rt_hip.h "a bounded sample") -- are found by the full
    content check behind the pass, which is then traced again from a fresh copy."""
    from raytracing_c_amd.configs import load_config
    from tests import _features as F
    from tests.test_gpu_query import _bbox, _oracle_trace
    hs, _ = load_config("spheres")
    w, h, s, b = 64, 48, 4, 4
    sc = C.byref(hs.scene)
    first = F.expected(hs, w, h, s, b)["sums"]
    _same(rt.render_features(hs, w, h, s, b), first, s)
    # triangles the camera sees: the oracle's first hits of rays through a grid on the image plane
    m = hs.scene.camera.view_matrix.rows
    M = np.array([[m[i][j] for j in range(4)] for i in range(3)], np.float64)
    gx, gy = np.meshgrid(np.linspace(-0.4, 0.4, 96), np.linspace(-0.3, 0.3, 72))
    d = np.stack([gx.ravel(), gy.ravel(), -np.full(gx.size, float(hs.scene.camera.focal_length))], 1)
    rays = np.zeros((len(d), 6), np.float32)
    rays[:, :3] = M[:, 3]
    rays[:, 3:] = d @ M[:, :3].T
    seen, _ = _oracle_trace(oracle, hs, np.ascontiguousarray(rays))
    ids = np.unique(seen["triangle"][seen["triangle"] >= 0])
    assert len(ids) > 100
    T = hs.scene.triangles
    n = int(T.len)
    zs = [np.ctypeslib.as_array(T.z[k], (n,)) for k in range(3)]
    saved = [z.copy() for z in zs]
    lo, hi = _bbox(hs)
    shift = np.float32(0.25 * (hi[2] - lo[2]))
    runs = [((n * 4 - 512) * k // 7 & ~7) // 4 for k in range(8)]
    k0 = next(int(i) for i in ids[len(ids) // 4:] if all(i + 64 <= r or i >= r + 128 for r in runs))
    try:
        for z in zs:
            z[k0:k0 + 64] += shift
        edited = F.expected(hs, w, h, s, b)["sums"]
        assert int((edited != first).any(axis=2).sum()) >= 20, "the edit must change what the camera sees"
        _same(rt.render_features(hs, w, h, s, b), edited, s)                # no rt_scene_touch
    finally:
        for k in range(3):
            zs[k][:] = saved[k]
            assert rt.lib.rt_scene_touch(sc, zs[k].ctypes.data, n * 4) in (0, 1), rt.last_error()
    _same(rt.render_features(hs, w, h, s, b), first, s)
