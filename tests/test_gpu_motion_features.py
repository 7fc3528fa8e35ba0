"""THE MOTION on the GPU (rt_scene_keep_geometry, rt_render_features_motion, rt_render_accumulate_features_motion,
rt_resolve_motion; rt_features_motion_kernel) against the CPU oracle chain of tests/_motion.py: all three motion sums and all ten
ordinary sums of every pixel equal, bit for bit -- soups of 65 and 513 triangles from both builders, kept at their first geometry and
refitted on the GPU once and twice; the pass-through scene with its front quads displaced; 21 x 13 (ragged tiles) at 1, 4 and 5
samples (eight sample lanes, five valid), 8 x 8 at 70 samples (two sample blocks); a sample range split on the device level; no
kept geometry; kept geometry gone with the copy; refusals."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 21, 13, 4


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


_scenes = {}


def _soup_scene(rt, n, builder, twice=False):
    """(name, hs, kept tiles, current tiles): the soup built at P, its geometry kept, refitted on the GPU to moved(amount=0.05) --
    `twice`: and then to another displacement, after the one keep.  Once per process; the tests only render it."""
    from tests import _motion as M, _refit
    key = (n, builder, twice)
    if key not in _scenes:
        soup = _refit.soup(n)
        hs = soup.build(builder)
        assert not hs.has_kept_geometry
        kept = M.leaf_tiles(hs)
        hs.keep_geometry()
        assert hs.has_kept_geometry
        hs.refit(*soup.moved(amount=0.05))
        if twice:
            hs.refit(*soup.moved(seed=7, amount=0.05))
        assert hs.has_kept_geometry                                  # (the refit kept the copy, and the snapshot with it)
        _scenes[key] = (f"soup{n}-{builder}{'-twice' if twice else ''}", hs, kept, M.leaf_tiles(hs))
    return _scenes[key]


def _passthrough_scene(rt):
    from tests import _motion as M
    if "passthrough" not in _scenes:
        hs, P = M.displaced_passthrough()
        kept = M.leaf_tiles(hs)
        hs.keep_geometry()
        hs.refit(P)
        _scenes["passthrough"] = ("passthrough", hs, kept, M.leaf_tiles(hs))
    return _scenes["passthrough"]


def _check(rt, scene, w, h, s, b):
    from tests import _features, _motion as M
    name, hs, kept, cur = scene
    ch = M.chain(hs, w, h, s, b)
    want_ten = _features.expected_cached("gpu-motion-" + name, hs, w, h, s, b)["sums"]
    want = M.expected_motion(ch, cur, kept)
    got = rt.render_features(hs, w, h, s, b, motion=True)
    assert got["motion_sums"].dtype == np.uint64 and got["motion_sums"].shape == (h, w, 3)
    diff = np.argwhere(got["motion_sums"] != want)
    assert len(diff) == 0, (name, len(diff), diff[:4].tolist())
    assert np.array_equal(got["sums"], want_ten), name
    assert np.array_equal(got["sums"], rt.render_features(hs, w, h, s, b)["sums"]), name      # ... and the plain pass's
    assert got["motion"].tobytes() == M.resolve_motion(want, s).tobytes(), name
    planes = _features.resolve(want_ten, s)
    for k in ("coverage", "albedo", "normal", "position"):
        assert got[k].tobytes() == planes[k].tobytes(), (name, k)
    return want, want_ten


@pytest.mark.parametrize("samples", [1, 4, 5])
@pytest.mark.parametrize("builder", ["reference", "sah"])
@pytest.mark.parametrize("n", [65, 513])
def test_soups_kept_and_refitted(rt, oracle, n, builder, samples):
    want, ten = _check(rt, _soup_scene(rt, n, builder), W, H, samples, BOUNCES)
    covered = ten[..., 0] != 0
    assert ((want != 0).any(axis=2) & covered).sum() * 4 >= covered.sum() >= 20


def test_refitted_twice_after_one_keep(rt, oracle):
    """the motion is measured against what was KEPT, not against the geometry before the last refit"""
    from tests import _motion as M
    scene = _soup_scene(rt, 65, "reference", twice=True)
    want, _ = _check(rt, scene, W, H, 4, BOUNCES)
    once = _soup_scene(rt, 65, "reference")
    assert not np.array_equal(scene[3], once[3]) and np.array_equal(scene[2], once[2]) and want.any()


def test_two_sample_blocks(rt, oracle):
    """8 x 8 at 70 samples: the shift is capped at 6, a pixel's samples are two units of 64 lanes, the second with six valid"""
    want, _ = _check(rt, _soup_scene(rt, 513, "reference"), 8, 8, 70, BOUNCES)
    assert want.any()


@pytest.mark.parametrize("bounces", [1, 3])
def test_pass_through_and_motion_meet(rt, oracle, bounces):
    """a back face that is passed through adds nothing; the front quad behind it has moved"""
    want, ten = _check(rt, _passthrough_scene(rt), W, H, 4, bounces)
    assert want.any() == (bounces == 3)


def test_a_sample_range_adds_up_on_the_device_level(rt, diag, oracle):
    """sample_first / sample_count on the cached copy the refit deformed (the diagnostic library names it): (0, 2) + (2, 3) into
    one pair of buffers = one call with 5 samples = the oracle chain; a part alone is the chain's part; rt_resolve_motion."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _features, _motion as M, _refit
    soup = _refit.soup(65)
    hs = soup.build("reference")
    smap = hs.slot_map()
    kept = M.leaf_tiles(hs)
    assert diag.rt_scene_keep_geometry(C.byref(hs.scene)) == 0, rt.last_error(diag)
    tri = hs.source_triangles.copy()
    P, N, UV = soup.moved(amount=0.05)
    tri["positions"], tri["normals"], tri["tex_coords"] = P, N, UV
    assert _refit.call_refit_on(diag, hs, tri, smap, "scene_refit_gpu") == 0, rt.last_error(diag)
    cur = M.leaf_tiles(hs)
    d = diag.rt_diag_cached_scene(C.byref(hs.scene))
    assert d and diag.rt_scene_has_kept_geometry(C.byref(hs.scene)) == 1
    assert diag.rt_set_camera(d, C.byref(hs.scene.camera)) == 0
    w, h, s, b = W, H, 5, BOUNCES
    try:
        def run(ranges):
            sums = torch.zeros((h, w, 10), dtype=torch.int64, device="cuda")
            msums = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
            for first, count in ranges:
                p = abi.RT_Render_Params(width=w, height=h, samples=s, max_bounces=b, world=1, sample_first=first, sample_count=count)
                assert diag.rt_render_accumulate_features_motion(d, C.byref(p), sums.data_ptr(), msums.data_ptr(), None) == 0, rt.last_error(diag)
            motion = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
            p = abi.RT_Render_Params(width=w, height=h, samples=s, max_bounces=b, world=1)
            assert diag.rt_resolve_motion(C.byref(p), msums.data_ptr(), motion.data_ptr(), None) == 0, rt.last_error(diag)
            torch.cuda.synchronize()
            return sums.cpu().numpy().view(np.uint64), msums.cpu().numpy().view(np.uint64), motion.cpu().numpy()
        want = M.expected_motion(M.chain(hs, w, h, s, b), cur, kept)
        ten = _features.expected_cached("gpu-motion-split", hs, w, h, s, b)["sums"]
        for ranges in ([(0, 0)], [(0, 2), (2, 3)]):
            sums, msums, motion = run(ranges)
            assert np.array_equal(msums, want) and np.array_equal(sums, ten), ranges
            assert motion.tobytes() == M.resolve_motion(want, s).tobytes()
        part = run([(2, 3)])
        want_part = M.expected_motion(M.chain(hs, w, h, s, b, (2, 3)), cur, kept)
        assert np.array_equal(part[1], want_part) and want_part.any() and not np.array_equal(want_part, want)
    finally:
        diag.rt_scene_invalidate(C.byref(hs.scene))


def test_no_kept_geometry_is_zero_motion_and_the_snapshot_goes_with_the_copy(rt, oracle):
    from tests import _refit
    soup = _refit.soup(65)
    hs = soup.build("reference")
    w, h, s, b = W, H, 4, BOUNCES
    assert not hs.has_kept_geometry                                  # (asks no device: nothing is cached yet)
    first = rt.render_features(hs, w, h, s, b, motion=True)          # the first frame of a sequence
    assert first["sums"][..., 0].any() and not first["motion_sums"].any() and not first["motion"].view(np.uint32).any()
    hs.keep_geometry()
    assert hs.has_kept_geometry
    still = rt.render_features(hs, w, h, s, b, motion=True)          # kept and unmoved: +0 bit for bit
    assert not still["motion_sums"].any() and np.array_equal(still["sums"], first["sums"])
    hs.refit(*soup.moved(amount=0.05))
    assert rt.render_features(hs, w, h, s, b, motion=True)["motion_sums"].any()
    rt.lib.rt_scene_invalidate(C.byref(hs.scene))
    assert not hs.has_kept_geometry
    again = rt.render_features(hs, w, h, s, b, motion=True)          # a new copy: no snapshot, zero motion
    assert not again["motion_sums"].any() and again["sums"][..., 0].any() and not hs.has_kept_geometry
    # a refit that falls back to scene_refit drops the copies, and the kept geometry with them
    hs.keep_geometry()
    hs.refit(*soup.moved(seed=3, amount=0.05), device="cpu")
    assert not hs.has_kept_geometry
    # an explicitly uploaded scene keeps on the caller's stream
    d = rt.lib.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error()
    try:
        assert rt.lib.rt_device_scene_keep_geometry(d, None) == 0, rt.last_error()
    finally:
        rt.lib.rt_scene_release(d)


def test_refusals_leave_the_outputs_untouched(rt):
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _refit
    hs = _refit.soup(65).build("reference")
    lib = rt.lib
    sums = np.full((H, W, 10), 7, np.uint64)
    msums = np.full((H, W, 3), 7, np.uint64)
    motion = np.full((H, W, 3), 7, np.float32)

    def refused(rc, text):
        assert rc != 0 and text in rt.last_error(), rt.last_error()
        assert (sums == 7).all() and (msums == 7).all() and (motion == 7).all()

    scene = C.byref(hs.scene)
    args = (None, sums.ctypes.data, motion.ctypes.data, msums.ctypes.data)
    refused(lib.rt_render_features_motion(None, W, H, 4, 4, *args), "scene is NULL")
    refused(lib.rt_render_features_motion(scene, 0, H, 4, 4, *args), "image size")
    refused(lib.rt_render_features_motion(scene, W, H, 0, 4, *args), "samples must be positive")
    refused(lib.rt_render_features_motion(scene, W, H, 4, -1, *args), "max_bounces")
    refused(lib.rt_render_features_motion(scene, W, H, 4, 4, None, None, None, None), "no output is wanted")
    p = abi.RT_Render_Params(width=W, height=H, samples=4, max_bounces=4, world=1)
    one = 0x1000                                                      # (never dereferenced: every call below is refused first)
    refused(lib.rt_render_accumulate_features_motion(None, C.byref(p), one, one, None), "device scene is NULL")
    refused(lib.rt_resolve_motion(C.byref(p), None, one, None), "d_motion_sums is NULL")
    refused(lib.rt_resolve_motion(C.byref(p), one, None, None), "d_motion is NULL")
    refused(lib.rt_resolve_motion(None, one, one, None), "render params are NULL")
    refused(lib.rt_scene_keep_geometry(None), "scene is NULL")
    refused(lib.rt_device_scene_keep_geometry(None, None), "device scene is NULL")
    d = lib.rt_scene_upload(scene)
    assert d, rt.last_error()
    try:
        refused(lib.rt_render_accumulate_features_motion(d, C.byref(p), one, None, None), "d_motion_sums is NULL")
        refused(lib.rt_render_accumulate_features_motion(d, C.byref(p), None, one, None), "d_sums is NULL")
        bad = abi.RT_Render_Params(width=W, height=H, samples=4, max_bounces=4, world=1, sample_first=3, sample_count=2)
        refused(lib.rt_render_accumulate_features_motion(d, C.byref(bad), one, one, None), "sample range")
    finally:
        lib.rt_scene_release(d)
    assert lib.rt_scene_has_kept_geometry(None) == 0
