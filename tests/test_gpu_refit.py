"""scene_refit_gpu (include/rt_hip.h, csrc/rt_refit.hip): the BVH of a deformed mesh refitted by GPU kernels, in place on the device
copy of the scene.  The host Scene afterwards holds scene_refit's bytes, and the next frame uploads nothing and renders the moved
geometry like the oracle does."""
import ctypes as C

import numpy as np
import pytest

from tests import _refit
from tests._refit import BUILDERS, SHAPES

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    yield rt
    rt.lib.rt_set_devices(1, 0)


def _timing(rt):
    from raytracing_c_amd import ctypes_abi as abi
    t = abi.RT_Frame_Timing()
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0
    return t


def _frame_equals_the_oracle(rt, hs, w, h, s, b, seed=9):
    """one frame; accum and the seven counters against the oracle on the host scene as it is now.  Returns (frame, its timing)."""
    from tests import _oracle
    want = _oracle.render(hs, w, h, s, b, seed=seed)
    got = rt.render_frame(hs, w, h, s, b, seed=seed, want_accum=True)
    t = _timing(rt)
    assert np.array_equal(want["accum"], got["accum"])
    for k in COUNTERS:
        assert want["counters"][k] == getattr(got["counters"], k), k
    return got, t


def _refitted_in_place(rt, hs, w, h, s, b, **moved):
    """frame, refit, frame: the second frame is the oracle's, uploads nothing, the copy verifies; a fresh upload gives the same"""
    first, _ = _frame_equals_the_oracle(rt, hs, w, h, s, b)
    hs.refit(device="gpu", **moved)
    second, t = _frame_equals_the_oracle(rt, hs, w, h, s, b)
    assert t.upload_ms == 0.0
    assert not np.array_equal(first["accum"], second["accum"]), "the deformation must be visible"
    assert rt.lib.rt_scene_verify(C.byref(hs.scene)) == 1
    rt.lib.rt_scene_invalidate(C.byref(hs.scene))
    fresh, t = _frame_equals_the_oracle(rt, hs, w, h, s, b)
    assert t.upload_ms > 0.0
    assert np.array_equal(fresh["accum"], second["accum"])
    assert fresh["counters"] == second["counters"]


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_tris", SHAPES)
def test_gpu_refit_writes_the_bytes_of_the_cpu_refit(rt, n_tris, builder):
    sp = _refit.soup(n_tris)
    gpu, cpu = sp.build(builder), sp.build(builder)
    original = _refit.raw_bytes(gpu)
    gpu.refit(device="gpu")                                           # the identity (and the upload: no copy yet)
    assert _refit.raw_bytes(gpu) == original
    P, N, UV = sp.moved()
    gpu.refit(positions=P, normals=N, uvs=UV, device="gpu")
    cpu.refit(positions=P, normals=N, uvs=UV, device="cpu")
    hg, ng, bg, mg, pg = _refit.scene_bytes(gpu)
    hc, nc, bc, mc, pc = _refit.scene_bytes(cpu)
    assert hg == hc
    assert ng == nc, "BVH nodes differ"
    assert bg == bc, "triangle block differs"
    assert mg == mc and pg == pc, "shader assignment differs"
    assert _refit.raw_bytes(gpu) != original
    assert rt.lib.rt_scene_verify(C.byref(gpu.scene)) == 1            # the copy's fingerprint is the host scene's
    gpu.refit(positions=sp.P, normals=sp.N, uvs=sp.UV, device="gpu")
    assert _refit.raw_bytes(gpu) == original


def test_refit_is_in_place(rt, oracle):
    sp = _refit.soup(513)
    hs = sp.build("reference")
    P, N, UV = sp.moved(amount=0.08)
    _refitted_in_place(rt, hs, 72, 40, 8, 4, positions=P, normals=N, uvs=UV)


def test_refit_of_the_helmet_on_its_sah_tree(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("helmet", builder="sah")
    P = hs.source_triangles["positions"].astype(np.float64)
    extent = float((P.reshape(-1, 3).max(axis=0) - P.reshape(-1, 3).min(axis=0)).max())
    # a smooth displacement, a function of the position alone: shared vertices stay shared
    k = 2.0 * np.pi * 1.5 / extent
    D = 0.04 * extent * np.stack([np.sin(k * P[..., 1]), np.sin(k * P[..., 2] + 1.0), np.cos(k * P[..., 0])], axis=-1)
    _refitted_in_place(rt, hs, 96, 54, 4, 6, positions=(P + D).astype(np.float32))


def test_queries_after_a_refit_equal_the_oracle(rt, oracle):
    from tests.test_gpu_query import _oracle_trace, _rays, _same_hits
    sp = _refit.soup(513)
    hs = sp.build("sah")
    rays = _rays(hs, 20000, np.random.default_rng(11))
    before = rt.closest_hits(hs, rays)                                # (makes the copy the refit then works on)
    _same_hits(_oracle_trace(oracle, hs, rays)[0], before)
    P, N, UV = sp.moved(amount=0.08)
    hs.refit(positions=P, normals=N, uvs=UV, device="gpu")
    want, _ = _oracle_trace(oracle, hs, rays)
    assert int((want["triangle"] >= 0).sum()) > len(rays) // 10
    got = rt.closest_hits(hs, rays)
    _same_hits(want, got)
    assert got.tobytes() != before.tobytes()
    assert rt.lib.rt_scene_verify(C.byref(hs.scene)) == 1


def test_refit_recomputes_the_edge_bound(rt, oracle):
    """The leaf blocks divide instead of using the short reciprocal once an edge component exceeds 2^38 (rt_launch.cpp): the
    copy's bound must follow a refit up AND down, exactly -- a scene blown up to 2^39 times its size and shrunk again."""
    from raytracing_c_amd.loaders import camera_from_trs
    from tests.test_gpu_random_scenes import make_scene
    hs = make_scene(31, 200)
    P0 = hs.source_triangles["positions"].copy()
    w, h, s, b = 72, 40, 8, 4
    small, _ = _frame_equals_the_oracle(rt, hs, w, h, s, b)
    for scale in (2.0 ** 39, 1.0):
        hs.refit(positions=P0 * np.float32(scale), device="gpu")
        hs.set_camera(camera_from_trs((0.1 * scale, 0.2 * scale, 3.5 * scale)), 0.9)
        got, t = _frame_equals_the_oracle(rt, hs, w, h, s, b)
        assert t.upload_ms == 0.0
        assert got["counters"].shades > 0
        rt.lib.rt_scene_invalidate(C.byref(hs.scene))
        fresh, t = _frame_equals_the_oracle(rt, hs, w, h, s, b)
        assert t.upload_ms > 0.0
        assert np.array_equal(fresh["accum"], got["accum"]) and fresh["counters"] == got["counters"]
    assert np.array_equal(got["accum"], small["accum"])


def test_nan_position_is_refitted_by_the_host(rt):
    sp = _refit.soup(65)
    gpu, cpu = sp.build("reference"), sp.build("reference")
    rt.render_frame(gpu, 32, 32, 2, 2)
    assert rt.lib.rt_scene_verify(C.byref(gpu.scene)) == 1
    P, N, UV = sp.moved()
    P[40, 2, 1] = np.nan
    gpu.refit(positions=P, normals=N, uvs=UV, device="gpu")
    cpu.refit(positions=P, normals=N, uvs=UV, device="cpu")
    assert _refit.scene_bytes(gpu) == _refit.scene_bytes(cpu)
    assert rt.lib.rt_scene_verify(C.byref(gpu.scene)) == -1           # the copy was dropped ...
    rt.render_frame(gpu, 32, 32, 2, 2)
    assert _timing(rt).upload_ms > 0.0                                # ... and the next frame uploads


def test_refit_rejections_reach_the_gpu_entry_point(rt):
    """the validation runs on the host before anything is launched: -1, a message, the bytes and the copy as they were"""
    sp = _refit.soup(65)
    hs = sp.build("sah")
    rt.render_frame(hs, 32, 32, 2, 2)
    before = _refit.raw_bytes(hs)
    smap = hs.slot_map().copy()
    smap[7] = smap[9] if hs.source_triangles["shader_data"][7] == hs.source_triangles["shader_data"][9] else hs.n_slots
    rt.lib.rt_clear_error()
    assert _refit.call_refit(hs, hs.source_triangles, smap, "scene_refit_gpu") == -1
    assert "scene_refit" in rt.last_error()
    assert _refit.raw_bytes(hs) == before
    assert rt.lib.rt_scene_verify(C.byref(hs.scene)) == 1


def test_refit_with_rehearsed_devices(rt, oracle):
    """the refit works on slot 0's copy; the copies of the other slots are dropped and uploaded again by their next frame"""
    from tests import _oracle
    sp = _refit.soup(513)
    hs = sp.build("reference")
    w, h, s, b = 96, 64, 4, 4
    P, N, UV = sp.moved(amount=0.08)
    try:
        assert rt.lib.rt_set_devices(3, 1) == 0
        a = rt.render_context(hs, w, h, s, b, n_threads=3)
        assert np.array_equal(a["image"], _oracle.render(hs, w, h, s, b)["image"])
        hs.refit(positions=P, normals=N, uvs=UV, device="gpu")
        many = rt.render_context(hs, w, h, s, b, n_threads=3)
        assert rt.lib.rt_set_devices(1, 0) == 0
        one = rt.render_context(hs, w, h, s, b, n_threads=1)
        assert np.array_equal(many["image"], one["image"])
        assert np.array_equal(one["image"], _oracle.render(hs, w, h, s, b)["image"])
        assert not np.array_equal(one["image"], a["image"])
    finally:
        rt.lib.rt_set_devices(1, 0)


def test_refit_staging_is_counted_and_given_back(rt, diag):
    """the staging of a refit is DevMem like the query staging: kept between calls, released with rt_diag_release_staging"""
    sp = _refit.soup(513)
    hs = sp.build("reference")
    P, N, UV = sp.moved()
    smap = hs.slot_map()                                                # (while the scene still holds the source's bytes)

    def refit(positions):
        tri = hs.source_triangles
        tri["positions"] = positions
        assert _refit.call_refit_on(diag, hs, tri, smap) == 0, rt.last_error(diag)

    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    base = diag.rt_diag_device_bytes_live()
    refit(P)
    held = diag.rt_diag_device_bytes_live() - base
    assert held > 0
    refit(sp.P)
    assert diag.rt_diag_device_bytes_live() - base == held              # warm: nothing more
    diag.rt_scene_invalidate(C.byref(hs.scene))
    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    assert diag.rt_diag_device_bytes_live() == base


@pytest.mark.parametrize("what", ["material", "texel"])
def test_an_unreported_edit_before_a_refit_is_not_absorbed(rt, oracle, what):
    """The refit takes the host bytes as the copy's new reference -- for the nodes and the triangle block, which it wrote on both
    sides.  A material record or a texel edited in place WITHOUT rt_scene_touch must not become part of that reference: the copy is
    dropped, the next frame uploads and shows the edit.  (The positions stay, so what changes in the frame is the edit alone.)"""
    sp = _refit.soup(513)
    hs = sp.build("reference")
    w, h, s, b = 72, 40, 8, 4
    first, _ = _frame_equals_the_oracle(rt, hs, w, h, s, b)
    if what == "material":
        for m in hs.materials:
            m.base_color.x, m.base_color.y, m.base_color.z = 0.05, 0.9, 0.1
    else:
        for arr in hs._image_arrays:
            arr[...] = 255 - arr
    hs.refit(device="gpu")
    second, t = _frame_equals_the_oracle(rt, hs, w, h, s, b)
    assert t.upload_ms > 0.0 or rt.lib.rt_scene_verify(C.byref(hs.scene)) != 1
    assert not np.array_equal(first["accum"], second["accum"]), "the edit must be visible"
    third, t = _frame_equals_the_oracle(rt, hs, w, h, s, b)             # and from here on the copy is kept again
    hs.refit(device="gpu")
    fourth, t = _frame_equals_the_oracle(rt, hs, w, h, s, b)
    assert t.upload_ms == 0.0 and rt.lib.rt_scene_verify(C.byref(hs.scene)) == 1
    assert np.array_equal(fourth["accum"], second["accum"])


def test_gpu_refit_of_a_depth_5_tree(rt):
    """more than 32 768 triangles: level 3 has 4 096 (node, child) lanes, the one level that refit_levels_kernel runs as a launch
    of several workgroups before the top three levels share one"""
    sp = _refit.soup(40000)
    gpu, cpu = sp.build("reference"), sp.build("reference")
    assert gpu.depth == 5 and gpu.n_nodes == 4681
    original = _refit.raw_bytes(gpu)
    P, N, UV = sp.moved()
    gpu.refit(positions=P, normals=N, uvs=UV, device="gpu")
    cpu.refit(positions=P, normals=N, uvs=UV, device="cpu")
    assert _refit.scene_bytes(gpu) == _refit.scene_bytes(cpu)
    assert _refit.raw_bytes(gpu) != original
    gpu.refit(positions=sp.P, normals=sp.N, uvs=sp.UV, device="gpu")
    assert _refit.raw_bytes(gpu) == original
