"""The shade block with ONE set of bilinear taps per hit (SharedTaps, raytracing_c_amd/csrc/rt_dev.hip.h): the form of the path
kernel that a scene gets whose materials' textures agree in width, height and stride (rt_materials_share_taps, decided by the host
for the resident copy; rt_get_shade_taps_form says which form the last launch ran).

Bar: BIT-EXACT against the CPU oracle everywhere -- unit level: every output float has the oracle's bits or both are NaN,
`terminate`, the RNG state and the `textured` increment are equal, in the general and in the shared form; frames: the whole u64
accumulators and all seven counters.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import _taps_scene as T
from tests._shade_inputs import same_bits

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")
SHARED, GENERAL = 1, 0
RT_TEST_SHARED_TAPS = 4


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _same_as_oracle(got_accum, got_counters, want, what=""):
    assert np.array_equal(got_accum, want["accum"]), f"radiance sums {what}"
    assert tuple(getattr(got_counters, k) for k in COUNTERS) == tuple(want["counters"][k] for k in COUNTERS), what


# ---------------------------------------------------------------------------------------------------------------------
# unit level

@pytest.fixture(scope="module")
def dscene(rt, diag):
    d = diag.rt_scene_upload(C.byref(T.scene().hs.scene))
    assert d, rt.last_error(diag)
    yield d
    diag.rt_scene_release(d)


def _run_shade(rt, diag, dscene, mode, order):
    it = T.items()
    n = len(order)
    tri, inp, seed = (np.ascontiguousarray(it[k][order]) for k in ("tri", "inp", "seed"))
    out, state, term, tex = np.zeros((n, 9), np.float32), np.zeros(n, np.uint32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    rc = diag.rt_test_shade(dscene, mode, n, tri.ctypes.data, inp.ctypes.data, seed.ctypes.data, out.ctypes.data, state.ctypes.data,
                            term.ctypes.data, tex.ctypes.data)
    assert rc == 0, rt.last_error(diag)
    return dict(out=out, state=state, terminate=term, textured=tex)


def test_the_items_reach_what_they_aim_at():
    """on the host: among the coordinates are both sides of a tile boundary and the last texel of every texture size, and the
    reference has textured and plain, continued and terminated items"""
    for w in (8, 5, 4, 3):
        texel = {int(np.float32(u - np.floor(u)) * np.float32(w)) for u in np.array(T.COORDS, np.float32)}
        assert {0, w - 1} <= texel, w
    assert {3, 4} <= {int(np.float32(u) * np.float32(8)) for u in T.COORDS if 0 <= u < 1}
    assert {3, 4} <= {int(np.float32(u) * np.float32(5)) for u in T.COORDS if 0 <= u < 1}
    ref, m = T.reference(), T.items()["material"]
    assert ref["textured"].any() and not ref["textured"].all()
    assert ref["terminate"][m == T.DEBUG_MATERIAL].all() and not ref["terminate"][m != T.DEBUG_MATERIAL].all()
    assert len(np.unique(ref["out"][m == 0][:, 6:9], axis=0)) > 50, "the emission texture of material 0 does not show"


@pytest.mark.parametrize("order", ["uniform", "mixed"])
@pytest.mark.parametrize("mode", [0, 1, 0 | RT_TEST_SHARED_TAPS, 1 | RT_TEST_SHARED_TAPS], ids=["general", "general-lds", "shared", "shared-lds"])
def test_shade_equals_the_oracle(rt, oracle, diag, dscene, mode, order):
    """64-item waves of one material (the record comes through the scalar cache) and waves that mix materials (vector loads)"""
    want = T.reference()
    idx = T.uniform_order() if order == "uniform" else T.mixed_order()
    got = _run_shade(rt, diag, dscene, mode, idx)
    ok = (np.all(same_bits(want["out"][idx], got["out"]), axis=1) & (want["terminate"][idx] == got["terminate"])
          & (want["state"][idx] == got["state"]) & (want["textured"][idx] == got["textured"]))
    bad = np.flatnonzero(~ok)
    if len(bad):
        j = int(bad[0])
        i, it = int(idx[j]), T.items()
        pytest.fail(f"mode {mode}, {order}: {len(bad)} of {len(idx)} entries differ; first: entry {j} (wave {j >> 6}, lane {j & 63}), item {i}, "
                    f"material {it['material'][i]}, uv {it['inp'][i, 12:14].tolist()}, seed {it['seed'][i]:#x}\n"
                    f"oracle: out {want['out'][i].tolist()} terminate {want['terminate'][i]} state {want['state'][i]:#x} textured {want['textured'][i]}\n"
                    f"device: out {got['out'][j].tolist()} terminate {got['terminate'][j]} state {got['state'][j]:#x} textured {got['textured'][j]}")


def test_shared_mode_is_refused_on_a_mixed_scene(rt, diag):
    sc = T.build(mixed=True)
    d = diag.rt_scene_upload(C.byref(sc.hs.scene))
    assert d, rt.last_error(diag)
    try:
        one = np.zeros(14, np.float32)
        tri, seed = np.array([sc.slots[0][0]], np.int32), np.zeros(1, np.uint32)
        out, state, term, tex = np.zeros(9, np.float32), np.zeros(1, np.uint32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        args = (1, tri.ctypes.data, one.ctypes.data, seed.ctypes.data, out.ctypes.data, state.ctypes.data, term.ctypes.data, tex.ctypes.data)
        assert diag.rt_test_shade(d, 1 | RT_TEST_SHARED_TAPS, *args) != 0 and "differ in size" in rt.last_error(diag)
        assert diag.rt_test_shade(d, 1, *args) == 0, rt.last_error(diag)
    finally:
        diag.rt_scene_release(d)


@pytest.mark.parametrize("mode", [0, 1], ids=["plain", "lds"])
def test_shade_hit_shared_equals_general(rt, diag, dscene, mode):
    """one path step (rt_test_shade_hit) on front-face hits of every triangle of the scene, in material-uniform and in mixed waves:
    the shared form returns the general form's bits, which tests/test_gpu_shade_hit.py holds against the oracle"""
    sc = T.scene()
    rng = np.random.default_rng(1404)
    slots = np.array([s for m in range(T.N_MATERIALS) for s in sc.slots[m] for _ in range(64)], np.int32)      # 128 items a material
    for order in (np.arange(len(slots)), rng.permutation(len(slots))):
        tri = np.ascontiguousarray(slots[order])
        n = len(tri)
        uv = rng.uniform(0.0, 0.5, (n, 2)).astype(np.float32)
        hit = np.ascontiguousarray(np.concatenate([np.full((n, 1), 2.0, np.float32), uv], axis=1))
        d = np.tile(np.array([0.1, -0.2, -1.0]), (n, 1)) + rng.normal(0, 0.05, (n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ray = np.ascontiguousarray(np.concatenate([np.tile([3.0, 0.5, 1.5], (n, 1)), d], axis=1), np.float32)
        carry = np.ascontiguousarray(rng.uniform(0.2, 1.0, (n, 6)), np.float32)
        seed, bounce = rng.integers(0, 2 ** 32, n, dtype=np.uint32), np.zeros(n, np.int32)
        got = {}
        for m in (mode, mode | RT_TEST_SHARED_TAPS):
            out, words = np.zeros((n, 15), np.float32), np.zeros((n, 5), np.uint32)
            rc = diag.rt_test_shade_hit(dscene, m, 8, n, tri.ctypes.data, hit.ctypes.data, ray.ctypes.data, carry.ctypes.data,
                                        seed.ctypes.data, bounce.ctypes.data, out.ctypes.data, words.ctypes.data)
            assert rc == 0, rt.last_error(diag)
            got[m] = (out, words)
        (a, wa), (b, wb) = got[mode], got[mode | RT_TEST_SHARED_TAPS]
        assert wa[:, 3].sum() > n // 2 and wa[:, 4].sum() > n // 4, "too few items were shaded, or too few with a texture"
        assert np.all(same_bits(a, b)) and np.array_equal(wa, wb)
    out, words = np.zeros((1, 15), np.float32), np.zeros((1, 5), np.uint32)
    assert diag.rt_test_shade_hit(dscene, 2 | RT_TEST_SHARED_TAPS, 8, 1, tri.ctypes.data, hit.ctypes.data, ray.ctypes.data, carry.ctypes.data,
                                  seed.ctypes.data, bounce.ctypes.data, out.ctypes.data, words.ctypes.data) != 0      # (RT_KParams has no shared form)


# ---------------------------------------------------------------------------------------------------------------------
# selection

def _frame(rt, hs, w, h, s, b, want_form, what):
    from tests import _oracle
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    form = rt.lib.rt_get_shade_taps_form()
    _same_as_oracle(got["accum"], got["counters"], _oracle.render(hs, w, h, s, b), what)
    assert form == want_form, what
    return got


def test_selection_and_in_place_edits(rt, oracle):
    """the scene qualifies; the same scene with an 8 x 8 albedo beside a 4 x 8 normal map in one material does not; a reported
    in-place edit that breaks the agreement moves the next frame to the general form, one that restores it moves it back"""
    w, h, s, b = 48, 16, 4, 3
    mixed = T.build(mixed=True)
    try:
        got = _frame(rt, mixed.hs, w, h, s, b, GENERAL, "mixed from the start")
        assert got["counters"].textured > 0
    finally:
        rt.lib.rt_scene_invalidate(C.byref(mixed.hs.scene))
    sc = T.build()
    hs = sc.hs
    try:
        first = _frame(rt, hs, w, h, s, b, SHARED, "as built")
        assert first["counters"].textured > 0
        mat0, size = hs.materials[0], C.sizeof(hs.materials[0])
        assert C.addressof(mat0.texture_normal.contents) == C.addressof(hs.images[1])
        # (a material that names ANOTHER image changes the list of blocks the scene check keeps, so rt_scene_touch drops the copy
        # and the next frame uploads -- 1 -- where it decides anew; 0, patched in place, would have to decide anew as well)
        mat0.texture_normal = C.pointer(hs.images[T.MIXED_IMAGE])
        assert rt.lib.rt_scene_touch(C.byref(hs.scene), C.addressof(mat0), size) in (0, 1), rt.last_error()
        second = _frame(rt, hs, w, h, s, b, GENERAL, "after the edit that breaks the agreement")
        assert not np.array_equal(first["accum"], second["accum"])
        mat0.texture_normal = C.pointer(hs.images[1])
        assert rt.lib.rt_scene_touch(C.byref(hs.scene), C.addressof(mat0), size) in (0, 1), rt.last_error()
        third = _frame(rt, hs, w, h, s, b, SHARED, "after the edit that restores it")
        assert np.array_equal(first["accum"], third["accum"])
        # a material record patched in place (the same textures, another roughness) is looked at again and still qualifies
        mat0.roughness = 0.25
        assert rt.lib.rt_scene_touch(C.byref(hs.scene), C.addressof(mat0), size) == 0, rt.last_error()
        fourth = _frame(rt, hs, w, h, s, b, SHARED, "after a patch that leaves the textures alone")
        assert not np.array_equal(first["accum"], fourth["accum"])
        # ... and an edit nobody reported is found by the frame's own scene check: the frame that is returned ran the general form
        mat0.texture_normal = C.pointer(hs.images[T.MIXED_IMAGE])
        _frame(rt, hs, w, h, s, b, GENERAL, "after an unreported edit")
    finally:
        rt.lib.rt_scene_invalidate(C.byref(hs.scene))


def test_a_scene_without_textures_keeps_the_general_form(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("quad")
    _frame(rt, hs, 16, 16, 4, 2, GENERAL, "quad.obj")


# ---------------------------------------------------------------------------------------------------------------------
# frames against the oracle

def test_render_accumulate(rt, oracle):
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _oracle
    hs = T.scene().hs
    w, h, s, b = 16, 16, 4, 3
    d = rt.lib.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error()
    try:
        accum = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
        p = abi.RT_Render_Params(w, h, s, b, 0x1234ABCD, 0, 1, 0, 0)
        assert rt.lib.rt_render_accumulate(d, C.byref(p), accum.data_ptr(), None) == 0, rt.last_error()
        torch.cuda.synchronize()
        got, counters = accum.cpu().numpy().view(np.uint64), rt.render.get_counters()
        assert rt.lib.rt_get_shade_taps_form() == SHARED
    finally:
        rt.lib.rt_scene_release(d)
    assert counters.textured > 0
    _same_as_oracle(got, counters, _oracle.render(hs, w, h, s, b))


def test_helmet_frame(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("helmet")
    got = _frame(rt, hs, 80, 45, 4, 3, SHARED, "helmet: its textures have one size")
    assert got["counters"].textured > 0


def test_two_views_in_one_launch(rt, oracle):
    from tests import _oracle
    from tests.test_gpu_views import _camera, _copy, _matrix, _rot_y
    hs = T.scene().hs
    w, h, s, b = 32, 16, 4, 3
    cam = hs.scene.camera
    cams = [_copy(cam), _camera(_rot_y(20.0) @ _matrix(cam), float(cam.fov))]
    seeds = [5, 0xBEEF]
    got = rt.render_views(hs, cams, w, h, s, b, seeds=seeds, want_accum=True)
    assert rt.lib.rt_get_shade_taps_form() == SHARED
    saved = _copy(cam)
    try:
        total = dict.fromkeys(COUNTERS, 0)
        for v, (c, sd) in enumerate(zip(cams, seeds)):
            hs.scene.camera = c
            want = _oracle.render(hs, w, h, s, b, seed=sd)
            assert np.array_equal(got[v]["accum"], want["accum"]), f"view {v}"
            for k in COUNTERS:
                total[k] += want["counters"][k]
        assert total["textured"] > 0
        assert tuple(getattr(got[0]["counters"], k) for k in COUNTERS) == tuple(total[k] for k in COUNTERS)      # (of the whole batch)
    finally:
        hs.scene.camera = saved
        rt.lib.rt_scene_invalidate(C.byref(hs.scene))
