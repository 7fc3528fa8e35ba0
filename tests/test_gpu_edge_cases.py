"""Edge cases of the render entry points (GPU): empty scene, tiny and ragged frames, one sample / one bounce, an image with
row padding and an alpha channel, a second frame on the same context."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _empty_scene():
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import Material, build_scene
    cam = np.eye(4, dtype=np.float32)
    z = np.zeros((0, 3, 3), np.float32)
    return build_scene(z, z, np.zeros((0, 3, 2), np.float32), np.zeros((0,), np.int32), [Material()], [], cam, 1.0,
                       procedural_background(64, 32))


def test_empty_scene_is_all_background(rt, oracle):
    """0 triangles: depth 0, one all-zero leaf group; every path is one ray into the environment."""
    from tests import _oracle
    hs = _empty_scene()
    assert hs.scene.bvh.depth == 0 and hs.scene.triangles.len == 8
    want = _oracle.render(hs, 40, 24, 3, 4)
    got = rt.render_frame(hs, 40, 24, 3, 4, want_accum=True)
    assert np.array_equal(want["accum"], got["accum"])
    assert np.array_equal(want["image"], got["image"])
    c = got["counters"]
    assert c.paths == 40 * 24 * 3 and c.rays == c.paths and c.backgrounds == c.paths and c.shades == 0


@pytest.mark.parametrize("w,h,s,b", [(1, 1, 1, 1), (1, 1, 5, 8), (3, 2, 2, 1), (33, 1, 4, 4), (1, 33, 4, 4), (8, 8, 1, 8),
                                     (65, 31, 1, 1), (8, 8, 2, 0)])
def test_tiny_and_ragged_frames(rt, oracle, w, h, s, b):
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    hs, _ = load_config("spheres")
    want = _oracle.render(hs, w, h, s, b)
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(want["accum"], got["accum"])
    assert np.array_equal(want["image"], got["image"])
    assert got["counters"].paths == w * h * s
    assert got["counters"].rays == want["counters"]["rays"]


def test_image_with_row_padding_and_alpha(rt, oracle):
    """Image.stride > width and components = 4 (driver.c:747-754 allocates RGB; codin images may carry more):
    pixel (x, y) component c lives at pixels[(x + y * stride) * components + c]; everything else stays untouched."""
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    hs, _ = load_config("spheres")
    w, h, stride, comp = 37, 21, 48, 4
    want = _oracle.render(hs, w, h, 4, 4)["image"]
    buf = np.full((h, stride, comp), 0xAB, np.uint8)
    ctx = abi.Rendering_Context()
    ctx.image.components = comp
    ctx.image.pixel_type = 0
    ctx.image.width = w
    ctx.image.stride = stride
    ctx.image.height = h
    ctx.image.pixels.data = buf.ctypes.data
    ctx.image.pixels.len = buf.size
    ctx.scene = C.pointer(hs.scene)
    ctx.samples = 4
    ctx.max_bounces = 4
    ctx.n_threads = 1
    ctx._current_chunk = 0
    rt.lib.rt_set_seed(0x1234ABCD)
    rt.lib.rt_clear_error()
    rt.lib.render_thread_proc(C.byref(ctx))
    assert rt.last_error() == ""
    assert rt.lib.rendering_context_is_finished(C.byref(ctx))
    assert np.array_equal(buf[:, :w, :3], want)
    assert np.all(buf[:, :w, 3] == 0xAB), "alpha channel must not be written"
    assert np.all(buf[:, w:, :] == 0xAB), "row padding must not be written"


def test_second_frame_on_the_same_scene_reuses_the_device_copy(rt, oracle):
    """Two Rendering_Contexts on one Scene* (what an animation loop does): same device scene, new camera honoured."""
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    hs, cfg = load_config("spheres")
    a = rt.render_context(hs, 64, 40, 2, 4)["image"]
    m = np.ctypeslib.as_array(hs.scene.camera.view_matrix.rows).reshape(4, 4).copy()
    m[0, 3] += 0.75                                                       # move the camera: the Scene pointer stays the same
    hs.set_camera(m, float(hs.scene.camera.fov))
    want = _oracle.render(hs, 64, 40, 2, 4)["image"]
    b = rt.render_context(hs, 64, 40, 2, 4)["image"]
    assert np.array_equal(b, want)
    assert not np.array_equal(a, b)


def _textured_quad():
    """two triangles with one textured material (4x4 albedo), looked at head on"""
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import Material, build_scene
    pos = np.array([[[-1, -1, 0], [1, -1, 0], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0]]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (2, 3, 1))
    uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], np.float32)
    tex = (np.arange(4 * 4 * 3, dtype=np.uint32) * 5 % 256).astype(np.uint8).reshape(4, 4, 3)
    cam = np.eye(4, dtype=np.float32)
    cam[2, 3] = 2.5
    mats = [Material(base_color=(0.9, 0.8, 0.7), roughness=0.6, texture_albedo=0)]
    return build_scene(pos, nrm, uv, np.zeros(2, np.int32), mats, [tex], cam, 1.0, procedural_background(64, 32))


def test_in_place_scene_edits_are_seen_by_the_next_frame(rt, oracle):
    """The reference reads the live Scene every frame (raytracer.c:596-720 holds no copy).  render_thread_proc keeps a
    device copy per Scene*, so it must notice host-side edits: a material colour, a vertex, a texture swapped for
    another Image, a single texel: all seen by the next frame without any call (the stamp before the frame, the full content
    check while the GPU renders it)."""
    from tests import _oracle
    hs = _textured_quad()
    w, h, s, b = 48, 32, 4, 3
    first = rt.render_context(hs, w, h, s, b)["image"]
    assert np.array_equal(first, _oracle.render(hs, w, h, s, b)["image"])

    hs.materials[0].base_color.x = 0.1                      # 1. material record edited in place
    got = rt.render_context(hs, w, h, s, b)["image"]
    assert np.array_equal(got, _oracle.render(hs, w, h, s, b)["image"])
    assert not np.array_equal(got, first)

    hs.soa_array()[6:9, :2] -= 0.25                         # 2. geometry edited in place: both triangles move back (z)
    got2 = rt.render_context(hs, w, h, s, b)["image"]
    assert np.array_equal(got2, _oracle.render(hs, w, h, s, b)["image"])
    assert not np.array_equal(got2, got)

    hs._image_arrays[0][...] = 255 - hs._image_arrays[0]   # 3. every texel rewritten (an image reloaded in place)
    got3 = rt.render_context(hs, w, h, s, b)["image"]
    assert np.array_equal(got3, _oracle.render(hs, w, h, s, b)["image"])
    assert not np.array_equal(got3, got2)

    hs._image_arrays[0][1, 2, 0] ^= 0x80                    # 4. ONE texel of a small image (hashed in full): seen
    got4 = rt.render_context(hs, w, h, s, b)["image"]
    assert np.array_equal(got4, _oracle.render(hs, w, h, s, b)["image"])
    assert not np.array_equal(got4, got3)


def _big_textured_quad(size=2048):
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import Material, build_scene
    pos = np.array([[[-1, -1, 0], [1, -1, 0], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0]]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (2, 3, 1))
    uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], np.float32)
    tex = np.random.default_rng(3).integers(40, 90, (size, size, 3), dtype=np.uint8)
    cam = np.eye(4, dtype=np.float32)
    cam[2, 3] = 2.2
    mats = [Material(base_color=(1.0, 1.0, 1.0), roughness=0.9, texture_albedo=0)]
    return build_scene(pos, nrm, uv, np.zeros(2, np.int32), mats, [tex], cam, 0.9, procedural_background(64, 32))


def test_scene_touch_patches_one_texel_of_a_2048_texture_without_a_re_upload(rt, oracle):
    """VERDICT r03 #9 / ADVICE r03: rt_scene_touch(scene, begin, bytes) -- "I wrote these bytes".  A SINGLE texel of a 12 MB
    texture changes in place (the 1-in-61 sampling of the full check can miss it); after the call the next frame shows it,
    equal to the oracle on the edited host scene, and nothing was uploaded again: the touched ROW was packed again."""
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _oracle
    hs = _big_textured_quad()
    w, h, s, b = 64, 64, 64, 3
    first = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(first["accum"], _oracle.render(hs, w, h, s, b)["accum"])
    tex = hs._image_arrays[0]
    # a block of texels would be easy to see; ONE texel needs a sample whose bilinear footprint contains it: pick one the oracle sees
    for (ty, tx) in [(1024, 1024), (1031, 1017), (700, 1300), (1500, 900), (999, 1111), (1200, 800), (860, 1240), (1100, 1150)]:
        old = tex[ty, tx].copy()
        tex[ty, tx] = (255, 255, 255)
        want = _oracle.render(hs, w, h, s, b)
        if not np.array_equal(want["accum"], first["accum"]):
            break
        tex[ty, tx] = old
    else:
        pytest.fail("no candidate texel is sampled by this frame")
    rc = rt.lib.rt_scene_touch(C.byref(hs.scene), tex[ty, tx:].ctypes.data, 3)
    assert rc == 0, rt.last_error()
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(got["accum"], want["accum"])
    t = abi.RT_Frame_Timing()
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0
    assert t.upload_ms == 0.0, "the texture row was patched: no upload of the scene"
    # the same through the reference's own entry point, and a vertex through rt_scene_touch
    soa = hs.soa_array()
    soa[6:9, :2] -= 0.125
    assert rt.lib.rt_scene_touch(C.byref(hs.scene), soa[6:].ctypes.data, 3 * soa.shape[1] * 4) in (0, 1)
    got2 = rt.render_context(hs, w, h, s, b)["image"]
    assert np.array_equal(got2, _oracle.render(hs, w, h, s, b)["image"])
    # a range that belongs to nothing the copy was made from: the copy is dropped, the next frame uploads
    junk = np.zeros(16, np.uint8)
    assert rt.lib.rt_scene_touch(C.byref(hs.scene), junk.ctypes.data, 16) == 1
    got3 = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(got3["accum"], _oracle.render(hs, w, h, s, b)["accum"])
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0 and t.upload_ms > 0.0


def test_in_place_vertex_edit_inside_a_large_block_is_seen_without_any_call(rt, oracle):
    """ONE vertex in the middle of 4 800 triangles moves in place -- outside the bytes the microsecond
    stamp samples.  The full content check runs on the calling thread while the GPU renders the frame; it throws the stale
    frame away, uploads and renders again: the caller gets the frame of the scene as it is, like the reference's."""
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    hs, _ = load_config("spheres")
    w, h, s, b = 64, 40, 4, 4
    a = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(a["accum"], _oracle.render(hs, w, h, s, b)["accum"])
    T = hs.scene.triangles
    i = int(T.len) // 2 + 37
    x0 = T.x[0][i]
    T.x[0][i] = x0 + 0.25
    want = _oracle.render(hs, w, h, s, b)
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(got["accum"], want["accum"])
    t = abi.RT_Frame_Timing()
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0
    assert t.upload_ms > 0.0 and t.verify_ms > 0.0            # (the check found the edit: the scene went up again)
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)    # unchanged now: checked again, nothing uploaded
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0
    assert np.array_equal(got["accum"], want["accum"]) and t.upload_ms == 0.0 and t.verify_ms > 0.0
    # a host that never edits in place opts out of the check (and tells the library when it does edit: rt_scene_touch)
    rt.lib.rt_scene_set_static(C.byref(hs.scene), 1)
    rt.render_frame(hs, w, h, s, b)
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0 and t.verify_ms == 0.0
    T.x[0][i] = x0
    assert rt.lib.rt_scene_touch(C.byref(hs.scene), C.addressof(T.x[0].contents) + 4 * i, 4) == 0
    back = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(back["accum"], a["accum"])
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0 and t.upload_ms == 0.0
    rt.lib.rt_scene_set_static(C.byref(hs.scene), 0)


def test_scene_rebuilt_at_the_same_address_is_not_served_from_the_cache(rt, oracle):
    """rt_scene_free() + scene_init() of a same-size scene into the same Scene struct very likely gets the same malloc
    blocks back; pointer identity cannot tell the two scenes apart.  scene_init / rt_scene_free drop the
    device copy, and the content stamp differs anyway."""
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _oracle
    hs = _textured_quad()
    w, h, s, b = 40, 24, 2, 3
    a = rt.render_context(hs, w, h, s, b)["image"]
    old_nodes, old_tris = hs.scene.bvh.nodes.data, C.cast(hs.scene.triangles.x[0], C.c_void_p).value
    # rebuild IN PLACE with different geometry (the quad shrunk to half its size)
    tri = np.zeros(2, abi.TRIANGLE_DTYPE)
    pos = np.array([[[-.5, -.5, 0], [.5, -.5, 0], [.5, .5, 0]], [[-.5, -.5, 0], [.5, .5, 0], [-.5, .5, 0]]], np.float32)
    tri["positions"] = pos
    tri["normals"] = np.tile(np.array([0, 0, 1], np.float32), (2, 3, 1))
    tri["tex_coords"] = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], np.float32)
    tri["shader_data"] = C.addressof(hs.materials)
    tri["shader_proc"] = rt.native.symbol_address("disney_shader_proc")
    rt.lib.rt_scene_free(C.byref(hs.scene))
    rt.lib.scene_init(C.byref(hs.scene), abi.Triangle_Slice(tri.ctypes.data, 2), abi.Allocator(None, None))
    same_blocks = (hs.scene.bvh.nodes.data == old_nodes and C.cast(hs.scene.triangles.x[0], C.c_void_p).value == old_tris)
    got = rt.render_context(hs, w, h, s, b)["image"]
    assert np.array_equal(got, _oracle.render(hs, w, h, s, b)["image"]), f"stale device scene (same blocks: {same_blocks})"
    assert not np.array_equal(got, a)


def test_non_u8_or_short_texture_is_refused(rt):
    """texture_index(): an Image that is not PT_u8, or whose pixels slice is shorter than stride*height*components, must be
    refused loudly instead of being uploaded as raw bytes / over-read."""
    hs = _textured_quad()
    hs.images[0].pixel_type = 1
    rt.lib.rt_clear_error()
    assert not rt.lib.rt_scene_upload(C.byref(hs.scene))
    assert "unusable Image" in rt.last_error()
    hs.images[0].pixel_type = 0
    hs.images[0].pixels.len = 4 * 4 * 3 - 1
    rt.lib.rt_clear_error()
    assert not rt.lib.rt_scene_upload(C.byref(hs.scene))
    assert "unusable Image" in rt.last_error()
    hs.images[0].pixels.len = 4 * 4 * 3
    d = rt.lib.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error()
    rt.lib.rt_scene_release(d)


@pytest.mark.parametrize("tw,th", [(37, 23), (5, 3), (64, 1), (1, 9), (130, 67)])
def test_textures_whose_size_is_not_a_multiple_of_the_tile(rt, oracle, diag, tw, th):
    """Textures live in 4x4-texel tiles on the device (rt_device.h, round 4).  Sizes that are no multiple of four, one texel
    wide or high: every fetch -- wrap, clamp at the last column / row, footprints across tile edges -- equals the oracle's
    bilinear fetch bit for bit, a frame using the texture equals the oracle's, and rows patched by rt_scene_touch land in
    the right tiles."""
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import Material, build_scene
    from tests import _oracle
    rng = np.random.default_rng(tw * 100 + th)
    pos = np.array([[[-1, -1, 0], [1, -1, 0], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0]]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (2, 3, 1))
    uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], np.float32)
    tex = rng.integers(0, 256, (th, tw, 3), dtype=np.uint8)
    cam = np.eye(4, dtype=np.float32)
    cam[2, 3] = 2.5
    hs = build_scene(pos, nrm, uv, np.zeros(2, np.int32), [Material(base_color=(0.9, 0.8, 0.7), roughness=0.6, texture_albedo=0)],
                     [tex], cam, 1.0, procedural_background(67, 33))
    n = 4000
    uvs = rng.uniform(-2, 2, (n, 2)).astype(np.float32)
    uvs[:8] = [[0, 0], [1, 1], [0.99999994, 0.99999994], [-1e-9, 0.5], [0.5, -1e-9], [1.0 - 0.5 / tw, 1.0 - 0.5 / th], [0.25, 0.75], [2.5, -0.5]]
    d = rt.diag.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error(rt.diag)
    try:
        for cimg in (hs.images[0], hs.background_image):
            want = np.zeros((n, 3), np.float32)
            for i in range(n):
                oracle.oracle_sample_texture_bilinear(C.byref(cimg), uvs[i, 0], uvs[i, 1], want[i].ctypes.data)
            hits = 0
            for t in (-1, 0, 1):
                got = np.zeros((n, 3), np.float32)
                if rt.diag.rt_test_texture(d, t, n, uvs.ctypes.data, got.ctypes.data) != 0:
                    continue
                hits += int(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
            assert hits >= 1, "no device texture reproduces the host image's fetches"
    finally:
        rt.diag.rt_scene_release(d)
    w, h, s, b = 40, 32, 8, 3
    first = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(first["accum"], _oracle.render(hs, w, h, s, b)["accum"])
    # rows r0 .. r1 rewritten in place, told to the library: a partial tile row at the bottom included
    arr = hs._image_arrays[0]
    r0, r1 = th // 3, th
    arr[r0:r1] = 255 - arr[r0:r1]
    assert rt.lib.rt_scene_touch(C.byref(hs.scene), arr[r0:].ctypes.data, (r1 - r0) * tw * 3) == 0, rt.last_error()
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(got["accum"], _oracle.render(hs, w, h, s, b)["accum"])
    assert not np.array_equal(got["accum"], first["accum"])


@pytest.mark.parametrize("k", [300.0, 1e5])
def test_scene_far_from_the_origin_renders_through_the_exact_slab_form(rt, oracle, k):
    """Deviation D9 has a domain (include/rt_math.h: RT_SLAB_FUSED_MAX_ORIGIN): rays whose origin is 256 units or more from
    the origin take the reference's (plane - o) * inv on the GPU like in the oracle -- every node block of this frame is the
    exact kind, no sky loop, no pyramid culling -- and the frame still equals the oracle's bit for bit."""
    from tests import _oracle
    from tests._far_scene import translated_spheres
    hs = translated_spheres(k)
    w, h, s, b = 160, 128, 4, 4
    want = _oracle.render(hs, w, h, s, b)
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(want["accum"], got["accum"])
    assert np.array_equal(want["image"], got["image"])
    c, wc = got["counters"], want["counters"]
    assert (c.rays, c.node_visits, c.leaf_visits, c.shades, c.backgrounds) == \
        (wc["rays"], wc["node_visits"], wc["leaf_visits"], wc["shades"], wc["backgrounds"])
    assert c.shades > 1000


def test_skipped_root_visits_are_reported(rt, oracle):
    """bench.py's roofline footnote: of the node visits the kernel reports (equal to the oracle's), rt_get_skipped_root_visits()
    says how many were counted without being executed -- the root visit of camera paths whose whole 8x8 tile sees only sky."""
    import ctypes as C
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    from tests._far_scene import translated_spheres
    hs, _ = load_config("spheres")
    w, h, s, b = 256, 256, 4, 4
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    want = _oracle.render(hs, w, h, s, b)
    assert np.array_equal(got["accum"], want["accum"]) and got["counters"].node_visits == want["counters"]["node_visits"]
    n = C.c_uint64(0)
    assert rt.lib.rt_get_skipped_root_visits(C.byref(n)) == 0, rt.last_error()
    assert 0 < n.value < w * h * s and n.value % s == 0            # whole pixels of whole tiles, not the whole frame
    assert n.value <= got["counters"].backgrounds and n.value <= got["counters"].node_visits
    far = translated_spheres(1e5)                                   # no ray of this frame may take the shortcut (include/rt_math.h, D9's domain)
    rt.render_frame(far, 64, 64, 2, 2)
    assert rt.lib.rt_get_skipped_root_visits(C.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("w,h,s", [(256, 144, 16), (640, 360, 16), (512, 512, 64)])
def test_every_workgroup_size_the_library_picks_gives_the_same_frame(rt, oracle, w, h, s):
    """The path kernel runs with 8-, 12- or 16-wave workgroups depending on the paths per wave slot of the launch (rt_launch.cpp:
    below 12 wave-fulls 8, below 40 twelve, else 16 -- 2 / 14 / 64 for these three frames on a 256-CU chip).  The launch geometry
    enters no result: each frame equals the oracle's."""
    from raytracing_c_amd.configs import load_config
    from tests import _oracle
    hs, _ = load_config("spheres")
    want = _oracle.render(hs, w, h, s, 4)
    got = rt.render_frame(hs, w, h, s, 4, want_accum=True)
    assert np.array_equal(want["accum"], got["accum"])
    c, wc = got["counters"], want["counters"]
    assert (c.rays, c.node_visits, c.leaf_visits, c.shades) == (wc["rays"], wc["node_visits"], wc["leaf_visits"], wc["shades"])


def test_scene_touch_does_not_absorb_an_edit_nobody_reported(rt, oracle):
    """two in-place edits, ONE reported.  rt_scene_touch() compares block fingerprints first: a block that changed and
    is not the one the reported range lies in means an edit nobody told about -- the copy is dropped (return 1) and the next frame
    uploads, instead of the unreported edit being taken into the new reference where no later check could find it."""
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _oracle
    hs = _big_textured_quad(256)
    w, h, s, b = 64, 64, 16, 3
    first = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(first["accum"], _oracle.render(hs, w, h, s, b)["accum"])
    tex = hs._image_arrays[0]
    tex[100:140, 100:140] = (255, 255, 255)                       # reported below
    soa = hs.soa_array()
    soa[6, :2] -= 0.125                                           # NOT reported: the z of the first vertex of both triangles
    rc = rt.lib.rt_scene_touch(C.byref(hs.scene), tex[100, 100:].ctypes.data, 40 * tex.shape[1] * 3)
    assert rc == 1, "a second, unreported edit must drop the copy"
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    want = _oracle.render(hs, w, h, s, b)
    assert np.array_equal(got["accum"], want["accum"]) and not np.array_equal(want["accum"], first["accum"])
    t = abi.RT_Frame_Timing()
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0 and t.upload_ms > 0.0
    # ... and a reported edit alone is patched in place
    tex[10:12, 10:200] = (0, 0, 0)
    assert rt.lib.rt_scene_touch(C.byref(hs.scene), tex[10, 10:].ctypes.data, 2 * tex.shape[1] * 3) == 0
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(got["accum"], _oracle.render(hs, w, h, s, b)["accum"])
    assert rt.lib.rt_get_frame_timing(C.byref(t)) == 0 and t.upload_ms == 0.0


def _picket_fence(n_slivers, depth_jitter, seed):
    """Thin vertical slivers (a third of a pixel to three pixels wide at 96 x 96) side by side across the view, each at its own depth:
    every 8 x 8 tile's pyramid cuts through sliver edges, most leaf groups keep a few of their eight triangles per tile."""
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.scene import Material, build_scene
    rng = np.random.default_rng(seed)
    xs = np.sort(rng.uniform(-1.2, 1.2, n_slivers + 1))
    tris = []
    for i in range(n_slivers):
        z = -3.0 - depth_jitter * rng.uniform(0.0, 1.0)
        x0, x1 = xs[i], xs[i + 1]
        y0, y1 = -1.2 + 0.3 * rng.uniform(0, 1), 1.2 - 0.3 * rng.uniform(0, 1)
        tris.append([[x0, y0, z], [x1, y0, z], [x0, y1, z]])
        tris.append([[x1, y0, z], [x1, y1, z], [x0, y1, z]])
    pos = np.asarray(tris, np.float32)
    nrm = np.tile(np.asarray([0, 0, 1], np.float32), (len(pos), 3, 1))
    uv = np.zeros((len(pos), 3, 2), np.float32)
    mats = [Material(base_color=(0.8, 0.7, 0.6), roughness=0.5, metalness=0.2)]
    return build_scene(pos, nrm, uv, np.zeros((len(pos),), np.int32), mats, [], np.eye(4, dtype=np.float32), 0.9,
                       procedural_background(64, 32))


@pytest.mark.parametrize("n_slivers,depth_jitter,seed", [(40, 0.0, 1), (200, 0.5, 2), (700, 2.0, 3)])
def test_slivers_across_tile_boundaries(rt, oracle, n_slivers, depth_jitter, seed):
    """The pyramid-culled LEAF blocks (rt_dev.hip.h pyramid_cull_tris, leaf_test_uniform) drop the triangles a tile's camera rays cannot
    touch: a frame full of sliver edges on and next to tile boundaries must still be the oracle's sums, image and counters bit for bit."""
    from tests import _oracle
    hs = _picket_fence(n_slivers, depth_jitter, seed)
    w, h, s, b = 96, 96, 64, 3
    want = _oracle.render(hs, w, h, s, b)
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(want["accum"], got["accum"])
    assert np.array_equal(want["image"], got["image"])
    c = got["counters"]
    for k in ("rays", "node_visits", "leaf_visits", "shades", "backgrounds"):
        assert getattr(c, k) == want["counters"][k], k
