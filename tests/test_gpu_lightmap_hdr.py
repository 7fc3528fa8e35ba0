"""HDR lightmaps on the GPU (rt_lightmap_texels, rt_lightmap_trace, rt_lightmap_resolve, rt_lightmap_dilate, rt_scene_lightmap;
rt_lightmap.hip) against the CPU oracle (tests/_lightmap_hdr.py): every list entry, all three u64 sums of every entry, the image and
the path counters equal, bit for bit -- three scenes and maps at 0, 1 and 8 bounces, 1 to 200 samples, a 3 x 3 map whose lanes end
on the same texel, lists shorter than a wave, the zero-normal triangle, a NaN vertex; sample and texel ranges that add up to the
whole; a launch that gives every workgroup work; the host level and its slices; a scene edit; no effect on frames, queries, probes
and lightmap_bake; the dilation against numpy."""
import ctypes as C
from dataclasses import astuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def uploaded(rt):
    """name -> (device scene, vertices tensor), uploaded on first use and released with the module."""
    import torch
    from tests import _lightmap_hdr as L
    held = {}

    def get(name):
        if name not in held:
            hs = L.scene(name)
            d = rt.lib.rt_scene_upload(C.byref(hs.scene))
            assert d, rt.last_error()
            held[name] = (d, torch.from_numpy(L.vertices(hs)).cuda())
        return held[name]
    yield get
    for d, _ in held.values():
        rt.lib.rt_scene_release(d)


def _params(rt, W, H, samples, b, first=0, count=0, seed=None, scale=1.0):
    from tests import _lightmap_hdr as L
    return rt.abi.RT_Lightmap_Params(width=W, height=H, samples=samples, sample_first=first, sample_count=count, max_bounces=b,
                                     seed=L.SEED if seed is None else seed, scale=scale)


def _list(rt, dv, W, H):
    """The device-level list -> (texels tensor (W * H, 8), n, the entries as LIGHTMAP_TEXEL_DTYPE)."""
    import torch
    d, verts = dv
    owner = torch.empty(W * H + H, dtype=torch.int32, device="cuda")
    texels = torch.full((W * H, 8), 7.0, dtype=torch.float32, device="cuda")
    count = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    assert rt.lib.rt_lightmap_texels(d, verts.data_ptr(), W, H, owner.data_ptr(), texels.data_ptr(), count.data_ptr(), None) == 0, rt.last_error()
    n = int(count.item())
    got = texels[:n].cpu().numpy().view(rt.abi.LIGHTMAP_TEXEL_DTYPE).reshape(n)
    assert (texels[n:] == 7.0).all()                                  # nothing behind the list is written
    return texels, n, got, owner[:W * H].cpu().numpy().reshape(H, W)


def _chain(rt, dv, W, H, samples, b, launches=None, scale=1.0):
    """The device-level chain: the list, one rt_lightmap_trace per (sample_first, sample_count, texel_first, texel_count) of
    `launches` (None: one launch of everything) into ONE sum buffer, then the resolve."""
    import torch
    texels, n, got, owner = _list(rt, dv, W, H)
    sums = torch.zeros((max(n, 1), 3), dtype=torch.int64, device="cuda")
    image = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    counters = []
    for first, count, j0, m in (launches or [(0, 0, 0, n)]):
        if m <= 0:
            continue
        p = _params(rt, W, H, samples, b, first, count)
        assert rt.lib.rt_lightmap_trace(dv[0], C.byref(p), texels.data_ptr(), j0, m, sums.data_ptr(), None) == 0, rt.last_error()
        counters.append(rt.get_lightmap_counters())
    p = _params(rt, W, H, samples, b, scale=scale)
    assert rt.lib.rt_lightmap_resolve(C.byref(p), n, texels.data_ptr(), sums.data_ptr(), image.data_ptr(), None) == 0, rt.last_error()
    torch.cuda.synchronize()
    return dict(texels=got, owner=owner, n=n, sums=sums[:n].cpu().numpy().view(np.uint64), image=image.cpu().numpy(), counters=counters)


def _same_texels(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    a, b = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (len(bad), bad[:4].tolist(), got[bad[0, 0]], want[bad[0, 0]])


def _same(got, e):
    _same_texels(got["texels"], e["texels"])
    assert np.array_equal(got["owner"], e["owner"])
    assert np.array_equal(got["sums"], e["sums"]), np.argwhere(got["sums"] != e["sums"])[:4].tolist()
    assert got["image"].tobytes() == e["image"].tobytes()


def _total(counters):
    return tuple(sum(v) for v in zip(*[astuple(c) for c in counters])) if counters else (0,) * 7


def _case_id(case):
    name, W, H, samples, b = case
    return f"{name}-{W}x{H}-s{samples}-b{b}"


def _cases():
    from tests import _lightmap_hdr as L
    return L.CASES


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_list_sums_image_and_counters_equal_the_oracle(rt, oracle, uploaded, case):
    from tests import _lightmap_hdr as L
    name, W, H, samples, b = case
    e = L.expected_case(case)
    got = _chain(rt, uploaded(name), W, H, samples, b)
    _same(got, e)
    c = got["counters"][0]
    assert (c.paths, c.rays, c.shades, c.backgrounds) == (e["paths"], e["rays"], e["shades"], e["backgrounds"]), (c, e["classes"])
    if b == 0:
        assert not got["sums"].any() and (c.rays, c.shades, c.backgrounds) == (0, 0, 0)
        assert (got["image"][..., :3] == 0).all() and (got["image"][..., 3] == (e["owner"] >= 0)).all()


def test_the_zero_normal_triangle_and_the_one_texel_map(rt, oracle, uploaded):
    """The 64-try guard: the zero-normal special triangle owns texels of the 40 x 48 map, their paths are given up -- counted, never
    cast, sums 0, .w = 1.  The 1 x 1 map is owned by SPECIAL_UVS' `origin` triangle."""
    from tests import _lightmap as LM
    from tests import _lightmap_hdr as L
    slots = LM.special_slots(L.scene("soup"))
    got = _chain(rt, uploaded("soup"), 40, 48, 5, 8)
    mine = got["texels"]["triangle"] == slots["zero_normal"]
    assert mine.sum() >= 5 and not got["texels"]["normal"][mine].any()
    assert not got["sums"][mine].any()
    flat = got["image"].reshape(-1, 4)[got["texels"]["texel"][mine]]
    assert (flat == (0.0, 0.0, 0.0, 1.0)).all()
    e = L.expected_case(("soup", 40, 48, 5, 8))
    assert e["classes"]["given_up"] >= 5 * int(mine.sum())
    one = _chain(rt, uploaded("soup"), 1, 1, 70, 8)
    assert one["n"] == 1 and int(one["texels"]["triangle"][0]) == slots["origin"] and one["sums"].any()


def test_sample_ranges_and_texel_ranges_add_up(rt, oracle, uploaded):
    from tests import _lightmap_hdr as L
    W, H, samples, b = 40, 48, 8, 8
    dv = uploaded("soup")
    e = L.expected(L.scene("soup"), W, H, samples, b, counters=False)
    whole = _chain(rt, dv, W, H, samples, b)
    _same(whole, e)
    n = whole["n"]
    assert n > 130
    w = _total(whole["counters"])
    assert w[0] == n * samples
    parts = _chain(rt, dv, W, H, samples, b, launches=[(0, 3, 0, n), (3, 5, 0, n)])
    _same(parts, e)
    assert _total(parts["counters"]) == w
    for cut in (1, 63, 64, n - 1):
        two = _chain(rt, dv, W, H, samples, b, launches=[(0, 0, 0, cut), (0, 0, cut, n - cut)])
        _same(two, e)
        assert _total(two["counters"]) == w, cut
    # a sample range alone is that range's sums: m x c = n x 3 is no multiple of the grab
    head = _chain(rt, dv, W, H, samples, b, launches=[(0, 3, 0, n)])
    e3 = L.expected(L.scene("soup"), W, H, samples, b, sample_range=(0, 3), counters=False)
    assert np.array_equal(head["sums"], e3["sums"]) and (n * 3) % 64 != 0


def test_a_96_x_96_map_against_the_oracle_in_full(rt, oracle, uploaded):
    from tests import _lightmap_hdr as L
    e = L.expected(L.scene("soup"), 96, 96, 4, 8, counters=False)
    got = _chain(rt, uploaded("soup"), 96, 96, 4, 8, scale=6.2831855)
    _same_texels(got["texels"], e["texels"])
    assert np.array_equal(got["sums"], e["sums"])
    assert got["image"].tobytes() == L.resolve(e["texels"], e["sums"], 96, 96, 4, 6.2831855).tobytes()
    assert got["counters"][0].paths == e["paths"]


def test_a_launch_that_gives_every_workgroup_work(rt, oracle, uploaded):
    """256 x 256 at 16 samples, launched once, against eight launches of itself by parts -- four sample ranges x two texel ranges
    -- and against the oracle on 500 picked list entries."""
    from tests import _lightmap_hdr as L
    W = H = 256
    dv = uploaded("soup")
    one = _chain(rt, dv, W, H, 16, 8)
    n = one["n"]
    assert n * 16 > 256 * 1024 * 2
    cut = n // 2 + 17
    parts = _chain(rt, dv, W, H, 16, 8, launches=[(s, 4, j0, m) for s in (0, 4, 8, 12) for j0, m in ((0, cut), (cut, n - cut))])
    assert len(parts["counters"]) == 8
    assert np.array_equal(one["sums"], parts["sums"]) and one["image"].tobytes() == parts["image"].tobytes() and one["sums"].any()
    total = _total(parts["counters"])
    assert total == _total(one["counters"]) and total[0] == n * 16
    pick = np.sort(np.random.default_rng(2025).choice(n, 500, replace=False))
    e = L.expected(L.scene("soup"), W, H, 16, 8, entries=pick, counters=False)
    _same_texels(one["texels"], e["texels"])
    assert np.array_equal(one["sums"][pick], e["sums"])


def _host(rt, hs, W, H, samples, b, **kw):
    from tests import _lightmap_hdr as L
    return rt.bake_lightmap(hs, W, H, samples, b, seed=L.SEED, return_sums=True, return_texels=True, **kw)


def test_host_level_equals_the_oracle_and_its_slices_add_up(rt, oracle, uploaded):
    """The host level on a small case against the oracle; then across its slice boundaries both ways.  768 x 768 x 6 samples at one
    bounce: the list is shorter than a slice (2^21 paths), so the call goes by sample ranges of 2^21 / n samples -- more than one
    launch; 1800 x 1800 x 1 sample: the list is longer than a slice and goes by texel ranges.  Both equal the device-level chain in
    ONE launch, which has no slices."""
    from tests import _lightmap_hdr as L
    hs = L.scene("soup")
    case = ("soup", 40, 48, 5, 8)
    e = L.expected_case(case)
    image, sums, texels = _host(rt, hs, 40, 48, 5, 8)
    _same_texels(texels, e["texels"])
    assert np.array_equal(sums, e["sums"]) and image.tobytes() == e["image"].tobytes()
    c = rt.get_lightmap_counters()
    assert (c.paths, c.rays) == (e["paths"], e["rays"])
    half = rt.bake_lightmap(hs, 40, 48, 5, 8, seed=L.SEED, sample_range=(2, 3), return_sums=True)[1]
    assert np.array_equal(half, L.expected(hs, 40, 48, 5, 8, sample_range=(2, 3), counters=False)["sums"])
    for W, samples in ((768, 6), (1800, 1)):
        image, sums, texels = _host(rt, hs, W, W, samples, 1)
        n = len(texels)
        slices = rt.abi.RT_LIGHTMAP_SLICE
        assert (n <= slices and n * samples > slices and slices // n < samples) if samples > 1 else n > slices, (W, n)
        assert rt.get_lightmap_counters().paths == n * samples
        one = _chain(rt, uploaded("soup"), W, W, samples, 1)
        _same_texels(texels, one["texels"])
        assert np.array_equal(sums, one["sums"]) and image.tobytes() == one["image"].tobytes() and sums.any()


def test_an_edit_nobody_reported_is_seen_by_the_next_call(rt, oracle):
    from tests import _lightmap_hdr as L
    hs = L.scene("soup")
    W = H = 16
    first = L.expected(hs, W, H, 5, 8, counters=False)
    assert np.array_equal(_host(rt, hs, W, H, 5, 8)[1], first["sums"])
    saved = [(m.base_color.x, m.base_color.y, m.base_color.z) for m in hs.materials]
    try:
        for m in hs.materials:
            m.base_color.x, m.base_color.y, m.base_color.z = 0.9, 0.1, 0.4
        edited = L.expected(hs, W, H, 5, 8, counters=False)
        assert (edited["sums"] != first["sums"]).any(), "the edit must change what the texels see"
        image, sums, _ = _host(rt, hs, W, H, 5, 8)                          # no rt_scene_touch
        assert np.array_equal(sums, edited["sums"]) and image.tobytes() == edited["image"].tobytes()
    finally:
        for m, v in zip(hs.materials, saved):
            m.base_color.x, m.base_color.y, m.base_color.z = v
    assert np.array_equal(_host(rt, hs, W, H, 5, 8)[1], first["sums"])


def test_frames_queries_probes_and_lightmap_bake_are_not_affected(rt, oracle):
    from tests import _lightmap as LM
    from tests import _lightmap_hdr as L
    hs = L.scene("soup")
    rng = np.random.default_rng(3)
    rays = np.zeros((500, 6), np.float32)
    rays[:, :3] = (0.1, 0.2, 3.5)
    rays[:, 3:] = rng.normal(size=(500, 3)) * (0.4, 0.4, 0.1) + (0.0, 0.0, -1.0)
    pos = np.array([(0.0, 0.0, 2.0), (0.5, 0.5, 0.5)], np.float32)

    def others():
        f = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
        q = rt.closest_hits(hs, rays)
        qc = rt.get_query_counters()
        pc, ps = rt.bake_probes(hs, pos, 40, 4, seed=9, return_sums=True)
        prc = rt.get_probe_counters()
        img, arr = LM.padded_image(20, 24, 3, 24, 7)
        rt.lib.rt_set_seed(L.SEED)
        rt.lib.lightmap_bake(C.byref(img), C.byref(hs.scene), 2)
        return f["image"].tobytes(), f["accum"].tobytes(), f["counters"], q.tobytes(), qc, ps.tobytes(), prc, arr.tobytes()
    before = others()
    e = L.expected_case(("soup", 40, 48, 5, 8))
    assert np.array_equal(_host(rt, hs, 40, 48, 5, 8)[1], e["sums"])
    assert rt.get_query_counters() == before[4] and rt.get_probe_counters() == before[6]
    assert others() == before
    assert rt.get_lightmap_counters().paths == e["paths"]            # ... and they leave the lightmap counters alone


def _dilation_cases():
    from tests import _lightmap_hdr as L
    return [(H, W) for H, W in L.DILATE_SIZES]


@pytest.mark.parametrize("size", _dilation_cases(), ids=lambda s: f"{s[1]}x{s[0]}")
def test_dilation_equals_numpy(rt, size):
    import torch
    from tests import _lightmap_hdr as L
    H, W = size
    for name, img in L.dilation_masks(H, W).items():
        for passes in L.DILATE_PASSES:
            t = torch.from_numpy(img).cuda()
            work = torch.empty_like(t)
            assert rt.lib.rt_lightmap_dilate(W, H, passes, t.data_ptr(), work.data_ptr(), None) == 0, rt.last_error()
            want = L.dilate(img, passes)
            got = t.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (name, passes, np.argwhere(got != want)[:4].tolist())
            if name == "islands" and passes == 8 and W >= 12:
                assert (want[0, :12, 3] > 0).all()                    # the islands met


def test_python_wrappers(rt, oracle, uploaded):
    import torch
    from tests import _lightmap_hdr as L
    case = ("soup", 40, 48, 5, 8)
    name, W, H, samples, b = case
    hs = L.scene(name)
    e = L.expected_case(case)
    assert rt.bake_lightmap(hs, W, H, samples, b, seed=L.SEED).tobytes() == e["image"].tobytes()
    want3 = L.dilate(L.resolve(e["texels"], e["sums"], W, H, samples, 2.0), 3)
    assert rt.bake_lightmap(hs, W, H, samples, b, 2.0, 3, seed=L.SEED).tobytes() == want3.tobytes()
    assert ((want3[..., 3] > 1).sum() > 0) and set(np.unique(want3[..., 3])) <= {0.0, 1.0, 2.0, 3.0, 4.0}
    rt.lib.rt_set_seed(L.SEED)                                        # seed=None is rt_get_seed()
    assert rt.bake_lightmap(hs, W, H, samples, max_bounces=b).tobytes() == e["image"].tobytes()
    d, verts = uploaded(name)
    texels, n = rt.lightmap_texels(d, verts, W, H)
    assert n == len(e["texels"])
    _same_texels(texels.cpu().numpy().view(rt.abi.LIGHTMAP_TEXEL_DTYPE).reshape(n), e["texels"])
    image, sums = rt.bake_lightmap_device(d, verts, W, H, samples, b, 2.0, 3, seed=L.SEED, texels=texels, return_sums=True)
    torch.cuda.synchronize()
    assert np.array_equal(sums.cpu().numpy().view(np.uint64), e["sums"]) and image.cpu().numpy().tobytes() == want3.tobytes()
    # progressive: two sample ranges into one buffer
    _, s2 = rt.bake_lightmap_device(d, verts, W, H, samples, b, seed=L.SEED, sample_range=(0, 2), return_sums=True)
    image, s2 = rt.bake_lightmap_device(d, verts, W, H, samples, b, seed=L.SEED, sample_range=(2, 3), sums=s2, return_sums=True)
    torch.cuda.synchronize()
    assert np.array_equal(s2.cpu().numpy().view(np.uint64), e["sums"]) and image.cpu().numpy().tobytes() == e["image"].tobytes()
    t = torch.from_numpy(np.array(e["image"])).cuda()
    assert rt.dilate_lightmap(t, 2).cpu().numpy().tobytes() == L.dilate(e["image"], 2).tobytes()
