"""The guided denoiser on the GPU (rt_guided_denoise, rt_guided_denoise_host, rt_render_denoised; rt_guided.hip) against the
numpy float32 restatement of its contract (tests/_guided.py): equal BIT FOR BIT (tobytes) -- every step up to one that exceeds both
image sides, both ping-pong parities, both demodulate settings, partial coverage and sky, weights that underflow through denormals
to 0, image sizes ragged against the 32 x 8 tile and degenerate ones, through the host call and through the device call on a
non-default stream; output aliasing the input; u8 / f32 / both; behind a frame; no effect on frames, queries and feature passes;
the staging given back.

ACROSS TILE BORDERS.  A workgroup filters a 32 x 8 tile of one phase sub-lattice; 37 x 21 has a second tile along x at step 1 only
and along y up to step 2.  With two or more tiles per phase in the direction named -- so that halo slots are filled from pixels
another workgroup filters, tile % tiles_x != 0, and blocks of the shorter phases own no pixel -- the filter is compared at
steps 1, 2, 4 (131 x 70, tiles_x != tiles_y), 8 (259 x 67) and 16 (513 x 129) in x and y, at steps 32 and 64 (2079 x 12) and 128
(4200 x 5) in x, and at steps 32, 64, 128 in y (19 x 1055, where phases_x = width < step), every iteration count from 1 up to each
size's last (BORDER_SIZES); behind a frame at 136 x 72 (steps 1, 2, 4 in x and y, 8 in y).  That a halo lost at such a step would
change at least 100 pixels of these very inputs is shown on the CPU (tests/test_guided_cpu.py).  Also: +inf sigmas, all and each."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
SIGMAS = (0.6, 0.2, 0.05)                       # colour, normal, position of the random-plane cases


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _planes(w, h, seed=1):
    """Random inputs: coverage from {0, 1/4, 1/2, 3/4, 1} with a block of sky (every feature 0 there); positions scaled by up to
    1e12 on one pixel in five, so that pl * pl * k_p runs from ~1 past 1e20 (r * r denormal) to 1e27 (0)."""
    rng = np.random.default_rng(seed)
    cov = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0], F32), (h, w))
    cov[h // 4:h // 4 + 6, w // 2:w // 2 + 9] = 0.0
    hit = (cov > 0)[..., None]
    normal = (rng.random((h, w, 3), dtype=F32) * cov[..., None]).astype(F32)
    albedo = (rng.random((h, w, 3), dtype=F32) * cov[..., None]).astype(F32)
    scale = np.where(rng.random((h, w)) < 0.2, 10.0 ** rng.uniform(6.0, 12.0, (h, w)), 1.0)[..., None]
    position = (rng.normal(size=(h, w, 3)) * 3.0 * scale * hit).astype(F32)
    color = (rng.gamma(2.0, 0.4, (h, w, 3))).astype(F32)
    out = dict(color=color, coverage=cov, albedo=albedo, normal=normal, position=position)
    for a in out.values():
        a.setflags(write=False)
    return out


_inputs = {}


def _shared(w, h):
    if (w, h) not in _inputs:
        _inputs[(w, h)] = _planes(w, h)
    return _inputs[(w, h)]


def _want(P, iterations, demodulate):
    from tests import _guided as G
    return G.guided(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], iterations, *SIGMAS, demodulate)


# Sizes at which a phase sub-lattice spans SEVERAL 32 x 8 tiles at the steps named: (w, h) -> (the largest iteration count run,
# {axis (0: x, 1: y): the steps at which the launch has >= 2 tiles along it AND a lost halo would change >= 100 pixels}).  The
# claims are proved of these very inputs on the CPU (tests/test_guided_cpu.py: test_the_border_sizes_would_catch_a_lost_halo);
# the smaller steps of each size have more tiles still.  Strips reach steps 32 .. 128 without the pixel count; in the tall one
# phases_x = width < step, so phases_x != phases_y.  A strip's long side is just past 2048 / 4096 / 1024 and not a multiple of its
# steps: the phases differ in length by one, so the last tile of the shorter ones is a block that owns no pixel; its short side
# is what gives the single sub-lattice column or row past the border its 100 pixels.
BORDER_SIZES = {
    (131, 70): (3, {0: (1, 2, 4), 1: (1, 2, 4)}),               # 5 x 9, 3 x 5, 2 x 3 tiles: tiles_x != tiles_y
    (259, 67): (4, {0: (8,), 1: (8,)}),                         # 2 x 2 at step 8; 3 x 3 at step 4
    (513, 129): (5, {0: (2, 16), 1: (2, 16)}),                  # 2 x 2 at step 16; 9 x 9 at step 2, the 9th empty in every phase but 0
    (2079, 12): (7, {0: (32, 64)}),                             # 65 or 64 sub-lattice columns at step 32, 33 or 32 at step 64
    (4200, 5): (8, {0: (128,)}),                                # 33 or 32 at step 128
    (19, 1055): (8, {1: (32, 64, 128)}),                        # 9 or 8 sub-lattice rows at step 128, 19 x 128 phases
}
_RECTANGLES = [(131, 70), (259, 67), (513, 129)]
_STRIPS = [(2079, 12), (4200, 5), (19, 1055)]
_COMBINATIONS = [("host", True), ("device", False), ("host", False), ("device", True)]
_wants = {}


def _shared_want(w, h, iterations, demodulate):
    """The restatement's output for _shared(w, h): computed once, shared by the paths, read-only."""
    key = (w, h, iterations, demodulate)
    if key not in _wants:
        _wants[key] = _want(_shared(w, h), iterations, demodulate)
        _wants[key].setflags(write=False)
    return _wants[key]


def _differing(got, want, step):
    """"" when equal in bits, else how many pixels differ and where the first ones sit on the last step's decomposition."""
    ys, xs = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=2))
    if len(ys) == 0:
        return ""
    first = ["(x, y) (%d, %d) phase (%d, %d) tile (%d, %d)" % (x, y, x % step, y % step, (x // step) // 32, (y // step) // 8)
             for x, y in zip(xs[:6].tolist(), ys[:6].tolist())]
    return "%d pixels differ; last step %d: %s" % (len(ys), step, "; ".join(first))


def _compare_planes(rt, w, h, iterations, demodulate, path, sigmas=SIGMAS):
    from tests import _guided as G
    P = _shared(w, h)
    if sigmas is SIGMAS:
        want = _shared_want(w, h, iterations, demodulate)
    else:
        want = G.guided(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], iterations, *sigmas, demodulate)
    kw = dict(iterations=iterations, sigma_color=sigmas[0], sigma_normal=sigmas[1], sigma_position=sigmas[2], demodulate=demodulate)
    if path == "host":
        got = rt.guided_denoise(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], **kw)
    else:
        got = _side_stream_call(rt, P, **kw)
    assert got.dtype == F32 and got.shape == want.shape
    message = _differing(got, want, 1 << (iterations - 1))
    assert not message, message
    assert got.tobytes() == want.tobytes()
    sky = P["coverage"] == 0
    assert sky.sum() >= 50 and got[sky].tobytes() == P["color"][sky].tobytes()
    assert np.isfinite(got).all()
    return got


def _side_stream_call(rt, P, **kw):
    """rt.guided_denoise on torch tensors, on a stream that is not the default one."""
    import torch
    side = torch.cuda.Stream()
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in P.items()}
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = rt.guided_denoise(t["color"], t["coverage"], t["albedo"], t["normal"], t["position"], **kw)
    side.synchronize()
    if isinstance(got, tuple):
        return tuple(g.cpu().numpy() for g in got)
    return got.cpu().numpy()


def test_some_weights_underflow_through_denormals():
    """(of the inputs, on the CPU: the case the random planes are scaled for exists)"""
    P = _shared(37, 21)
    N = P["normal"] * F32(2.0) - P["coverage"][..., None]
    e = P["position"][:, 1:] - P["position"][:, :-1]
    pl = (N[:, :-1] * e).sum(axis=2).astype(np.float64)
    D = pl * pl / (SIGMAS[2] * SIGMAS[2])
    r2 = 0.140625 / (1.0 + D) ** 2
    assert (D > 1e20).sum() >= 10 and ((r2 < 1.17e-38) & (r2 > 1.5e-45)).sum() >= 3 and (r2 < 1e-46).sum() >= 3


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 8])
def test_random_planes_37x21(rt, iterations, demodulate, path):
    """37 x 21: odd, ragged against the tile, two tiles wide and three high at step 1.  At 5 iterations the last step is 16 in a
    height of 21 (most taps fall outside), at 8 it is 128, beyond both sides: every pixel is its own sub-lattice."""
    P = _shared(37, 21)
    want = _want(P, iterations, demodulate)
    kw = dict(iterations=iterations, sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2], demodulate=demodulate)
    if path == "host":
        got = rt.guided_denoise(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], **kw)
    else:
        got = _side_stream_call(rt, P, **kw)
    assert got.dtype == F32 and got.shape == want.shape
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(diff) == 0, (len(diff), diff[:4].tolist())
    assert got.tobytes() == want.tobytes()
    sky = P["coverage"] == 0
    assert sky.sum() >= 50 and got[sky].tobytes() == P["color"][sky].tobytes()
    assert np.isfinite(got).all()


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("w,h,iterations", [(w, h, k) for w, h in _RECTANGLES for k in range(1, BORDER_SIZES[(w, h)][0] + 1)])
def test_random_planes_across_tile_borders(rt, w, h, iterations, demodulate, path):
    """Where 37 x 21 has ONE tile per phase in x from step 2 and in y from step 4 on, these sizes have at least two in both
    directions at every step they run (BORDER_SIZES): the block -> (phase, tile) -> origin decode with tile % tiles_x != 0, halo
    columns and rows filled from the pixels another workgroup filters, tiles_x != tiles_y, blocks of the smaller phases that own no
    pixel.  Every iteration count from 1, so that the first one that fails names the step."""
    _compare_planes(rt, w, h, iterations, demodulate, path)


@pytest.mark.parametrize("w,h,iterations,path,demodulate", [(w, h, k) + _COMBINATIONS[(k + i) % 4] for i, (w, h) in enumerate(_STRIPS)
                                                            for k in range(1, BORDER_SIZES[(w, h)][0] + 1)])
def test_random_planes_on_strips(rt, w, h, iterations, path, demodulate):
    """Steps 32, 64 and 128 with two tiles: along x on strips of 12 and 5 rows, along y on one of 19 columns, where phases_x =
    min(step, width) = 19 while phases_y = step.  The four (path, demodulate) combinations take turns over the iteration counts:
    each occurs at least once per strip."""
    _compare_planes(rt, w, h, iterations, demodulate, path)


INF = float("inf")


@pytest.mark.parametrize("sigmas", [(INF, INF, INF), (INF, SIGMAS[1], SIGMAS[2]), (SIGMAS[0], INF, SIGMAS[2]), (SIGMAS[0], SIGMAS[1], INF)],
                         ids=["all", "color", "normal", "position"])
def test_infinite_sigmas(rt, sigmas):
    """rt_hip.h: a sigma of +inf switches its term off, k = 1 / (inf * inf) = 0 -- on the GPU as in the restatement, bit for bit,
    all three and each alone, at 131 x 70 with 3 iterations.  The term must be finite to be switched off (0 * inf is NaN on both
    sides, and the contract asks for finite inputs): the largest pl * pl these planes can give stays far below the f32 maximum."""
    w, h = 131, 70
    P = _shared(w, h)
    pl_max = 3.0 * (2.0 * float(P["normal"].max()) + 1.0) * 2.0 * float(np.abs(P["position"]).max())
    assert pl_max * pl_max < 1e36
    got = _compare_planes(rt, w, h, 3, True, "host", sigmas)
    _compare_planes(rt, w, h, 3, False, "device", sigmas)
    assert got.tobytes() != _shared_want(w, h, 3, True).tobytes()             # (the sigma reached the kernel)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 40), (40, 1), (33, 9)])
def test_degenerate_sizes(rt, w, h):
    rng = np.random.default_rng(w * 100 + h)
    cov = rng.choice(np.array([0.0, 0.5, 1.0, 1.0], F32), (h, w))
    P = dict(color=rng.random((h, w, 3), dtype=F32), coverage=cov, albedo=rng.random((h, w, 3), dtype=F32),
             normal=rng.random((h, w, 3), dtype=F32), position=rng.normal(size=(h, w, 3)).astype(F32))
    for iterations, demodulate in ((1, True), (4, False), (7, True)):
        want = _want(P, iterations, demodulate)
        kw = dict(iterations=iterations, sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2], demodulate=demodulate)
        got = rt.guided_denoise(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], **kw)
        assert got.tobytes() == want.tobytes(), (iterations, demodulate)
        assert _side_stream_call(rt, P, **kw).tobytes() == want.tobytes(), (iterations, demodulate)


def _raw_device(rt, P, iterations, demodulate, want_out, want_image, alias=False):
    """rt_guided_denoise itself: (f32 output or None, u8 output or None); alias: d_out is d_color."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    h, w = P["coverage"].shape
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in P.items()}
    out = t["color"] if alias else torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
    img = torch.full((h, w, 3), 0x55, dtype=torch.uint8, device="cuda")
    work = torch.empty((rt.lib.rt_guided_work_bytes(w, h),), dtype=torch.uint8, device="cuda")
    p = abi.RT_Guided_Params(iterations=iterations, sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2],
                             demodulate=1 if demodulate else 0)
    torch.cuda.synchronize()
    rc = rt.lib.rt_guided_denoise(w, h, C.byref(p), t["color"].data_ptr(), t["coverage"].data_ptr(),
                                  t["albedo"].data_ptr() if demodulate else None, t["normal"].data_ptr(), t["position"].data_ptr(),
                                  out.data_ptr() if want_out else None, img.data_ptr() if want_image else None, work.data_ptr(), None)
    assert rc == 0, rt.last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), img.cpu().numpy()


def test_output_may_alias_the_colour_input(rt):
    P = _shared(37, 21)
    for iterations, demodulate in ((1, True), (4, True), (3, False)):
        want = _want(P, iterations, demodulate)
        apart, _ = _raw_device(rt, P, iterations, demodulate, True, False)
        alias, _ = _raw_device(rt, P, iterations, demodulate, True, False, alias=True)
        assert apart.tobytes() == want.tobytes() and alias.tobytes() == want.tobytes(), (iterations, demodulate)


def test_u8_only_f32_only_and_both(rt):
    from tests import _guided as G
    P = _shared(37, 21)
    want = _want(P, 3, True)
    enc = G.encode_u8(want)
    assert len(np.unique(enc)) > 100 and (enc == 255).any()                   # the encode is exercised over its range, clamp included
    out, img = _raw_device(rt, P, 3, True, True, True)
    assert out.tobytes() == want.tobytes() and img.tobytes() == enc.tobytes()
    out, img = _raw_device(rt, P, 3, True, True, False)
    assert out.tobytes() == want.tobytes() and (img == 0x55).all()
    out, img = _raw_device(rt, P, 3, True, False, True)
    assert (out == 7.0).all() and img.tobytes() == enc.tobytes()
    # the host call and the Python wrapper
    got, gimg = rt.guided_denoise(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], iterations=3,
                                  sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2], image=True)
    assert got.tobytes() == want.tobytes() and gimg.tobytes() == enc.tobytes()
    from raytracing_c_amd import ctypes_abi as abi
    fp = C.POINTER(C.c_float)
    planes = abi.RT_Features(*[np.ascontiguousarray(P[k]).ctypes.data_as(fp) for k in ("coverage", "albedo", "normal", "position")])
    p = abi.RT_Guided_Params(iterations=3, sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2], demodulate=1)
    only = np.full((21, 37, 3), 0x55, np.uint8)
    assert rt.lib.rt_guided_denoise_host(37, 21, C.byref(p), P["color"].ctypes.data, C.byref(planes), None, only.ctypes.data) == 0, rt.last_error()
    assert only.tobytes() == enc.tobytes()


def _chain(rt, hs, w, h, s, b):
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _guided as G
    frame = rt.render_frame(hs, w, h, s, b, want_linear=True)
    feats = rt.render_features(hs, w, h, s, b)
    cov = feats["coverage"]
    assert (cov == 1).sum() >= 50 and (cov == 0).sum() >= 50
    sp = G.sigma_position(feats["position"], cov)
    for demodulate in (True, False):
        want = G.guided(frame["linear"], cov, feats["albedo"], feats["normal"], feats["position"], 4, 1.0, 0.2, sp, demodulate)
        enc = G.encode_u8(want)
        got = rt.guided_denoise(frame["linear"], cov, feats["albedo"], feats["normal"], feats["position"], demodulate=demodulate)
        assert got.tobytes() == want.tobytes(), (demodulate, _differing(got, want, 8))      # (sigma_position: the wrapper's default)
        r = rt.render_denoised(hs, w, h, s, b, demodulate=demodulate)
        assert r["linear_noisy"].tobytes() == frame["linear"].tobytes()
        assert r["linear_denoised"].tobytes() == want.tobytes(), (demodulate, _differing(r["linear_denoised"], want, 8))
        assert r["image"].tobytes() == enc.tobytes()
    # the Image's layout: stride > width, 4 components; what is not a pixel's r, g, b stays
    stride, comp = w + 3, 4
    pixels = np.full((h, stride, comp), 0x55, np.uint8)
    image = abi.Image()
    image.components, image.pixel_type, image.width, image.stride, image.height = comp, 0, w, stride, h
    image.pixels.data, image.pixels.len = pixels.ctypes.data, pixels.size
    p = abi.RT_Guided_Params(iterations=4, sigma_color=1.0, sigma_normal=0.2, sigma_position=sp, demodulate=0)
    rt.lib.rt_set_seed(0x1234ABCD)
    assert rt.lib.rt_render_denoised(C.byref(hs.scene), C.byref(image), s, b, C.byref(p), None, None) == 0, rt.last_error()
    assert pixels[:, :w, :3].tobytes() == enc.tobytes()
    assert (pixels[:, w:] == 0x55).all() and (pixels[:, :, 3] == 0x55).all()
    assert rt.render.get_counters() == frame["counters"]                      # the frame's counters describe the call


def test_behind_a_frame_random_scene(rt, oracle):
    from tests.test_gpu_random_scenes import make_scene
    _chain(rt, make_scene(6, 400), 40, 24, 4, 8)


def test_behind_a_frame_across_tile_borders(rt, oracle):
    """136 x 72, few samples: the chain's 4 iterations have 5 x 9, 3 x 5, 2 x 3 and 1 x 2 tiles per phase (steps 1, 2, 4, 8), where
    40 x 24 has one from step 2 on -- the filter behind a real frame's buffers, and the padded Image, with tile borders in them."""
    from tests.test_gpu_random_scenes import make_scene
    _chain(rt, make_scene(6, 400), 136, 72, 2, 4)


def test_behind_a_frame_passthrough_scene(rt, oracle):
    from tests import _features as F
    _chain(rt, F.passthrough_scene(), 16, 16, 4, 3)


def test_frames_queries_and_feature_passes_are_not_affected(rt, oracle):
    from tests import _features as F
    from tests.test_gpu_features import _camera_rays
    hs = F.passthrough_scene()
    rays = _camera_rays(hs, 500)
    P = _shared(37, 21)

    def everything():
        f = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
        q = rt.closest_hits(hs, rays)
        qc = rt.get_query_counters()
        feats = rt.render_features(hs, 16, 16, 2, 3)
        return f["image"].tobytes(), f["accum"].tobytes(), f["counters"], q.tobytes(), qc, feats["sums"].tobytes()
    before = everything()
    want = _want(P, 4, True)
    kw = dict(iterations=4, sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2])
    assert rt.guided_denoise(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], **kw).tobytes() == want.tobytes()
    assert rt.get_query_counters() == before[4] and rt.render.get_counters() == before[2]
    assert _side_stream_call(rt, P, **kw).tobytes() == want.tobytes()
    assert rt.get_query_counters() == before[4] and rt.render.get_counters() == before[2]
    assert everything() == before
    # a filter call while a frame is in flight on a lane
    ticket, pixels, keep = rt.frame_begin(hs, 48, 40, 4, 4, seed=7)
    got = rt.guided_denoise(P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], **kw)
    counters = rt.frame_end(ticket)
    assert got.tobytes() == want.tobytes() and pixels.tobytes() == before[0] and counters == before[2]


def test_the_staging_is_given_back(rt, diag):
    """The host-level staging is 131 B per pixel -- 13 f32 in, 3 f32 and 3 u8 out, 64 B of work -- kept between calls and released
    by the teardown of the device's staging, to the byte (the diagnostic library's own count)."""
    P = _shared(37, 21)
    want = _want(P, 2, True)
    kw = dict(iterations=2, sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2], image=True, lib=diag)
    args = [P[k] for k in ("color", "coverage", "albedo", "normal", "position")]
    assert rt.guided_denoise(*args, **kw)[0].tobytes() == want.tobytes()      # (the device slot itself exists now)
    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    base = diag.rt_diag_device_bytes_live()
    assert rt.guided_denoise(*args, **kw)[0].tobytes() == want.tobytes()
    held = diag.rt_diag_device_bytes_live() - base
    assert held == 37 * 21 * (13 * 4 + 3 * 4 + 3 + 64), held
    assert rt.guided_denoise(*args, **kw)[0].tobytes() == want.tobytes()
    assert diag.rt_diag_device_bytes_live() - base == held                    # warm: nothing more
    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    assert diag.rt_diag_device_bytes_live() == base
    assert rt.guided_denoise(*args, **kw)[0].tobytes() == want.tobytes()      # ... and it comes back when needed
    assert diag.rt_diag_release_staging() == 0
