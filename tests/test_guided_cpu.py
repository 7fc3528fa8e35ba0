"""The guided denoiser (include/rt_hip.h: rt_guided_work_bytes, rt_guided_denoise, rt_guided_denoise_host, rt_render_denoised)
without a GPU: the exported names, every argument error reported before the device is touched, and the CONTRACT itself -- its
numpy restatement (tests/_guided.py), which the GPU tests compare the kernel with bit for bit, must be a denoiser: a constant
stays constant, edges between surfaces stay, noise drops on real frames, sky is returned as it came, and with every
edge-stopping term switched off it is the plain 5 x 5 B-spline a-trous transform.  And of the GPU tests' own inputs: at every
size, step and direction where they claim to compare the filter across the borders of its 32 x 8 workgroup tiles, a halo that never
arrived would change at least 100 pixels."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["rt_guided_work_bytes", "rt_guided_denoise", "rt_guided_denoise_host", "rt_render_denoised"]
F32 = np.float32


def _fails(lib, call, *words):
    from raytracing_c_amd.native import last_error
    lib.rt_clear_error()
    assert call() == -1
    msg = last_error(lib)
    for w in words:
        assert w in msg, msg
    lib.rt_clear_error()


def test_symbols_and_python_entry_points():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    for n in NAMES:
        assert n in abi.EXPORTED_SYMBOLS
        assert getattr(rt.lib, n) is not None and getattr(rt.diag, n) is not None
    assert C.sizeof(abi.RT_Guided_Params) == 20
    assert callable(rt.guided_denoise) and callable(rt.render_denoised)
    assert rt.lib.rt_guided_work_bytes(1920, 1080) == 64 * 1920 * 1080
    _fails(rt.lib, lambda: rt.lib.rt_guided_work_bytes(0, 4), "rt_guided_work_bytes", "image size")
    _fails(rt.lib, lambda: rt.lib.rt_guided_work_bytes(1 << 15, (1 << 13) + 1), "rt_guided_work_bytes", "image size")


def test_argument_errors_before_the_device_is_touched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    w = h = 4
    color = np.full((h, w, 3), 7.0, F32)
    plane = np.full((h, w, 3), 0.5, F32)
    out = np.full((h, w, 3), 7.0, F32)
    img = np.full((h, w, 3), 0x55, np.uint8)
    fp = C.POINTER(C.c_float)
    pp = plane.ctypes.data_as(fp)

    def params(**kw):
        p = abi.RT_Guided_Params(iterations=2, sigma_color=1.0, sigma_normal=0.2, sigma_position=1.0, demodulate=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def planes(**kw):
        f = abi.RT_Features(pp, pp, pp, pp)
        for k, v in kw.items():
            setattr(f, k, v)
        return C.byref(f)
    c, o, i = color.ctypes.data, out.ctypes.data, img.ctypes.data
    bad_params = [(dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(iterations=-1), "iterations"),
                  (dict(sigma_color=0.0), "sigma_color"), (dict(sigma_color=-1.0), "sigma_color"), (dict(sigma_color=float("nan")), "sigma_color"),
                  (dict(sigma_normal=0.0), "sigma_normal"), (dict(sigma_normal=float("nan")), "sigma_normal"),
                  (dict(sigma_position=-0.5), "sigma_position"), (dict(sigma_position=float("nan")), "sigma_position"),
                  (dict(demodulate=2), "demodulate")]
    who = "rt_guided_denoise_host"
    host = lib.rt_guided_denoise_host
    for kw, word in bad_params:
        _fails(lib, lambda: host(w, h, params(**kw), c, planes(), o, i), who, word)
    _fails(lib, lambda: host(w, h, None, c, planes(), o, i), who, "params are NULL")
    _fails(lib, lambda: host(0, h, params(), c, planes(), o, i), who, "image size")
    _fails(lib, lambda: host(w, -2, params(), c, planes(), o, i), who, "image size")
    _fails(lib, lambda: host(1 << 15, (1 << 13) + 1, params(), c, planes(), o, i), who, "too large")
    _fails(lib, lambda: host(w, h, params(), None, planes(), o, i), who, "color is NULL")
    _fails(lib, lambda: host(w, h, params(), c, None, o, i), who, "planes is NULL")
    _fails(lib, lambda: host(w, h, params(), c, planes(coverage=None), o, i), who, "coverage is NULL")
    _fails(lib, lambda: host(w, h, params(), c, planes(albedo=None), o, i), who, "albedo is NULL")
    _fails(lib, lambda: host(w, h, params(), c, planes(normal=None), o, i), who, "normal is NULL")
    _fails(lib, lambda: host(w, h, params(), c, planes(position=None), o, i), who, "position is NULL")
    _fails(lib, lambda: host(w, h, params(), c, planes(), None, None), who, "no output")
    # device level (the pointers are never read: every case fails first)
    who = "rt_guided_denoise"
    dev = lib.rt_guided_denoise
    work = np.zeros(64 * w * h + 16, np.uint8)
    k = work.ctypes.data + (-work.ctypes.data) % 16
    p = plane.ctypes.data
    for kw, word in bad_params:
        _fails(lib, lambda: dev(w, h, params(**kw), c, p, p, p, p, o, i, k, None), who, word)
    _fails(lib, lambda: dev(w, h, None, c, p, p, p, p, o, i, k, None), who, "params are NULL")
    _fails(lib, lambda: dev(w, 0, params(), c, p, p, p, p, o, i, k, None), who, "image size")
    _fails(lib, lambda: dev(1 << 14, (1 << 14) + 1, params(), c, p, p, p, p, o, i, k, None), who, "too large")
    _fails(lib, lambda: dev(w, h, params(), None, p, p, p, p, o, i, k, None), who, "d_color is NULL")
    _fails(lib, lambda: dev(w, h, params(), c, None, p, p, p, o, i, k, None), who, "d_coverage is NULL")
    _fails(lib, lambda: dev(w, h, params(), c, p, None, p, p, o, i, k, None), who, "d_albedo is NULL")
    _fails(lib, lambda: dev(w, h, params(), c, p, p, None, p, o, i, k, None), who, "d_normal is NULL")
    _fails(lib, lambda: dev(w, h, params(), c, p, p, p, None, o, i, k, None), who, "d_position is NULL")
    _fails(lib, lambda: dev(w, h, params(), c, p, p, p, p, None, None, k, None), who, "no output")
    _fails(lib, lambda: dev(w, h, params(), c, p, p, p, p, o, i, None, None), who, "d_work is NULL")
    _fails(lib, lambda: dev(w, h, params(), c, p, p, p, p, o, i, k + 4, None), who, "16-byte aligned")
    # behind a frame (the scene is never read)
    who = "rt_render_denoised"
    rd = lib.rt_render_denoised
    scene = abi.Scene()
    s = C.byref(scene)

    def image(**kw):
        im = abi.Image()
        im.components, im.pixel_type, im.width, im.stride, im.height = 3, 0, w, w, h
        im.pixels.data, im.pixels.len = i, img.size
        for k_, v in kw.items():
            setattr(im, k_, v)
        return C.byref(im)
    for kw, word in bad_params:
        _fails(lib, lambda: rd(s, image(), 2, 2, params(**kw), o, o), who, word)
    _fails(lib, lambda: rd(None, image(), 2, 2, params(), o, o), who, "scene is NULL")
    _fails(lib, lambda: rd(s, None, 2, 2, params(), o, o), who, "image is NULL")
    _fails(lib, lambda: rd(s, image(), 2, 2, None, o, o), who, "params are NULL")
    _fails(lib, lambda: rd(s, image(width=0), 2, 2, params(), o, o), who, "image size")
    _fails(lib, lambda: rd(s, image(width=1 << 15, stride=1 << 15, height=(1 << 13) + 1), 2, 2, params(), o, o), who, "too large")
    _fails(lib, lambda: rd(s, image(components=2), 2, 2, params(), o, o), who, "3 components")
    _fails(lib, lambda: rd(s, image(stride=w - 1), 2, 2, params(), o, o), who, "stride")
    _fails(lib, lambda: rd(s, image(), 0, 2, params(), o, o), who, "samples")
    _fails(lib, lambda: rd(s, image(), 1 << 40, 2, params(), o, o), who, "samples")
    _fails(lib, lambda: rd(s, image(), 2, -1, params(), o, o), who, "max_bounces")
    no_pixels = image()
    no_pixels._obj.pixels.data = None
    _fails(lib, lambda: rd(s, no_pixels, 2, 2, params(), o, None), who, "no output")
    assert (color == 7.0).all() and (out == 7.0).all() and (img == 0x55).all() and not work.any()
    # the Python entry points report the library's text
    with pytest.raises(RuntimeError, match="iterations must be 1 .. 8"):
        rt.guided_denoise(color, plane[..., 0], plane, plane, plane, iterations=9, sigma_position=1.0)


def test_fails_loudly_without_a_device_and_touches_nothing():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("quad")
    w = h = 8
    plane = np.full((h, w, 3), 0.5, F32)
    out = np.full((h, w, 3), 7.0, F32)
    img = np.full((h, w, 3), 0x55, np.uint8)
    fp = C.POINTER(C.c_float)
    planes = abi.RT_Features(*[plane.ctypes.data_as(fp)] * 4)
    p = abi.RT_Guided_Params(iterations=2, sigma_color=1.0, sigma_normal=0.2, sigma_position=1.0, demodulate=1)
    rt.lib.rt_clear_error()
    assert rt.lib.rt_guided_denoise_host(w, h, C.byref(p), plane.ctypes.data, C.byref(planes), out.ctypes.data, img.ctypes.data) == -1
    assert "no HIP device" in rt.last_error()
    image, _k = rt.scene.make_image(img)
    image.pixels.data = img.ctypes.data
    rt.lib.rt_clear_error()
    assert rt.lib.rt_render_denoised(C.byref(hs.scene), C.byref(image), 2, 2, C.byref(p), out.ctypes.data, out.ctypes.data) == -1
    assert "no HIP device" in rt.last_error()
    assert (out == 7.0).all() and (img == 0x55).all()
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.guided_denoise(plane, plane[..., 0], plane, plane, plane, sigma_position=1.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.render_denoised(hs, w, h, 2, 2, sigma_position=1.0)
    rt.lib.rt_clear_error()


# ---- the contract ---------------------------------------------------------------------------------------------------------------

def test_a_constant_image_stays_constant():
    """c' = sum(w c) / sum(w) of a constant c: each of the 25 products and 24 + 24 additions and the division rounds once, so an
    iteration moves the value by at most 27 x 2^-24 relative, whatever the features make of the weights."""
    from tests import _guided as G
    rng = np.random.default_rng(11)
    h, w = 19, 23
    cov = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], F32), (h, w))
    normal = rng.random((h, w, 3), dtype=F32)
    position = (rng.normal(size=(h, w, 3)) * 3.0).astype(F32)
    albedo = rng.random((h, w, 3), dtype=F32)
    value = np.array([0.7310586, 1.9, 0.0123], F32)
    color = np.broadcast_to(value, (h, w, 3)).copy()
    for it in (1, 4, 8):
        out = G.guided(color, cov, albedo, normal, position, it, 0.3, 0.2, 0.5, demodulate=False)
        rel = np.abs(out.astype(np.float64) / value.astype(np.float64) - 1.0).max()
        assert rel <= it * 27 * 2.0 ** -24, (it, rel)


def _two_planes():
    """64 x 48: a sky band on top; below it two planes that meet at x = 32 with different normals and albedos, constant irradiance
    per side; multiplicative gamma noise of shape 16 -- the mean of 16 exponentially distributed samples, relative sigma 0.25: the
    reference driver's default 16 spp, the frame the filter is meant for.  (Measured once at shape 4, relative sigma 0.5: the
    columns next to the edge kept their side's mean within 3.5 %, but columns far from it wandered by up to 6.4 % -- residual
    noise of the separate sub-lattices, not leakage across the edge.)"""
    rng = np.random.default_rng(2024)
    h, w, band, edge = 48, 64, 8, 32
    cov = np.ones((h, w), F32)
    cov[:band] = 0.0
    ys, xs = np.mgrid[0:h, 0:w].astype(F32)
    left = xs < edge
    n = np.where(left[..., None], np.array([0.0, 0.0, 1.0], F32), np.array([1.0, 0.0, 0.0], F32)).astype(F32)
    normal = (n * F32(0.5) + F32(0.5)) * cov[..., None]
    a = np.where(left[..., None], np.array([0.8, 0.3, 0.2], F32), np.array([0.3, 0.6, 0.8], F32)).astype(F32)
    albedo = a * cov[..., None]
    pos = np.where(left[..., None], np.stack([xs * 0.1, ys * 0.1, np.zeros_like(xs)], -1),
                   np.stack([np.full_like(xs, edge * 0.1), ys * 0.1, (edge - xs) * 0.1], -1)).astype(F32) * cov[..., None]
    truth = (a * np.where(left, F32(1.0), F32(0.6))[..., None]).astype(F32)
    truth[:band] = np.array([0.4, 0.6, 0.9], F32)
    noise = rng.gamma(16.0, 1.0 / 16.0, (h, w, 3)).astype(F32)
    noisy = truth * noise
    noisy[:band] = truth[:band]
    return dict(cov=cov, normal=normal, albedo=albedo, position=pos, truth=truth, noisy=noisy, band=band, edge=edge, left=left)


def test_edges_between_surfaces_stay_and_noise_drops():
    from tests import _guided as G
    S = _two_planes()
    sp = G.sigma_position(S["position"], S["cov"])
    out = G.guided(S["noisy"], S["cov"], S["albedo"], S["normal"], S["position"], 4, 1.0, 0.2, sp, True)
    band, edge = S["band"], S["edge"]
    assert out[:band].tobytes() == S["noisy"][:band].tobytes()
    worst = 0.0
    for x in list(range(0, edge - 1)) + list(range(edge + 2, 64)):          # two or more pixels from the edge
        got = out[band:, x].astype(np.float64).mean(axis=0)
        want = S["truth"][band, x].astype(np.float64)
        worst = max(worst, float(np.abs(got / want - 1.0).max()))
    print("largest deviation of a column mean from its side's value:", worst)
    assert worst <= 0.05

    def rms(img, side):
        m = side.copy()
        m[:band] = False
        return float(np.sqrt(((img[m].astype(np.float64) - S["truth"][m]) ** 2).mean()))
    sides = sorted(((rms(S["noisy"], m), rms(out, m)) for m in (S["left"], ~S["left"])))
    print("rms noisy -> filtered, quieter side first:", sides)
    before, after = sides[0]
    assert after * 5.0 <= before


SHAPE = (40, 24, 4, 4)                       # width, height, samples, bounces of the real frames


@pytest.fixture(scope="module")
def frames():
    """name -> (noisy linear frame, its feature planes, a 2048 spp frame): once, shared, read-only."""
    from raytracing_c_amd.configs import load_config
    from tests import _features as F, _oracle
    from tests.test_gpu_random_scenes import make_scene
    w, h, s, b = SHAPE
    scenes = dict(quad=load_config("quad")[0], spheres=load_config("spheres")[0], random6=make_scene(6, 400),
                  passthrough=F.passthrough_scene())
    out = {}
    for name, hs in scenes.items():
        planes = F.resolve(F.expected_cached(name, hs, w, h, s, b)["sums"], s)
        noisy = _oracle.render(hs, w, h, s, b)["linear"]
        clean = _oracle.render(hs, w, h, 2048, b)["linear"]
        for a in (noisy, clean, *planes.values()):
            a.setflags(write=False)
        out[name] = (noisy, planes, clean)
    return out


@pytest.mark.parametrize("name", ["quad", "spheres", "random6", "passthrough"])
def test_real_frames_get_closer_to_the_converged_frame(frames, name):
    from tests import _guided as G
    noisy, pl, clean = frames[name]
    full, sky = pl["coverage"] == 1.0, pl["coverage"] == 0.0
    assert full.sum() >= 100 and sky.sum() >= 100

    def rms(a):
        return float(np.sqrt(((a[full].astype(np.float64) - clean[full]) ** 2).mean()))
    sp = G.sigma_position(pl["position"], pl["coverage"])
    for demodulate in (True, False):
        out = G.guided(noisy, pl["coverage"], pl["albedo"], pl["normal"], pl["position"], 4, 1.0, 0.2, sp, demodulate)
        print(name, "demodulate", demodulate, "rms noisy", rms(noisy), "filtered", rms(out))
        assert rms(out) < rms(noisy)
        if name == "quad":
            assert rms(out) <= 0.2 * rms(noisy)
        assert out[sky].tobytes() == noisy[sky].tobytes()


def test_infinite_sigmas_give_the_plain_atrous_transform():
    """Every edge-stopping term off: r = 1, the weights are the B-spline's; computed independently in float64, with the weights
    of the taps inside the image renormalised."""
    from tests import _guided as G
    rng = np.random.default_rng(5)
    h, w, it = 21, 37, 4
    color = rng.random((h, w, 3), dtype=F32)
    cov = np.ones((h, w), F32)
    normal = rng.random((h, w, 3), dtype=F32)
    position = rng.normal(size=(h, w, 3)).astype(F32)
    inf = float("inf")
    got = G.guided(color, cov, None, normal, position, it, inf, inf, inf, demodulate=False)
    k1 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    c = color.astype(np.float64)
    for i in range(it):
        s = 1 << i
        num, den = np.zeros_like(c), np.zeros((h, w))
        for y in range(h):
            for x in range(w):
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        yy, xx = y + s * dy, x + s * dx
                        if 0 <= yy < h and 0 <= xx < w:
                            wt = k1[dy + 2] * k1[dx + 2]
                            num[y, x] += wt * c[yy, xx]
                            den[y, x] += wt
        c = num / den[..., None]
    assert np.abs(got - c).max() <= 1e-5


# ---- the sizes the GPU tests run: would they catch a fault in the filter's tiling? ---------------------------------------------------

def _tiling(w, h, s):
    """The launch of one step as the header of rt_guided.hip states it: (phases_x, phases_y, tiles_x, tiles_y, the number of
    blocks of a phase other than (0, 0) whose tile holds no pixel).  Block = phase + n_phases * tile, phase = px + phases_x * py,
    tile = tx + tiles_x * ty; its pixels are x = px + s * (32 tx + i), y = py + s * (8 ty + j)."""
    phases_x, phases_y = min(s, w), min(s, h)
    sub_x, sub_y = (w + s - 1) // s, (h + s - 1) // s                          # the largest sub-lattice, that of phase (0, 0)
    tiles_x, tiles_y = (sub_x + 31) // 32, (sub_y + 7) // 8
    empty = sum(1 for py in range(phases_y) for px in range(phases_x) for ty in range(tiles_y) for tx in range(tiles_x)
                if (px, py) != (0, 0) and (px + s * 32 * tx >= w or py + s * 8 * ty >= h))
    return phases_x, phases_y, tiles_x, tiles_y, empty


def _border_claims():
    from tests.test_gpu_guided import BORDER_SIZES
    return [(w, h, s, axis) for (w, h), (_, axes) in BORDER_SIZES.items() for axis, steps in axes.items() for s in steps]


def test_the_lost_halo_variant_leaves_the_restatement_alone():
    """lost_halo=None is the contract, byte for byte (every expectation above is unchanged); a step that is not run loses nothing."""
    from tests import _guided as G
    from tests.test_gpu_guided import SIGMAS, _planes
    P = _planes(37, 21)
    a = (P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], 3, *SIGMAS, True)
    want = G.guided(*a)
    assert G.guided(*a, lost_halo=None).tobytes() == want.tobytes()
    never = dict(step=8, axis=0)
    assert G.guided(*a, lost_halo=never).tobytes() == want.tobytes() and "pairs" not in never
    lost = dict(step=1, axis=0)                                               # 37 wide: two tiles at step 1
    assert G.guided(*a, lost_halo=lost).tobytes() != want.tobytes() and lost["pairs"] > 0


@pytest.mark.parametrize("w,h,step,axis", _border_claims())
def test_the_border_sizes_would_catch_a_lost_halo(w, h, step, axis):
    """A table of sizes proves nothing by itself.  For every (size, step, axis) that tests/test_gpu_guided.py claims to compare
    across tile borders: the launch has at least two tiles along the axis and blocks that own no pixel; at least 100 (pixel, tap)
    pairs cross a tile border with a weight that counts; and a filter whose halo never arrived at that step (_guided.guided's
    lost_halo) would differ from the contract in the bits of at least 100 pixels OF THESE INPUTS."""
    from tests import _guided as G
    from tests.test_gpu_guided import BORDER_SIZES, SIGMAS, _planes
    phases_x, phases_y, tiles_x, tiles_y, empty = _tiling(w, h, step)
    assert (tiles_x, tiles_y)[axis] >= 2, (tiles_x, tiles_y)
    if step == 1:
        assert (phases_x, phases_y) == (1, 1)                                 # the image itself: there is no phase but (0, 0)
    elif (w, h, step) == (131, 70, 2):
        assert empty == 0                                                     # 66 or 65 columns, 35 rows: 3 x 5 tiles in every phase
    else:                                                                     # (513 x 129 has step 2 with such blocks)
        assert empty >= 1, empty
    iterations = step.bit_length()                                            # the count whose last step this is
    assert iterations <= BORDER_SIZES[(w, h)][0]
    if (w, h) == (19, 1055):
        assert (phases_x, phases_y) == (19, step)                             # phases_x = width < step
    P = _planes(w, h)
    a = (P["color"], P["coverage"], P["albedo"], P["normal"], P["position"], iterations, *SIGMAS, True)
    lost = dict(step=step, axis=axis)
    want, without = G.guided(*a), G.guided(*a, lost_halo=lost)
    differing = int((want.view(np.uint32) != without.view(np.uint32)).any(axis=2).sum())
    print(w, h, "step", step, "axis", axis, "tiles", tiles_x, tiles_y, "empty blocks", empty, "pairs", lost["pairs"], "pixels", differing)
    assert lost["pairs"] >= 100, lost["pairs"]
    assert differing >= 100, differing


def test_37x21_has_one_tile_in_x_from_step_2_on():
    """Why the sizes above exist: the workhorse of the GPU tests never has a second tile along x beyond step 1 (y: beyond 2)."""
    for i in range(1, 8):
        assert _tiling(37, 21, 1 << i)[2] == 1                                # ceil(ceil(37 / s) / 32) = 1 for s >= 2
    assert [_tiling(37, 21, s)[3] for s in (1, 2, 4)] == [3, 2, 1]
