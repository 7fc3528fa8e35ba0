"""Feature-guided upsampling on the GPU (rt_guided_upsample, rt_guided_upsample_host, rt_render_upsampled; rt_upsample.hip) against
the numpy float32 restatement of its contract (tests/_upsample.py): equal BIT FOR BIT (tobytes), f32 and u8, through the host path
and once through the device path on a non-default stream.

The kernel's workgroup writes a 16 x 8 tile of full pixels over the 8 x 4 low pixels under it and a halo of one.  Sizes (w x h):
2 x 2 -- one low pixel, every tap but one outside --, 4 x 2, 6 x 10 and 66 x 38 (wl odd); 130 x 70 and 258 x 66: 9 x 9 and 17 x 9 tiles, ragged
against them; the strips 2 x 260 and 516 x 2: 33 tiles in a column and in a row.  The inputs (tests/_upsample.py: case) have a
sky band, partial coverages, a block of pixels with positions of 3e19 that takes the sum_w > 0 fallback, and low planes jittered
against the full ones.  That a lost halo, clamped taps, exchanged weight sets and a division in place of the fallback would each
change these very inputs' output -- at every multi-tile size at least 100 pixels -- is shown on the CPU (tests/test_upsample_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import _upsample as U

pytestmark = pytest.mark.gpu

F32 = np.float32
ORDER = ("coverage", "albedo", "normal", "position")


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


_wants = {}


def want(w, h, sigmas=U.SIGMAS, demodulate=True):
    """(out, image) of the restatement, once per case, shared, read-only."""
    key = (w, h, sigmas, demodulate)
    if key not in _wants:
        c = U.case(w, h)
        out = U.upsample(c["color_low"], c["low"], c["full"], *sigmas, demodulate)
        img = U.encode_u8(out)
        out.setflags(write=False)
        img.setflags(write=False)
        _wants[key] = (out, img)
    return _wants[key]


def _same(got, expected, what):
    assert got.dtype == expected.dtype and got.shape == expected.shape, what
    bad = np.argwhere(got.view(np.uint32 if got.dtype == F32 else np.uint8) != expected.view(np.uint32 if got.dtype == F32 else np.uint8))
    assert got.tobytes() == expected.tobytes(), (what, len(bad), bad[:6].tolist())


def _host(rt, w, h, sigmas, demodulate):
    c = U.case(w, h)
    return rt.guided_upsample(c["color_low"], c["low"], c["full"], sigma_normal=sigmas[0], sigma_position=sigmas[1],
                              demodulate=demodulate, image=True)


def _device(rt, w, h, sigmas, demodulate):
    """rt.guided_upsample on torch tensors, on a stream that is not the default one."""
    import torch
    c = U.case(w, h)
    side = torch.cuda.Stream()
    col = torch.from_numpy(np.array(c["color_low"])).cuda()
    low = {k: torch.from_numpy(np.array(c["low"][k])).cuda() for k in ORDER}
    full = {k: torch.from_numpy(np.array(c["full"][k])).cuda() for k in ORDER}
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out, img = rt.guided_upsample(col, low, full, sigma_normal=sigmas[0], sigma_position=sigmas[1], demodulate=demodulate, image=True)
    side.synchronize()
    return out.cpu().numpy(), img.cpu().numpy()


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("w,h", U.SIZES)
def test_upsample_host(rt, w, h, demodulate):
    out, img = _host(rt, w, h, U.SIGMAS, demodulate)
    _same(out, want(w, h, U.SIGMAS, demodulate)[0], "out")
    _same(img, want(w, h, U.SIGMAS, demodulate)[1], "image")
    assert np.isfinite(out).all()
    c = U.case(w, h)
    if c["aimed"].any() and demodulate:                                               # the fallback: the low pixel under the full pixel
        ys, xs = np.nonzero(c["aimed"])
        m_q = c["low"]["albedo"] + ((F32(1.0) - c["low"]["coverage"]) + F32(1e-3))[..., None]
        m_p = c["full"]["albedo"] + ((F32(1.0) - c["full"]["coverage"]) + F32(1e-3))[..., None]
        assert out[ys, xs].tobytes() == ((c["color_low"] / m_q)[ys >> 1, xs >> 1] * m_p[ys, xs]).tobytes()


@pytest.mark.parametrize("sigmas", U.SIGMA_SETS[1:])
@pytest.mark.parametrize("w,h", [(66, 38), (130, 70), (2, 260), (516, 2)])
def test_upsample_one_sigma_infinite(rt, w, h, sigmas):
    out, img = _host(rt, w, h, sigmas, True)
    _same(out, want(w, h, sigmas)[0], "out")
    _same(img, want(w, h, sigmas)[1], "image")
    assert out.tobytes() != want(w, h)[0].tobytes()


@pytest.mark.parametrize("w,h,demodulate", [(130, 70, True), (258, 66, False), (6, 10, True)])
def test_upsample_device_level_on_torch_tensors(rt, w, h, demodulate):
    out, img = _device(rt, w, h, U.SIGMAS, demodulate)
    _same(out, want(w, h, U.SIGMAS, demodulate)[0], "out")
    _same(img, want(w, h, U.SIGMAS, demodulate)[1], "image")


def test_upsample_without_an_albedo_when_demodulate_is_off(rt):
    w, h = 66, 38
    c = U.case(w, h)
    low, full = dict(c["low"], albedo=None), dict(c["full"], albedo=None)
    out = rt.guided_upsample(c["color_low"], low, full, sigma_normal=U.SIGMAS[0], sigma_position=U.SIGMAS[1], demodulate=False)
    _same(out, want(w, h, U.SIGMAS, False)[0], "out")
    with pytest.raises(RuntimeError, match="albedo is NULL and demodulate is set"):
        rt.guided_upsample(c["color_low"], low, full, sigma_normal=U.SIGMAS[0], sigma_position=U.SIGMAS[1], demodulate=True)


def test_upsample_every_output_alone_and_both(rt):
    """d_out alone, d_image alone, both -- on the host level and on the device level; what is not wanted is not written."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    w, h = 130, 70
    c = U.case(w, h)
    w_out, w_img = want(w, h)
    o = rt.guided_upsample(c["color_low"], c["low"], c["full"], sigma_normal=U.SIGMAS[0], sigma_position=U.SIGMAS[1])
    _same(o, w_out, "host out alone")
    none, i = rt.guided_upsample(c["color_low"], c["low"], c["full"], sigma_normal=U.SIGMAS[0], sigma_position=U.SIGMAS[1], image=True,
                                 out=False)
    assert none is None
    _same(i, w_img, "host image alone")
    t = [torch.from_numpy(np.array(a)).cuda() for a in (c["color_low"], *[c["low"][k] for k in ORDER], *[c["full"][k] for k in ORDER])]
    work = torch.empty((rt.lib.rt_guided_upsample_work_bytes(w, h),), dtype=torch.uint8, device="cuda")
    p = abi.RT_Upsample_Params(*U.SIGMAS, 1, 0)
    for flags in ((True, False), (False, True), (True, True)):
        out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
        img = torch.full((h, w, 3), 0x55, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert rt.lib.rt_guided_upsample(w, h, C.byref(p), *[x.data_ptr() for x in t], out.data_ptr() if flags[0] else None,
                                         img.data_ptr() if flags[1] else None, work.data_ptr(), None) == 0, rt.last_error()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == w_out.tobytes() if flags[0] else bool((out == 7.0).all()), flags
        assert img.cpu().numpy().tobytes() == w_img.tobytes() if flags[1] else bool((img == 0x55).all()), flags


# ---- behind a frame -----------------------------------------------------------------------------------------------------------------

SHAPE = (64, 36, 16, 8)                                                               # w, h, samples, max_bounces
GUIDE_SAMPLES = 4
SEED = 77


def _spheres():
    from raytracing_c_amd.configs import load_config
    return load_config("spheres")[0]


def _pieces(rt, hs, guide_samples, guided):
    """rt_render_upsampled's pipeline called piece by piece: dict(linear_low, linear_upsampled, linear_out or None, image, counters)."""
    from raytracing_c_amd import ctypes_abi as abi
    w, h, s, b = SHAPE
    f = rt.render_frame(hs, w // 2, h // 2, s, b, seed=SEED, want_linear=True)
    low = rt.render_features(hs, w // 2, h // 2, s, b)
    full = rt.render_features(hs, w, h, guide_samples or s, b)
    up, img = rt.guided_upsample(f["linear"], low, full, sigma_normal=0.2, sigma_position=SIGMA_POSITION, image=True)
    res = dict(linear_low=f["linear"], linear_upsampled=up, linear_out=None, image=img, counters=f["counters"])
    if guided is not None:
        res["linear_out"], res["image"] = rt.guided_denoise(up, *[full[k] for k in ORDER], image=True, **guided)
    return res


SIGMA_POSITION = 0.3
GUIDED = dict(iterations=3, sigma_color=1.0, sigma_normal=0.2, sigma_position=SIGMA_POSITION, demodulate=True)


@pytest.mark.parametrize("guide_samples,guided", [(GUIDE_SAMPLES, GUIDED), (GUIDE_SAMPLES, None), (0, GUIDED)])
def test_render_upsampled_is_its_pieces(rt, oracle, guide_samples, guided):
    hs = _spheres()
    w, h, s, b = SHAPE
    before_frame = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
    before_denoised = rt.render_denoised(hs, 48, 40, 4, 4, seed=7, sigma_position=SIGMA_POSITION)
    pieces = _pieces(rt, hs, guide_samples, guided)
    got = rt.render_upsampled(hs, w, h, s, b, seed=SEED, guide_samples=guide_samples, sigma_normal=0.2, sigma_position=SIGMA_POSITION,
                              guided=guided)
    assert rt.render.get_counters() == pieces["counters"]                            # the 32 x 18 frame's
    _same(got["linear_low"], pieces["linear_low"], "linear_low")
    _same(got["linear_upsampled"], pieces["linear_upsampled"], "linear_upsampled")
    if guided is not None:
        _same(got["linear_out"], pieces["linear_out"], "linear_out")
        assert got["linear_out"].tobytes() != got["linear_upsampled"].tobytes()
    else:
        assert "linear_out" not in got
    _same(got["image"], pieces["image"], "image")                                     # the encoding of the last stage
    from tests import _guided as G
    _same(got["image"], G.encode_u8(got["linear_out"] if guided is not None else got["linear_upsampled"]), "image")
    assert np.isfinite(got["linear_upsampled"]).all() and len(np.unique(got["linear_upsampled"])) > 1000
    # what follows returns what it returns without the call before it
    after_frame = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
    after_denoised = rt.render_denoised(hs, 48, 40, 4, 4, seed=7, sigma_position=SIGMA_POSITION)
    assert after_frame["image"].tobytes() == before_frame["image"].tobytes() and after_frame["accum"].tobytes() == before_frame["accum"].tobytes()
    assert after_frame["counters"] == before_frame["counters"]
    for k in before_denoised:
        assert after_denoised[k].tobytes() == before_denoised[k].tobytes(), k


def test_render_upsampled_fewer_guide_samples_change_the_guides(rt, oracle):
    """guide_samples reaches the full-resolution feature pass: 4 and 16 samples give other planes, and so another frame; the low
    frame is the same."""
    hs = _spheres()
    w, h, s, b = SHAPE
    a = rt.render_upsampled(hs, w, h, s, b, seed=SEED, guide_samples=GUIDE_SAMPLES, sigma_position=SIGMA_POSITION)
    z = rt.render_upsampled(hs, w, h, s, b, seed=SEED, guide_samples=0, sigma_position=SIGMA_POSITION)
    full = rt.render_upsampled(hs, w, h, s, b, seed=SEED, guide_samples=s, sigma_position=SIGMA_POSITION)
    assert a["linear_low"].tobytes() == z["linear_low"].tobytes()
    assert a["linear_upsampled"].tobytes() != z["linear_upsampled"].tobytes()
    for k in z:
        assert z[k].tobytes() == full[k].tobytes(), k                                 # 0 means the frame's sample count
    with pytest.raises(RuntimeError, match="guide_samples"):
        rt.render_upsampled(hs, w, h, s, b, guide_samples=s + 1, sigma_position=SIGMA_POSITION)
    with pytest.raises(RuntimeError, match="odd"):
        rt.render_upsampled(hs, w + 1, h, s, b, sigma_position=SIGMA_POSITION)
