"""Temporal accumulation (include/rt_hip.h: rt_temporal_history_bytes, rt_temporal_accumulate, rt_temporal_accumulate_host,
rt_history_*, rt_render_temporal) without a GPU: the exported names, every argument error reported before the device is touched,
and the CONTRACT itself -- its numpy restatement (tests/_temporal.py), which the GPU tests compare the kernel with bit for bit, must
be an accumulator: under equal cameras it is the running mean's recursion, a surface the camera uncovers restarts while the
surfaces that continue keep their history, and real frames of a moving camera get closer to the converged frame."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["rt_temporal_history_bytes", "rt_temporal_accumulate", "rt_temporal_accumulate_host", "rt_history_create", "rt_history_reset",
         "rt_history_destroy", "rt_render_temporal"]
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
        for lib in (rt.lib, rt.diag):
            assert getattr(lib, n) is not None
    for path in ("librt_hip_v1.so", "librt_hip_v2.so"):
        import os
        dll = C.CDLL(os.path.join(os.path.dirname(rt.native.LIB_PATH), path))
        for n in NAMES:
            assert getattr(dll, n) is not None
    assert C.sizeof(abi.RT_Temporal_Params) == 20 and C.sizeof(abi.RT_History_Planes) == 40
    assert callable(rt.temporal_accumulate) and callable(rt.render_temporal) and callable(rt.History)
    assert rt.lib.rt_temporal_history_bytes(1920, 1080) == 48 * 1920 * 1080
    _fails(rt.lib, lambda: rt.lib.rt_temporal_history_bytes(0, 4), "rt_temporal_history_bytes", "image size")
    _fails(rt.lib, lambda: rt.lib.rt_temporal_history_bytes(1 << 15, (1 << 13) + 1), "rt_temporal_history_bytes", "image size")


def test_argument_errors_before_the_device_is_touched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    w = h = 4
    color = np.full((h, w, 3), 7.0, F32)
    plane = np.full((h, w, 3), 0.5, F32)
    out = np.full((h, w, 3), 7.0, F32)
    length = np.full((h, w), 7.0, F32)
    img = np.full((h, w, 3), 0x55, np.uint8)
    hist = np.full(2 * 48 * w * h + 16, 0x55, np.uint8)
    fp = C.POINTER(C.c_float)
    pp = plane.ctypes.data_as(fp)
    cam = abi.Camera()
    cm = C.byref(cam)

    def params(**kw):
        p = abi.RT_Temporal_Params(alpha=0.1, max_history=32, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def planes(**kw):
        f = abi.RT_Features(pp, pp, pp, pp)
        for k, v in kw.items():
            setattr(f, k, v)
        return C.byref(f)

    def hplanes(**kw):
        f = abi.RT_History_Planes(pp, pp, pp, pp, pp)
        for k, v in kw.items():
            setattr(f, k, v)
        return C.byref(f)
    c, o, ln, i = color.ctypes.data, out.ctypes.data, length.ctypes.data, img.ctypes.data
    nan, inf = float("nan"), float("inf")
    bad_params = [(dict(alpha=0.0), "alpha"), (dict(alpha=-0.5), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=nan), "alpha"),
                  (dict(alpha=inf), "alpha"), (dict(max_history=0), "max_history"), (dict(max_history=-3), "max_history"),
                  (dict(max_history=(1 << 20) + 1), "max_history"),
                  (dict(normal_tolerance=0.0), "normal_tolerance"), (dict(normal_tolerance=-1.0), "normal_tolerance"),
                  (dict(normal_tolerance=nan), "normal_tolerance"),
                  (dict(plane_tolerance=0.0), "plane_tolerance"), (dict(plane_tolerance=-inf), "plane_tolerance"),
                  (dict(plane_tolerance=nan), "plane_tolerance"), (dict(demodulate=2), "demodulate"), (dict(demodulate=-1), "demodulate")]
    who = "rt_temporal_accumulate_host"
    host = lib.rt_temporal_accumulate_host
    for kw, word in bad_params:
        _fails(lib, lambda: host(w, h, params(**kw), cm, cm, c, planes(), hplanes(), hplanes(), o, ln, i), who, word)
    _fails(lib, lambda: host(w, h, None, cm, cm, c, planes(), hplanes(), hplanes(), o, ln, i), who, "params are NULL")
    _fails(lib, lambda: host(0, h, params(), cm, cm, c, planes(), hplanes(), hplanes(), o, ln, i), who, "image size")
    _fails(lib, lambda: host(w, -2, params(), cm, cm, c, planes(), hplanes(), hplanes(), o, ln, i), who, "image size")
    _fails(lib, lambda: host(1 << 15, (1 << 13) + 1, params(), cm, cm, c, planes(), hplanes(), hplanes(), o, ln, i), who, "too large")
    _fails(lib, lambda: host(w, h, params(), None, cm, c, planes(), hplanes(), hplanes(), o, ln, i), who, "camera is NULL")
    _fails(lib, lambda: host(w, h, params(), cm, None, c, planes(), hplanes(), hplanes(), o, ln, i), who, "previous_camera is NULL")
    _fails(lib, lambda: host(w, h, params(), cm, cm, None, planes(), hplanes(), hplanes(), o, ln, i), who, "color is NULL")
    _fails(lib, lambda: host(w, h, params(), cm, cm, c, None, hplanes(), hplanes(), o, ln, i), who, "planes is NULL")
    for k in ("coverage", "albedo", "normal", "position"):
        _fails(lib, lambda: host(w, h, params(), cm, cm, c, planes(**{k: None}), hplanes(), hplanes(), o, ln, i), who, k + " is NULL")
    for k in ("color", "length", "coverage", "normal", "position"):
        _fails(lib, lambda: host(w, h, params(), cm, cm, c, planes(), hplanes(**{k: None}), hplanes(), o, ln, i), who, "history_in->" + k)
        _fails(lib, lambda: host(w, h, params(), cm, cm, c, planes(), hplanes(), hplanes(**{k: None}), o, ln, i), who, "history_out->" + k)
    _fails(lib, lambda: host(w, h, params(), cm, cm, c, planes(), hplanes(), None, None, None, None), who, "no output")
    # device level (the pointers are never read: every case fails first)
    who = "rt_temporal_accumulate"
    dev = lib.rt_temporal_accumulate
    a = hist.ctypes.data + (-hist.ctypes.data) % 16
    b = a + 48 * w * h
    p = plane.ctypes.data
    for kw, word in bad_params:
        _fails(lib, lambda: dev(w, h, params(**kw), cm, cm, c, p, p, p, p, a, b, o, ln, i, None), who, word)
    _fails(lib, lambda: dev(w, h, None, cm, cm, c, p, p, p, p, a, b, o, ln, i, None), who, "params are NULL")
    _fails(lib, lambda: dev(w, 0, params(), cm, cm, c, p, p, p, p, a, b, o, ln, i, None), who, "image size")
    _fails(lib, lambda: dev(1 << 14, (1 << 14) + 1, params(), cm, cm, c, p, p, p, p, a, b, o, ln, i, None), who, "too large")
    _fails(lib, lambda: dev(w, h, params(), None, cm, c, p, p, p, p, a, b, o, ln, i, None), who, "camera is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, None, c, p, p, p, p, a, b, o, ln, i, None), who, "previous_camera is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, None, p, p, p, p, a, b, o, ln, i, None), who, "d_color is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, None, p, p, p, a, b, o, ln, i, None), who, "d_coverage is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, None, p, p, a, b, o, ln, i, None), who, "d_albedo is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, None, p, a, b, o, ln, i, None), who, "d_normal is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, p, None, a, b, o, ln, i, None), who, "d_position is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, p, p, a, None, o, ln, i, None), who, "d_history_out is NULL")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, p, p, a, b + 4, o, ln, i, None), who, "16-byte aligned")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, p, p, a + 8, b, o, ln, i, None), who, "16-byte aligned")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, p, p, a, a, o, ln, i, None), who, "overlap")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, p, p, a, b - 16, o, ln, i, None), who, "overlap")
    _fails(lib, lambda: dev(w, h, params(), cm, cm, c, p, p, p, p, b - 16, a, o, ln, i, None), who, "overlap")
    # the history object and the call behind a frame (the scene is never read)
    lib.rt_clear_error()
    assert not lib.rt_history_create(0, 4) and "image size" in rt.last_error()
    assert not lib.rt_history_create(1 << 15, (1 << 13) + 1) and "image size" in rt.last_error()
    _fails(lib, lambda: lib.rt_history_reset(None), "rt_history_reset", "history is NULL")
    lib.rt_history_destroy(None)
    hist_obj = lib.rt_history_create(w, h)
    assert hist_obj and lib.rt_history_reset(hist_obj) == 0
    who = "rt_render_temporal"
    rd = lib.rt_render_temporal
    scene = abi.Scene()
    s = C.byref(scene)

    def image(**kw):
        im = abi.Image()
        im.components, im.pixel_type, im.width, im.stride, im.height = 3, 0, w, w, h
        im.pixels.data, im.pixels.len = i, img.size
        for k_, v in kw.items():
            setattr(im, k_, v)
        return C.byref(im)

    def guided(**kw):
        g = abi.RT_Guided_Params(iterations=2, sigma_color=1.0, sigma_normal=0.2, sigma_position=1.0, demodulate=1)
        for k_, v in kw.items():
            setattr(g, k_, v)
        return C.byref(g)
    for kw, word in bad_params:
        _fails(lib, lambda: rd(s, image(), 2, 2, hist_obj, params(**kw), None, o, o, ln), who, word)
    _fails(lib, lambda: rd(s, image(), 2, 2, hist_obj, params(), guided(iterations=9), o, o, ln), who, "iterations")
    _fails(lib, lambda: rd(s, image(), 2, 2, hist_obj, params(), guided(sigma_normal=nan), o, o, ln), who, "sigma_normal")
    _fails(lib, lambda: rd(None, image(), 2, 2, hist_obj, params(), None, o, o, ln), who, "scene is NULL")
    _fails(lib, lambda: rd(s, None, 2, 2, hist_obj, params(), None, o, o, ln), who, "image is NULL")
    _fails(lib, lambda: rd(s, image(), 2, 2, None, params(), None, o, o, ln), who, "history is NULL")
    _fails(lib, lambda: rd(s, image(), 2, 2, hist_obj, None, None, o, o, ln), who, "params are NULL")
    _fails(lib, lambda: rd(s, image(width=0), 2, 2, hist_obj, params(), None, o, o, ln), who, "image size")
    _fails(lib, lambda: rd(s, image(width=1 << 15, stride=1 << 15, height=(1 << 13) + 1), 2, 2, hist_obj, params(), None, o, o, ln), who, "too large")
    _fails(lib, lambda: rd(s, image(components=2), 2, 2, hist_obj, params(), None, o, o, ln), who, "3 components")
    _fails(lib, lambda: rd(s, image(stride=w - 1), 2, 2, hist_obj, params(), None, o, o, ln), who, "stride")
    _fails(lib, lambda: rd(s, image(), 0, 2, hist_obj, params(), None, o, o, ln), who, "samples")
    _fails(lib, lambda: rd(s, image(), 2, -1, hist_obj, params(), None, o, o, ln), who, "max_bounces")
    _fails(lib, lambda: rd(s, image(width=w + 1, stride=w + 1), 2, 2, hist_obj, params(), None, o, o, ln), who, "and the history 4x4")
    no_pixels = image()
    no_pixels._obj.pixels.data = None
    _fails(lib, lambda: rd(s, no_pixels, 2, 2, hist_obj, params(), None, o, None, None), who, "no output")
    lib.rt_history_destroy(hist_obj)
    assert (color == 7.0).all() and (out == 7.0).all() and (length == 7.0).all() and (img == 0x55).all() and (hist == 0x55).all()
    # the Python entry points report the library's text
    with pytest.raises(RuntimeError, match=r"alpha must be in \(0, 1\]"):
        rt.temporal_accumulate(color, plane[..., 0], plane, plane, plane, cam, alpha=2.0)
    with pytest.raises(RuntimeError, match="image size"):
        rt.History(0, 3)


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
    keep = plane.copy()
    out = np.full((h, w, 3), 7.0, F32)
    img = np.full((h, w, 3), 0x55, np.uint8)
    fp = C.POINTER(C.c_float)
    planes = abi.RT_Features(*[plane.ctypes.data_as(fp)] * 4)
    hout = abi.RT_History_Planes(*[out.ctypes.data_as(fp)] * 5)
    p = abi.RT_Temporal_Params(alpha=0.1, max_history=8, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
    cam = hs.scene.camera
    rt.lib.rt_clear_error()
    assert rt.lib.rt_temporal_accumulate_host(w, h, C.byref(p), C.byref(cam), None, plane.ctypes.data, C.byref(planes), None, C.byref(hout),
                                              out.ctypes.data, out.ctypes.data, img.ctypes.data) == -1
    assert "no HIP device" in rt.last_error()
    rt.lib.rt_clear_error()
    assert rt.lib.rt_temporal_accumulate(w, h, C.byref(p), C.byref(cam), None, plane.ctypes.data, plane.ctypes.data, plane.ctypes.data,
                                         plane.ctypes.data, plane.ctypes.data, None, out.ctypes.data & ~15, out.ctypes.data, None, None,
                                         None) == -1
    assert "no HIP device" in rt.last_error()
    with rt.History(w, h) as history:                     # (creating, resetting and destroying one needs no device)
        history.reset()
        image, _k = rt.scene.make_image(img)
        image.pixels.data = img.ctypes.data
        rt.lib.rt_clear_error()
        assert rt.lib.rt_render_temporal(C.byref(hs.scene), C.byref(image), 2, 2, history.handle, C.byref(p), None, out.ctypes.data,
                                         out.ctypes.data, out.ctypes.data) == -1
        assert "no HIP device" in rt.last_error()
        with pytest.raises(RuntimeError, match="no HIP device"):
            rt.render_temporal(hs, w, h, 2, 2, history)
    assert (out == 7.0).all() and (img == 0x55).all() and plane.tobytes() == keep.tobytes()
    with pytest.raises(RuntimeError, match="no HIP device"):
        rt.temporal_accumulate(plane, plane[..., 0], plane, plane, plane, cam)
    rt.lib.rt_clear_error()


# ---- the contract ---------------------------------------------------------------------------------------------------------------

W2, H2, BAND = 64, 48, 8
FOCAL = 1.4


def _camera_at(x):
    M = np.eye(4, dtype=F32)
    M[0, 3] = x
    return M, F32(FOCAL)


def _two_planes(cam_x, seed):
    """64 x 48 seen from (cam_x, 0, 0) down -z: a sky band on top; below it a far plane z = -6 and, in front of it where x < 0, a
    near plane z = -3, both facing the camera, different albedos, constant irradiance per plane; multiplicative gamma noise of
    shape 16 (the reference driver's default 16 spp).  Pixel (x, y) looks through its centre (fx = x, the contract's convention)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H2, 0:W2].astype(np.float64)
    dx, dy, dz = (xs / (W2 * 0.5) - 1.0) * (W2 / H2), -(ys / (H2 * 0.5) - 1.0), -FOCAL
    near = (cam_x + dx * (3.0 / FOCAL)) < 0.0
    t = np.where(near, 3.0 / FOCAL, 6.0 / FOCAL)
    pos = np.stack([cam_x + dx * t, dy * t, np.full_like(xs, dz) * t], -1)
    cov = np.ones((H2, W2), F32)
    cov[:BAND] = 0.0
    plane_id = np.where(near, 1, 0)
    plane_id[:BAND] = -1
    n = np.broadcast_to(np.array([0.0, 0.0, 1.0], F32), (H2, W2, 3))
    a = np.where(near[..., None], np.array([0.8, 0.3, 0.2], F32), np.array([0.3, 0.6, 0.8], F32)).astype(F32)
    truth = (a * np.where(near, F32(1.0), F32(0.6))[..., None]).astype(F32)
    truth[:BAND] = np.array([0.4, 0.6, 0.9], F32)
    noisy = truth * rng.gamma(16.0, 1.0 / 16.0, (H2, W2, 3)).astype(F32)
    noisy[:BAND] = truth[:BAND]
    c3 = cov[..., None]
    return dict(color=noisy, coverage=cov, albedo=a * c3, normal=(n * F32(0.5) + F32(0.5)) * c3, position=pos.astype(F32) * c3,
                truth=truth, plane_id=plane_id, world=pos)


def _args(S):
    return [S[k] for k in ("color", "coverage", "albedo", "normal", "position")]


@pytest.mark.parametrize("demodulate", [True, False])
def test_equal_cameras_give_the_running_mean_recursion(demodulate):
    """K = 5 frames of different noise over fixed guides: hx = x, ax = 0, the centre tap alone has weight -- the history colour is
    h + (c - h) * a with a = max(1 / (n + 1), alpha), n = min(len, max_history), len' = n + 1 -- bit for bit, and the length
    runs 1, 2, 3, 4 and stays at max_history + 1 = 4 (n is what is capped; the frame itself counts one more)."""
    from tests import _temporal as T
    cam = _camera_at(0.25)
    frames = [_two_planes(0.25, 100 + k) for k in range(5)]
    alpha, cap = F32(0.05), 3
    hist, h_c, h_len = None, None, None
    hit = frames[0]["coverage"] > 0
    for k, S in enumerate(frames):
        r = T.accumulate(*_args(S), cam, cam, hist, alpha=alpha, max_history=cap, demodulate=demodulate)
        m = S["albedo"] + ((F32(1.0) - S["coverage"]) + F32(1e-3))[..., None] if demodulate else None
        c = S["color"] / m if demodulate else S["color"]
        if k == 0:
            h_c, h_len = c, F32(1.0)
        else:
            n = min(h_len, F32(cap))
            a = max(F32(1.0) / (n + F32(1.0)), alpha)
            h_c, h_len = h_c + (c - h_c) * a, n + F32(1.0)
        assert h_len == min(k + 1, cap + 1)
        assert (r["length"][hit] == h_len).all() and (r["length"][~hit] == 0).all()
        assert r["history"]["color"][hit].tobytes() == h_c[hit].tobytes(), k
        want_out = h_c * m if demodulate else h_c
        assert r["out"][hit].tobytes() == want_out[hit].tobytes(), k
        assert r["out"][~hit].tobytes() == S["color"][~hit].tobytes()                # sky: the input, bit for bit
        assert (r["cls"][~hit] == T.SKY).all()
        pid = S["plane_id"]                                                          # inner: the three zero-weight taps are on the pixel's plane too
        inner = np.zeros_like(hit)
        inner[:-1, :-1] = hit[:-1, :-1] & (pid[:-1, :-1] == pid[:-1, 1:]) & (pid[:-1, :-1] == pid[1:, :-1]) & (pid[:-1, :-1] == pid[1:, 1:])
        assert inner.sum() >= 2000
        assert (r["cls"][inner] == (T.NO_HISTORY if k == 0 else T.ALL_VALID)).all()
        assert (r["cls"][hit & ~inner] == (T.NO_HISTORY if k == 0 else T.SOME_VALID)).all()
        hist = r["history"]
    # the accumulated frame is closer to the truth than the last frame alone
    def rms(x):
        return float(np.sqrt(((x[hit].astype(np.float64) - frames[0]["truth"][hit]) ** 2).mean()))
    print("rms of the last frame", rms(frames[-1]["color"]), "accumulated", rms(r["out"]))
    assert rms(r["out"]) < 0.7 * rms(frames[-1]["color"])                            # (a 4-frame mean: 0.5 in expectation)


def test_alpha_one_returns_the_current_frame():
    """a = max(1 / (n + 1), 1) = 1: c' = h + (c - h) * 1, the current frame up to the two roundings of the subtraction and the
    addition, each at most 2^-24 of its result: |c' - c| <= 2^-23 (|c| + |h|).  The length still counts."""
    from tests import _temporal as T
    cam = _camera_at(0.0)
    A, B = _two_planes(0.0, 1), _two_planes(0.0, 2)
    first = T.accumulate(*_args(A), cam, None, None, alpha=1.0, demodulate=False)
    r = T.accumulate(*_args(B), cam, cam, first["history"], alpha=1.0, demodulate=False)
    hit = A["coverage"] > 0
    bound = 2.0 ** -23 * (np.abs(B["color"].astype(np.float64)) + np.abs(A["color"].astype(np.float64)))
    assert (np.abs(r["out"].astype(np.float64) - B["color"]) <= bound).all()
    assert (r["length"][hit] == 2).all()
    assert first["out"].tobytes() == A["color"].tobytes() and (first["length"][hit] == 1).all()   # no history: the frame itself


def test_an_uncovered_surface_restarts_and_continuing_surfaces_keep_their_history():
    """The camera moves 0.6 to the right: the near plane's edge moves left by twice as many pixels as the far plane's points, and
    a strip of the far plane appears that the old camera saw the near plane in front of.  Those pixels fetch near-plane history,
    3 units off their tangent plane at a depth of 6: rejected by the plane test (both planes have the same normal: the normal
    test cannot tell them apart), len = 1.  Pixels whose four taps show their own plane in the old frame: len = 2."""
    from tests import _temporal as T
    old, new = _two_planes(0.0, 5), _two_planes(0.6, 6)
    first = T.accumulate(*_args(old), _camera_at(0.0), None, None)
    r = T.accumulate(*_args(new), _camera_at(0.6), _camera_at(0.0), first["history"])
    # where the old camera saw every pixel's point, in float64, independently of the restatement
    P = new["world"]
    hx = ((P[..., 0] * FOCAL / -P[..., 2]) / (W2 / H2) + 1.0) * (W2 * 0.5)
    hy = (-(P[..., 1] * FOCAL / -P[..., 2]) + 1.0) * (H2 * 0.5)
    x0, y0 = np.floor(hx).astype(int), np.floor(hy).astype(int)
    inside = (x0 >= 0) & (x0 + 1 < W2) & (y0 >= 0) & (y0 + 1 < H2)
    xc, yc = np.clip(x0, 0, W2 - 2), np.clip(y0, 0, H2 - 2)
    taps = np.stack([old["plane_id"][yc + j, xc + i] for j in (0, 1) for i in (0, 1)], -1)
    mine = new["plane_id"][..., None]
    uncovered = inside & (new["plane_id"] == 0) & (taps == 1).all(-1)
    continuing = inside & (new["plane_id"] >= 0) & (taps == mine).all(-1)
    print("uncovered", int(uncovered.sum()), "continuing", int(continuing.sum()),
          "near", int((continuing & (new["plane_id"] == 1)).sum()), "far", int((continuing & (new["plane_id"] == 0)).sum()))
    assert uncovered.sum() >= 50 and (continuing & (new["plane_id"] == 1)).sum() >= 50 and (continuing & (new["plane_id"] == 0)).sum() >= 50
    assert (r["length"][uncovered] == 1).all() and (r["cls"][uncovered] == T.PLANE_REJECTED).all()
    assert (r["length"][continuing] == 2).all() and (r["cls"][continuing] == T.ALL_VALID).all()
    assert r["out"][uncovered].tobytes() == _demodulated_and_back(new)[uncovered].tobytes()
    sky = new["coverage"] == 0
    assert r["out"][sky].tobytes() == new["color"][sky].tobytes() and (r["length"][sky] == 0).all()
    # with the plane test off the strip is reused wrongly (the test is what keeps it out)
    off = T.accumulate(*_args(new), _camera_at(0.6), _camera_at(0.0), first["history"], plane_tolerance=float("inf"))
    assert (off["length"][uncovered] == 2).all()


def _demodulated_and_back(S):
    m = S["albedo"] + ((F32(1.0) - S["coverage"]) + F32(1e-3))[..., None]
    return (S["color"] / m) * m


SHAPE = (40, 24, 4, 4)                       # width, height, samples, bounces of the real frames
STEPS = (0.3, 0.6, 1.0, 1.7, 2.5)            # image motion of frame k + 1 against frame k, in pixels at the scene's median depth


@pytest.fixture(scope="module")
def sequences():
    """name -> (six (noisy linear frame, feature planes, camera), the 2048 spp frame of the last camera): once, shared, read-only.
    The camera moves along its own x axis."""
    from raytracing_c_amd.configs import load_config
    from tests import _features as F, _oracle, _temporal as T
    w, h, s, b = SHAPE
    out = {}
    for name in ("quad", "spheres"):
        hs = load_config(name)[0]
        cam = hs.scene.camera
        M0, focal = T.camera_of(cam)
        origin = M0[:3, 3].copy()
        frames, offset = [], 0.0
        pixel = None
        try:
            for k in range(6):
                for i in range(3):
                    cam.view_matrix.rows[i][3] = float(F32(origin[i] + F32(offset) * M0[i, 0]))
                planes = F.resolve(F.expected_cached("%s@%d" % (name, k), hs, w, h, s, b)["sums"], s)
                noisy = _oracle.render(hs, w, h, s, b, seed=1000 + k)["linear"]
                for a in (noisy, *planes.values()):
                    a.setflags(write=False)
                frames.append((noisy, planes, T.camera_of(cam)))
                if pixel is None:                                                    # the world size of a pixel at the median depth
                    full = planes["coverage"] == 1.0
                    depth = np.median(np.linalg.norm(planes["position"][full].astype(np.float64) - origin, axis=1))
                    pixel = depth * (w / h) / (float(focal) * w * 0.5)
                if k < 5:
                    offset += STEPS[k] * pixel
            clean = _oracle.render(hs, w, h, 2048, b)["linear"]
            clean.setflags(write=False)
        finally:
            for i in range(3):
                cam.view_matrix.rows[i][3] = float(origin[i])
        out[name] = (frames, clean)
    return out


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("name", ["quad", "spheres"])
def test_real_frames_of_a_moving_camera_get_closer_to_the_converged_frame(sequences, name, demodulate):
    from tests import _temporal as T
    frames, clean = sequences[name]
    hist, prev = None, None
    for noisy, pl, cam in frames:
        r = T.accumulate(noisy, pl["coverage"], pl["albedo"], pl["normal"], pl["position"], cam, prev, hist, demodulate=demodulate)
        hist, prev = r["history"], cam
    keep = (pl["coverage"] == 1.0) & (r["length"] >= 2)
    assert keep.sum() >= 100, keep.sum()

    def rms(a):
        return float(np.sqrt(((a[keep].astype(np.float64) - clean[keep]) ** 2).mean()))
    print(name, "demodulate", demodulate, "pixels", int(keep.sum()), "mean length", float(r["length"][keep].mean()),
          "rms last noisy frame", rms(noisy), "accumulated", rms(r["out"]), "ratio", rms(r["out"]) / rms(noisy))
    assert rms(r["out"]) < rms(noisy)
