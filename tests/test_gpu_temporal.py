"""Temporal accumulation on the GPU (rt_temporal_accumulate, rt_temporal_accumulate_host, rt_history_*, rt_render_temporal;
rt_temporal.hip) against the numpy float32 restatement of its contract (tests/_temporal.py): equal BIT FOR BIT (tobytes) -- the
output, every plane of the new history, the length and the u8 image; every class of pixel the contract distinguishes; both
demodulate settings, each tolerance finite and +inf; sizes ragged against the 32 x 8 tile and degenerate ones; through the host call
and through the device call on a non-default stream; no history; output aliasing the input; every output alone; behind a frame with
equal and with moving cameras, with and without the guided filter (also at 136 x 72, where the filter has tile borders); a first frame against rt_render_denoised; reset; no effect on frames, queries, feature passes and the
guided filter; the staging given back and a history used after that."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
TOLERANCES = [(0.3, 0.02), (INF, 0.02), (0.3, INF)]           # normal, plane
KW = dict(alpha=0.2, max_history=3)


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _rot_y(angle, t):
    M = np.eye(4, dtype=F32)
    c, s = np.cos(angle), np.sin(angle)
    M[0, 0], M[0, 2], M[2, 0], M[2, 2] = c, s, -s, c
    M[:3, 3] = t
    return M


FOCAL = F32(1.4)
CAM_OLD = (_rot_y(0.0, (0.0, 0.0, 0.0)), FOCAL)
CAM_NEW = (_rot_y(0.11, (0.45, -0.12, 0.05)), FOCAL)


def _view(cam, w, h, seed, special):
    """What `cam` sees of two planes facing +z -- far z = -6, near z = -3 where x < -0.2 -- as feature planes with coverage from
    {1/4 .. 1}, a block of sky, and when `special`: a block of pixels whose point lies behind both cameras, a block with another
    normal, a block pushed half a unit off its plane, single pixels nudged by a thousandth."""
    rng = np.random.default_rng(seed)
    M, focal = cam
    M = M.astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.stack([((xs + 0.13) / (w * 0.5) - 1.0) * (w / h), -((ys + 0.13) / (h * 0.5) - 1.0), np.full_like(xs, -float(focal))], -1)
    D = d @ M[:3, :3].T
    o = M[:3, 3]
    s_near, s_far = (-3.0 - o[2]) / D[..., 2], (-6.0 - o[2]) / D[..., 2]
    near = (o[0] + D[..., 0] * s_near) < -0.2
    W = o + D * np.where(near, s_near, s_far)[..., None]
    n = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (h, w, 3)).copy()
    cov = rng.choice(np.array([0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 1.0, 1.0], F32), (h, w))
    W += rng.normal(size=(h, w, 3)) * 1e-3 * (rng.random((h, w, 1)) < 0.3)
    if special:
        W[h // 2:h // 2 + 4, w // 8:w // 8 + 7] = (0.3, 0.2, 4.0)                     # behind both cameras
        n[h // 8:h // 8 + 4, w // 2:w // 2 + 8] = (0.8, 0.0, 0.6)                     # another normal
        W[(3 * h) // 4:(3 * h) // 4 + 4, w // 2:w // 2 + 8, 2] += 0.5                 # off the plane
        if w * h > 27:
            cov[0:3, 0:min(9, w)] = 0.0
    else:
        cov[h // 3:h // 3 + 5, (2 * w) // 3:(2 * w) // 3 + 6] = 0.0                   # sky in the history where the new frame has none
    c3 = cov[..., None]
    albedo = (rng.random((h, w, 3), dtype=F32) * c3).astype(F32)
    color = rng.gamma(2.0, 0.4, (h, w, 3)).astype(F32)
    out = dict(color=color, coverage=cov, albedo=albedo, normal=((n * 0.5 + 0.5) * c3).astype(F32), position=(W * c3).astype(F32))
    for a in out.values():
        a.setflags(write=False)
    return out


def _args(P):
    return [P[k] for k in ("color", "coverage", "albedo", "normal", "position")]


_cases = {}


def _case(w, h):
    """(the new frame's planes, the history of two old frames) -- once per size, shared, read-only."""
    from tests import _temporal as T
    if (w, h) not in _cases:
        hist = None
        for seed in (1, 2):
            hist = T.accumulate(*_args(_view(CAM_OLD, w, h, seed + 10 * w, False)), CAM_OLD, CAM_OLD, hist, **KW)["history"]
        for a in hist.values():
            a.setflags(write=False)
        _cases[(w, h)] = (_view(CAM_NEW, w, h, 3 + 10 * w, True), hist)
    return _cases[(w, h)]


def _want(P, hist, demodulate, tol, prev=CAM_OLD, kw=KW):
    from tests import _temporal as T
    r = T.accumulate(*_args(P), CAM_NEW, prev, hist, normal_tolerance=tol[0], plane_tolerance=tol[1], demodulate=demodulate, **kw)
    r["image"] = T.encode_u8(r["out"])
    return r


def _same(got, want, what=""):
    for k in ("out", "length", "image"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        diff = np.argwhere(got[k] != want[k])
        assert got[k].tobytes() == want[k].tobytes(), (what, k, len(diff), diff[:4].tolist())
    for k in ("color", "length", "coverage", "normal", "position"):
        assert got["history"][k].tobytes() == want["history"][k].tobytes(), (what, "history", k)


def _host(rt, P, hist, demodulate, tol, prev=CAM_OLD, lib=None, kw=KW):
    return rt.temporal_accumulate(*_args(P), CAM_NEW, prev, hist, normal_tolerance=tol[0], plane_tolerance=tol[1], demodulate=demodulate,
                                  image=True, lib=lib, **kw)


def _device(rt, P, hist, demodulate, tol, prev=CAM_OLD, kw=KW):
    """rt.temporal_accumulate on torch tensors, on a stream that is not the default one."""
    import torch
    from tests import _temporal as T
    side = torch.cuda.Stream()
    t = [torch.from_numpy(np.array(a)).cuda() for a in _args(P)]
    th = None if hist is None else torch.from_numpy(T.pack_history(hist)).cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = rt.temporal_accumulate(*t, CAM_NEW, prev, th, normal_tolerance=tol[0], plane_tolerance=tol[1], demodulate=demodulate,
                                     image=True, **kw)
    side.synchronize()
    rec = got["history"].cpu().numpy()
    assert not rec[2, ..., 3].any()                                                   # the fourth component of (W, 0)
    return dict(out=got["out"].cpu().numpy(), length=got["length"].cpu().numpy(), image=got["image"].cpu().numpy(),
                history=T.unpack_history(rec))


def test_every_class_occurs():
    """(of the inputs, on the CPU: the cases the synthetic planes are made for exist)"""
    from tests import _temporal as T
    P, hist = _case(37, 21)
    cls = _want(P, hist, True, TOLERANCES[0])["cls"]
    counts = {T.CLASS_NAMES[k]: int((cls == k).sum()) for k in range(9)}
    print(counts)
    for k in (T.SKY, T.BEHIND, T.OUTSIDE, T.NORMAL_REJECTED, T.PLANE_REJECTED, T.SOME_VALID, T.ALL_VALID):
        assert (cls == k).sum() >= 20, counts
    assert (cls == T.NO_HISTORY).sum() == 0
    assert len(np.unique(hist["length"])) >= 3                                         # 0 (sky), 1 and 2 frames of history


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("tol", TOLERANCES)
def test_synthetic_planes_37x21(rt, tol, demodulate, path):
    """37 x 21: odd, ragged against the tile, two tiles wide and three high."""
    P, hist = _case(37, 21)
    want = _want(P, hist, demodulate, tol)
    got = (_host if path == "host" else _device)(rt, P, hist, demodulate, tol)
    _same(got, want)
    sky = P["coverage"] == 0
    assert got["out"][sky].tobytes() == P["color"][sky].tobytes() and (got["length"][sky] == 0).all()
    assert np.isfinite(got["out"]).all() and len(np.unique(got["length"])) >= 4
    assert len(np.unique(want["image"])) > 100 and (want["image"] == 255).any()       # the encode over its range, clamp included


@pytest.mark.parametrize("w,h", [(1, 1), (1, 40), (40, 1), (33, 9)])
def test_degenerate_sizes(rt, w, h):
    P, hist = _case(w, h)
    for demodulate, tol in ((True, TOLERANCES[0]), (False, TOLERANCES[1]), (True, (INF, INF))):
        want = _want(P, hist, demodulate, tol)
        _same(_host(rt, P, hist, demodulate, tol), want, ("host", demodulate, tol))
        _same(_device(rt, P, hist, demodulate, tol), want, ("device", demodulate, tol))


# (alpha, max_history, the factor on the input history's lengths): alpha = 1 and a history of one frame; max_history = 2, under which
# no new length reaches 4; the smallest alpha and the largest max_history the call admits, with lengths far below the cap, around it
# (4 x 2^18 = 2^20) and all above it -- there len = n + 1 = 1048577 needs 21 of float32's 24 bits, and a = 1 / len
PARAMETER_EDGES = [(1.0, 1, 1), (0.2, 2, 1), (2.0 ** -24, 2 ** 20, 1), (2.0 ** -24, 2 ** 20, 2 ** 18), (2.0 ** -24, 2 ** 20, 2 ** 22)]


def scaled_history(hist, scale):
    """The history with its length plane multiplied (exactly: a power of two) by scale."""
    hist = dict(hist)
    hist["length"] = (hist["length"] * F32(scale)).astype(F32)
    return hist


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("alpha,max_history,scale", PARAMETER_EDGES)
def test_parameter_edges_37x21(rt, alpha, max_history, scale, path):
    """The new frame of the synthetic case over tests/test_gpu_variance.py's history with lengths 1 .. 6 (times the scale), at the
    ends of alpha and max_history.  What these settings reach is shown on the CPU (tests/test_variance_cpu.py)."""
    from tests.test_gpu_variance import moments_case
    P, hist, _ = moments_case(37, 21)
    hist, kw = scaled_history(hist, scale), dict(alpha=alpha, max_history=max_history)
    want = _want(P, hist, True, TOLERANCES[0], kw=kw)
    got = (_host if path == "host" else _device)(rt, P, hist, True, TOLERANCES[0], kw=kw)
    _same(got, want, (alpha, max_history, scale))
    assert np.isfinite(got["out"]).all() and np.isfinite(got["length"]).all()


def test_no_history(rt):
    from tests import _temporal as T
    P, _ = _case(37, 21)
    for demodulate in (True, False):
        want = _want(P, None, demodulate, TOLERANCES[0], prev=None)
        hit = P["coverage"] > 0
        assert (want["cls"][hit] == T.NO_HISTORY).all() and (want["length"][hit] == 1).all()
        _same(_host(rt, P, None, demodulate, TOLERANCES[0], prev=None), want, "host")
        _same(_device(rt, P, None, demodulate, TOLERANCES[0], prev=None), want, "device")


def _raw_device(rt, P, hist, want_out, want_length, want_image, alias=False):
    """rt_temporal_accumulate itself on the NULL stream: (f32 output, length, u8 output, new history); alias: d_out is d_color."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.temporal import as_camera
    from tests import _temporal as T
    h, w = P["coverage"].shape
    t = [torch.from_numpy(np.array(a)).cuda() for a in _args(P)]
    th = torch.from_numpy(T.pack_history(hist)).cuda()
    new = torch.full((3, h, w, 4), 7.0, dtype=torch.float32, device="cuda")
    out = t[0] if alias else torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
    length = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
    img = torch.full((h, w, 3), 0x55, dtype=torch.uint8, device="cuda")
    p = abi.RT_Temporal_Params(alpha=KW["alpha"], max_history=KW["max_history"], normal_tolerance=TOLERANCES[0][0],
                               plane_tolerance=TOLERANCES[0][1], demodulate=1)
    cam, prev = as_camera(CAM_NEW), as_camera(CAM_OLD)
    torch.cuda.synchronize()
    rc = rt.lib.rt_temporal_accumulate(w, h, C.byref(p), C.byref(cam), C.byref(prev), *[x.data_ptr() for x in t], th.data_ptr(),
                                       new.data_ptr(), out.data_ptr() if want_out else None, length.data_ptr() if want_length else None,
                                       img.data_ptr() if want_image else None, None)
    assert rc == 0, rt.last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), length.cpu().numpy(), img.cpu().numpy(), T.unpack_history(new.cpu().numpy())


def test_output_may_alias_the_colour_input(rt):
    P, hist = _case(37, 21)
    want = _want(P, hist, True, TOLERANCES[0])
    apart = _raw_device(rt, P, hist, True, False, False)
    alias = _raw_device(rt, P, hist, True, False, False, alias=True)
    assert apart[0].tobytes() == want["out"].tobytes() and alias[0].tobytes() == want["out"].tobytes()
    assert alias[3]["color"].tobytes() == want["history"]["color"].tobytes()


def test_every_output_alone_and_all_together(rt):
    P, hist = _case(37, 21)
    want = _want(P, hist, True, TOLERANCES[0])
    for flags in ((True, False, False), (False, True, False), (False, False, True), (False, False, False), (True, True, True)):
        out, length, img, new = _raw_device(rt, P, hist, *flags)
        assert out.tobytes() == want["out"].tobytes() if flags[0] else (out == 7.0).all(), flags
        assert length.tobytes() == want["length"].tobytes() if flags[1] else (length == 7.0).all(), flags
        assert img.tobytes() == want["image"].tobytes() if flags[2] else (img == 0x55).all(), flags
        for k in new:
            assert new[k].tobytes() == want["history"][k].tobytes(), (flags, k)      # the history is written whatever else is
    # the host call with single outputs
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.temporal import _history_planes, as_camera
    fp = C.POINTER(C.c_float)
    planes = abi.RT_Features(*[np.ascontiguousarray(P[k]).ctypes.data_as(fp) for k in ("coverage", "albedo", "normal", "position")])
    h_in, _keep = _history_planes(21, 37, hist)
    p = abi.RT_Temporal_Params(alpha=KW["alpha"], max_history=KW["max_history"], normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
    cam, prev = as_camera(CAM_NEW), as_camera(CAM_OLD)
    only = np.full((21, 37, 3), 0x55, np.uint8)
    assert rt.lib.rt_temporal_accumulate_host(37, 21, C.byref(p), C.byref(cam), C.byref(prev), P["color"].ctypes.data, C.byref(planes),
                                              C.byref(h_in), None, None, None, only.ctypes.data) == 0, rt.last_error()
    assert only.tobytes() == want["image"].tobytes()
    length = np.full((21, 37), 7.0, F32)
    assert rt.lib.rt_temporal_accumulate_host(37, 21, C.byref(p), C.byref(cam), C.byref(prev), P["color"].ctypes.data, C.byref(planes),
                                              C.byref(h_in), None, None, length.ctypes.data, None) == 0, rt.last_error()
    assert length.tobytes() == want["length"].tobytes()


# ---- behind a frame -------------------------------------------------------------------------------------------------------------

SHAPE = (40, 24, 4, 4)
SEEDS = (11, 22, 33)
OFFSETS = (0.0, 0.19, 0.6)                 # of the moving camera along its x axis: 0.7 and 2.2 pixels at the spheres' median depth


def _spheres():
    from raytracing_c_amd.configs import load_config
    return load_config("spheres")[0]


def _move(hs, origin, right, offset):
    for i in range(3):
        hs.scene.camera.view_matrix.rows[i][3] = float(F32(origin[i] + F32(offset) * right[i]))


def _chain_inputs(rt, hs, offsets, lib=None, shape=None):
    """Per frame: (rt_render_frame's linear output, rt_render_features' planes, the camera) -- the restatement's inputs."""
    from tests import _temporal as T
    w, h, s, b = shape or SHAPE
    M0, _ = T.camera_of(hs.scene.camera)
    origin, right = M0[:3, 3].copy(), M0[:3, 0].copy()
    frames = []
    for seed, off in zip(SEEDS, offsets):
        _move(hs, origin, right, off)
        lin = rt.render_frame(hs, w, h, s, b, seed=seed, want_linear=True, lib=lib)["linear"]
        frames.append((lin, rt.render_features(hs, w, h, s, b, lib=lib), T.camera_of(hs.scene.camera)))
    _move(hs, origin, right, 0.0)
    return frames, origin, right


@pytest.mark.parametrize("demodulate", [False, True])
def test_equal_cameras_on_a_real_scene_give_the_recursion(rt, oracle, demodulate):
    """Three seeds of one view through rt_render_temporal: the recursion over the three rt_render_frame linear frames (divided
    by the modulation first and multiplied with it afterwards when demodulate is set)."""
    hs = _spheres()
    w, h, s, b = SHAPE
    frames, _, _ = _chain_inputs(rt, hs, (0.0, 0.0, 0.0))
    pl = frames[0][1]
    cov = pl["coverage"]
    hit = cov > 0                        # (partial coverage keeps its centre tap too: the old and new guides are the same bits)
    assert (cov == 1.0).sum() >= 100 and ((cov > 0) & (cov < 1)).sum() >= 10
    m = pl["albedo"] + ((F32(1.0) - cov) + F32(1e-3))[..., None]
    alpha, cap = F32(0.05), F32(64)
    with rt.History(w, h) as history:
        h_c, n_frames = None, F32(0.0)
        for k, seed in enumerate(SEEDS):
            r = rt.render_temporal(hs, w, h, s, b, history, seed=seed, demodulate=demodulate)
            lin = frames[k][0]
            assert r["linear_noisy"].tobytes() == lin.tobytes()
            c = lin / m if demodulate else lin
            if k == 0:
                h_c, n_frames = c, F32(1.0)
            else:
                n = min(n_frames, cap)
                h_c, n_frames = h_c + (c - h_c) * max(F32(1.0) / (n + F32(1.0)), alpha), n + F32(1.0)
            want = h_c * m if demodulate else h_c
            assert (r["length"][hit] == k + 1).all() and (r["length"][~hit] == 0).all()
            assert r["linear_out"][hit].tobytes() == want[hit].tobytes(), k
            assert r["linear_out"][~hit].tobytes() == lin[~hit].tobytes()


def _moving_camera_chain(rt, hs, shape, guided, iterations):
    """Three frames while the camera moves sideways; the history lengths the restatement gives per frame."""
    from tests import _guided as G, _temporal as T
    w, h, s, b = shape
    frames, origin, right = _chain_inputs(rt, hs, OFFSETS, shape=shape)
    sp = G.sigma_position(frames[0][1]["position"], frames[0][1]["coverage"])
    gkw = dict(iterations=iterations, sigma_color=1.0, sigma_normal=0.2, sigma_position=sp, demodulate=True)
    hist, prev, lengths = None, None, []
    try:
        with rt.History(w, h) as history:
            for k, (seed, off) in enumerate(zip(SEEDS, OFFSETS)):
                lin, pl, cam = frames[k]
                want = T.accumulate(lin, pl["coverage"], pl["albedo"], pl["normal"], pl["position"], cam, prev, hist)
                hist, prev = want["history"], cam
                last = want["out"]
                if guided:
                    last = G.guided(last, pl["coverage"], pl["albedo"], pl["normal"], pl["position"], gkw["iterations"], gkw["sigma_color"],
                                    gkw["sigma_normal"], sp, True)
                _move(hs, origin, right, off)
                r = rt.render_temporal(hs, w, h, s, b, history, seed=seed, guided=gkw if guided else None)
                assert r["linear_noisy"].tobytes() == lin.tobytes(), k
                assert r["length"].tobytes() == want["length"].tobytes(), k
                differ = np.argwhere((r["linear_out"].view(np.uint32) != last.view(np.uint32)).any(axis=2))
                assert r["linear_out"].tobytes() == last.tobytes(), (k, len(differ), differ[:6, ::-1].tolist())       # (x, y)
                assert r["image"].tobytes() == T.encode_u8(last).tobytes(), k
                lengths.append(want["length"])
    finally:
        _move(hs, origin, right, 0.0)
    return lengths


@pytest.mark.parametrize("guided", [False, True])
def test_chain_with_a_moving_camera(rt, oracle, guided):
    """Three frames while the camera moves sideways: rt_render_temporal equals the restatement chained over each frame's
    rt_render_frame linear output and rt_render_features planes (then tests/_guided.py where the filter is on) -- linear_out,
    length and the Image's bytes; the history keeps the UNFILTERED accumulation (or frame 2 would differ)."""
    lengths = _moving_camera_chain(rt, _spheres(), SHAPE, guided, 3)
    # (of the 179 pixels that see a sphere) reuse over three frames, restarts, and bilinear mixes of history lengths
    assert (lengths[2] == 3).sum() >= 50 and (lengths[2] == 1).sum() >= 5 and ((lengths[2] > 1) & (lengths[2] < 3)).sum() >= 10


def test_chain_with_the_filter_across_tile_borders(rt, oracle):
    """The same chain at 136 x 72 with 4 iterations: 5 x 9, 3 x 5, 2 x 3 and 1 x 2 tiles per phase at steps 1, 2, 4, 8, where 40 x 24
    has a single one from step 2 on.  Here the filter's colour input is the accumulation's output buffer, not the frame's.  A
    random scene that covers most of the image: of the 5 605 hit pixels of the third frame 3 732 have three frames of history,
    1 384 restart and 489 mix lengths (the restatement over the CPU oracle's planes)."""
    from tests.test_gpu_random_scenes import make_scene
    lengths = _moving_camera_chain(rt, make_scene(6, 400), (136, 72, 2, 4), True, 4)
    assert (lengths[2] == 3).sum() >= 3000 and (lengths[2] == 1).sum() >= 1000 and ((lengths[2] > 1) & (lengths[2] < 3)).sum() >= 300


def test_reset_gives_first_frame_output_again(rt, oracle):
    hs = _spheres()
    w, h, s, b = SHAPE
    with rt.History(w, h) as history:
        first = rt.render_temporal(hs, w, h, s, b, history, seed=5)
        second = rt.render_temporal(hs, w, h, s, b, history, seed=5)
        hit = first["length"] > 0
        assert (first["length"][hit] == 1).all() and (second["length"][hit] == 2).all() and hit.sum() >= 100
        history.reset()
        again = rt.render_temporal(hs, w, h, s, b, history, seed=5)
        for k in ("image", "linear_noisy", "linear_out", "length"):
            assert again[k].tobytes() == first[k].tobytes(), k


def test_a_first_frame_without_demodulation_is_the_denoised_frame(rt, oracle):
    """rt_render_temporal and rt_render_denoised are one pipeline.  With no usable history and no demodulation the accumulation
    writes the colour's own bits, so the filter behind it sees what rt_render_denoised's filter sees: the same Image, the same
    filtered and noisy frames, byte for byte, and a history of one frame wherever something is hit.  Then the other way round
    and once more, for the filter's buffers, which the two entry points share."""
    from tests import _guided as G
    hs = _spheres()
    w, h, s, b = SHAPE
    pl = rt.render_features(hs, w, h, s, b)
    gkw = dict(iterations=3, sigma_color=1.0, sigma_normal=0.2, sigma_position=G.sigma_position(pl["position"], pl["coverage"]),
               demodulate=True)
    hit = pl["coverage"] > 0
    assert hit.sum() >= 100 and (~hit).sum() >= 100

    def temporal():
        with rt.History(w, h) as history:
            return rt.render_temporal(hs, w, h, s, b, history, seed=SEEDS[0], demodulate=False, guided=gkw)

    def denoised():
        return rt.render_denoised(hs, w, h, s, b, seed=SEEDS[0], **gkw)

    def same(t, d, what):
        assert t["image"].tobytes() == d["image"].tobytes(), what
        assert t["linear_out"].tobytes() == d["linear_denoised"].tobytes(), what
        assert t["linear_noisy"].tobytes() == d["linear_noisy"].tobytes(), what
        assert (t["length"][hit] == 1).all() and (t["length"][~hit] == 0).all(), what
    t0 = temporal()
    d0 = denoised()
    same(t0, d0, "temporal, denoised")
    assert d0["linear_denoised"].tobytes() != d0["linear_noisy"].tobytes()            # (the filter ran)
    d1 = denoised()
    t1 = temporal()
    d2 = denoised()
    same(t1, d1, "denoised, temporal")
    same(t1, d2, "temporal, denoised again")
    same(t0, d2, "first and last")


def test_frames_queries_feature_passes_and_the_filter_are_not_affected(rt, oracle):
    from tests import _features as F
    from tests.test_gpu_features import _camera_rays
    hs = F.passthrough_scene()
    rays = _camera_rays(hs, 500)
    P, hist = _case(37, 21)

    def everything():
        f = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
        q = rt.closest_hits(hs, rays)
        qc = rt.get_query_counters()
        feats = rt.render_features(hs, 16, 16, 2, 3)
        g = rt.guided_denoise(*_args(P), iterations=2, sigma_position=0.5)
        return f["image"].tobytes(), f["accum"].tobytes(), f["counters"], q.tobytes(), qc, feats["sums"].tobytes(), g.tobytes()
    before = everything()
    want = _want(P, hist, True, TOLERANCES[0])
    _same(_host(rt, P, hist, True, TOLERANCES[0]), want)
    assert rt.get_query_counters() == before[4] and rt.render.get_counters() == before[2]
    _same(_device(rt, P, hist, True, TOLERANCES[0]), want)
    with rt.History(16, 16) as history:
        rt.render_temporal(hs, 16, 16, 2, 3, history)
        rt.render_temporal(hs, 16, 16, 2, 3, history, guided=dict(sigma_position=0.5))
    assert rt.get_query_counters() == before[4]
    assert everything() == before
    # an accumulation while a frame is in flight on a lane
    ticket, pixels, keep = rt.frame_begin(hs, 48, 40, 4, 4, seed=7)
    got = _host(rt, P, hist, True, TOLERANCES[0])
    counters = rt.frame_end(ticket)
    _same(got, want)
    assert pixels.tobytes() == before[0] and counters == before[2]


def test_the_staging_is_given_back_and_a_history_restarts(rt, diag, oracle):
    """The host-level staging is 211 B per pixel -- 13 + 11 f32 of planes, two histories of 48 B, 3 + 1 f32 and 3 u8 out -- kept
    between calls and released by the teardown of the device's staging, to the byte (the diagnostic library's own count); the
    memory of an RT_History goes with it, and the history's next frame starts from nothing instead of reading freed memory."""
    P, hist = _case(37, 21)
    want = _want(P, hist, True, TOLERANCES[0])
    _same(_host(rt, P, hist, True, TOLERANCES[0], lib=diag), want)                    # (the device slot itself exists now)
    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    base = diag.rt_diag_device_bytes_live()
    _same(_host(rt, P, hist, True, TOLERANCES[0], lib=diag), want)
    held = diag.rt_diag_device_bytes_live() - base
    assert held == 37 * 21 * (13 * 4 + 11 * 4 + 2 * 48 + 3 * 4 + 4 + 3), held
    _same(_host(rt, P, hist, True, TOLERANCES[0], lib=diag), want)
    assert diag.rt_diag_device_bytes_live() - base == held                            # warm: nothing more
    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    assert diag.rt_diag_device_bytes_live() == base
    # a history across the teardown
    hs = _spheres()
    w, h, s, b = SHAPE
    history = rt.History(w, h, lib=diag)
    first = rt.render_temporal(hs, w, h, s, b, history, seed=5)
    second = rt.render_temporal(hs, w, h, s, b, history, seed=5)
    hit = first["length"] > 0
    assert (second["length"][hit] == 2).all()
    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    with_scene = diag.rt_diag_device_bytes_live()                                     # (the scene copy and the workspace stay)
    again = rt.render_temporal(hs, w, h, s, b, history, seed=5)
    for k in ("image", "linear_out", "length"):
        assert again[k].tobytes() == first[k].tobytes(), k                            # from nothing
    third = rt.render_temporal(hs, w, h, s, b, history, seed=5)
    assert third["length"].tobytes() == second["length"].tobytes()                    # ... and on from there
    assert diag.rt_diag_device_bytes_live() - with_scene >= 2 * 48 * w * h
    history.close()
    assert diag.rt_diag_release_staging() == 0
    assert diag.rt_diag_device_bytes_live() == with_scene
