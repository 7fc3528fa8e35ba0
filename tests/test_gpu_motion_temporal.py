"""THE ACCUMULATION WITH MOTION on the GPU (rt_temporal_accumulate_motion, rt_temporal_accumulate_motion_host,
rt_history_set_motion behind rt_render_temporal / rt_render_svgf; rt_temporal_motion_kernel, rt_temporal_moments_motion_kernel)
against the numpy float32 restatement of tests/_motion.py: equal BIT FOR BIT -- out, the three history planes, length, the u8
image, and the moments and the variance where they are carried -- at 67 x 35 and 33 x 9 (several 32 x 8 tiles, ragged edges),
through the host call and the device call, with and without a history; zero motion against the motionless entry points; the
pipeline over a soup that is kept, refitted and seen by a moving camera for three frames; a history with motion off."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(67, 35), (33, 9)]
VSIGMAS = dict(sigma_normal=0.2, sigma_position=0.5)


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _args(P):
    return [P[k] for k in ("color", "coverage", "albedo", "normal", "position")]


def _moments(w, h):
    """the moments that go with the case's history: any finite pair per surface pixel, (0, 0) on sky"""
    from tests import _motion as M
    _, hist, _ = M.motion_case(w, h)
    m1 = np.random.default_rng(w * h).gamma(2.0, 0.3, (h, w)).astype(F32)
    mom = np.stack([m1, m1 * m1 + F32(0.01)], -1).astype(F32)
    mom[hist["coverage"] == 0] = 0
    return mom


def _want(w, h, with_history, moments, demodulate, motion=None):
    from tests import _motion as M, _temporal as T, _variance as V, test_gpu_temporal as G
    P, hist, mot = M.motion_case(w, h)
    mot = mot if motion is None else motion
    mom = _moments(w, h) if moments and with_history else None
    r = M.accumulate_motion(*_args(P), mot, G.CAM_NEW, G.CAM_OLD if with_history else None, hist if with_history else None, mom,
                            with_moments=moments, demodulate=demodulate, **M.MOTION_KW)
    r["image"] = T.encode_u8(r["out"])
    if moments:
        r["variance"] = V.variance(r["history"], r["moments"], **VSIGMAS)
    return r


def _same(got, want, moments, what=""):
    keys = ("out", "length", "image") + (("moments", "variance") if moments else ())
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        diff = np.argwhere(got[k] != want[k])
        assert got[k].tobytes() == want[k].tobytes(), (what, k, len(diff), diff[:4].tolist())
    for k in ("color", "length", "coverage", "normal", "position"):
        assert got["history"][k].tobytes() == want["history"][k].tobytes(), (what, "history", k)


def _host(rt, w, h, with_history, moments, demodulate, motion):
    from tests import _motion as M, test_gpu_temporal as G
    P, hist, _ = M.motion_case(w, h)
    kw = dict(M.MOTION_KW, demodulate=demodulate, image=True, motion=motion)
    prev, hist = (G.CAM_OLD, hist) if with_history else (None, None)
    if moments:
        return rt.temporal_accumulate_moments(*_args(P), G.CAM_NEW, prev, hist, _moments(w, h) if with_history else None, **VSIGMAS, **kw)
    return rt.temporal_accumulate(*_args(P), G.CAM_NEW, prev, hist, **kw)


def _device(rt, w, h, with_history, moments, demodulate, motion):
    """... on torch tensors, on a stream that is not the default one"""
    import torch
    from tests import _motion as M, _temporal as T, test_gpu_temporal as G
    P, hist, _ = M.motion_case(w, h)
    side = torch.cuda.Stream()
    t = [torch.from_numpy(np.array(a)).cuda() for a in _args(P)]
    th = torch.from_numpy(T.pack_history(hist)).cuda() if with_history else None
    tm = None
    if moments and with_history:
        rec = np.zeros((h, w, 4), F32)
        rec[..., :2] = _moments(w, h)
        tm = torch.from_numpy(rec).cuda()
    tmot = None if motion is None else torch.from_numpy(np.array(motion)).cuda()
    kw = dict(M.MOTION_KW, demodulate=demodulate, image=True, motion=tmot)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if moments:
            got = rt.temporal_accumulate_moments(*t, G.CAM_NEW, G.CAM_OLD if with_history else None, th, tm, **VSIGMAS, **kw)
        else:
            got = rt.temporal_accumulate(*t, G.CAM_NEW, G.CAM_OLD if with_history else None, th, **kw)
    side.synchronize()
    out = {k: got[k].cpu().numpy() for k in ("out", "length", "image") + (("variance",) if moments else ())}
    out["history"] = T.unpack_history(got["history"].cpu().numpy())
    if moments:
        rec = got["moments"].cpu().numpy()
        assert not rec[..., 2:].any()
        out["moments"] = np.ascontiguousarray(rec[..., :2])
    return out


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_planes(rt, w, h, moments, path):
    from tests import _motion as M
    _, _, motion = M.motion_case(w, h)
    run = _host if path == "host" else _device
    for demodulate in (True, False):
        want = _want(w, h, True, moments, demodulate)
        _same(run(rt, w, h, True, moments, demodulate, motion), want, moments, (path, demodulate))
        assert len(np.unique(want["length"])) >= 4
    # no history: the first frame of a sequence -- the motion is read by nothing that is kept
    _same(run(rt, w, h, False, moments, True, motion), _want(w, h, False, moments, True), moments, (path, "no history"))


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
def test_zero_motion_equals_the_motionless_entry_points(rt, w, h, moments, path):
    run = _host if path == "host" else _device
    zero = np.zeros((h, w, 3), F32)
    with_zero = run(rt, w, h, True, moments, True, zero)
    without = run(rt, w, h, True, moments, True, None)               # rt_temporal_accumulate / _moments themselves
    _same(with_zero, without, moments, path)
    _same(with_zero, _want(w, h, True, moments, True, motion=zero), moments, path)


def test_a_missing_motion_plane_is_refused(rt):
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.temporal import _history_planes, _params, as_camera
    from raytracing_c_amd.guided import _host_frame
    from tests import _motion as M, test_gpu_temporal as G
    w, h = SIZES[1]
    P, hist, motion = M.motion_case(w, h)
    params = _params(0.2, 3, 0.8, 0.02, True)
    cam, prev = as_camera(G.CAM_NEW), as_camera(G.CAM_OLD)
    col, planes, _keep = _host_frame(*_args(P))
    h_in, _k1 = _history_planes(h, w, hist)
    h_out, new = _history_planes(h, w)
    out = np.full((h, w, 3), 7, F32)
    rc = rt.lib.rt_temporal_accumulate_motion_host(w, h, C.byref(params), C.byref(cam), C.byref(prev), col, C.byref(planes), C.byref(h_in),
                                                   C.byref(h_out), out.ctypes.data, None, None, None, None, None, None, None)
    assert rc != 0 and "motion is NULL" in rt.last_error(), rt.last_error()
    assert (out == 7).all() and not any(a.any() for a in new.values())
    t = [torch.from_numpy(np.array(a)).cuda() for a in _args(P)]
    d_out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
    d_hist = torch.full((3, h, w, 4), 7.0, dtype=torch.float32, device="cuda")
    rc = rt.lib.rt_temporal_accumulate_motion(w, h, C.byref(params), C.byref(cam), None, *[x.data_ptr() for x in t], None,
                                              d_hist.data_ptr(), d_out.data_ptr(), None, None, None, None, None, None, None, None)
    assert rc != 0 and "d_motion is NULL" in rt.last_error(), rt.last_error()
    torch.cuda.synchronize()
    assert (d_out == 7).all() and (d_hist == 7).all()
    # moments given select the moments form, with its rules: a history without its moments
    d_mot = torch.from_numpy(np.array(motion)).cuda()
    d_prev = torch.zeros((3, h, w, 4), dtype=torch.float32, device="cuda")
    d_mom = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rc = rt.lib.rt_temporal_accumulate_motion(w, h, C.byref(params), C.byref(cam), C.byref(prev), *[x.data_ptr() for x in t],
                                              d_prev.data_ptr(), d_hist.data_ptr(), d_out.data_ptr(), None, None, None, None,
                                              d_mom.data_ptr(), None, None, d_mot.data_ptr())
    assert rc != 0 and "without its moments" in rt.last_error(), rt.last_error()
    assert rt.lib.rt_history_set_motion(None, 1) != 0 and "history is NULL" in rt.last_error()


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------

PIPE = (32, 24, 4, 4)                       # w, h, samples, max_bounces
AMOUNTS = (None, 0.02, 0.03)                # frame k is rendered after keep + refit to moved(seed=k, amount)


def _pipeline(rt, svgf, motion=True):
    """Three frames of soup(513): before frames 1 and 2 the geometry is kept and the mesh refitted, and the camera moves.  Per
    frame (what the call returned, the restatement over rt_render_frame's linear and rt_render_features_motion's planes)."""
    from tests import _guided as G, _motion as M, _refit, _temporal as T, _variance as V
    from tests.test_gpu_temporal import OFFSETS, SEEDS, _move
    w, h, s, b = PIPE
    soup = _refit.soup(513)
    hs = soup.build("reference")
    M0, _ = T.camera_of(hs.scene.camera)
    origin, right = M0[:3, 3].copy(), M0[:3, 0].copy()
    hist = mom = prev = None
    frames = []
    sp = None
    with rt.History(w, h, motion=motion) as history:
        for k, (seed, off, amount) in enumerate(zip(SEEDS, OFFSETS, AMOUNTS)):
            if amount is not None:
                hs.keep_geometry()
                hs.refit(*soup.moved(seed=k, amount=amount))
            _move(hs, origin, right, off)
            lin = rt.render_frame(hs, w, h, s, b, seed=seed, want_linear=True)["linear"]
            pl = rt.render_features(hs, w, h, s, b, motion=True)
            cam = T.camera_of(hs.scene.camera)
            mot = pl["motion"] if motion else np.zeros_like(pl["motion"])
            planes = [pl[n] for n in ("coverage", "albedo", "normal", "position")]
            if sp is None:
                sp = G.sigma_position(pl["position"], pl["coverage"])
            acc = M.accumulate_motion(lin, *planes, mot, cam, prev, hist, mom, with_moments=svgf)
            want = dict(linear_out=acc["out"], length=acc["length"], cls=acc["cls"], motion=pl["motion"])
            if svgf:
                var = V.variance(acc["history"], acc["moments"], sigma_normal=0.2, sigma_position=sp)
                want["linear_out"], _ = V.guided(acc["out"], *planes, var, iterations=3, sigma_color=4.0, sigma_normal=0.2,
                                                 sigma_position=sp, demodulate=True)
                want["variance"] = var
                got = rt.render_svgf(hs, w, h, s, b, history, seed=seed, iterations=3, sigma_position=sp)
            else:
                got = rt.render_temporal(hs, w, h, s, b, history, seed=seed)
            assert got["linear_noisy"].tobytes() == lin.tobytes(), k
            hist, mom, prev = acc["history"], acc.get("moments"), cam
            frames.append((got, want))
    return frames


@pytest.mark.parametrize("svgf", [False, True])
def test_pipeline_over_a_deforming_mesh(rt, oracle, svgf):
    from tests import _temporal as T
    frames = _pipeline(rt, svgf)
    for k, (got, want) in enumerate(frames):
        assert got["length"].tobytes() == want["length"].tobytes(), k
        bad = np.argwhere((got["linear_out"].view(np.uint32) != want["linear_out"].view(np.uint32)).any(axis=2))
        assert got["linear_out"].tobytes() == want["linear_out"].tobytes(), (k, len(bad), bad[:6, ::-1].tolist())
        assert got["image"].tobytes() == T.encode_u8(want["linear_out"]).tobytes(), k
        if svgf:
            assert got["variance"].tobytes() == want["variance"].tobytes(), k
    assert not frames[0][1]["motion"].view(np.uint32).any()          # the first frame: nothing kept
    for k in (1, 2):
        moved = (frames[k][1]["motion"] != 0).any(axis=2)
        reused = frames[k][1]["length"] > 1
        assert moved.sum() >= 50 and (moved & reused).sum() >= 20, (k, int(moved.sum()), int((moved & reused).sum()))


def test_a_history_with_motion_off_renders_what_it_rendered_before(rt, oracle):
    """the same deforming sequence on a history that never heard of motion and on one that had it switched on and off again: the
    plain accumulation's restatement (tests/_temporal.py through accumulate_motion with zero motion), for both"""
    frames = _pipeline(rt, False, motion=False)
    for k, (got, want) in enumerate(frames):
        assert got["length"].tobytes() == want["length"].tobytes() and got["linear_out"].tobytes() == want["linear_out"].tobytes(), k
    with_motion = _pipeline(rt, False)
    assert any(a[0]["linear_out"].tobytes() != b[0]["linear_out"].tobytes() for a, b in zip(frames[1:], with_motion[1:]))
    # switched on and off again, against a fresh history, frame by frame on one unmoved scene
    from raytracing_c_amd.configs import load_config
    hs = load_config("spheres")[0]
    w, h, s, b = PIPE
    with rt.History(w, h, motion=True) as one, rt.History(w, h) as fresh:
        one.set_motion(False)
        for seed in (5, 6):
            a = rt.render_temporal(hs, w, h, s, b, one, seed=seed)
            c = rt.render_temporal(hs, w, h, s, b, fresh, seed=seed)
            assert a["linear_out"].tobytes() == c["linear_out"].tobytes() and a["length"].tobytes() == c["length"].tobytes()
