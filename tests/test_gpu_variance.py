"""Variance-guided denoising on the GPU (rt_temporal_accumulate_moments, rt_guided_denoise_variance, rt_render_svgf and their
host-level forms; rt_variance.hip) against the numpy float32 restatement of its three contracts (tests/_variance.py): equal BIT FOR
BIT (tobytes), through the host path and through the device path on a non-default stream.

The moments pass and the variance launch run on tests/test_gpu_temporal.py's synthetic planes (imported, not edited) with a random
moments plane -- some m2 < m1 * m1 -- and random history lengths 1 .. 6, at 37 x 21 (2 x 3 tiles of the variance kernel) and 131 x 70,
with every tolerance pair, both demodulate settings, +inf sigmas together and each alone, degenerate sizes, no history, every output
alone, d_out == d_color; out, history, length and image are rt_temporal_accumulate's.  Every tile of those inputs stages the halo:
designed_case builds the ones that do not, for tests/test_gpu_variance_tiles.py.  The variance-guided filter runs at
tests/test_gpu_guided.py's sizes, for the reason it has them, over variance planes that span 0 and eight decades.  That every class of
pixel occurs and that a lost halo or a prefilter on the lattice would change at least 100 pixels OF THESE VERY INPUTS is shown on the
CPU (tests/test_variance_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_guided import SIGMAS, _shared
from tests.test_gpu_temporal import CAM_NEW, CAM_OLD, TOLERANCES, _args, _case, _move, _spheres

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
KW = dict(alpha=0.2, max_history=5)
VSIGMAS = (0.2, 0.5)                           # normal, position of the variance estimate
VSIGMA_SETS = [VSIGMAS, (INF, INF), (INF, 0.5), (0.2, INF)]
MOMENT_SIZES = [(37, 21), (131, 70)]
FSIGMAS = (4.0,) + SIGMAS[1:]                  # colour (in standard deviations), normal, position of the filter cases
# (w, h, iterations) of the filter cases; the last step is 1 << (iterations - 1)
FILTER_CASES = ([(37, 21, i) for i in (1, 2, 5)] + [(40, 24, i) for i in (1, 2)] + [(131, 70, i) for i in (1, 2, 3)]
                + [(259, 67, 4), (513, 129, 5)] + [(w, h, i) for (w, h) in ((2079, 12), (4200, 5), (19, 1055)) for i in (6, 7, 8)])


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


# ---- inputs, once per size, shared, read-only ---------------------------------------------------------------------------------------

_mcases = {}


def moments_case(w, h):
    """(the new frame's planes, a history with lengths 1 .. 6, its moments (h, w, 2): m2 < m1 * m1 in blocks of 4 x 3 pixels, a third
    of them, so that taps which agree carry a negative variance through the blend)."""
    if (w, h) not in _mcases:
        P, hist = _case(w, h)
        rng = np.random.default_rng(700 + 3 * w + h)
        surface = hist["coverage"] > 0
        hist = dict(hist)
        hist["length"] = np.where(surface, rng.integers(1, 7, (h, w)), 0).astype(F32)
        m1 = rng.gamma(2.0, 0.4, (h, w)).astype(F32)
        ys, xs = np.mgrid[0:h, 0:w]
        below = (xs // 4 + ys // 3) % 3 == 0
        m2 = (m1 * m1 * np.where(below, rng.uniform(0.3, 0.9, (h, w)), rng.uniform(1.0, 2.0, (h, w))).astype(F32)).astype(F32)
        mom = (np.stack([m1, m2], -1) * surface[..., None]).astype(F32)
        for a in (*hist.values(), mom):
            a.setflags(write=False)
        _mcases[(w, h)] = (P, hist, mom)
    return _mcases[(w, h)]


_dcases = {}
DESIGNED_SIZES = [(131, 70), (97, 27), (65, 17)]


def designed_case(w, h, variant=0):
    """(the new frame's planes, a history, its moments) under a STATIC camera -- previous and current camera are CAM_OLD --, made tile
    by tile of the variance launch so that whole 32 x 8 tiles leave before the halo, which moments_case never does.  The new frame is
    the history's own view with another colour: hx == x exactly, tap 0 has weight 1 and is valid, and the new length is
    min(L0, max_history) + 1.  Tile t = ty * tiles_x + tx has class t % 6:
      0  L0 = 5: long.                   1  L0 = 3: exactly 4.0, long at the boundary.        2  L0 = nextafter(3, 0): short by one ulp.
      3  L0 = 5 but for short pixels with L0 = 1, alternately one single pixel (a row from {0, 3, 4, 7}, the first or the last
         column) and the two rows of ONE wave (rows 2v, 2v + 1, v cycling 0 .. 3), both clipped to a ragged tile.
      4  the NEW frame is sky over the whole tile.       5  L0 = 5, the left half of the (clipped) tile is sky in the new frame.
    variant: other seeds."""
    from tests import _temporal as T
    from tests.test_gpu_temporal import _view
    if (w, h, variant) not in _dcases:
        old = _view(CAM_OLD, w, h, 5 + 10 * w + 1000 * variant, False)
        hist = dict(T.accumulate(*_args(old), CAM_OLD, CAM_OLD, None)["history"])
        rng = np.random.default_rng(w + h + 1000 * variant)
        P = {k: np.array(v) for k, v in old.items()}
        P["color"] = rng.gamma(2.0, 0.4, (h, w, 3)).astype(F32)
        surface = hist["coverage"] > 0
        m1 = rng.gamma(2.0, 0.4, (h, w)).astype(F32)
        ys, xs = np.mgrid[0:h, 0:w]
        below = (xs // 4 + ys // 3) % 3 == 0
        m2 = (m1 * m1 * np.where(below, rng.uniform(0.3, 0.9, (h, w)), rng.uniform(1.0, 2.0, (h, w))).astype(F32)).astype(F32)
        mom = (np.stack([m1, m2], -1) * surface[..., None]).astype(F32)
        L0 = np.zeros((h, w), F32)
        tiles_x, n3 = (w + 31) // 32, 0
        for ty in range((h + 7) // 8):
            for tx in range(tiles_x):
                rows, cols = slice(ty * 8, min(h, ty * 8 + 8)), slice(tx * 32, min(w, tx * 32 + 32))
                th, tw = rows.stop - rows.start, cols.stop - cols.start
                cls = (ty * tiles_x + tx) % 6
                L0[rows, cols] = {1: 3.0, 2: np.nextafter(F32(3.0), F32(0.0))}.get(cls, 5.0)
                if cls == 3:
                    if n3 % 2 == 0:
                        row, col = min((0, 3, 4, 7)[(n3 // 2) % 4], th - 1), (0, tw - 1)[(n3 // 2) % 2]
                        L0[rows.start + row, cols.start + col] = 1.0
                    else:
                        v = min((n3 // 2) % 4, (th - 1) // 2)
                        L0[rows.start + 2 * v:min(rows.stop, rows.start + 2 * v + 2), cols] = 1.0
                    n3 += 1
                elif cls in (4, 5):
                    cols = cols if cls == 4 else slice(cols.start, cols.start + (tw + 1) // 2)
                    for k in ("coverage", "albedo", "normal", "position"):
                        P[k][rows, cols] = 0.0
        hist["length"] = np.where(surface, L0, 0).astype(F32)
        for a in (*P.values(), *hist.values(), mom):
            a.setflags(write=False)
        _dcases[(w, h, variant)] = (P, hist, mom)
    return _dcases[(w, h, variant)]


def designed_want(w, h, max_history=5, variant=0):
    """The restatement over designed_case under the static camera: moments_want's dict."""
    P, hist, mom = designed_case(w, h, variant)
    return moments_want(P, hist, mom, True, TOLERANCES[0], VSIGMAS, cam=CAM_OLD, kw=dict(alpha=0.2, max_history=max_history))


def moments_want(P, hist, mom, demodulate, tol, vs, prev=CAM_OLD, cam=CAM_NEW, kw=KW):
    from tests import _temporal as T, _variance as V
    r = V.accumulate_moments(*_args(P), cam, prev, hist, mom, normal_tolerance=tol[0], plane_tolerance=tol[1],
                             demodulate=demodulate, **kw)
    r["variance"] = V.variance(r["history"], r["moments"], *vs)
    r["image"] = T.encode_u8(r["out"])
    return r


_vplanes = {}


def variance_plane(w, h):
    """A variance for tests/test_gpu_guided.py's planes of that size: 0 on one pixel in seven, otherwise 1e-7 .. 10."""
    if (w, h) not in _vplanes:
        rng = np.random.default_rng(900 + w + 5 * h)
        v = np.where(rng.random((h, w)) < 0.15, 0.0, 10.0 ** rng.uniform(-7.0, 1.0, (h, w))).astype(F32)
        v.setflags(write=False)
        _vplanes[(w, h)] = v
    return _vplanes[(w, h)]


_fwants = {}


def filter_want(w, h, iterations, demodulate=True, sigmas=FSIGMAS):
    from tests import _variance as V
    key = (w, h, iterations, demodulate, sigmas)
    if key not in _fwants:
        P = _shared(w, h)
        _fwants[key] = V.guided(*_args(P), variance_plane(w, h), iterations, *sigmas, demodulate)
        for a in _fwants[key]:
            a.setflags(write=False)
    return _fwants[key]


# ---- the moments pass and the variance launch ---------------------------------------------------------------------------------------

def _pack_moments(mom):
    rec = np.zeros(mom.shape[:2] + (4,), F32)
    rec[..., :2] = mom
    return rec


def _mhost(rt, P, hist, mom, demodulate, tol, vs, prev=CAM_OLD, cam=CAM_NEW, kw=KW):
    return rt.temporal_accumulate_moments(*_args(P), cam, prev, hist, mom, normal_tolerance=tol[0], plane_tolerance=tol[1],
                                          demodulate=demodulate, sigma_normal=vs[0], sigma_position=vs[1], image=True, **kw)


def _mdevice(rt, P, hist, mom, demodulate, tol, vs, prev=CAM_OLD, cam=CAM_NEW, kw=KW):
    """rt.temporal_accumulate_moments on torch tensors, on a stream that is not the default one."""
    import torch
    from tests import _temporal as T
    side = torch.cuda.Stream()
    t = [torch.from_numpy(np.array(a)).cuda() for a in _args(P)]
    th = None if hist is None else torch.from_numpy(T.pack_history(hist)).cuda()
    tm = None if mom is None else torch.from_numpy(_pack_moments(mom)).cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = rt.temporal_accumulate_moments(*t, cam, prev, th, tm, normal_tolerance=tol[0], plane_tolerance=tol[1],
                                             demodulate=demodulate, sigma_normal=vs[0], sigma_position=vs[1], image=True, **kw)
    side.synchronize()
    rec = got["moments"].cpu().numpy()
    assert not rec[..., 2:].any()                                                     # (m1, m2, 0, 0)
    return dict(out=got["out"].cpu().numpy(), length=got["length"].cpu().numpy(), image=got["image"].cpu().numpy(),
                history=T.unpack_history(got["history"].cpu().numpy()), moments=rec[..., :2].copy(),
                variance=got["variance"].cpu().numpy())


def _msame(got, want, what=""):
    for k in ("out", "length", "image", "moments", "variance"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        diff = np.argwhere(got[k] != want[k])
        assert got[k].tobytes() == want[k].tobytes(), (what, k, len(diff), diff[:4].tolist())
    for k in ("color", "length", "coverage", "normal", "position"):
        assert got["history"][k].tobytes() == want["history"][k].tobytes(), (what, "history", k)


def _is_the_plain_accumulation(rt, got, P, hist, demodulate, tol, prev=CAM_OLD):
    plain = rt.temporal_accumulate(*_args(P), CAM_NEW, prev, hist, normal_tolerance=tol[0], plane_tolerance=tol[1],
                                   demodulate=demodulate, image=True, **KW)
    for k in ("out", "length", "image"):
        assert got[k].tobytes() == plain[k].tobytes(), k
    for k in plain["history"]:
        assert got["history"][k].tobytes() == plain["history"][k].tobytes(), k


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("tol", TOLERANCES)
@pytest.mark.parametrize("w,h", MOMENT_SIZES)
def test_moments_and_variance(rt, w, h, tol, demodulate, path):
    """37 x 21: 2 x 3 tiles of the variance kernel, ragged against them; 131 x 70: 5 x 9."""
    P, hist, mom = moments_case(w, h)
    want = moments_want(P, hist, mom, demodulate, tol, VSIGMAS)
    got = (_mhost if path == "host" else _mdevice)(rt, P, hist, mom, demodulate, tol, VSIGMAS)
    _msame(got, want)
    sky = P["coverage"] == 0
    assert not got["variance"][sky].any() and not got["moments"][sky].any()
    assert np.isfinite(got["variance"]).all() and (got["variance"] >= 0).all() and len(np.unique(got["variance"])) > 100
    _is_the_plain_accumulation(rt, got, P, hist, demodulate, tol)


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("vs", VSIGMA_SETS)
@pytest.mark.parametrize("w,h", MOMENT_SIZES)
def test_variance_sigmas_finite_and_infinite(rt, w, h, vs, path):
    P, hist, mom = moments_case(w, h)
    want = moments_want(P, hist, mom, True, TOLERANCES[0], vs)
    _msame((_mhost if path == "host" else _mdevice)(rt, P, hist, mom, True, TOLERANCES[0], vs), want, (w, h, vs))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 40), (40, 1), (33, 9)])
def test_moments_degenerate_sizes(rt, w, h):
    P, hist, mom = moments_case(w, h)
    for demodulate, tol, vs in ((True, TOLERANCES[0], VSIGMAS), (False, TOLERANCES[1], (INF, INF)), (True, (INF, INF), (INF, 0.5))):
        want = moments_want(P, hist, mom, demodulate, tol, vs)
        _msame(_mhost(rt, P, hist, mom, demodulate, tol, vs), want, ("host", demodulate, tol, vs))
        _msame(_mdevice(rt, P, hist, mom, demodulate, tol, vs), want, ("device", demodulate, tol, vs))


def test_moments_without_a_history(rt):
    P, _, _ = moments_case(37, 21)
    for demodulate in (True, False):
        want = moments_want(P, None, None, demodulate, TOLERANCES[0], VSIGMAS, prev=None)
        hit = P["coverage"] > 0
        assert want["classes"]["fresh"][hit].all() and (want["length"][hit] == 1).all() and want["classes"]["short"][hit].all()
        assert len(np.unique(want["variance"])) > 100                                 # the 7 x 7 estimate everywhere, boosted by 4
        _msame(_mhost(rt, P, None, None, demodulate, TOLERANCES[0], VSIGMAS, prev=None), want, "host")
        _msame(_mdevice(rt, P, None, None, demodulate, TOLERANCES[0], VSIGMAS, prev=None), want, "device")


def _raw_moments(rt, P, hist, mom, want_out, want_length, want_image, want_variance, alias=False, call=None):
    """rt_temporal_accumulate_moments itself on the NULL stream; alias: d_out is d_color.  call: replaces the C call (refusals)."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.temporal import as_camera
    from tests import _temporal as T
    h, w = P["coverage"].shape
    t = [torch.from_numpy(np.array(a)).cuda() for a in _args(P)]
    th = torch.from_numpy(T.pack_history(hist)).cuda()
    tm = torch.from_numpy(_pack_moments(mom)).cuda()
    new = torch.full((3, h, w, 4), 7.0, dtype=torch.float32, device="cuda")
    new_m = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda")
    out = t[0] if alias else torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
    length = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
    var = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
    img = torch.full((h, w, 3), 0x55, dtype=torch.uint8, device="cuda")
    p = abi.RT_Temporal_Params(alpha=KW["alpha"], max_history=KW["max_history"], normal_tolerance=TOLERANCES[0][0],
                               plane_tolerance=TOLERANCES[0][1], demodulate=1)
    vp = abi.RT_Variance_Params(*VSIGMAS)
    cam, prev = as_camera(CAM_NEW), as_camera(CAM_OLD)
    torch.cuda.synchronize()
    a = dict(w=w, h=h, p=p, cam=cam, prev=prev, frame=[x.data_ptr() for x in t], h_in=th.data_ptr(), h_out=new.data_ptr(),
             out=out.data_ptr() if want_out else None, length=length.data_ptr() if want_length else None,
             image=img.data_ptr() if want_image else None, vp=vp, m_in=tm.data_ptr(), m_out=new_m.data_ptr(),
             var=var.data_ptr() if want_variance else None)
    if call is None:
        rc = rt.lib.rt_temporal_accumulate_moments(w, h, C.byref(p), C.byref(cam), C.byref(prev), *a["frame"], a["h_in"], a["h_out"],
                                                   a["out"], a["length"], a["image"], C.byref(vp), a["m_in"], a["m_out"], a["var"], None)
        assert rc == 0, rt.last_error()
    else:
        call(a)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), length.cpu().numpy(), img.cpu().numpy(), var.cpu().numpy(), T.unpack_history(new.cpu().numpy()),
            new_m.cpu().numpy())


def test_moments_every_output_alone_all_together_and_aliased(rt):
    P, hist, mom = moments_case(37, 21)
    want = moments_want(P, hist, mom, True, TOLERANCES[0], VSIGMAS)
    for flags in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                  (False, False, False, False), (True, True, True, True)):
        out, length, img, var, new, new_m = _raw_moments(rt, P, hist, mom, *flags)
        assert out.tobytes() == want["out"].tobytes() if flags[0] else (out == 7.0).all(), flags
        assert length.tobytes() == want["length"].tobytes() if flags[1] else (length == 7.0).all(), flags
        assert img.tobytes() == want["image"].tobytes() if flags[2] else (img == 0x55).all(), flags
        assert var.tobytes() == want["variance"].tobytes() if flags[3] else (var == 7.0).all(), flags
        for k in new:
            assert new[k].tobytes() == want["history"][k].tobytes(), (flags, k)      # the history and the moments whatever else is
        assert new_m[..., :2].tobytes() == want["moments"].tobytes() and not new_m[..., 2:].any(), flags
    alias = _raw_moments(rt, P, hist, mom, True, False, False, True, alias=True)      # d_out == d_color
    assert alias[0].tobytes() == want["out"].tobytes() and alias[3].tobytes() == want["variance"].tobytes()
    assert alias[5][..., :2].tobytes() == want["moments"].tobytes()
    # the host call with single outputs
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.temporal import _history_planes, as_camera
    fp = C.POINTER(C.c_float)
    planes = abi.RT_Features(*[np.ascontiguousarray(P[k]).ctypes.data_as(fp) for k in ("coverage", "albedo", "normal", "position")])
    h_in, _keep = _history_planes(21, 37, hist)
    p = abi.RT_Temporal_Params(alpha=KW["alpha"], max_history=KW["max_history"], normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
    vp = abi.RT_Variance_Params(*VSIGMAS)
    cam, prev = as_camera(CAM_NEW), as_camera(CAM_OLD)
    m_in = np.ascontiguousarray(mom)

    def host(m_out, var, vparams=vp):
        return rt.lib.rt_temporal_accumulate_moments_host(37, 21, C.byref(p), C.byref(cam), C.byref(prev), P["color"].ctypes.data,
                                                          C.byref(planes), C.byref(h_in), None, None, None, None,
                                                          None if vparams is None else C.byref(vparams), m_in.ctypes.data,
                                                          None if m_out is None else m_out.ctypes.data,
                                                          None if var is None else var.ctypes.data)
    only = np.full((21, 37), 7.0, F32)
    assert host(None, only) == 0, rt.last_error()
    assert only.tobytes() == want["variance"].tobytes()
    only_m = np.full((21, 37, 2), 7.0, F32)
    assert host(only_m, None, None) == 0, rt.last_error()                             # (no variance wanted: vp is not read)
    assert only_m.tobytes() == want["moments"].tobytes()


def test_moments_refused_arguments_leave_the_outputs_untouched(rt):
    from raytracing_c_amd import ctypes_abi as abi
    P, hist, mom = moments_case(37, 21)
    lib = rt.lib

    def refused(change, word):
        def call(a):
            a = dict(a)
            change(a)
            rc = lib.rt_temporal_accumulate_moments(a["w"], a["h"], C.byref(a["p"]), C.byref(a["cam"]), C.byref(a["prev"]), *a["frame"],
                                                    a["h_in"], a["h_out"], a["out"], a["length"], a["image"],
                                                    None if a["vp"] is None else C.byref(a["vp"]), a["m_in"], a["m_out"], a["var"], None)
            assert rc == -1 and word in rt.last_error(), (word, rt.last_error())
        out, length, img, var, new, new_m = _raw_moments(rt, P, hist, mom, True, True, True, True, call=call)
        assert (out == 7.0).all() and (length == 7.0).all() and (img == 0x55).all() and (var == 7.0).all() and (new_m == 7.0).all()
        assert all((v == 7.0).all() for v in new.values())

    refused(lambda a: a.update(m_in=None), "without its moments")
    refused(lambda a: a.update(h_in=None), "without their history")
    refused(lambda a: a.update(m_out=None), "d_moments_out is NULL")
    refused(lambda a: a.update(m_out=a["m_in"] + 16 * 5), "overlap")
    refused(lambda a: a.update(m_out=a["m_out"] + 4), "aligned")
    refused(lambda a: a.update(vp=None), "variance params are NULL")
    refused(lambda a: a.update(vp=abi.RT_Variance_Params(float("nan"), 1.0)), "sigma_normal")
    refused(lambda a: a.update(vp=abi.RT_Variance_Params(0.2, 0.0)), "sigma_position")
    refused(lambda a: a.update(w=0), "size")
    assert lib.rt_temporal_moments_bytes(37, 21) == 37 * 21 * 16 and lib.rt_temporal_moments_bytes(0, 4) == -1
    assert lib.rt_guided_variance_work_bytes(37, 21) == 37 * 21 * 64 and lib.rt_guided_variance_work_bytes(4, -1) == -1
    # the host level: a history without moments, moments without a history, no output
    h, w = 21, 37
    for kw, word in ((dict(history=hist, moments=None), "without its moments"), (dict(history=None, moments=mom), "without their history")):
        with pytest.raises(RuntimeError, match=word):
            rt.temporal_accumulate_moments(*_args(P), CAM_NEW, CAM_OLD, **kw, sigma_position=0.5, **KW)
    # the filter: no variance, a wrong iteration count
    G = _shared(37, 21)
    fp = C.POINTER(C.c_float)
    planes = abi.RT_Features(*[np.ascontiguousarray(G[k]).ctypes.data_as(fp) for k in ("coverage", "albedo", "normal", "position")])
    gp = abi.RT_Guided_Params(2, *FSIGMAS, 1)
    out, vout = np.full((h, w, 3), 7.0, F32), np.full((h, w), 7.0, F32)
    v = np.ascontiguousarray(variance_plane(w, h))
    assert lib.rt_guided_denoise_variance_host(w, h, C.byref(gp), G["color"].ctypes.data, C.byref(planes), out.ctypes.data, None, None,
                                               vout.ctypes.data) == -1 and "variance is NULL" in rt.last_error()
    gp.iterations = 9
    assert lib.rt_guided_denoise_variance_host(w, h, C.byref(gp), G["color"].ctypes.data, C.byref(planes), out.ctypes.data, None,
                                               v.ctypes.data, vout.ctypes.data) == -1 and "iterations" in rt.last_error()
    gp.iterations = 2
    assert lib.rt_guided_denoise_variance_host(w, h, C.byref(gp), G["color"].ctypes.data, C.byref(planes), None, None, v.ctypes.data,
                                               None) == -1 and "no output" in rt.last_error()
    assert (out == 7.0).all() and (vout == 7.0).all()


# ---- the variance-guided filter -----------------------------------------------------------------------------------------------------

def _fhost(rt, P, v, **kw):
    r = rt.guided_denoise_variance(*_args(P), v, **kw)
    return r["out"], r["variance"]


def _fdevice(rt, P, v, **kw):
    import torch
    side = torch.cuda.Stream()
    t = [torch.from_numpy(np.array(a)).cuda() for a in (*_args(P), v)]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = rt.guided_denoise_variance(*t, **kw)
    side.synchronize()
    return r["out"].cpu().numpy(), r["variance"].cpu().numpy()


def _fcompare(rt, w, h, iterations, demodulate, path, sigmas=FSIGMAS):
    from tests.test_gpu_guided import _differing
    P, v = _shared(w, h), variance_plane(w, h)
    want, want_v = filter_want(w, h, iterations, demodulate, sigmas)
    kw = dict(iterations=iterations, sigma_color=sigmas[0], sigma_normal=sigmas[1], sigma_position=sigmas[2], demodulate=demodulate)
    got, got_v = (_fhost if path == "host" else _fdevice)(rt, P, v, **kw)
    message = _differing(got, want, 1 << (iterations - 1))
    assert not message, message
    assert got.tobytes() == want.tobytes()
    bad = np.argwhere(got_v.view(np.uint32) != want_v.view(np.uint32))
    assert got_v.tobytes() == want_v.tobytes(), (len(bad), bad[:6].tolist())
    sky = P["coverage"] == 0
    assert sky.sum() >= 50 and got[sky].tobytes() == P["color"][sky].tobytes() and got_v[sky].tobytes() == v[sky].tobytes()
    assert np.isfinite(got).all() and np.isfinite(got_v).all()
    return got


@pytest.mark.parametrize("path,demodulate", [("host", True), ("device", False)])
@pytest.mark.parametrize("w,h,iterations", FILTER_CASES)
def test_variance_guided_filter(rt, w, h, iterations, path, demodulate):
    _fcompare(rt, w, h, iterations, demodulate, path)


@pytest.mark.parametrize("w,h,iterations", [(37, 21, 3), (131, 70, 3)])
def test_variance_guided_filter_other_parities_and_sigmas(rt, w, h, iterations):
    _fcompare(rt, w, h, iterations, False, "host")
    _fcompare(rt, w, h, iterations, True, "device")
    for sigmas in ((4.0, INF, INF), (0.5, 0.2, INF), (INF, INF, 0.05)):
        _fcompare(rt, w, h, iterations, True, "device", sigmas)


@pytest.mark.parametrize("w,h,iterations", [(37, 21, 3), (131, 70, 3), (259, 67, 4)])
def test_infinite_sigma_color_is_the_guided_filter(rt, w, h, iterations):
    """With sigma_color = +inf the colour equals rt_guided_denoise's with sigma_color = +inf, on the GPU, bit for bit -- whatever the
    variance; the variance is still filtered."""
    P, v = _shared(w, h), variance_plane(w, h)
    kw = dict(iterations=iterations, sigma_color=INF, sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2])
    plain = rt.guided_denoise(*_args(P), **kw)
    for f in (_fhost, _fdevice):
        got, got_v = f(rt, P, v, **kw)
        assert got.tobytes() == plain.tobytes()
        assert got_v.tobytes() == filter_want(w, h, iterations, True, (INF,) + SIGMAS[1:])[1].tobytes()
    assert plain.tobytes() != rt.guided_denoise(*_args(P), **dict(kw, sigma_color=SIGMAS[0])).tobytes()


def test_filter_outputs_alone_and_image(rt):
    from tests import _guided as G
    P, v = _shared(37, 21), variance_plane(37, 21)
    want, want_v = filter_want(37, 21, 2)
    kw = dict(iterations=2, sigma_color=FSIGMAS[0], sigma_normal=FSIGMAS[1], sigma_position=FSIGMAS[2], image=True)
    r = rt.guided_denoise_variance(*_args(P), v, **kw)
    assert r["image"].tobytes() == G.encode_u8(want).tobytes() and r["out"].tobytes() == want.tobytes()
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    t = [torch.from_numpy(np.array(a)).cuda() for a in (*_args(P), v)]
    work = torch.empty((rt.lib.rt_guided_variance_work_bytes(37, 21),), dtype=torch.uint8, device="cuda")
    gp = abi.RT_Guided_Params(2, *FSIGMAS, 1)
    for flags in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        out = torch.full((21, 37, 3), 7.0, dtype=torch.float32, device="cuda")
        img = torch.full((21, 37, 3), 0x55, dtype=torch.uint8, device="cuda")
        vout = torch.full((21, 37), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert rt.lib.rt_guided_denoise_variance(37, 21, C.byref(gp), *[x.data_ptr() for x in t[:5]], out.data_ptr() if flags[0] else None,
                                                 img.data_ptr() if flags[1] else None, work.data_ptr(), None, t[5].data_ptr(),
                                                 vout.data_ptr() if flags[2] else None) == 0, rt.last_error()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes() if flags[0] else bool((out == 7.0).all()), flags
        assert img.cpu().numpy().tobytes() == r["image"].tobytes() if flags[1] else bool((img == 0x55).all()), flags
        assert vout.cpu().numpy().tobytes() == want_v.tobytes() if flags[2] else bool((vout == 7.0).all()), flags


# ---- behind a frame -----------------------------------------------------------------------------------------------------------------

SEEDS5 = (11, 22, 33, 44, 55)
OFFSETS5 = (0.0, 0.19, 0.6, 0.6, 0.41)         # of the moving camera along its x axis (tests/test_gpu_temporal.py's, and two more)
SVGF_SHAPES = [(40, 24, 4, 4), (136, 72, 4, 4)]


def svgf_chain_inputs(rt, hs, shape, lib=None):
    """Per frame: (rt_render_frame's linear output, rt_render_features' planes, the camera) -- the restatement's inputs."""
    from tests import _temporal as T
    w, h, s, b = shape
    M0, _ = T.camera_of(hs.scene.camera)
    origin, right = M0[:3, 3].copy(), M0[:3, 0].copy()
    frames = []
    for seed, off in zip(SEEDS5, OFFSETS5):
        _move(hs, origin, right, off)
        lin = rt.render_frame(hs, w, h, s, b, seed=seed, want_linear=True, lib=lib)["linear"]
        frames.append((lin, rt.render_features(hs, w, h, s, b, lib=lib), T.camera_of(hs.scene.camera)))
    _move(hs, origin, right, 0.0)
    return frames, origin, right


def svgf_parameters(frames, iterations=3):
    from tests import _guided as G
    sp = G.sigma_position(frames[0][1]["position"], frames[0][1]["coverage"])
    return dict(variance_sigmas=dict(sigma_normal=0.2, sigma_position=sp),
                guided_params=dict(iterations=iterations, sigma_color=4.0, sigma_normal=0.2, sigma_position=sp, demodulate=True))


@pytest.mark.parametrize("shape", SVGF_SHAPES)
def test_svgf_chain_with_a_moving_camera(rt, oracle, shape):
    """Five frames while the camera moves: every frame's linear_out, length, variance and Image equal the restatement chained over
    the GPU's own noisy frames and feature planes; the variance returned is the filter's INPUT.  At 136 x 72 some frame has a
    tile of the variance launch that holds a surface and no short pixel, so that its workgroup leaves before the halo."""
    from tests import _temporal as T, _variance as V
    hs = _spheres()
    w, h, s, b = shape
    frames, origin, right = svgf_chain_inputs(rt, hs, shape)
    par = svgf_parameters(frames)
    g = par["guided_params"]
    hist = mom = prev = None
    short_and_long, tile_counts = [], []
    try:
        with rt.History(w, h) as history:
            for k, (seed, off) in enumerate(zip(SEEDS5, OFFSETS5)):
                lin, pl, cam = frames[k]
                want = V.svgf_frame(lin, pl, cam, prev, hist, mom, **par)
                hist, mom, prev = want["history"], want["moments"], cam
                _move(hs, origin, right, off)
                r = rt.render_svgf(hs, w, h, s, b, history, seed=seed, iterations=g["iterations"], sigma_color=g["sigma_color"],
                                   sigma_normal=g["sigma_normal"], sigma_position=g["sigma_position"])
                assert r["linear_noisy"].tobytes() == lin.tobytes(), k
                assert r["length"].tobytes() == want["length"].tobytes(), k
                bad = np.argwhere(r["variance"].view(np.uint32) != want["variance"].view(np.uint32))
                assert r["variance"].tobytes() == want["variance"].tobytes(), (k, len(bad), bad[:6, ::-1].tolist())
                bad = np.argwhere((r["linear_out"].view(np.uint32) != want["linear_out"].view(np.uint32)).any(axis=2))
                assert r["linear_out"].tobytes() == want["linear_out"].tobytes(), (k, len(bad), bad[:6, ::-1].tolist())
                assert r["image"].tobytes() == T.encode_u8(want["linear_out"]).tobytes(), k
                assert want["variance_out"].tobytes() != want["variance"].tobytes()
                short_and_long.append((int(want["classes"]["short"].sum()), int(want["classes"]["long"].sum())))
                tile_counts.append(V.tile_counts(want["history"]["length"], want["history"]["coverage"]))
    finally:
        _move(hs, origin, right, 0.0)
    print(short_and_long)
    for k, counts in enumerate(tile_counts):
        print("frame", k, "tiles of the variance launch:", counts)
    if (w, h) == (136, 72):                    # (40 x 24 has six tiles, each with a silhouette: none is long throughout)
        assert any(counts["early return with surface"] >= 1 for counts in tile_counts), tile_counts     # the launch's common path
    assert short_and_long[0][1] == 0 and short_and_long[4][1] >= 20 and short_and_long[4][0] >= 5     # both branches of the variance


def test_svgf_reset_refusal_and_render_temporal_afterwards(rt, oracle):
    hs = _spheres()
    w, h, s, b = SVGF_SHAPES[0]
    sp = 0.3
    with rt.History(w, h) as history, rt.History(w, h) as plain:
        first = rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=sp)
        second = rt.render_svgf(hs, w, h, s, b, history, seed=6, sigma_position=sp)
        hit = first["length"] > 0
        assert (first["length"][hit] == 1).all() and (second["length"][hit] == 2).all() and hit.sum() >= 100
        assert first["variance"][hit].any() and not first["variance"][~hit].any()
        history.reset()
        again = rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=sp)
        for k in first:
            assert again[k].tobytes() == first[k].tobytes(), k
        # rt_render_temporal after rt_render_svgf: allowed, and what a chain that never had moments gives
        p1 = rt.render_temporal(hs, w, h, s, b, plain, seed=5)
        p2 = rt.render_temporal(hs, w, h, s, b, plain, seed=7)
        t2 = rt.render_temporal(hs, w, h, s, b, history, seed=7)
        assert again["length"].tobytes() == p1["length"].tobytes()
        for k in p2:
            assert t2[k].tobytes() == p2[k].tobytes(), k
        # ... which leaves a history without moments: refused, outputs untouched, until the reset
        with pytest.raises(RuntimeError, match="rt_history_reset"):
            rt.render_svgf(hs, w, h, s, b, history, seed=8, sigma_position=sp)
        t3 = rt.render_temporal(hs, w, h, s, b, history, seed=8)                       # (the refusal changed nothing)
        p3 = rt.render_temporal(hs, w, h, s, b, plain, seed=8)
        assert t3["linear_out"].tobytes() == p3["linear_out"].tobytes() and t3["length"].tobytes() == p3["length"].tobytes()
        history.reset()
        fresh = rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=sp)
        for k in first:
            assert fresh[k].tobytes() == first[k].tobytes(), k
        with pytest.raises(RuntimeError, match="sigma_position"):
            rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=-1.0)
        with pytest.raises(RuntimeError, match="the history"):
            rt.render_svgf(hs, w + 1, h, s, b, history, seed=5, sigma_position=sp)


def test_svgf_staging_is_given_back_and_the_history_restarts(rt, diag, oracle):
    hs = _spheres()
    w, h, s, b = SVGF_SHAPES[0]
    history = rt.History(w, h, lib=diag)
    first = rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=0.3)
    second = rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=0.3)
    assert diag.rt_diag_release_staging() == 0, rt.last_error(diag)
    with_scene = diag.rt_diag_device_bytes_live()                                     # (the scene copy and the workspace stay)
    again = rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=0.3)
    for k in first:
        assert again[k].tobytes() == first[k].tobytes(), k                            # from nothing
    third = rt.render_svgf(hs, w, h, s, b, history, seed=5, sigma_position=0.3)
    for k in second:
        assert third[k].tobytes() == second[k].tobytes(), k                           # ... and on from there
    assert diag.rt_diag_device_bytes_live() - with_scene >= 2 * (48 + 16) * w * h
    history.close()
    assert diag.rt_diag_release_staging() == 0
    assert diag.rt_diag_device_bytes_live() == with_scene


def test_everything_else_returns_the_same_bytes(rt, oracle):
    from tests import _features as F
    from tests.test_gpu_features import _camera_rays
    hs = F.passthrough_scene()
    rays = _camera_rays(hs, 500)
    P, hist, mom = moments_case(37, 21)
    G = _shared(37, 21)

    def everything():
        f = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
        q = rt.closest_hits(hs, rays)
        qc = rt.get_query_counters()
        feats = rt.render_features(hs, 16, 16, 2, 3)
        g = rt.guided_denoise(*_args(G), iterations=2, sigma_position=0.5)
        t = rt.temporal_accumulate(*_args(P), CAM_NEW, CAM_OLD, hist, image=True, **KW)
        return (f["image"].tobytes(), f["accum"].tobytes(), f["counters"], q.tobytes(), qc, feats["sums"].tobytes(), g.tobytes(),
                t["out"].tobytes(), t["image"].tobytes(), t["length"].tobytes(), *[v.tobytes() for v in t["history"].values()])
    before = everything()
    want = moments_want(P, hist, mom, True, TOLERANCES[0], VSIGMAS)
    _msame(_mhost(rt, P, hist, mom, True, TOLERANCES[0], VSIGMAS), want)
    assert rt.get_query_counters() == before[4] and rt.render.get_counters() == before[2]
    _msame(_mdevice(rt, P, hist, mom, True, TOLERANCES[0], VSIGMAS), want)
    _fcompare(rt, 37, 21, 2, True, "host")
    _fcompare(rt, 37, 21, 2, True, "device")
    with rt.History(16, 16) as history:
        rt.render_svgf(hs, 16, 16, 2, 3, history, sigma_position=0.5)
        rt.render_svgf(hs, 16, 16, 2, 3, history, sigma_position=0.5)
    assert rt.get_query_counters() == before[4]
    assert everything() == before
