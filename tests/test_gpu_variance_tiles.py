"""The variance launch (rt_variance_kernel) tile by tile, on the GPU, BIT FOR BIT against tests/_variance.py: a workgroup stages the
7 x 7 halo only if one of its surface pixels has a new history shorter than 4 frames; every other workgroup stores var_t and leaves,
which after the first frames of a sequence is nearly every one -- and which tests/test_gpu_variance.py's random lengths never reach.
tests/test_gpu_variance.py's designed_case puts whole tiles on either side of that decision and on its boundary: long throughout,
exactly 4.0, short by one ulp, long but for one pixel or for the two rows of one wave, all sky, half sky; full and ragged.  That these
inputs hold every class of tile, and that a decision taken per wave or against another threshold would change at least 100 of their
pixels, is shown on the CPU (tests/test_variance_cpu.py).  Also here: the moments pass at the ends of alpha and max_history."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_temporal import CAM_OLD, PARAMETER_EDGES, TOLERANCES, _args, scaled_history
from tests.test_gpu_variance import (DESIGNED_SIZES, VSIGMAS, _mdevice, _mhost, _msame, _pack_moments, designed_case, designed_want,
                                     moments_case, moments_want)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _variance_by_tile(got, want, what=""):
    """The variance against the restatement's; a mismatch names the first pixels (x, y) with their tile and the tile's class."""
    from tests import _variance as V
    bad = np.argwhere(got.view(np.uint32) != want["variance"].view(np.uint32))
    if len(bad):
        c = V.tile_classes(want["history"]["length"], want["history"]["coverage"])
        where = [dict(x=int(x), y=int(y), tile=(int(x) // V.TILE_W, int(y) // V.TILE_H), got=float(got[y, x]),
                      want=float(want["variance"][y, x]), kind=V.TILE_KINDS[c["kind"][y // V.TILE_H, x // V.TILE_W]],
                      sky=bool(c["sky"][y // V.TILE_H, x // V.TILE_W]), ragged=bool(c["ragged"][y // V.TILE_H, x // V.TILE_W]))
                 for y, x in bad[:6]]
        raise AssertionError((what, "variance", len(bad), where))


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("max_history", [5, 2])
@pytest.mark.parametrize("w,h", DESIGNED_SIZES)
def test_designed_tiles(rt, w, h, max_history, path):
    """max_history = 5: early returns (full, ragged, with sky pixels, at exactly 4.0), halo tiles (short by one ulp; one short pixel;
    one short wave), sky tiles.  max_history = 2 caps every length at 3: the same planes with every surface tile in the window."""
    P, hist, mom = designed_case(w, h)
    want = designed_want(w, h, max_history)
    got = (_mhost if path == "host" else _mdevice)(rt, P, hist, mom, True, TOLERANCES[0], VSIGMAS, cam=CAM_OLD,
                                                    kw=dict(alpha=0.2, max_history=max_history))
    _variance_by_tile(got["variance"], want, (w, h, max_history, path))
    _msame(got, want, (w, h, max_history, path))
    assert np.isfinite(got["variance"]).all() and not got["variance"][P["coverage"] == 0].any()


def test_an_early_return_stores_into_buffers_that_hold_something_else(rt):
    """rt_temporal_accumulate_moments itself on the NULL stream, twice into the SAME output buffers: over a sentinel, then -- without
    refilling -- another designed input of the same size over the first result.  A workgroup that leaves without storing would keep
    the sentinel the first time and the first call's variance the second time."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.temporal import as_camera
    from tests import _temporal as T, _variance as V
    w, h = DESIGNED_SIZES[0]
    new = torch.full((3, h, w, 4), 7.0, dtype=torch.float32, device="cuda")
    new_m = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
    length = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
    var = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
    p = abi.RT_Temporal_Params(alpha=0.2, max_history=5, normal_tolerance=TOLERANCES[0][0], plane_tolerance=TOLERANCES[0][1], demodulate=1)
    vp = abi.RT_Variance_Params(*VSIGMAS)
    cam = as_camera(CAM_OLD)
    wants = [designed_want(w, h, 5, variant) for variant in (0, 1)]
    early = [np.isin(_kinds(wt), (V.ALL_SKY, V.EARLY)) for wt in wants]                # per pixel: its tile is all sky or returns early
    changed = wants[0]["variance"].view(np.uint32) != wants[1]["variance"].view(np.uint32)
    assert (changed & early[1]).sum() >= 1000                                         # (stale values there would be wrong values)
    for variant, want in enumerate(wants):
        P, hist, mom = designed_case(w, h, variant)
        t = [torch.from_numpy(np.array(a)).cuda() for a in _args(P)]
        th = torch.from_numpy(T.pack_history(hist)).cuda()
        tm = torch.from_numpy(_pack_moments(mom)).cuda()
        torch.cuda.synchronize()
        rc = rt.lib.rt_temporal_accumulate_moments(w, h, C.byref(p), C.byref(cam), C.byref(cam), *[x.data_ptr() for x in t],
                                                   th.data_ptr(), new.data_ptr(), out.data_ptr(), length.data_ptr(), None, C.byref(vp),
                                                   tm.data_ptr(), new_m.data_ptr(), var.data_ptr(), None)
        assert rc == 0, rt.last_error()
        torch.cuda.synchronize()
        _variance_by_tile(var.cpu().numpy(), want, ("call", variant))
        assert out.cpu().numpy().tobytes() == want["out"].tobytes() and length.cpu().numpy().tobytes() == want["length"].tobytes()
        rec = new_m.cpu().numpy()
        assert rec[..., :2].tobytes() == want["moments"].tobytes() and not rec[..., 2:].any(), variant
        got = T.unpack_history(new.cpu().numpy())
        for k in got:
            assert got[k].tobytes() == want["history"][k].tobytes(), (variant, k)


def _kinds(want):
    """Per pixel: the kind of its tile (an index into tests/_variance.py's TILE_KINDS)."""
    from tests import _variance as V
    h, w = want["length"].shape
    kind = V.tile_classes(want["history"]["length"], want["history"]["coverage"])["kind"]
    ys, xs = np.mgrid[0:h, 0:w]
    return kind[ys // V.TILE_H, xs // V.TILE_W]


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("alpha,max_history,scale", PARAMETER_EDGES)
def test_moments_parameter_edges_37x21(rt, alpha, max_history, scale, path):
    """tests/test_gpu_temporal.py's parameter edges through the moments pass and the variance launch (moments_case's history with
    lengths 1 .. 6, times the scale).  What these settings reach is shown on the CPU (tests/test_variance_cpu.py)."""
    P, hist, mom = moments_case(37, 21)
    hist, kw = scaled_history(hist, scale), dict(alpha=alpha, max_history=max_history)
    want = moments_want(P, hist, mom, True, TOLERANCES[0], VSIGMAS, kw=kw)
    got = (_mhost if path == "host" else _mdevice)(rt, P, hist, mom, True, TOLERANCES[0], VSIGMAS, kw=kw)
    _variance_by_tile(got["variance"], want, (alpha, max_history, scale, path))
    _msame(got, want, (alpha, max_history, scale, path))
    assert np.isfinite(got["out"]).all() and np.isfinite(got["variance"]).all() and np.isfinite(got["moments"]).all()
