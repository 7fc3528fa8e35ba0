"""Tests of the tests of feature-guided upsampling, without a GPU: on the exact inputs tests/test_gpu_upsample.py runs
(tests/_upsample.py: case), four ways a kernel could go wrong change the restatement's output -- a lost halo, clamped instead of
skipped taps, exchanged weight sets, a division where the fallback belongs -- so a bit-for-bit comparison against the restatement
sees each of them.  And what the contract is for: on a noisy synthetic frame it is closer to the full-resolution truth than
replication and than the unguided spline, and no colour crosses a depth edge."""
import numpy as np
import pytest

from tests import _upsample as U

F32 = np.float32


def _run(w, h, mutation=None, sigmas=U.SIGMAS, demodulate=True, counts=None, clean=False):
    c = U.case(w, h, clean)
    return U.upsample(c["color_low"], c["low"], c["full"], *sigmas, demodulate, mutation=mutation, counts=counts)


def _changed(a, b):
    """Pixels whose bits differ (a NaN differs from everything that is not the same NaN)."""
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)


_wants = {}


def _want(w, h):
    if (w, h) not in _wants:
        _wants[(w, h)] = _run(w, h)
    return _wants[(w, h)]


@pytest.mark.parametrize("w,h", U.SIZES)
def test_the_inputs_have_every_class_of_pixel(w, h):
    c = U.case(w, h)
    want = _want(w, h)
    assert want.shape == (h, w, 3) and want.dtype == F32 and np.isfinite(want).all()
    assert np.isfinite(c["color_low"]).all() and all(np.isfinite(a).all() for a in (*c["low"].values(), *c["full"].values()))
    if w * h >= 60:
        cov = c["full"]["coverage"]
        assert c["aimed"].sum() >= 3 and ((cov > 0) & (cov < 1)).sum() >= min(w, 3)   # (the sky line of a strip is 2 pixels)
    if h >= 10:
        assert c["sky"].sum() >= w and (c["low"]["coverage"] == 0).sum() >= w // 2


@pytest.mark.parametrize("w,h", U.MULTI_TILE_SIZES + U.STRIP_SIZES)
@pytest.mark.parametrize("mutation", ["lost_halo", "clamp", "swap"])
def test_a_lost_halo_clamped_taps_and_exchanged_weights_change_100_pixels_at_every_multi_tile_size(w, h, mutation):
    assert _changed(_run(w, h, mutation), _want(w, h)).sum() >= 100


@pytest.mark.parametrize("w,h", U.SINGLE_TILE_SIZES)
@pytest.mark.parametrize("mutation", ["clamp", "swap"])
def test_clamped_taps_and_exchanged_weights_change_the_single_tile_sizes(w, h, mutation):
    """(a lost halo cannot show with one tile)  At 2 x 2 there is one low pixel: every pixel is that pixel's colour times its own
    modulation whatever the weights, and only clamping -- nine taps in place of one -- rounds differently."""
    changed = _changed(_run(w, h, mutation), _want(w, h)).sum()
    if (w, h) == (2, 2) and mutation == "swap":
        return
    assert changed >= 1


@pytest.mark.parametrize("w,h", [s for s in U.SIZES if s[0] * s[1] >= 60])
@pytest.mark.parametrize("sigmas", U.SIGMA_SETS)
def test_the_division_changes_every_pixel_aimed_at_the_fallback(w, h, sigmas):
    c = U.case(w, h)
    counts = {}
    want = _run(w, h, sigmas=sigmas, counts=counts)
    assert np.isfinite(want).all()
    assert (counts["fallback"] == c["aimed"]).all()                                   # the fallback is taken there and nowhere else
    got = _run(w, h, "divide", sigmas=sigmas)
    assert (_changed(got, want) == c["aimed"]).all() and np.isnan(got[c["aimed"]]).all()
    # ... where the result is the low pixel under the full pixel, times the full pixel's modulation
    ys, xs = np.nonzero(c["aimed"])
    m_q = c["low"]["albedo"] + ((F32(1.0) - c["low"]["coverage"]) + F32(1e-3))[..., None]
    m_p = c["full"]["albedo"] + ((F32(1.0) - c["full"]["coverage"]) + F32(1e-3))[..., None]
    under = (c["color_low"] / m_q)[ys >> 1, xs >> 1] * m_p[ys, xs]
    assert want[ys, xs].tobytes() == under.tobytes()


def _rms(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def test_closer_to_the_truth_than_replication_and_than_the_unguided_spline():
    """64 x 48, two planes, a depth edge, a 3-pixel albedo checker, a sky band, gamma noise of 16 samples on the 32 x 24 colour: three
    numbers this test computes, compared with each other."""
    w, h = 64, 48
    c = U.case(w, h, clean=True)
    contract = _rms(_run(w, h, clean=True), c["truth"])
    nearest = _rms(np.repeat(np.repeat(c["color_low"], 2, axis=0), 2, axis=1), c["truth"])
    spline = _rms(_run(w, h, sigmas=(U.INF, U.INF), demodulate=False, clean=True), c["truth"])
    print(f"rms error: contract {contract:.4f}, nearest replication {nearest:.4f}, unguided spline {spline:.4f}")
    assert contract < nearest and contract < spline


def test_no_colour_crosses_the_depth_edge():
    """With another colour on the near plane's low pixels, every far-plane pixel -- those next to the edge among them -- keeps its
    bits: a tap across the edge has pl = 7 and, at sigma_position 0.02, r * r < 1e-10, far below half an ulp of the sum it is added
    to.  The near plane's pixels change."""
    w, h = 64, 48
    c = U.case(w, h, clean=True)
    near_low = c["near"][::2, ::2]
    other = np.where(near_low[..., None], c["color_low"] * F32(3.0), c["color_low"]).astype(F32)
    kw = dict(sigma_normal=0.2, sigma_position=0.02)
    a = U.upsample(c["color_low"], c["low"], c["full"], **kw)
    b = U.upsample(other, c["low"], c["full"], **kw)
    far = ~c["near"] & ~c["sky"]
    beside = far & (np.roll(c["near"], 1, axis=1) | np.roll(c["near"], 2, axis=1) | np.roll(c["near"], 1, axis=0))
    assert beside.sum() >= 30                                                         # far-plane pixels with taps on the near plane
    assert a[far].tobytes() == b[far].tobytes()
    assert _changed(a, b)[c["near"]].all()
    # ... and the unguided spline does carry it across
    kw = dict(sigma_normal=U.INF, sigma_position=U.INF)
    assert _changed(U.upsample(c["color_low"], c["low"], c["full"], **kw), U.upsample(other, c["low"], c["full"], **kw))[beside].any()
