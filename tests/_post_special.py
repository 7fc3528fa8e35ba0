"""Inputs of the post passes whose colour plane is NOT all in [0, 1], and what the restatements (tests/_guided, _temporal, _variance)
give for them: a uniform colour in [0, 1) with six special pixels -- NaN, +inf, -inf, -0, a denormal, a value above 1; three of
them sky (coverage 0), three surface -- over the feature planes the other post-pass tests use, at 37 x 21 with one filter
iteration; the temporal accumulation, which has no iteration and no spatial tap, has six such pixels in its history's colour too.
TEST INFRASTRUCTURE ONLY.  tests/test_encode_cpu.py checks on the CPU that these cases are worth running: between 1 % and 25 % of
the restatement's output pixels are NaN, at least one of them sky and one surface; tests/test_gpu_post_encode.py runs them on the
GPU."""
import numpy as np

F = np.float32
W, H = 37, 21
NAN, INF, DENORMAL, ABOVE = F("nan"), F("inf"), F(1e-40), F(3.5)
#            sky                    surface                 surface                  sky                        surface                    sky
SPECIALS = [(NAN, NAN, NAN), (NAN, F(0.5), F(0.25)), (INF, INF, F(0.125)), (-INF, F(-0.0), DENORMAL), (F(-0.0), DENORMAL, ABOVE), (ABOVE, F(2.0), F(-0.0))]
SPECIAL_IS_SKY = [True, False, False, True, False, True]
PASSES = ("guided", "temporal", "variance")


def special_color(coverage, seed):
    """(colour f32 (h, w, 3) uniform in [0, 1) but for the six SPECIALS, their (y, x) list).  The sky pixels are the first, the middle
    and the last pixel with coverage 0 in row-major order, the surface pixels three with coverage > 0 spread likewise."""
    rng = np.random.default_rng(seed)
    color = rng.random(coverage.shape + (3,), dtype=F)
    sky, surface = np.argwhere(coverage == 0), np.argwhere(coverage > 0)
    assert len(sky) >= 3 and len(surface) >= 3
    picks = {True: [sky[0], sky[len(sky) // 2], sky[-1]], False: [surface[len(surface) // 7], surface[len(surface) // 2], surface[-(len(surface) // 5)]]}
    where = []
    for value, is_sky in zip(SPECIALS, SPECIAL_IS_SKY):
        y, x = picks[is_sky].pop(0)
        color[y, x] = value
        where.append((int(y), int(x)))
    color.setflags(write=False)
    return color, where


_cases = {}


def case(name):
    """dict(P: the frame's planes with the special colour, where: the special pixels, want: the restatement's dict(out, image), and the
    pass's further inputs: hist (temporal), variance (variance)) -- once per pass, shared, read-only."""
    from tests import _guided as G, _temporal as T, _variance as V
    from tests.test_gpu_guided import SIGMAS, _shared
    from tests.test_gpu_temporal import CAM_NEW, CAM_OLD, KW, TOLERANCES, _args, _case
    from tests.test_gpu_variance import FSIGMAS, variance_plane
    if name in _cases:
        return _cases[name]
    c = {}
    if name == "temporal":
        # the accumulation has no spatial taps: a NaN of the frame stays in its pixel.  The history's colour plane gets the six
        # SPECIALS too, on pixels that have a history, and the reprojection's four taps spread those
        P, hist = _case(W, H)
        hist = dict(hist)
        hist["color"] = np.array(hist["color"])
        kept = np.argwhere((hist["coverage"] > 0) & (hist["length"] > 0))
        for k, value in enumerate(SPECIALS):
            y, x = kept[len(kept) * (k + 1) // 7]
            hist["color"][y, x] = value
        hist["color"].setflags(write=False)
        c["hist"] = hist
    else:
        P = _shared(W, H)
    P = dict(P)
    P["color"], c["where"] = special_color(P["coverage"], 40 + PASSES.index(name))
    c["P"] = P
    with np.errstate(all="ignore"):
        if name == "guided":
            out = G.guided(*_args(P), 1, *SIGMAS, True)
        elif name == "temporal":
            out = T.accumulate(*_args(P), CAM_NEW, CAM_OLD, hist, normal_tolerance=TOLERANCES[0][0], plane_tolerance=TOLERANCES[0][1],
                               demodulate=True, **KW)["out"]
        else:
            c["variance"] = variance_plane(W, H)
            out = V.guided(*_args(P), c["variance"], 1, *FSIGMAS, True)[0]
        c["want"] = dict(out=out, image=G.encode_u8(out))
    for a in c["want"].values():
        a.setflags(write=False)
    _cases[name] = c
    return c


def nan_pixels(out):
    """(h, w) bool: a channel of the pixel is NaN."""
    return np.isnan(out).any(axis=2)


def same_bits_or_both_nan(got, want):
    """(h, w, 3) bool."""
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
