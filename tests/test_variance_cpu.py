"""Variance-guided denoising without a GPU: the CONTRACTS themselves -- their numpy restatement (tests/_variance.py), which the GPU
tests compare the kernels with bit for bit -- must extend the accumulation and the filter without changing them, must estimate a
variance, and must denoise; and the inputs of tests/test_gpu_variance.py and tests/test_gpu_variance_tiles.py must be able to tell a
wrong kernel from a right one -- the latter's must hold every class of tile of the variance launch."""
import numpy as np
import pytest

F32 = np.float32
INF = float("inf")


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("tol", [(0.3, 0.02), (INF, 0.02), (0.3, INF)])
def test_the_moments_leave_the_accumulation_alone(tol, demodulate):
    """1. out, length and history of accumulate_moments are _temporal.accumulate's, bit for bit: tests/test_gpu_temporal.py's
    synthetic case at 37 x 21, all three tolerance pairs; with a history and without."""
    from tests import _temporal as T, _variance as V
    from tests.test_gpu_temporal import CAM_NEW, CAM_OLD, KW, _args, _case
    from tests.test_gpu_variance import moments_case
    P, hist = _case(37, 21)
    _, hist6, mom = moments_case(37, 21)
    for hi, mo, prev in ((hist, mom, CAM_OLD), (hist6, mom, CAM_OLD), (None, None, None)):
        kw = dict(normal_tolerance=tol[0], plane_tolerance=tol[1], demodulate=demodulate, **KW)
        want = T.accumulate(*_args(P), CAM_NEW, prev, hi, **kw)
        got = V.accumulate_moments(*_args(P), CAM_NEW, prev, hi, mo, **kw)
        assert got["out"].tobytes() == want["out"].tobytes() and got["length"].tobytes() == want["length"].tobytes()
        for k in want["history"]:
            assert got["history"][k].tobytes() == want["history"][k].tobytes(), k
        blended = np.isin(want["cls"], (T.SOME_VALID, T.ALL_VALID))
        assert (got["classes"]["blended"] == blended).all() and (got["classes"]["sky"] == (want["cls"] == T.SKY)).all()


@pytest.mark.parametrize("w,h,iterations", [(37, 21, 3), (131, 70, 3), (259, 67, 4)])
def test_infinite_sigma_color_is_the_guided_filter(w, h, iterations):
    """2. With sigma_color = inf, _variance.guided equals _guided.guided bit for bit, whatever the variance."""
    from tests import _guided as G, _variance as V
    from tests.test_gpu_guided import SIGMAS, _shared
    from tests.test_gpu_temporal import _args
    from tests.test_gpu_variance import variance_plane
    P = _shared(w, h)
    for demodulate in (True, False):
        want = G.guided(*_args(P), iterations, INF, SIGMAS[1], SIGMAS[2], demodulate)
        got, v = V.guided(*_args(P), variance_plane(w, h), iterations, INF, SIGMAS[1], SIGMAS[2], demodulate)
        assert got.tobytes() == want.tobytes()
        assert v.tobytes() != variance_plane(w, h).tobytes()
    assert V.guided(*_args(P), variance_plane(w, h), iterations, 4.0, SIGMAS[1], SIGMAS[2], True)[0].tobytes() != want.tobytes()


def test_the_temporal_variance_is_the_population_variance():
    """3. Equal cameras, constant guides, K = 32 frames of i.i.d. noise on a 24 x 16 plane, max_history >= K: var_t after frame K is
    the float64 population variance of the pixel's K luminances.

    The tolerance, from the f32 recursion's rounding (u = 2^-24, the unit roundoff).  With alpha small and max_history >= K the
    weight of frame k is a = 1 / k, so m1 and m2 are the running means of L and L * L.  One step m' = h + (x - h) * a makes three
    rounded operations on quantities no larger than max(x, h) <= X := the largest L * L of the pixel (and max L for m1), each with
    a relative error <= u, so it adds an absolute error <= 3 u X to m2; the error already in h is carried with the factor
    (1 - a) <= 1.  L itself carries 5 roundings (three products, two sums of positive terms) and S = L * L one more, 2 * 5 + 1 = 11
    relative roundings against the float64 square of the float64 luminance, which this test removes by taking the float64
    reference from the float32 L (the contract's L): left are 1 u for S.  After K steps |dm2| <= (3 K + 1) u X.  Likewise
    |dm1| <= 3 K u max L, and d(m1 * m1) <= 2 m1 |dm1| + u m1^2 <= (6 K + 1) u X (m1 <= max L, max L^2 = X); the subtraction adds
    u m2 <= u X.  Together |dvar| <= (9 K + 3) u X: relative to var, (9 K + 3) * 2^-24 * X / var -- of the order K * 2^-23 *
    m2 / var, as expected.  Asserted per pixel with that pixel's own X and var."""
    from tests import _variance as V
    K, w, h = 32, 24, 16
    rng = np.random.default_rng(5)
    cam = (np.eye(4, dtype=F32), F32(1.4))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    Wp = np.stack([(xs - w / 2) * 0.1, (ys - h / 2) * 0.1, np.full_like(xs, -4.0)], -1)
    cov = np.ones((h, w), F32)
    albedo = np.full((h, w, 3), 0.5, F32)
    normal = np.broadcast_to(np.array([0.5, 0.5, 1.0], F32), (h, w, 3)).copy()
    position = Wp.astype(F32)
    hist = mom = None
    lums = []
    for k in range(K):
        color = rng.gamma(2.0, 0.4, (h, w, 3)).astype(F32)
        r = V.accumulate_moments(color, cov, albedo, normal, position, cam, cam, hist, mom, alpha=1e-3, max_history=64,
                                 demodulate=False)
        hist, mom = r["history"], r["moments"]
        lums.append(V.luminance(color))                                              # the contract's L, float32
        assert (r["length"] == k + 1).all()
    L = np.stack(lums).astype(np.float64)
    want = L.var(axis=0)                                                              # population variance
    X = (L * L).max(axis=0)
    bound = (9 * K + 3) * 2.0 ** -24 * X
    err = np.abs(r["var_t"].astype(np.float64) - want)
    print("largest |var_t - var| / bound:", float((err / bound).max()), "largest relative error:", float((err / want).max()),
          "largest relative bound:", float((bound / want).max()))
    assert (err <= bound).all()
    assert (r["classes"]["long"]).all() and not r["classes"]["clamped"].any()
    var = V.variance(hist, mom, 0.2, 1.0)
    assert var.tobytes() == r["var_t"].tobytes()                                      # a long history: the temporal variance itself


SHAPE = (40, 24, 4, 4)


@pytest.fixture(scope="module")
def oracle_chain():
    """Eight oracle frames of the spheres under tests/test_gpu_temporal.py's camera offsets (there and back), their feature planes
    and cameras, and the 2048 spp frame of the last camera."""
    from raytracing_c_amd.configs import load_config
    from tests import _features as F, _oracle, _temporal as T
    from tests.test_gpu_temporal import OFFSETS, _move
    w, h, s, b = SHAPE
    hs = load_config("spheres")[0]
    M0, _ = T.camera_of(hs.scene.camera)
    origin, right = M0[:3, 3].copy(), M0[:3, 0].copy()
    frames = []
    try:
        for k in range(8):
            _move(hs, origin, right, OFFSETS[(0, 1, 2, 1)[k % 4]])
            planes = F.resolve(F.expected_cached("spheres@svgf%d" % k, hs, w, h, s, b)["sums"], s)
            frames.append((_oracle.render(hs, w, h, s, b, seed=2000 + k)["linear"], planes, T.camera_of(hs.scene.camera)))
        clean = _oracle.render(hs, w, h, 2048, b)["linear"]
    finally:
        _move(hs, origin, right, 0.0)
    return frames, clean


def test_the_contract_is_a_denoiser(oracle_chain):
    """4. The restated rt_render_svgf chain has a lower RMS error against the 2048 spp frame than the unfiltered accumulation of the
    same chain.  The fixed-sigma chain's (_temporal + _guided, defaults) is printed and recorded in profiles/variance.md, not
    asserted.  Recorded: last noisy frame 0.07232, accumulated 0.03764, svgf 0.03448, fixed sigma 0.03453 (RMS over the 177 pixels
    that see a sphere; 155 of them with a history of 4 frames or more)."""
    from tests import _guided as G, _temporal as T, _variance as V
    frames, clean = oracle_chain
    sp = G.sigma_position(frames[0][1]["position"], frames[0][1]["coverage"])
    par = dict(variance_sigmas=dict(sigma_normal=0.2, sigma_position=sp),
               guided_params=dict(iterations=4, sigma_color=4.0, sigma_normal=0.2, sigma_position=sp, demodulate=True))
    hist = mom = prev = hist_t = None
    for lin, pl, cam in frames:
        r = V.svgf_frame(lin, pl, cam, prev, hist, mom, **par)
        t = T.accumulate(lin, pl["coverage"], pl["albedo"], pl["normal"], pl["position"], cam, prev, hist_t)
        hist, mom, hist_t, prev = r["history"], r["moments"], t["history"], cam
    assert t["out"].tobytes() == r["accumulated"].tobytes()
    fixed = G.guided(t["out"], pl["coverage"], pl["albedo"], pl["normal"], pl["position"], 4, 1.0, 0.2, sp, True)
    hit = pl["coverage"] > 0
    assert hit.sum() >= 100

    def rms(a):
        return float(np.sqrt(((a[hit].astype(np.float64) - clean[hit]) ** 2).mean()))
    print("pixels", int(hit.sum()), "rms: last noisy frame", rms(lin), "accumulated", rms(r["accumulated"]), "svgf", rms(r["linear_out"]),
          "fixed sigma", rms(fixed), "short", int(r["classes"]["short"].sum()), "long", int(r["classes"]["long"].sum()))
    assert rms(r["linear_out"]) < rms(r["accumulated"])
    assert r["classes"]["long"].sum() >= 20 and r["classes"]["short"].sum() >= 5


# ---- 5. the GPU tests' inputs can tell a wrong kernel from a right one -------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(37, 21), (131, 70)])
def test_every_class_of_pixel_occurs(w, h):
    from tests.test_gpu_temporal import TOLERANCES
    from tests.test_gpu_variance import VSIGMAS, moments_case, moments_want
    P, hist, mom = moments_case(w, h)
    before = ((mom[..., 1] < mom[..., 0] * mom[..., 0]) & (hist["coverage"] > 0)).sum()
    assert before >= 100 and set(np.unique(hist["length"])) == {0, 1, 2, 3, 4, 5, 6}
    for tol in TOLERANCES:
        r = moments_want(P, hist, mom, True, tol, VSIGMAS)
        counts = {k: int(v.sum()) for k, v in r["classes"].items()}
        counts["blended and clamped"] = int((r["classes"]["blended"] & r["classes"]["clamped"]).sum())
        counts["blended and short"] = int((r["classes"]["blended"] & r["classes"]["short"]).sum())
        print(w, h, tol, counts)
        for k, n in counts.items():
            assert n >= 20, (k, counts)


@pytest.mark.parametrize("w,h", [(37, 21), (131, 70)])
def test_the_window_would_catch_a_lost_halo(w, h):
    """A 7 x 7 window whose taps in another 32 x 8 tile never arrived differs in the bits of >= 100 pixels, along x and along y."""
    from tests import _variance as V
    from tests.test_gpu_temporal import TOLERANCES
    from tests.test_gpu_variance import VSIGMA_SETS, moments_case, moments_want
    P, hist, mom = moments_case(w, h)
    for vs in VSIGMA_SETS:
        r = moments_want(P, hist, mom, True, TOLERANCES[0], vs)
        assert V.variance(r["history"], r["moments"], *vs, lost_halo=None).tobytes() == r["variance"].tobytes()
        for axis in (0, 1):
            lost = V.variance(r["history"], r["moments"], *vs, lost_halo=dict(axis=axis))
            differing = int((lost.view(np.uint32) != r["variance"].view(np.uint32)).sum())
            print(w, h, vs, "axis", axis, "pixels", differing)
            assert differing >= (100 if (w, h, axis) != (37, 21, 0) else 40), differing   # 37 wide: 6 columns x 21 rows see the border


def _filter_claims():
    from tests.test_gpu_variance import FILTER_CASES
    return [c for c in FILTER_CASES if c != (37, 21, 5)]          # (step 16 of 37 x 21 has one pixel per phase and row: no neighbours)


def _last_step_with_two_tiles(w, h, iterations):
    """The largest step of the run at which some phase sub-lattice spans two 32 x 8 tiles."""
    for i in reversed(range(iterations)):
        s = 1 << i
        if (w + s - 1) // s > 32 or (h + s - 1) // s > 8:
            return s
    raise AssertionError((w, h, iterations))


@pytest.mark.parametrize("w,h,iterations", _filter_claims())
def test_the_filter_sizes_would_catch_a_lost_halo_and_a_prefilter_on_the_lattice(w, h, iterations):
    """For every (size, iteration count) of the GPU filter cases: a filter whose cross-tile taps never arrived at the last step that
    has two tiles -- the run's last step, except 2079 x 12 at 8 iterations, whose step 128 has a single tile per phase: step 64
    there -- differs from the contract in the bits of >= 100 pixels of these inputs (colour or variance); and wherever a step >= 2
    runs, so does a 3 x 3 prefilter taken at spacing s."""
    from tests import _variance as V
    from tests.test_gpu_guided import _shared
    from tests.test_gpu_temporal import _args
    from tests.test_gpu_variance import FSIGMAS, filter_want, variance_plane
    P, v = _shared(w, h), variance_plane(w, h)
    want, want_v = filter_want(w, h, iterations)
    step = _last_step_with_two_tiles(w, h, iterations)
    assert step == 1 << (iterations - 1) or (w, h, iterations) == (2079, 12, 8)

    def differing(res):
        return int(((res[0].view(np.uint32) != want.view(np.uint32)).any(axis=2) | (res[1].view(np.uint32) != want_v.view(np.uint32))).sum())
    n = sum(differing(V.guided(*_args(P), v, iterations, *FSIGMAS, True, lost_halo=dict(step=step, axis=axis)))
            for axis in (0, 1) if ((w, h)[axis] + step - 1) // step > (32, 8)[axis])
    print(w, h, iterations, "lost halo at step", step, "pixels", n)
    assert n >= 100, n
    if iterations >= 2:
        n = differing(V.guided(*_args(P), v, iterations, *FSIGMAS, True, prefilter_on_lattice=True))
        print(w, h, iterations, "prefilter on the lattice: pixels", n)
        assert n >= 100, n
    else:
        assert differing(V.guided(*_args(P), v, iterations, *FSIGMAS, True, prefilter_on_lattice=True)) == 0


def test_the_wrong_readings_leave_the_restatement_alone():
    from tests import _variance as V
    from tests.test_gpu_guided import _shared
    from tests.test_gpu_temporal import _args
    from tests.test_gpu_variance import FSIGMAS, filter_want, variance_plane
    P, v = _shared(37, 21), variance_plane(37, 21)
    want, want_v = filter_want(37, 21, 2)
    got = V.guided(*_args(P), v, 2, *FSIGMAS, True, lost_halo=dict(step=8, axis=0), prefilter_on_lattice=False)
    assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == want_v.tobytes()
    assert (want_v >= 0).all() and np.isfinite(want_v).all() and len(np.unique(np.floor(np.log10(v[v > 0])))) >= 7


# ---- 6. the variance launch's tiles: the GPU tests' inputs reach every class of tile, and would expose a wrong tile decision ---------

NEARLY_4 = np.nextafter(F32(4.0), F32(0.0))                    # 3.9999998


def _tiles_of_one_length(r, value):
    """The number of tiles with a surface whose every surface pixel has exactly that new length."""
    from tests import _variance as V
    length, cov = r["history"]["length"], r["history"]["coverage"]
    h, w = cov.shape
    return sum(1 for _, _, ys, xs in V.tiles(h, w) if (cov[ys, xs] != 0).any() and (length[ys, xs][cov[ys, xs] != 0] == value).all())


@pytest.mark.parametrize("w,h", [(131, 70), (97, 27), (65, 17)])
def test_the_designed_input_has_every_class_of_tile(w, h):
    """tests/test_gpu_variance.py's designed_case at alpha = 0.2, max_history = 5: tiles that return early (ragged ones and ones
    with sky pixels among them), sky tiles, halo tiles, tiles at exactly 4.0 and tiles one ulp below.  Measured at 131 x 70: 23 early
    returns with surface (6 ragged, 8 with sky pixels), 15 halo tiles (8 all short), 7 all sky; 97 x 27: 7, 6 (3), 3; 65 x 17: 4, 3
    (2), 2.  With max_history = 2 no tile returns early with surface."""
    from tests import _variance as V
    from tests.test_gpu_variance import DESIGNED_SIZES, designed_case, designed_want
    assert (w, h) in DESIGNED_SIZES
    P, hist, _ = designed_case(w, h)
    r = designed_want(w, h, 5)
    assert not r["classes"]["fresh"].any() and r["classes"]["clamped"].sum() >= 100
    assert set(np.unique(r["length"]).tolist()) == {0.0, 2.0, float(NEARLY_4), 4.0, 6.0}
    assert (r["length"][P["coverage"] != 0] == np.minimum(hist["length"], F32(5.0))[P["coverage"] != 0] + F32(1.0)).all()
    n = V.tile_counts(r["history"]["length"], r["history"]["coverage"])
    n["exactly 4.0"], n["3.9999998"] = _tiles_of_one_length(r, F32(4.0)), _tiles_of_one_length(r, NEARLY_4)
    halo = n["halo tile with long pixels"] + n["halo tile all short"]
    print(w, h, n)
    c = V.tile_classes(r["history"]["length"], r["history"]["coverage"])
    assert c["count"](V.EARLY, ragged_=False) >= 1 and c["count"](V.HALO_ALL_SHORT, ragged_=True) >= 1     # full and ragged, told apart
    least = (10, 3, 3, 3, 5, 2, 2) if (w, h) == (131, 70) else (1, 1, 1, 1, 1, 1, 1)
    got = (n["early return with surface"], n["early and ragged"], n["early with sky pixels"], n["all sky"], halo, n["exactly 4.0"],
           n["3.9999998"])
    assert all(g >= l for g, l in zip(got, least)), (got, least)
    assert n["halo tile with long pixels"] >= 1 and n["halo tile all short"] >= 1
    capped = designed_want(w, h, 2)
    n2 = V.tile_counts(capped["history"]["length"], capped["history"]["coverage"])
    print(w, h, "max_history 2:", n2)
    assert n2["early return with surface"] == 0 and n2["halo tile all short"] >= 5 and n2["all sky"] == n["all sky"]
    assert set(np.unique(capped["length"]).tolist()) == {0.0, 2.0, 3.0} and not capped["classes"]["long"].any()


def test_the_random_lengths_have_no_early_return():
    """Why designed_case exists: moments_case(131, 70) draws a length per pixel, so every one of its 45 tiles stages the halo."""
    from tests import _variance as V
    from tests.test_gpu_temporal import TOLERANCES
    from tests.test_gpu_variance import VSIGMAS, moments_case, moments_want
    P, hist, mom = moments_case(131, 70)
    for tol in TOLERANCES:
        r = moments_want(P, hist, mom, True, tol, VSIGMAS)
        n = V.tile_counts(r["history"]["length"], r["history"]["coverage"])
        assert n["early return with surface"] == 0 and n["all sky"] == 0 and n["halo tile with long pixels"] == 45, n


@pytest.mark.parametrize("w,h", [(131, 70), (97, 27)])
def test_the_designed_input_would_catch_a_wrong_tile_decision(w, h):
    """A decision taken per wave instead of per workgroup, and a workgroup threshold of 3 against the pixel's 4, each change the bits
    of >= 100 pixels of the designed input (measured: 156 and 162 for the wave, 1577 and 608 for the threshold)."""
    from tests import _variance as V
    from tests.test_gpu_variance import VSIGMAS, designed_want
    r = designed_want(w, h, 5)
    same = V.variance(r["history"], r["moments"], *VSIGMAS, tile_decision=None, tile_threshold=None)
    assert same.tobytes() == r["variance"].tobytes()
    assert V.variance(r["history"], r["moments"], *VSIGMAS, tile_threshold=4.0).tobytes() == r["variance"].tobytes()
    for kw in (dict(tile_decision="wave"), dict(tile_threshold=3.0)):
        wrong = V.variance(r["history"], r["moments"], *VSIGMAS, **kw)
        differing = int((wrong.view(np.uint32) != r["variance"].view(np.uint32)).sum())
        print(w, h, kw, "pixels", differing)
        assert differing >= 100, (kw, differing)


def test_a_second_designed_input_differs_where_tiles_return_early():
    """The two inputs of the GPU test that stores twice into the same buffers: a result left behind by the first call is wrong for
    the second on >= 1000 pixels of tiles that return early."""
    from tests import _variance as V
    from tests.test_gpu_variance import designed_want
    a, b = designed_want(131, 70, 5, 0), designed_want(131, 70, 5, 1)
    c = V.tile_classes(b["history"]["length"], b["history"]["coverage"])
    ys, xs = np.mgrid[0:70, 0:131]
    early = c["kind"][ys // V.TILE_H, xs // V.TILE_W] == V.EARLY
    assert ((a["variance"].view(np.uint32) != b["variance"].view(np.uint32)) & early).sum() >= 1000
    assert V.tile_counts(a["history"]["length"], a["history"]["coverage"]) == V.tile_counts(b["history"]["length"], b["history"]["coverage"])


def test_the_parameter_edges_reach_what_they_are_for():
    """tests/test_gpu_temporal.py's PARAMETER_EDGES over the 37 x 21 history with lengths 1 .. 6: both restatements stay finite at all
    five; the new lengths reach 1048577.0 = 2^20 + 1 where the scaled lengths reach the cap; with max_history <= 2 every surface
    pixel is short; and the moments leave the accumulation alone there too."""
    from tests import _temporal as T
    from tests.test_gpu_temporal import CAM_NEW, CAM_OLD, PARAMETER_EDGES, TOLERANCES, _args, scaled_history
    from tests.test_gpu_variance import VSIGMAS, moments_case, moments_want
    assert PARAMETER_EDGES == [(1.0, 1, 1), (0.2, 2, 1), (2.0 ** -24, 2 ** 20, 1), (2.0 ** -24, 2 ** 20, 2 ** 18),
                               (2.0 ** -24, 2 ** 20, 2 ** 22)]
    P, hist, mom = moments_case(37, 21)
    for alpha, max_history, scale in PARAMETER_EDGES:
        scaled, kw = scaled_history(hist, scale), dict(alpha=alpha, max_history=max_history)
        assert set(np.unique(scaled["length"]).tolist()) == {k * float(scale) for k in range(7)}
        plain = T.accumulate(*_args(P), CAM_NEW, CAM_OLD, scaled, **kw)
        r = moments_want(P, scaled, mom, True, TOLERANCES[0], VSIGMAS, kw=kw)
        assert plain["out"].tobytes() == r["out"].tobytes() and plain["length"].tobytes() == r["length"].tobytes()
        for a in (r["out"], r["length"], r["moments"], r["variance"], r["history"]["color"]):
            assert np.isfinite(a).all(), (alpha, max_history, scale)
        blended = r["classes"]["blended"]
        print(alpha, max_history, scale, "largest length", float(r["length"].max()), "short", int(r["classes"]["short"].sum()),
              "long", int(r["classes"]["long"].sum()), "blended", int(blended.sum()))
        assert blended.sum() >= 100
        if scale >= 2 ** 18:
            assert r["length"].max() == F32(1048577.0) and (r["length"] == F32(1048577.0)).sum() >= 20
        if max_history <= 2:
            assert not r["classes"]["long"].any() and r["classes"]["short"].sum() >= 100
        else:
            assert r["classes"]["long"].sum() >= 20 and r["classes"]["short"].sum() >= 20
