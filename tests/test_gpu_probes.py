"""Light probes on the GPU (rt_probe_trace, rt_probe_project, rt_probe_resolve, rt_scene_probes; rt_probes.hip) against the CPU
oracle (tests/_probes.py): every record, all 27 u64 sums of every probe, the coefficients and the path count equal, bit for bit --
probes outside the geometry, inside a closed sphere, between back-facing quads, on a vertex, far away and with a NaN coordinate, in
shapes from one path to lists that are refilled many times; sample ranges and probe slices that add up to the whole; a launch that
gives every workgroup work; the host level and its slices; no effect on frames, queries and their counters."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M64 = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def uploaded(rt):
    """name -> device scene, uploaded on first use and released with the module."""
    from tests import _probes as P
    held = {}

    def get(name):
        if name not in held:
            hs, _ = P.scene(name)
            d = rt.lib.rt_scene_upload(C.byref(hs.scene))
            assert d, rt.last_error()
            held[name] = d
        return held[name]
    yield get
    for d in held.values():
        rt.lib.rt_scene_release(d)


def _chain(rt, d, positions, samples, max_bounces, ranges=None, probe_first=0, seed=None):
    """The device-level chain: one rt_probe_trace + rt_probe_project per sample range into ONE sum buffer, then rt_probe_resolve.
    -> dict(records [per range], sums, coeffs, counters [per range])."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from tests import _probes as P
    n = len(positions)
    pos = torch.from_numpy(np.ascontiguousarray(positions, np.float32)).cuda()
    sums = torch.zeros((n, 9, 3), dtype=torch.int64, device="cuda")
    coeffs = torch.full((n, 9, 3), 7.0, dtype=torch.float32, device="cuda")
    records, counters = [], []
    for first, count in (ranges or [(0, 0)]):
        p = abi.RT_Probe_Params(samples=samples, sample_first=first, sample_count=count, max_bounces=max_bounces,
                                seed=P.SEED if seed is None else seed, probe_first=probe_first)
        m = count if count else samples - first
        rec = torch.full((n, m, 8), 7.0, dtype=torch.float32, device="cuda")
        assert rt.lib.rt_probe_trace(d, C.byref(p), n, pos.data_ptr(), rec.data_ptr(), None) == 0, rt.last_error()
        assert rt.lib.rt_probe_project(C.byref(p), n, rec.data_ptr(), sums.data_ptr(), None) == 0, rt.last_error()
        counters.append(rt.get_probe_counters())
        records.append(rec.cpu().numpy().view(abi.PROBE_SAMPLE_DTYPE).reshape(n, m))
    p = abi.RT_Probe_Params(samples=samples, max_bounces=max_bounces)
    assert rt.lib.rt_probe_resolve(C.byref(p), n, sums.data_ptr(), coeffs.data_ptr(), None) == 0, rt.last_error()
    torch.cuda.synchronize()
    return dict(records=records, sums=sums.cpu().numpy().view(np.uint64), coeffs=coeffs.cpu().numpy(), counters=counters)


def _same_records(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got.view(np.uint32).reshape(got.shape + (8,)) != want.view(np.uint32).reshape(want.shape + (8,)))
    assert len(bad) == 0, (len(bad), bad[:4].tolist(), got.ravel()[:2], want.ravel()[:2])


def _same(got, e):
    _same_records(got["records"][0], e["records"])
    assert np.array_equal(got["sums"], e["sums"]), np.argwhere(got["sums"] != e["sums"])[:4].tolist()
    assert got["coeffs"].tobytes() == e["coeffs"].tobytes()
    assert got["counters"][0].paths == e["paths"]


def _case_id(case):
    name, (n, count, first, samples), b = case
    return f"{name}-{n}x{count}-b{b}"


def _cases():
    from tests import _probes as P
    return P.gpu_cases()


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_records_sums_and_coefficients_equal_the_oracle(rt, oracle, uploaded, case):
    from tests import _probes as P
    name, shape, b = case
    n, count, first, samples = shape
    hs, placements = P.scene(name)
    e = P.expected_case(name, shape, b)
    got = _chain(rt, uploaded(name), P.tiled(placements, n), samples, b, ranges=[(first, count)])
    _same(got, e)
    rec = got["records"][0]
    assert (rec["pad"] == 0).all()
    if b == 0:                                           # no ray is cast: zero radiance, no first hit, all sums 0
        assert not rec["radiance"].any() and np.isposinf(rec["t"]).all() and not got["sums"].any() and not got["coeffs"].any()
        c = got["counters"][0]
        assert (c.rays, c.shades, c.backgrounds) == (0, 0, 0)
    else:
        c = got["counters"][0]
        k = e["classes"]
        assert c.backgrounds == k["miss"] + k["background"] and c.rays >= c.paths


def test_sample_ranges_and_probe_slices_add_up(rt, oracle, uploaded):
    from tests import _probes as P
    shape = P.SHAPES[1]
    n, count, first, samples = shape
    hs, placements = P.scene("passthrough")
    pos = P.tiled(placements, n)
    d = uploaded("passthrough")
    e = P.expected_case("passthrough", shape, 8)
    whole = _chain(rt, d, pos, samples, 8)
    _same(whole, e)
    parts = _chain(rt, d, pos, samples, 8, ranges=[(0, 30), (30, 40)])
    assert np.array_equal(parts["sums"], e["sums"]) and parts["coeffs"].tobytes() == e["coeffs"].tobytes()
    _same_records(np.concatenate(parts["records"], axis=1), e["records"])
    # positions[1:] with probe_first = 1 is rows 1.. of the whole
    tail = _chain(rt, d, pos[1:], samples, 8, probe_first=1)
    _same_records(tail["records"][0], e["records"][1:])
    assert np.array_equal(tail["sums"], e["sums"][1:]) and tail["coeffs"].tobytes() == e["coeffs"][1:].tobytes()
    # the counters of the parts add up to the whole's
    from dataclasses import astuple
    w = astuple(whole["counters"][0])
    assert tuple(a + b for a, b in zip(*[astuple(c) for c in parts["counters"]])) == w
    head = _chain(rt, d, pos[:1], samples, 8)
    assert tuple(a + b for a, b in zip(astuple(head["counters"][0]), astuple(tail["counters"][0]))) == w
    assert w[0] == n * count


def test_a_launch_that_gives_every_workgroup_work(rt, oracle, uploaded):
    """64 x 4096 on spheres, 262 144 paths: one launch against eight launches of 512 samples each -- records and sums equal bit for
    bit, counters additive -- and 2 000 records picked by a fixed seed against the oracle."""
    from dataclasses import astuple
    from tests import _probes as P
    hs, placements = P.scene("spheres")
    n, samples, b = 64, 4096, 8
    pos = P.tiled(placements[:4], n)                     # (finite positions: outside, inside a sphere, on a vertex, far away)
    d = uploaded("spheres")
    one = _chain(rt, d, pos, samples, b)
    eight = _chain(rt, d, pos, samples, b, ranges=[(k * 512, 512) for k in range(8)])
    rec = one["records"][0]
    _same_records(np.concatenate(eight["records"], axis=1), rec)
    assert np.array_equal(one["sums"], eight["sums"]) and one["coeffs"].tobytes() == eight["coeffs"].tobytes()
    assert one["sums"].any()
    total = tuple(sum(v) for v in zip(*[astuple(c) for c in eight["counters"]]))
    assert total == astuple(one["counters"][0]) and total[0] == n * samples
    rng = np.random.default_rng(2024)
    pick = np.stack([rng.integers(0, n, 2000), rng.integers(0, samples, 2000)], 1)
    e = P.expected(hs, pos, samples, b, pick=pick, classes=False)
    _same_records(rec[pick[:, 0], pick[:, 1]], e["records"])


def _host(rt, hs, positions, samples, b, **kw):
    from tests import _probes as P
    return rt.bake_probes(hs, positions, samples, b, seed=P.SEED, return_sums=True, **kw)


def test_host_level_equals_the_device_level_chain(rt, oracle, uploaded):
    from tests import _probes as P
    shape = P.SHAPES[3]
    n, count, first, samples = shape
    hs, placements = P.scene("passthrough")
    e = P.expected_case("passthrough", shape, 8)
    coeffs, sums, rec = _host(rt, hs, P.tiled(placements, n), samples, 8, sample_range=(first, count), return_samples=True)
    _same_records(rec, e["records"])
    assert np.array_equal(sums, e["sums"]) and coeffs.tobytes() == e["coeffs"].tobytes()
    assert rt.get_probe_counters().paths == e["paths"]
    # each output alone
    p = rt.abi.RT_Probe_Params(samples=samples, sample_first=first, sample_count=count, max_bounces=8, seed=P.SEED)
    pos = P.tiled(placements, n)
    only = np.zeros((n, 9, 3), np.float32)
    assert rt.lib.rt_scene_probes(C.byref(hs.scene), C.byref(p), n, pos.ctypes.data, only.ctypes.data, None, None) == 0, rt.last_error()
    assert only.tobytes() == e["coeffs"].tobytes()
    only = np.zeros((n, count), rt.abi.PROBE_SAMPLE_DTYPE)
    assert rt.lib.rt_scene_probes(C.byref(hs.scene), C.byref(p), n, pos.ctypes.data, None, None, only.ctypes.data) == 0, rt.last_error()
    _same_records(only, e["records"])


def test_host_level_slices(rt, oracle):
    """5 x 2^20 samples on spheres at max_bounces = 2: three groups of probes (2 + 2 + 1 per slice of 2^21 paths); and one probe
    of 2^21 + 2^19 samples, which is split by sample range.  Both equal the sum of host calls over their parts."""
    from tests import _probes as P
    hs, placements = P.scene("spheres")
    pos = P.tiled(placements[:4], 5)
    samples = 1 << 20
    coeffs, sums = _host(rt, hs, pos, samples, 2)
    assert rt.get_probe_counters().paths == 5 * samples
    for lo, hi in ((0, 2), (2, 4), (4, 5), (1, 3)):
        c, s = _host(rt, hs, pos[lo:hi], samples, 2, probe_first=lo)
        assert np.array_equal(s, sums[lo:hi]) and c.tobytes() == coeffs[lo:hi].tobytes(), (lo, hi)
    halves = [_host(rt, hs, pos, samples, 2, sample_range=r)[1] for r in ((0, 1 << 19), (1 << 19, 1 << 19))]
    assert np.array_equal(halves[0] + halves[1], sums)                       # (uint64: the sum wraps mod 2^64 like the device's)
    long = (1 << 21) + (1 << 19)
    c1, s1 = _host(rt, hs, pos[1:2], long, 2, probe_first=1)
    assert rt.get_probe_counters().paths == long
    parts = [_host(rt, hs, pos[1:2], long, 2, probe_first=1, sample_range=r)[1] for r in ((0, 1 << 20), (1 << 20, long - (1 << 20)))]
    assert np.array_equal(parts[0] + parts[1], s1) and c1.tobytes() == P.resolve(s1, long).tobytes()
    # the first 2^20 samples of that probe are the first call's probe 1
    assert np.array_equal(parts[0], sums[1:2])


def test_an_edit_nobody_reported_is_seen_by_the_next_call(rt, oracle):
    """rt_scene_probes runs through the frame path's scene check: a material edited in place between two calls, without
    rt_scene_touch, is what the second call shades with."""
    from tests import _probes as P
    hs, placements = P.scene("spheres")
    pos = P.tiled(placements, 3)
    samples, b = 70, 8
    first = P.expected(hs, pos, samples, b, classes=False)
    c, s = _host(rt, hs, pos, samples, b)
    assert np.array_equal(s, first["sums"]) and c.tobytes() == first["coeffs"].tobytes()
    saved = [(m.base_color.x, m.base_color.y, m.base_color.z) for m in hs.materials]
    try:
        for m in hs.materials:
            m.base_color.x, m.base_color.y, m.base_color.z = 0.9, 0.1, 0.4
        edited = P.expected(hs, pos, samples, b, classes=False)
        assert (edited["sums"] != first["sums"]).any(), "the edit must change what the probes see"
        c, s = _host(rt, hs, pos, samples, b)                                # no rt_scene_touch
        assert np.array_equal(s, edited["sums"]) and c.tobytes() == edited["coeffs"].tobytes()
    finally:
        for m, v in zip(hs.materials, saved):
            m.base_color.x, m.base_color.y, m.base_color.z = v
    c, s = _host(rt, hs, pos, samples, b)
    assert np.array_equal(s, first["sums"])


def test_frames_queries_and_their_counters_are_not_affected(rt, oracle):
    from tests import _probes as P
    hs, placements = P.scene("passthrough")
    rng = np.random.default_rng(3)
    rays = np.zeros((500, 6), np.float32)
    rays[:, :3] = (0.0, 0.0, 3.5)
    rays[:, 3:] = rng.normal(size=(500, 3)) * (0.4, 0.4, 0.1) + (0.0, 0.0, -1.0)

    def frame_and_query():
        f = rt.render_frame(hs, 48, 40, 4, 4, seed=7, want_accum=True)
        q = rt.closest_hits(hs, rays)
        return f["image"].tobytes(), f["accum"].tobytes(), f["counters"], q.tobytes(), rt.get_query_counters()
    before = frame_and_query()
    shape = P.SHAPES[1]
    e = P.expected_case("passthrough", shape, 8)
    c, s = _host(rt, hs, P.tiled(placements, shape[0]), shape[3], 8)
    assert np.array_equal(s, e["sums"])
    assert rt.get_query_counters() == before[4]
    assert rt.render.get_counters() == before[2]
    assert rt.get_probe_counters().paths == e["paths"]
    assert frame_and_query() == before
    assert rt.get_probe_counters().paths == e["paths"]                       # ... and frames and queries leave the probe counters alone


def test_python_wrappers(rt, oracle, uploaded):
    import torch
    from tests import _probes as P
    shape = P.SHAPES[1]
    n, count, first, samples = shape
    hs, placements = P.scene("passthrough")
    pos = P.tiled(placements, n)
    e = P.expected_case("passthrough", shape, 8)
    assert rt.bake_probes(hs, pos, samples, 8, seed=P.SEED).tobytes() == e["coeffs"].tobytes()
    coeffs, rec = rt.bake_probes(hs, pos, samples, 8, seed=P.SEED, return_samples=True)
    _same_records(rec, e["records"])
    frac, mean = rt.probe_visibility(rec)
    t = e["records"]["t"].astype(np.float64)
    for i in range(n):
        hit = np.isfinite(t[i])
        assert frac[i] == hit.sum() / count and (np.isnan(mean[i]) if not hit.any() else mean[i] == t[i][hit].sum() / hit.sum())
    assert (frac > 0).any() and (frac < 1).any()
    # seed=None is rt_get_seed()
    rt.lib.rt_set_seed(P.SEED)
    assert rt.bake_probes(hs, pos, samples, 8).tobytes() == e["coeffs"].tobytes()
    # torch device tensors
    d = uploaded("passthrough")
    tc, ts, tr = rt.bake_probes_device(d, torch.from_numpy(pos).cuda(), samples, 8, seed=P.SEED, return_sums=True, return_samples=True)
    torch.cuda.synchronize()
    assert tc.cpu().numpy().tobytes() == e["coeffs"].tobytes()
    assert np.array_equal(ts.cpu().numpy().view(np.uint64), e["sums"])
    _same_records(tr.cpu().numpy().view(rt.abi.PROBE_SAMPLE_DTYPE).reshape(n, count), e["records"])
    # the coefficients stand for the radiance: the band-0 term is the mean radiance times sqrt(4 pi)
    mean_rad = e["records"]["radiance"].astype(np.float64).mean(axis=1)
    assert rt.sh9_radiance(coeffs, (0.0, 0.0, 1.0)).shape == (n, 3) and rt.sh9_irradiance(coeffs, (0.0, 0.0, 1.0)).shape == (n, 3)
    assert np.allclose(coeffs[:, 0, :] * 0.282095, mean_rad, rtol=1e-4, atol=1e-6)
