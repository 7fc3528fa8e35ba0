"""Batch ray queries on the GPU (include/rt_hip.h: rt_query_closest, rt_query_occluded, rt_scene_hits, rt_scene_occluded,
rt_get_query_counters) against the CPU oracle.  Every comparison is exact, on bit patterns: closest hits and visit counts against
oracle_trace_rays_counted(), finite bounds and full records against oracle_ray_scene_hit() called per ray with hit.distance =
t_max (the reference's own protocol), occlusion flags against `triangle >= 0` of the same call."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")
RT_EPS = np.float32(1e-4)


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    import re
    text = open(os.path.join(os.path.dirname(ASSETS), "include", "rt_math.h")).read()
    m = re.search(r"#define\s+RT_EPS\s+([0-9.eE+-]+)f", text)
    assert m and np.float32(float(m.group(1))) == RT_EPS, "RT_EPS of this file is the reference's EPSILON (rt_math.h)"
    return rt


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bbox(hs):
    T = hs.scene.triangles
    n = int(T.len)
    pts = [np.concatenate([np.ctypeslib.as_array(getattr(T, ax)[k], (n,)) for k in range(3)]) for ax in "xyz"]
    return np.array([p.min() for p in pts], np.float64), np.array([p.max() for p in pts], np.float64)


def _rays(hs, n, rng, special=True):
    """The mix the traversal's own parity test uses: half from outside aimed into the scene box, half from inside in random
    directions, and a few hundred awkward ones -- axis-aligned, a zero component, an origin on a box face, NaN, directions scaled
    by 2^+-30, -0 / infinity in the direction."""
    lo, hi = _bbox(hs)
    c, e = (lo + hi) / 2, np.maximum(hi - lo, 1e-3)
    rays = np.zeros((n, 6), np.float32)
    k = n // 2
    o = c + rng.normal(size=(k, 3)) * e * 1.5
    d = c + rng.uniform(-0.5, 0.5, (k, 3)) * e - o
    rays[:k, :3] = o
    rays[:k, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    d = rng.normal(size=(n - k, 3))
    rays[k:, :3] = c + rng.uniform(-0.5, 0.5, (n - k, 3)) * e
    rays[k:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    if special:
        m = min(600, n // 8)
        for j, i in enumerate(rng.choice(n, m, replace=False)):
            kind = j % 6
            if kind == 0:
                rays[i, 3:] = 0
                rays[i, 3 + j % 3] = 1.0 if (j // 3) % 2 else -1.0
            elif kind == 1:
                rays[i, 3 + j % 3] = 0.0
            elif kind == 2:
                rays[i, j % 3] = np.float32(lo[j % 3] if (j // 3) % 2 else hi[j % 3])
            elif kind == 3:
                rays[i, rng.integers(0, 6)] = np.nan
            elif kind == 4:
                rays[i, 3:] *= np.float32(2.0 ** (30 if (j // 6) % 2 else -30))
            else:
                rays[i, 3 + j % 3] = -0.0 if (j // 6) % 2 else np.inf
    return np.ascontiguousarray(rays)


def _oracle_trace(oracle, hs, rays):
    """oracle_trace_rays_counted: RAY_HIT_DTYPE records and (node, leaf) visits."""
    from raytracing_c_amd import ctypes_abi as abi
    n = len(rays)
    t, tri, uv = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
    visits = (C.c_uint64 * 2)()
    oracle.oracle_trace_rays_counted(C.byref(hs.scene), n, rays.ctypes.data, t.ctypes.data, tri.ctypes.data, uv.ctypes.data, visits)
    out = np.zeros(n, abi.RAY_HIT_DTYPE)
    out["t"], out["triangle"], out["u"], out["v"] = t, tri, uv[:, 0], uv[:, 1]
    return out, (int(visits[0]), int(visits[1]))


def _oracle_hits(oracle, hs, rays, t_max, poison=0xA5):
    """oracle_ray_scene_hit per ray with hit.distance = t_max[i] on entry, on Hit records filled with `poison` bytes."""
    from raytracing_c_amd import ctypes_abi as abi
    n = len(rays)
    hits = np.frombuffer(bytes([poison]) * (88 * n), abi.HIT_DTYPE).copy()
    hits["distance"] = t_max
    tri = np.zeros(n, np.int32)
    rp, hp, tp = rays.ctypes.data, hits.ctypes.data, tri.ctypes.data
    f, sc = oracle.oracle_ray_scene_hit, C.byref(hs.scene)
    RP, HP, TP = C.POINTER(abi.Ray), C.POINTER(abi.Hit), C.POINTER(C.c_int32)
    for i in range(n):
        f(C.cast(rp + 24 * i, RP), sc, C.cast(hp + 88 * i, HP), C.cast(tp + 4 * i, TP))
    return hits, tri


class _Dev:
    """An uploaded scene and torch tensors for the device-level calls."""

    def __init__(self, rt, hs, lib=None):
        self.rt, self.lib = rt, lib or rt.lib
        self.d = self.lib.rt_scene_upload(C.byref(hs.scene))
        assert self.d, rt.last_error(self.lib)

    def close(self):
        self.lib.rt_scene_release(self.d)

    def closest(self, rays, t_max=None, full=False, stream=None):
        import torch
        from raytracing_c_amd import ctypes_abi as abi
        r = torch.from_numpy(rays).cuda()
        tm = None if t_max is None else torch.from_numpy(np.ascontiguousarray(t_max, np.float32)).cuda()
        out = self.rt.closest_hits_device(self.d, r, tm, full=full, stream=stream, lib=self.lib)
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        if full:
            return out[0].cpu().numpy().view(abi.RAY_HIT_DTYPE).reshape(-1), out[1].cpu().numpy().view(abi.DEVICE_HIT_DTYPE).reshape(-1)
        return out.cpu().numpy().view(abi.RAY_HIT_DTYPE).reshape(-1)

    def occluded(self, rays, t_max=None, stream=None):
        import torch
        r = torch.from_numpy(rays).cuda()
        tm = None if t_max is None else torch.from_numpy(np.ascontiguousarray(t_max, np.float32)).cuda()
        out = self.rt.occluded_device(self.d, r, tm, stream=stream, lib=self.lib)
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _same_hits(want, got):
    assert np.array_equal(want["triangle"], got["triangle"])
    for f in ("t", "u", "v"):
        assert np.array_equal(_bits(want[f]), _bits(got[f])), f


def _scenes():
    from raytracing_c_amd.configs import load_config
    from raytracing_c_amd.loaders import load_model
    from tests.test_gpu_random_scenes import make_scene
    for asset in ("quad.obj", "fov_test.obj", "sheen.glb", "spheres.glb", "tower.obj", "helmet.glb"):
        yield asset, load_model(os.path.join(ASSETS, asset))
    yield "helmet-sah", load_config("helmet", builder="sah")[0]
    yield "random", make_scene(4, 900)
    hs = make_scene(3, 700)
    nodes = np.ctypeslib.as_array(C.cast(hs.scene.bvh.nodes.data, C.POINTER(C.c_float)), (int(hs.scene.bvh.nodes.len) * 48,))
    nb = nodes.reshape(-1, 2, 24)
    nb[1::3] = nb[1::3, ::-1].copy()               # inverted boxes: the LDS node blocks must not be used
    yield "inverted", hs


SCENE_NAMES = ["quad.obj", "fov_test.obj", "sheen.glb", "spheres.glb", "tower.obj", "helmet.glb", "helmet-sah", "random", "inverted"]


@pytest.fixture(scope="module")
def scenes():
    return dict(_scenes())


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_closest_hit_equals_the_oracle_with_its_visit_counts(rt, oracle, scenes, name):
    hs = scenes[name]
    rays = _rays(hs, 30000, np.random.default_rng(11))
    want, visits = _oracle_trace(oracle, hs, rays)
    n_hit = int((want["triangle"] >= 0).sum())
    assert n_hit > len(rays) // 10, "the oracle alone must hit with more than a tenth of the rays"
    dev = _Dev(rt, hs)
    try:
        got = dev.closest(rays)
        _same_hits(want, got)
        c = rt.get_query_counters()
        assert (c.rays, c.hits, c.node_visits, c.leaf_visits) == (len(rays), n_hit, visits[0], visits[1])
        # the host form: same records through rt_scene_hits, same counters
        host = rt.closest_hits(hs, rays)
        _same_hits(want, host)
        c = rt.get_query_counters()
        assert (c.rays, c.hits, c.node_visits, c.leaf_visits) == (len(rays), n_hit, visits[0], visits[1])
        # occlusion with no bound: the flag is `triangle >= 0`, with no more visits than the closest hit took
        flags = dev.occluded(rays)
        assert np.array_equal(flags, (want["triangle"] >= 0).astype(np.uint8))
        a = rt.get_query_counters()
        assert (a.rays, a.hits) == (len(rays), n_hit)
        assert a.node_visits <= visits[0] and a.leaf_visits <= visits[1]
        assert np.array_equal(rt.occluded(hs, rays), flags)
    finally:
        dev.close()


def _bounds(want, rng):
    """t_max per ray from {true distance x 0.5, x 0.999, x 1, x 1.001, a random value, 0, EPSILON, infinity, NaN}."""
    n = len(want)
    t = want["t"].astype(np.float32)
    true = np.where(want["triangle"] >= 0, t, np.float32(1.0))
    kind = rng.integers(0, 9, n)
    tm = np.empty(n, np.float32)
    for k, f in enumerate((0.5, 0.999, 1.0, 1.001)):
        tm[kind == k] = (true * np.float32(f))[kind == k]
    tm[kind == 4] = rng.uniform(0, 4 * float(np.nanmedian(true)), n).astype(np.float32)[kind == 4]
    tm[kind == 5] = 0.0
    tm[kind == 6] = RT_EPS
    tm[kind == 7] = np.inf
    tm[kind == 8] = np.nan
    return tm


@pytest.mark.parametrize("name", ["helmet.glb", "tower.obj", "spheres.glb", "inverted"])
def test_finite_bounds_full_records_and_occlusion(rt, oracle, scenes, name):
    from raytracing_c_amd import ctypes_abi as abi
    hs = scenes[name]
    rng = np.random.default_rng(29)
    rays = _rays(hs, 12000, rng)
    free, _ = _oracle_trace(oracle, hs, rays)
    t_max = _bounds(free, rng)
    want, wtri = _oracle_hits(oracle, hs, rays, t_max)
    hit = wtri >= 0
    assert hit.sum() > len(rays) // 10 and (~hit & (free["triangle"] >= 0)).sum() > 100, "bounds must cut real hits off"
    dev = _Dev(rt, hs)
    try:
        got, rec = dev.closest(rays, t_max, full=True)
        assert np.array_equal(got["triangle"], wtri)
        assert np.array_equal(_bits(got["t"]), _bits(want["distance"]))          # (a miss: the entry bound, NaN payload included)
        assert np.array_equal(rec["triangle"], wtri)
        assert np.array_equal(_bits(rec["distance"]), _bits(want["distance"]))
        for f in ("normal", "normal_geo", "point", "tangent", "bitangent", "tex_coords"):
            assert np.array_equal(_bits(rec[f][hit]), _bits(want[f][hit])), f
            assert not rec[f][~hit].view(np.uint32).any(), f
        assert (rec["material"][~hit] == -1).all() and (rec["material"][hit] >= 0).all()
        host = rt.closest_hits(hs, rays, t_max)                                       # rt_scene_closest: all four fields
        assert host.tobytes() == got.tobytes()
        # the host form fills Hit as the reference does: everything on a hit (shader from the host triangle), nothing on a miss
        hits = np.frombuffer(bytes([0xA5]) * (88 * len(rays)), abi.HIT_DTYPE).copy()
        hits["distance"] = t_max
        tri = np.full(len(rays), 12345, np.int32)
        assert rt.lib.rt_scene_hits(C.byref(hs.scene), len(rays), rays.ctypes.data, hits.ctypes.data, tri.ctypes.data) == 0, rt.last_error()
        assert np.array_equal(tri, wtri)
        assert hits.tobytes() == want.tobytes()                                      # (poisoned misses included)
        aos = hs.scene.triangles.aos
        for i in np.flatnonzero(hit)[:200]:
            assert hits["shader_data"][i] == (aos[int(wtri[i])].shader.data or 0)
            assert hits["shader_proc"][i] == (aos[int(wtri[i])].shader.proc or 0)
        # occlusion under the same bounds
        closest = rt.get_query_counters()
        flags = dev.occluded(rays, t_max)
        assert np.array_equal(flags, hit.astype(np.uint8))
        a = rt.get_query_counters()
        assert a.hits == int(hit.sum()) and a.node_visits <= closest.node_visits and a.leaf_visits <= closest.leaf_visits
        assert np.array_equal(rt.occluded(hs, rays, t_max), flags)
    finally:
        dev.close()


def test_any_hit_takes_strictly_fewer_visits_on_the_helmet(rt, oracle, scenes):
    hs = scenes["helmet.glb"]
    rng = np.random.default_rng(3)
    lo, hi = _bbox(hs)
    c, e = (lo + hi) / 2, hi - lo
    n = 50000
    o = c + rng.normal(size=(n, 3)) / np.linalg.norm(rng.normal(size=(n, 3)), axis=1, keepdims=True) * e.max() * 2
    d = c + rng.uniform(-0.2, 0.2, (n, 3)) * e - o
    rays = np.ascontiguousarray(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1), np.float32)
    want, visits = _oracle_trace(oracle, hs, rays)
    assert (want["triangle"] >= 0).sum() > n // 2
    dev = _Dev(rt, hs)
    try:
        assert np.array_equal(dev.occluded(rays), (want["triangle"] >= 0).astype(np.uint8))
        a = rt.get_query_counters()
        assert a.node_visits < visits[0] and a.leaf_visits < visits[1], (a, visits)
    finally:
        dev.close()


PRIME = 100003
LARGE = 3 * (1 << 20) + 17        # crosses the host form's slice boundary (RT_QUERY_SLICE = 2^20 rays) three times


@pytest.mark.parametrize("n", [1, 63, 64, 65, PRIME])
def test_batch_shapes(rt, oracle, scenes, n):
    hs = scenes["tower.obj"]
    rays = _rays(hs, max(n, 4096), np.random.default_rng(n), special=n > 1000)[:n].copy()
    want, visits = _oracle_trace(oracle, hs, rays)
    dev = _Dev(rt, hs)
    try:
        _same_hits(want, dev.closest(rays))
        c = rt.get_query_counters()
        assert (c.rays, c.node_visits, c.leaf_visits) == (n, visits[0], visits[1])
        host = rt.closest_hits(hs, rays)
        _same_hits(want, host)
        assert np.array_equal(dev.occluded(rays), (want["triangle"] >= 0).astype(np.uint8))
        assert np.array_equal(rt.occluded(hs, rays), (want["triangle"] >= 0).astype(np.uint8))
    finally:
        dev.close()


def test_a_batch_of_millions_crosses_the_slice_boundary(rt, oracle, scenes):
    from raytracing_c_amd import ctypes_abi as abi
    assert LARGE > 2 * abi.RT_QUERY_SLICE, "the batch must cross the host form's slice boundary"
    hs = scenes["helmet.glb"]
    rays = _rays(hs, LARGE, np.random.default_rng(77))
    want, visits = _oracle_trace(oracle, hs, rays)
    n_hit = int((want["triangle"] >= 0).sum())
    dev = _Dev(rt, hs)
    try:
        _same_hits(want, dev.closest(rays))
        c = rt.get_query_counters()
        assert (c.rays, c.hits, c.node_visits, c.leaf_visits) == (LARGE, n_hit, visits[0], visits[1])
    finally:
        dev.close()
    _same_hits(want, rt.closest_hits(hs, rays))
    hits, tri = rt.closest_hits(hs, rays, full=True)
    assert np.array_equal(tri, want["triangle"]) and np.array_equal(_bits(hits["distance"]), _bits(want["t"]))
    c = rt.get_query_counters()                                    # the slices' counters summed
    assert (c.rays, c.hits, c.node_visits, c.leaf_visits) == (LARGE, n_hit, visits[0], visits[1])
    assert np.array_equal(rt.occluded(hs, rays), (want["triangle"] >= 0).astype(np.uint8))


def test_results_do_not_depend_on_stream_workgroup_size_repetition_or_a_frame_in_flight(rt, oracle, scenes, diag):
    import torch
    from raytracing_c_amd.scene import make_image
    hs = scenes["spheres.glb"]
    rays = _rays(hs, 40000, np.random.default_rng(19))
    want, visits = _oracle_trace(oracle, hs, rays)
    dev = _Dev(rt, hs)
    try:
        first = dev.closest(rays)
        _same_hits(want, first)
        assert first.tobytes() == dev.closest(rays).tobytes()                              # repeated
        side = torch.cuda.Stream()
        assert first.tobytes() == dev.closest(rays, stream=side).tobytes()                 # another stream
        assert np.array_equal(dev.occluded(rays, stream=side), (want["triangle"] >= 0).astype(np.uint8))
    finally:
        dev.close()
    # the launch picks 8 waves per workgroup for batches that fit the 8-wave grid and 16 above; the diagnostic library forces either
    for waves in ("8", "16"):
        os.environ["RT_QUERY_WG_WAVES"] = waves
        try:
            dd = _Dev(rt, hs, lib=diag)
            try:
                _same_hits(want, dd.closest(rays))
                c = rt.get_query_counters(lib=diag)
                assert (c.node_visits, c.leaf_visits) == visits
            finally:
                dd.close()
        finally:
            del os.environ["RT_QUERY_WG_WAVES"]
    # a frame in flight (on its lane's non-blocking stream): the query is answered meanwhile, and the frame is rt_render_frame's, byte for byte
    w, h, s, b = 256, 160, 8, 4
    ref = rt.render_frame(hs, w, h, s, b)
    before = rt.render.get_counters()
    out = np.zeros((h, w, 3), np.uint8)
    img, _keep = make_image(out)
    img.pixels.data = out.ctypes.data
    ticket = rt.lib.rt_frame_begin(C.byref(hs.scene), C.byref(img), s, b)
    assert ticket >= 0, rt.last_error()
    host = rt.closest_hits(hs, rays)
    assert rt.lib.rt_frame_end(ticket) == 0, rt.last_error()
    _same_hits(want, host)
    assert np.array_equal(out, ref["image"])
    assert rt.render.get_counters() == before                      # the frame's counters, not disturbed by the query
    # counters of a render are what they are without queries before it
    rt.occluded(hs, rays)
    again = rt.render_frame(hs, w, h, s, b)
    assert again["counters"] == ref["counters"] and np.array_equal(again["image"], ref["image"])


def test_residency_edits_are_seen_by_the_next_query(rt, oracle):
    from raytracing_c_amd.configs import load_config
    hs, _ = load_config("spheres")
    rays = _rays(hs, 20000, np.random.default_rng(41), special=False)
    sc = C.byref(hs.scene)

    def both():
        want, _ = _oracle_trace(oracle, hs, rays)
        got = rt.closest_hits(hs, rays)
        _same_hits(want, got)
        return want

    a = both()
    T = hs.scene.triangles
    n = int(T.len)
    zs = [np.ctypeslib.as_array(T.z[k], (n,)) for k in range(3)]
    saved = [z.copy() for z in zs]
    lo, hi = _bbox(hs)
    shift = np.float32(0.25 * (hi[2] - lo[2]))
    ids = np.unique(a["triangle"][a["triangle"] >= 0])          # (the arrays are padded: edit triangles the rays do hit)
    i0, j0 = int(ids[len(ids) // 4]), int(ids[len(ids) // 2])
    # an edit that is reported: rt_scene_touch patches the copy, the next query sees it
    for z in zs:
        z[i0:i0 + 600] += shift
    for k in range(3):
        assert rt.lib.rt_scene_touch(sc, zs[k][i0:].ctypes.data, 600 * 4) in (0, 1), rt.last_error()
    b = both()
    assert a.tobytes() != b.tobytes(), "the edit must change what the rays hit"
    # an edit nobody reported, in the middle of a block: the content check behind the first slice finds it
    for z in zs:
        z[j0:j0 + 64] -= shift
    c = both()
    assert c.tobytes() != b.tobytes(), "the edit must change what the rays hit"
    # rt_scene_set_static: the content check is off.  An edit nobody reports, outside the few bytes the per-call stamp samples (a
    # block above 4 KB: 8 runs of 512 bytes spread evenly over it, rt_hip.h "a bounded sample"), is NOT seen -- the query answers
    # from the copy -- until the host tells (rt_scene_touch), and then it is.
    rt.lib.rt_scene_set_static(sc, 1)
    try:
        before = both()
        runs = [((n * 4 - 512) * k // 7 & ~7) // 4 for k in range(8)]
        k0 = next(int(i) for i in ids if all(i + 64 <= r or i >= r + 128 for r in runs) and not (i0 - 64 < i < i0 + 600)
                  and not (j0 - 64 < i < j0 + 64))
        for z in zs:
            z[k0:k0 + 64] += shift
        want, _ = _oracle_trace(oracle, hs, rays)
        assert want.tobytes() != before.tobytes(), "the edit must change what the rays hit"
        assert rt.closest_hits(hs, rays).tobytes() == before.tobytes(), "static: an unreported edit is not looked for"
        for k in range(3):
            assert rt.lib.rt_scene_touch(sc, zs[k][k0:].ctypes.data, 64 * 4) in (0, 1), rt.last_error()
        both()
        for k in range(3):
            zs[k][:] = saved[k]
            assert rt.lib.rt_scene_touch(sc, zs[k].ctypes.data, n * 4) in (0, 1)
        c = both()
        assert c.tobytes() == a.tobytes()
    finally:
        rt.lib.rt_scene_set_static(sc, 0)
