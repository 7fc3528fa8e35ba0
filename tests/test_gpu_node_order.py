"""The order word of a full node block (node_enter, csrc/rt_dev.hip.h): for the FAST slab forms the eight children are ordered
by a 19-comparator network on exact 32-bit keys, (bits(t_minv) - bits(RT_EPS)) << 3 | child for a candidate and 0xFFFFFFF8 | child
otherwise; a block in which a distance could overflow the key (raw >= 0x1FFFFFFF, about 1.8e15) is redone by the rank sort.

Checked here: the unit kernel rt_test_node_order (both device forms and the guard on distances a test chooses) against a numpy
model of the reference's selection loop raytracer.c:459-468 -- nearest candidate first, the first found (lowest index) on ties,
candidates only; the guard on both sides of its bound; that the crafted cases catch a network with any one comparator dropped
(in numpy); and frames and rays of a scene whose entry distances lie below, across and above the bound, against the oracle.

The guard: the largest of the eight raw values compared with 0x1FFFFFFF -- silent at 0x1FFFFFFE (the largest raw value whose
key is exact), firing from 0x1FFFFFFF on, a non-candidate's distance counting too.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")

EPS_BITS = 0x38D1B717                    # bits(RT_EPS = 0.0001f)
INF_BITS = 0x7F800000
RAW_END = 0x1FFFFFFF                     # raw = bits - EPS_BITS; keys are exact below this
MISS_KEY = 0xFFFFFFF8
NETWORK = [(0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7), (0, 1), (2, 3), (4, 5), (6, 7),
           (2, 4), (3, 5), (1, 4), (3, 6), (1, 2), (3, 4), (5, 6)]
COUNTERS = ("paths", "rays", "node_visits", "leaf_visits", "shades", "backgrounds", "textured")


def test_the_constants_belong_to_rt_eps():
    assert int(np.float32(0.0001).view(np.uint32)) == EPS_BITS
    assert ((RAW_END - 1) << 3 | 7) < MISS_KEY and (RAW_END << 3) == MISS_KEY
    assert 1.8e15 < float(np.uint32(EPS_BITS + RAW_END).view(np.float32)) < 1.9e15


# ---- the models ---------------------------------------------------------------------------------------------------------

def selection_loop(bits, cand):
    """raytracer.c:459-468 over n cases at once: eight times, the smallest distance among the candidates not yet taken, the
    first found on ties.  Returns (order (n, 8) with -1 past the count, count (n,))."""
    n = len(bits)
    dist = np.where(cand, bits.view(np.float32), np.float32(np.inf)).astype(np.float32)
    order = np.full((n, 8), -1, np.int64)
    count = np.zeros(n, np.int64)
    for i in range(8):
        j = np.argmin(dist, axis=1)                                  # the first minimum: `<` in the loop keeps the first found
        found = dist[np.arange(n), j] < np.inf
        order[found, i] = j[found]
        count += found
        dist[np.arange(n), j] = np.inf
    return order, count


def word_fields(words):
    w = np.asarray(words, np.uint32).astype(np.int64)
    return np.stack([(w >> (3 * m)) & 7 for m in range(8)], axis=1), (w >> 24) & 0xFF


def keys_of(bits, cand):
    raw = (bits.astype(np.int64) - EPS_BITS) & 0xFFFFFFFF
    k = np.arange(8, dtype=np.int64)[None, :]
    return np.where(cand, ((raw << 3) & 0xFFFFFFFF) | k, MISS_KEY | k), raw


def network_word(bits, cand, comparators):
    """The keyed form in numpy: keys, the comparators in order, the low three bits of the sorted keys, the count."""
    key, _ = keys_of(bits, cand)
    key = key.copy()
    for a, b in comparators:
        lo, hi = np.minimum(key[:, a], key[:, b]), np.maximum(key[:, a], key[:, b])
        key[:, a], key[:, b] = lo, hi
    w = np.zeros(len(bits), np.int64)
    for m in range(8):
        w |= (key[:, m] & 7) << (3 * m)
    return (w | (cand.sum(axis=1).astype(np.int64) << 24)).astype(np.uint32)


def guard_model(bits):
    _, raw = keys_of(bits, np.ones_like(bits, bool))
    return (raw.max(axis=1) >= RAW_END).astype(np.uint32)


def agrees(words, order, count):
    """per case: the count field and the first `count` entries of the word equal the selection loop's"""
    got_order, got_count = word_fields(words)
    ok = got_count == count
    for m in range(8):
        ok &= (m >= count) | (got_order[:, m] == order[:, m])
    return ok


# ---- the cases ----------------------------------------------------------------------------------------------------------

def f32_bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def crafted_cases():
    """(bits (n, 8) uint32, cand (n, 8) bool): every distance below the guard's bound"""
    B, Cd = [], []

    def add(bits, cand):
        B.append(np.asarray(bits, np.uint32))
        Cd.append(np.asarray(cand, bool))

    one = int(f32_bits(1.0))
    # all eight at RT_EPS, with every set of candidates: 0 ... 8 candidates, every child a miss among them
    for mask in range(256):
        add([EPS_BITS] * 8, [(mask >> k) & 1 for k in range(8)])
    # two distances, every split: all ties inside a group, every set of indices nearer than the rest
    for mask in range(256):
        add([one if (mask >> k) & 1 else one + 64 for k in range(8)], [1] * 8)
    # pairs 1 ulp apart, in both index orders, the other six missing / farther / nearer
    for i, j in itertools.combinations(range(8), 2):
        for lo, hi in ((i, j), (j, i)):
            for base in (EPS_BITS, one, int(f32_bits(3.0e14))):
                for others in ("miss", "far", "near"):
                    bits = [base + 5 if others == "far" else EPS_BITS] * 8
                    cand = [others != "miss"] * 8
                    pair = base + 7 if others == "near" else base
                    bits[lo], bits[hi] = pair, pair + 1
                    cand[lo] = cand[hi] = True
                    add(bits, cand)
    # equal distances on non-adjacent indices, a nearer and a farther child between them
    for i, j in ((0, 2), (0, 7), (1, 5), (3, 6), (2, 7), (0, 4)):
        bits = [one + 16 * k for k in range(8)]
        bits[i] = bits[j] = one + 40
        add(bits, [1] * 8)
        add(bits, [k != (i + 1) % 8 for k in range(8)])
    # eight distinct distances: every rotation of the sorted and of the reversed list, and seeded permutations
    ramp = [int(f32_bits(0.5 * (k + 1))) for k in range(8)]
    for r in range(8):
        add(ramp[r:] + ramp[:r], [1] * 8)
        add((ramp[::-1])[r:] + (ramp[::-1])[:r], [1] * 8)
    rng = np.random.default_rng(19)
    for _ in range(512):
        add(rng.permutation(ramp), [1] * 8)
    # distances spanning 1e-4 ... 1e15, 0 ... 8 candidates
    for n_cand in range(9):
        for _ in range(12):
            d = np.maximum(np.float32(1e-4), (10.0 ** rng.uniform(-4, 15, 8)).astype(np.float32))
            cand = np.zeros(8, bool)
            cand[rng.choice(8, n_cand, replace=False)] = True
            add(f32_bits(d), cand)
    add(f32_bits([1e-4, 1e15, 1e-3, 1e14, 1.0, 1e7, 1e-2, 1e11]), [1] * 8)
    return np.stack(B), np.stack(Cd)


def random_cases(n, seed):
    """Mixed: exact ties at RT_EPS, distances 1 - 15 ulp apart, wide-range values, misses; all below the guard's bound."""
    rng = np.random.default_rng(seed)
    wide = np.maximum(np.float32(1e-4), (10.0 ** rng.uniform(-4, 15, (n, 8))).astype(np.float32)).view(np.uint32)
    close = (int(f32_bits(2.5)) + rng.integers(0, 16, (n, 8))).astype(np.uint32)
    kind = rng.integers(0, 4, (n, 8))
    bits = np.where(kind == 0, np.uint32(EPS_BITS), np.where(kind == 1, close, wide)).astype(np.uint32)
    whole = rng.integers(0, 3, n)                                   # a third of the cases: all eight close together
    bits[whole == 0] = close[whole == 0]
    cand = rng.random((n, 8)) < rng.choice([0.25, 0.6, 1.0], (n, 1))
    assert not guard_model(bits).any()
    return bits, cand


def guard_cases():
    """(bits, cand, fires): around raw = 0x1FFFFFFE / 0x1FFFFFFF, for a candidate and for a non-candidate"""
    one = int(f32_bits(1.0))
    B, Cd, F = [], [], []
    for raw, fires in ((RAW_END - 2, 0), (RAW_END - 1, 0), (RAW_END, 1), (RAW_END + 1, 1), (0x20000000, 1), (0x3FFFFFFF, 1),
                       (INF_BITS - EPS_BITS, 1)):
        for k in range(8):
            for is_cand in (True, False):
                if is_cand and raw == INF_BITS - EPS_BITS:
                    continue                                          # an infinite entry distance is never a candidate's
                bits = [one + 3 * j for j in range(8)]
                cand = [j % 3 != 1 for j in range(8)]
                bits[k], cand[k] = EPS_BITS + raw, is_cand
                B.append(bits), Cd.append(cand), F.append(fires)
    # only NON-candidates are huge; every candidate near
    B.append([EPS_BITS, int(f32_bits(4e15)), one, int(f32_bits(1e30)), EPS_BITS, INF_BITS, one, one])
    Cd.append([1, 0, 1, 0, 1, 0, 1, 1]), F.append(1)
    # the bound is on the largest value, not on bits that several values set between them
    B.append([EPS_BITS + 0x10000000, EPS_BITS + 0x0FFFFFFF] + [one] * 6), Cd.append([1] * 8), F.append(0)
    # two candidates whose keys would collide with each other or with a miss key if the block were not redone
    B.append([EPS_BITS + 0x20000005, EPS_BITS + 5, one, one, one, one, one, one]), Cd.append([1] * 8), F.append(1)
    B.append([EPS_BITS + RAW_END, one, one, one, one, one, one, one]), Cd.append([1, 0, 1, 1, 1, 1, 1, 1]), F.append(1)
    return np.array(B, np.uint32), np.array(Cd, bool), np.array(F, np.uint32)


def device_words(diag, bits, cand):
    bits = np.ascontiguousarray(bits, np.uint32)
    flags = np.ascontiguousarray(cand, np.uint8)
    out = np.zeros((len(bits), 3), np.uint32)
    import raytracing_c_amd as rt
    assert diag.rt_test_node_order(len(bits), bits.ctypes.data, flags.ctypes.data, out.ctypes.data) == 0, rt.last_error(diag)
    return out[:, 0], out[:, 1], out[:, 2]


# ---- without a GPU: the models against each other -------------------------------------------------------------------------

def test_the_network_model_is_the_selection_loop():
    for bits, cand in (crafted_cases(), random_cases(3000, 5)):
        order, count = selection_loop(bits, cand)
        assert not guard_model(bits).any()
        assert agrees(network_word(bits, cand, NETWORK), order, count).all()


def test_a_dropped_comparator_fails_the_crafted_cases():
    """The mutant check: the network less any ONE of its 19 comparators orders some crafted case wrongly, so the crafted list
    would catch a kernel whose network lacks it."""
    bits, cand = crafted_cases()
    order, count = selection_loop(bits, cand)
    for drop in range(len(NETWORK)):
        mutant = NETWORK[:drop] + NETWORK[drop + 1:]
        assert not agrees(network_word(bits, cand, mutant), order, count).all(), NETWORK[drop]


# ---- the unit kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cases", ["crafted", "random"])
def test_order_words(diag, cases):
    bits, cand = crafted_cases() if cases == "crafted" else random_cases(3000, 7)
    assert 500 < len(bits) < 5000
    order, count = selection_loop(bits, cand)
    assert set(count.tolist()) == set(range(9))
    keyed, ranked, guard = device_words(diag, bits, cand)
    assert not guard.any()
    bad = ~agrees(keyed, order, count)
    assert not bad.any(), (int(bad.sum()), bits[bad][0], cand[bad][0], hex(int(keyed[bad][0])))
    assert agrees(ranked, order, count).all()
    assert np.array_equal(keyed, ranked)                              # the whole word, the places past the count too


@pytest.mark.gpu
def test_guard(diag):
    bits, cand, fires = guard_cases()
    assert np.array_equal(guard_model(bits), fires)
    order, count = selection_loop(bits, cand)
    keyed, ranked, guard = device_words(diag, bits, cand)
    assert np.array_equal(guard, fires), np.nonzero(guard != fires)[0]
    assert agrees(ranked, order, count).all()                         # what a guarded block returns
    quiet = fires == 0
    assert quiet.sum() >= 32 and np.array_equal(keyed[quiet], ranked[quiet])
    assert agrees(keyed[quiet], order[quiet], count[quiet]).all()


# ---- frames and rays where the rank sort really takes over ---------------------------------------------------------------
# spheres.glb seen from EYE along -z, scaled by a power of two ABOUT THE EYE: the same picture, every distance from the camera
# times 2^k, and camera rays that still take the FAST slab form (their origin stays within RT_SLAB_FUSED_MAX_ORIGIN = 256 of the
# world's origin; a camera scaled along with the scene would send every ray through the min / max form, which never builds
# keys).  The spheres lie 8 - 16 units from the eye.
#   2^30  below: entry distances around 1e10, the keys order nearly every block;
#   2^43  across: the spheres are hit at 7e13 - 1.4e14, and the rays near the middle column and row of the picture, nearly parallel
#         to a slab (|d| < 0.015), have entry distances beyond 1.8e15 for the children they pass beside: such a block is redone by
#         the rank sort while hits prune the traversal, so the order matters to the counters;
#   2^49  above: every entry distance beyond the scene's near side is; the triangle test overflows there (edge^2 x distance >
#         FLT_MAX for this tessellation from 2^44 on), so the oracle's frame is background only -- finite, and its node and leaf
#         visits still count every candidate of every block.
EYE = np.array([0.3, 0.8, 12.0], np.float32)


def spheres_about_camera(k):
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.loaders import load_model_data
    from raytracing_c_amd.scene import build_scene
    d = load_model_data(os.path.join(ASSETS, "spheres.glb"))
    cam = np.eye(4, dtype=np.float32)
    a = np.tan(d["camera"][1] / 2) / 32                   # half a pixel of the 32 x 32 frames, about both axes: one column and one
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])      # row of pixels look along -z, their
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])      # rays nearly parallel to two slabs
    cam[:3, :3] = ry @ rx
    cam[:3, 3] = EYE
    pos = (EYE + (d["positions"] - EYE) * np.float32(2.0 ** k)).astype(np.float32)
    return build_scene(pos, d["normals"], d["uvs"], d["material_ids"], d["materials"], d["images"], cam, d["camera"][1],
                       procedural_background()), EYE


def entry_distances(hs, o, d):
    """t_minv of the populated children of the nodes right under the root -- full node blocks that nearly every ray which
    enters the scene's box takes -- for rays (o, d), in float64: the margins asserted on it are factors, not ulps"""
    nodes = np.asarray(hs.nodes_array(), np.float64)                  # (n, 6, 8): rows min x y z, max x y z of the eight children
    populated = lambda nd: (nd[0] <= nd[3]) & ((nd[3] - nd[0] + nd[4] - nd[1] + nd[5] - nd[2]) > 0)      # (an empty child is all zero)
    inv = 1.0 / d
    out = []
    for child in np.nonzero(populated(nodes[0]))[0]:
        nd = nodes[1 + child]
        t0 = (nd[None, 0:3, :] - o[:, :, None]) * inv[:, :, None]
        t1 = (nd[None, 3:6, :] - o[:, :, None]) * inv[:, :, None]
        out.append(np.maximum(1e-4, np.minimum(t0, t1).max(axis=1))[:, populated(nd)])
    return np.concatenate(out, axis=1)


SCALES = {30: "below", 43: "across", 49: "above"}
BOUND = float(np.uint32(EPS_BITS + RAW_END).view(np.float32))


def rays_from_the_camera(hs, eye, n, seed):
    """FAST rays (origin within a unit of the camera, no zero component) towards points of the scene"""
    rng = np.random.default_rng(seed)
    T = hs.scene.triangles
    m = int(T.len)
    pts = np.stack([np.ctypeslib.as_array(T.x[0], (m,)), np.ctypeslib.as_array(T.y[0], (m,)), np.ctypeslib.as_array(T.z[0], (m,))], 1)
    o = eye[None, :].astype(np.float64) + rng.uniform(-1, 1, (n, 3))
    tgt = pts[rng.integers(0, m, n)].astype(np.float64) * rng.uniform(0.7, 1.3, (n, 1))
    d = tgt - o
    d[0::4, 0] *= 1e-3                                                # nearly parallel to the x slabs, to the y slabs: entry
    d[1::4, 1] *= 1e-3                                                # distances 1000 times the scene's for the boxes passed beside
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)


@pytest.mark.parametrize("k", sorted(SCALES))
def test_the_scaled_scenes_are_what_they_are_for(oracle, k):
    """On the CPU: the oracle renders a finite frame -- with hits where the triangle test does not overflow -- and the entry
    distances of the test rays lie where the scale puts them"""
    from tests import _oracle
    hs, eye = spheres_about_camera(k)
    want = _oracle.render(hs, 32, 32, 4, 4)
    assert want["counters"]["backgrounds"] > 0 and (want["counters"]["shades"] > 500) == (SCALES[k] != "above")
    assert 0 < want["image"].mean() < 255
    rays = rays_from_the_camera(hs, eye, 2048, 3).astype(np.float64)
    t = entry_distances(hs, rays[:, :3], rays[:, 3:])
    over = (t >= 2 * BOUND).any(axis=1)                                # a block with such a child is redone by the rank sort
    under = (t <= BOUND / 2).all(axis=1)
    if SCALES[k] == "below":
        assert under.mean() > 0.95
    elif SCALES[k] == "above":
        assert over.mean() > 0.95
    else:
        assert over.mean() > 0.2 and under.mean() > 0.2


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(SCALES))
def test_scaled_frames_equal_the_oracle(oracle, k):
    import raytracing_c_amd as rt
    from tests import _oracle
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    hs, _ = spheres_about_camera(k)
    w, h, s, b = 32, 32, 4, 4
    want = _oracle.render(hs, w, h, s, b)
    got = rt.render_frame(hs, w, h, s, b, want_accum=True)
    assert np.array_equal(want["image"], got["image"])
    assert np.array_equal(want["accum"], got["accum"])
    for name in COUNTERS:
        assert want["counters"][name] == getattr(got["counters"], name), name


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(SCALES))
def test_scaled_rays_through_the_full_node_blocks(oracle, diag, k):
    """The production traversal without a pyramid -- every node block a full one, from LDS (mode 0) and through L1 / L2 (mode 2)
    -- on FAST rays whose root block already meets the distances of the scale: hits and visit totals equal the oracle's."""
    import raytracing_c_amd as rt
    from tests.test_gpu_trace_stream import _gpu_trace, _oracle_trace, _same
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    hs, eye = spheres_about_camera(k)
    rays = rays_from_the_camera(hs, eye, 4096, 3)
    want = _oracle_trace(oracle, hs, rays)
    assert ((want[1] >= 0).sum() > len(rays) // 10) == (SCALES[k] != "above") and want[3][0] > len(rays) and want[3][1] > 0
    d = rt.diag.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error(rt.diag)
    try:
        for mode in (0, 2):
            _same(want, _gpu_trace(rt, d, rays, None, 48, mode))
    finally:
        rt.diag.rt_scene_release(d)
