"""One path step at unit level: shade_hit() of raytracing_c_amd/csrc/rt_dev.hip.h in its three instances and feature_hit() of
rt_features.hip on the hand-aimed hits of tests/_step_inputs.py, item by item against oracle_fill_hit + oracle_path_step
(include/rt_hip_diag.h: rt_test_shade_hit, rt_test_feature_hit).  tests/test_step_inputs_cpu.py shows, with the oracle alone, that
the list reaches the arms it aims at and that the two oracle functions are the code oracle_cast_ray runs.

Bar: BIT-EXACT -- every output float (next origin, direction, tint, emission, radiance) has the oracle's bit pattern or both are
NaN; the RNG state, the bounce count, `done` and the increments of the `shades` and `textured` counters are equal.  No tolerance
anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import _step_inputs as T

pytestmark = pytest.mark.gpu

MODES = {0: "ShadeParams", 1: "ShadeParamsLds", 2: "RT_KParams"}


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def dscene(rt, diag):
    d = diag.rt_scene_upload(C.byref(T.step_scene().hs.scene))
    assert d, rt.last_error(diag)
    yield d
    diag.rt_scene_release(d)


# ---------------------------------------------------------------------------------------------------------------------
# lane orders: `order` lists item indices (an item may appear more than once); entry j is lane j & 63 of wave j >> 6.  Which items
# shade and which pass through is the oracle's outcome (it does not depend on max_bounces).

def _shaded():
    return T.step_reference(T.MAX_BOUNCES[1])["words"][:, 3] == 1


def _material():
    """the device material of every item's triangle"""
    return T.step_scene().variant[T.step_items()["tri"]]


def _order_uniform_front():
    """whole waves of ONE material, all front faces: every lane is inside shade_hit()'s `else`, the record comes through the scalar
    cache.  The shading items of each material, padded with its own first items to a multiple of 64."""
    shaded, mat = _shaded(), _material()
    out = []
    for k in np.unique(mat[shaded]):
        idx = np.flatnonzero(shaded & (mat == k))
        out.append(np.concatenate([idx, idx[:(-len(idx)) % 64]]))
    return np.concatenate(out)


def _order_scattered_back():
    """every item once, shuffled: back faces at random places of every wave, and a back face in lane 0 of every wave -- shade()'s
    readfirstlane then reads a lane that is not the wave's lane 0"""
    shaded = _shaded()
    order = np.random.default_rng(7130).permutation(len(shaded))
    for w in range(0, len(order), 64):
        back = np.flatnonzero(~shaded[order[w:w + 64]])
        assert len(back), "a wave of the shuffled order has no back face"
        order[[w, w + back[0]]] = order[[w + back[0], w]]
    return order


def _order_lonely():
    """waves with exactly ONE shading lane, at every position 1 .. 63 (lane 37 among them), between 63 back faces; then two waves of
    back faces only, where shade() is not reached at all"""
    shaded, mat = _shaded(), _material()
    rng = np.random.default_rng(7131)
    back, front = np.flatnonzero(~shaded), np.flatnonzero(shaded)
    waves = []
    mats = np.unique(mat[front])
    for j, lane in enumerate(list(range(1, 64)) * 2):
        w = rng.choice(back, 64, replace=False)
        of_mat = front[mat[front] == mats[j % len(mats)]]
        w[lane] = of_mat[(j // len(mats)) % len(of_mat)]
        waves.append(w)
    waves += [rng.choice(back, 64, replace=False), rng.choice(back, 64, replace=False)]
    return np.concatenate(waves)


def _order_uniform_plus_one():
    """the uniform order with n = 64 k + 1: the last wave's only lane, of another material than the wave before it"""
    shaded, mat = _shaded(), _material()
    order = _order_uniform_front()
    odd = int(np.flatnonzero(shaded & (mat != mat[order[-1]]))[0])
    return np.concatenate([order, [odd]])


ORDERS = {"uniform front": _order_uniform_front, "scattered back faces": _order_scattered_back, "lonely shading lane": _order_lonely,
          "uniform + 1": _order_uniform_plus_one}


def test_the_lane_orders_are_what_they_say():
    shaded, mat = _shaded(), _material()
    o = _order_uniform_front()
    assert len(o) % 64 == 0 and np.all(shaded[o]) and all(len(np.unique(mat[o[j:j + 64]])) == 1 for j in range(0, len(o), 64))
    assert set(o.tolist()) == set(np.flatnonzero(shaded).tolist())
    o = _order_scattered_back()
    assert sorted(o.tolist()) == list(range(len(shaded))) and not np.any(shaded[o[::64]])
    waves = [o[j:j + 64] for j in range(0, len(o) - 63, 64)]
    assert all(2 <= np.sum(~shaded[w]) <= 62 for w in waves) and all(len(np.unique(mat[w][shaded[w]])) >= 2 for w in waves)
    o = _order_lonely()
    counts = shaded[o].reshape(-1, 64).sum(axis=1)
    assert np.all(counts[:-2] == 1) and np.all(counts[-2:] == 0) and not np.any(shaded[o[::64]])
    assert set(np.argmax(shaded[o].reshape(-1, 64)[:-2], axis=1).tolist()) == set(range(1, 64))
    assert len(np.unique(mat[o][shaded[o]])) == len(np.unique(mat[shaded]))
    o = _order_uniform_plus_one()
    assert len(o) % 64 == 1 and mat[o[-1]] != mat[o[-2]]


def _run_step(rt, diag, dscene, mode, max_bounces, order):
    it = T.step_items()
    n = len(order)
    slot, hit, ray, carry, seed = (np.ascontiguousarray(it[k][order]) for k in ("slot", "hit", "ray", "carry", "seed"))
    b_in = np.ascontiguousarray(T.bounce_in(max_bounces)[order])
    out, words = np.full((n, 15), 7.0, np.float32), np.full((n, 5), 0xDEAD, np.uint32)
    rc = diag.rt_test_shade_hit(dscene, mode, max_bounces, n, slot.ctypes.data, hit.ctypes.data, ray.ctypes.data, carry.ctypes.data,
                                seed.ctypes.data, b_in.ctypes.data, out.ctypes.data, words.ctypes.data)
    assert rc == 0, rt.last_error(diag)
    return dict(out=out, words=words)


def _row(a):
    names = ("origin", "direction", "tint", "emission", "radiance")
    return ", ".join(f"{names[k]} {a[3 * k:3 * k + 3].tolist()}" for k in range(5))


def _words(w):
    return f"rng {int(w[0]):#x} bounce {int(np.int32(w[1]))} done {int(w[2])} shades +{int(w[3])} textured +{int(w[4])}"


@pytest.mark.parametrize("max_bounces", T.MAX_BOUNCES, ids=[f"bounces{b}" for b in T.MAX_BOUNCES])
@pytest.mark.parametrize("mode", list(MODES), ids=[f"mode{m}" for m in MODES])
def test_shade_hit_equals_the_oracle(rt, oracle, diag, dscene, mode, max_bounces):
    """shade_hit<ShadeParams> (mode 0, the wavefront shade kernel's), <ShadeParamsLds> (1, the path kernel's) and <RT_KParams> (2,
    cast_ray_lane's) on the whole list of hits in four lane orders.  Each order equals the oracle entry by entry, and so an item's
    result is the same in every order."""
    it, want = T.step_items(), T.step_reference(max_bounces)
    per_order = {}
    for name, make in ORDERS.items():
        order = make()
        got = _run_step(rt, diag, dscene, mode, max_bounces, order)
        ok = np.all(T.same_bits(want["out"][order], got["out"]), axis=1) & np.all(want["words"][order] == got["words"], axis=1)
        bad = np.flatnonzero(~ok)
        if len(bad):
            j = int(bad[0])
            i = int(order[j])
            pytest.fail(f"shade_hit<{MODES[mode]}>, max_bounces {max_bounces}, order '{name}': {len(bad)} of {len(order)} entries differ; "
                        f"first: entry {j} (wave {j >> 6}, lane {j & 63})\n{T.describe_step_item(i, max_bounces)}\n"
                        f"oracle: {_row(want['out'][i])}; {_words(want['words'][i])}\n"
                        f"device: {_row(got['out'][j])}; {_words(got['words'][j])}")
        first = np.full(len(it["slot"]), -1)
        first[order[::-1]] = np.arange(len(order))[::-1]                # the first entry of every item
        per_order[name] = (first, got)
    base_first, base = per_order["scattered back faces"]                # holds every item
    assert np.all(base_first >= 0)
    for name, (first, got) in per_order.items():
        k = np.flatnonzero(first >= 0)
        same = (np.all(T.same_bits(base["out"][base_first[k]], got["out"][first[k]]), axis=1)
                & np.all(base["words"][base_first[k]] == got["words"][first[k]], axis=1))
        assert np.all(same), (name, T.describe_step_item(int(k[np.flatnonzero(~same)[0]]), max_bounces))


def test_feature_hit_equals_the_oracle(rt, oracle, diag, dscene):
    """feature_hit<ShadeParamsLds> -- the feature kernel's copy of the face test and the pass-through -- on the same hits: the flag and
    the advanced origin are the path step's, the position is the filled hit's point, the normal is the debug proc's emission on the
    step's shader input, the albedo is the material's (x its texture)"""
    it, want = T.step_items(), T.feature_reference()
    for name in ("scattered back faces", "lonely shading lane", "uniform + 1"):
        order = ORDERS[name]()
        n = len(order)
        slot, hit, ray = (np.ascontiguousarray(it[k][order]) for k in ("slot", "hit", "ray"))
        out, flag = np.full((n, 12), 7.0, np.float32), np.full(n, -1, np.int32)
        rc = diag.rt_test_feature_hit(dscene, n, slot.ctypes.data, hit.ctypes.data, ray.ctypes.data, out.ctypes.data, flag.ctypes.data)
        assert rc == 0, rt.last_error(diag)
        ok = np.all(T.same_bits(want["out"][order], out), axis=1) & (want["flag"][order] == flag)
        bad = np.flatnonzero(~ok)
        if len(bad):
            j = int(bad[0])
            i = int(order[j])
            names = ("origin", "albedo", "normal", "position")
            row = lambda a: ", ".join(f"{names[k]} {a[3 * k:3 * k + 3].tolist()}" for k in range(4))      # noqa: E731
            pytest.fail(f"feature_hit, order '{name}': {len(bad)} of {n} entries differ; first: entry {j} (wave {j >> 6}, lane {j & 63})\n"
                        f"{T.describe_step_item(i)}\noracle: flag {want['flag'][i]}, {row(want['out'][i])}\ndevice: flag {flag[j]}, {row(out[j])}")


def test_what_the_entry_points_refuse(rt, diag, dscene):
    it = T.step_items()
    n = 4
    slot, hit, ray, carry, seed = (np.array(it[k][:n]) for k in ("slot", "hit", "ray", "carry", "seed"))
    b_in = np.zeros(n, np.int32)
    out, words, flag = np.zeros((n, 15), np.float32), np.zeros((n, 5), np.uint32), np.zeros(n, np.int32)

    def step(mode=1, slot=slot, hit=hit):
        return diag.rt_test_shade_hit(dscene, mode, 4, n, slot.ctypes.data, hit.ctypes.data, ray.ctypes.data, carry.ctypes.data,
                                      seed.ctypes.data, b_in.ctypes.data, out.ctypes.data, words.ctypes.data)

    def feature(slot=slot, hit=hit):
        return diag.rt_test_feature_hit(dscene, n, slot.ctypes.data, hit.ctypes.data, ray.ctypes.data, out.ctypes.data, flag.ctypes.data)

    assert step() == 0 and feature() == 0, rt.last_error(diag)
    assert step(mode=3) != 0 and "mode 3" in rt.last_error(diag)
    n_slots = T.step_scene().hs.n_slots
    for bad_slot in (-1, n_slots):
        s = slot.copy()
        s[2] = bad_slot
        assert step(slot=s) != 0 and "item 2 names triangle slot" in rt.last_error(diag)
        assert feature(slot=s) != 0 and "item 2 names triangle slot" in rt.last_error(diag)
    for bad_u in (np.nan, np.inf):
        h = hit.copy()
        h[1, 1] = bad_u
        assert step(hit=h) != 0 and "item 1" in rt.last_error(diag) and "non-finite texture coordinates" in rt.last_error(diag)
        assert feature(hit=h) != 0 and "non-finite texture coordinates" in rt.last_error(diag)
