"""The shade block, the BRDF sampler, the environment lookup and the camera rays at unit level: shade(), sample_disney(),
background_lookup() and primary_ray() of raytracing_c_amd/csrc/rt_dev.hip.h on the hand-aimed inputs of tests/_shade_inputs.py,
item by item against the oracle's unit functions (include/rt_hip_diag.h: rt_test_shade, rt_test_brdf, rt_test_background,
rt_test_primary_ray).  tests/test_shade_inputs_cpu.py shows, with the oracle alone, that the lists reach the arms they aim at.

Bar: BIT-EXACT -- every output float has the oracle's bit pattern or both are NaN, `terminate`, the RNG state afterwards (of
terminated items too) and the `textured` increment are equal.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import _shade_inputs as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


@pytest.fixture(scope="module")
def dscene(rt, diag):
    d = diag.rt_scene_upload(C.byref(S.shade_scene().hs.scene))
    assert d, rt.last_error(diag)
    yield d
    diag.rt_scene_release(d)


def _first_bad(ok_rows):
    bad = np.flatnonzero(~ok_rows)
    return (len(bad), int(bad[0])) if len(bad) else (0, -1)


# ---------------------------------------------------------------------------------------------------------------------
# lane orders: `order` lists item indices (an item may appear more than once); entry j is lane j & 63 of wave j >> 6

def _order_sorted():
    """whole waves of ONE material: the items of each variant, padded with its own first items to a multiple of 64"""
    v = S.shade_items()["variant"]
    out = []
    for k in range(int(v.max()) + 1):
        idx = np.flatnonzero(v == k)
        out.append(np.concatenate([idx, idx[:(-len(idx)) % 64]]))
    return np.concatenate(out)


def _order_interleaved():
    v = S.shade_items()["variant"]
    order = np.random.default_rng(7010).permutation(len(v))
    waves = [v[order[j:j + 64]] for j in range(0, len(order), 64)]
    assert all(len(np.unique(w)) >= 2 for w in waves), "a wave of the interleaved order is material-uniform"
    return order


def _order_sorted_plus_one():
    """... and a last wave of ONE lane, whose material is not that of the wave before it"""
    v = S.shade_items()["variant"]
    order = _order_sorted()
    odd = int(np.flatnonzero(v != v[order[-1]])[0])
    return np.concatenate([order, [odd]])


ORDERS = {"sorted": _order_sorted, "interleaved": _order_interleaved, "sorted+1": _order_sorted_plus_one}


def _run_shade(rt, diag, dscene, mode, order):
    it = S.shade_items()
    n = len(order)
    tri, inp, seed = (np.ascontiguousarray(it[k][order]) for k in ("tri", "inp", "seed"))
    out, state, term, tex = np.zeros((n, 9), np.float32), np.zeros(n, np.uint32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    rc = diag.rt_test_shade(dscene, mode, n, tri.ctypes.data, inp.ctypes.data, seed.ctypes.data, out.ctypes.data, state.ctypes.data,
                            term.ctypes.data, tex.ctypes.data)
    assert rc == 0, rt.last_error(diag)
    return dict(out=out, state=state, terminate=term, textured=tex)


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
def test_shade_equals_the_oracle(rt, oracle, diag, dscene, mode):
    """shade<ShadeParams> (mode 0) and shade<ShadeParamsLds> (mode 1: the path kernel's instance, sRGB scale table in LDS) on the
    whole shade-level list in three lane orders: whole waves of one material (the record comes through the scalar cache), every
    wave mixed (vector loads), and the uniform order with n = 64 k + 1 (the last wave's first active lane is its only one).  Each
    order equals the oracle item by item, and so the three agree with each other."""
    it, want = S.shade_items(), S.shade_reference()
    sorted_order = _order_sorted()
    assert len(sorted_order) % 64 == 0 and all(len(np.unique(it["variant"][sorted_order[j:j + 64]])) == 1 for j in range(0, len(sorted_order), 64))
    assert set(sorted_order.tolist()) == set(range(len(it["tri"])))
    per_order = {}
    for name, make in ORDERS.items():
        order = make()
        got = _run_shade(rt, diag, dscene, mode, order)
        ok = (np.all(S.same_bits(want["out"][order], got["out"]), axis=1) & (want["terminate"][order] == got["terminate"])
              & (want["state"][order] == got["state"]) & (want["textured"][order] == got["textured"]))
        n_bad, j = _first_bad(ok)
        if n_bad:
            i = int(order[j])
            pytest.fail(f"mode {mode}, order {name}: {n_bad} of {len(order)} entries differ; first: entry {j} (wave {j >> 6}, lane {j & 63})\n"
                        f"{S.describe_shade_item(i)}\n"
                        f"oracle: out {want['out'][i].tolist()} terminate {want['terminate'][i]} state {want['state'][i]:#x} textured {want['textured'][i]}\n"
                        f"device: out {got['out'][j].tolist()} terminate {got['terminate'][j]} state {got['state'][j]:#x} textured {got['textured'][j]}")
        first = np.full(len(it["tri"]), -1)
        first[order[::-1]] = np.arange(len(order))[::-1]                # the first entry of every item
        per_order[name] = {k: a[first] for k, a in got.items()}
    for name in ("interleaved", "sorted+1"):
        for k, a in per_order["sorted"].items():
            b = per_order[name][k]
            same = np.all(S.same_bits(a, b), axis=1) if k == "out" else a == b
            assert np.all(same), (name, k, S.describe_shade_item(int(np.flatnonzero(~same)[0])))


def test_brdf_equals_the_oracle(rt, oracle, diag):
    it, want = S.brdf_items(), S.brdf_reference()
    n = len(it["seed"])
    out_dir, brdf, state = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.uint32)
    rc = diag.rt_test_brdf(n, it["params"].ctypes.data, it["in_dir"].ctypes.data, it["seed"].ctypes.data, out_dir.ctypes.data,
                           brdf.ctypes.data, state.ctypes.data)
    assert rc == 0, rt.last_error(diag)
    ok = (np.all(S.same_bits(want["out_dir"], out_dir), axis=1) & np.all(S.same_bits(want["brdf"], brdf), axis=1) & (want["state"] == state))
    n_bad, i = _first_bad(ok)
    assert n_bad == 0, (f"{n_bad} of {n} items differ; first: item {i}, (roughness, metalness, sheen, sheen_tint, aniso2, base) "
                        f"{it['params'][i].tolist()}, in_dir {it['in_dir'][i].tolist()}, seed {it['seed'][i]:#x}, lobe draws {want['draws'][i]}\n"
                        f"oracle: out_dir {want['out_dir'][i].tolist()} brdf {want['brdf'][i].tolist()} state {want['state'][i]:#x}\n"
                        f"device: out_dir {out_dir[i].tolist()} brdf {brdf[i].tolist()} state {state[i]:#x}")


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
def test_background_equals_the_oracle(rt, oracle, diag, dscene, mode):
    dirs, want = S.background_dirs(), S.background_reference()
    got = np.zeros_like(want)
    rc = diag.rt_test_background(dscene, mode, len(dirs), dirs.ctypes.data, got.ctypes.data)
    assert rc == 0, rt.last_error(diag)
    n_bad, i = _first_bad(np.all(S.same_bits(want, got), axis=1))
    if n_bad:
        u, v = S.background_uv(dirs[i:i + 1])
        pytest.fail(f"mode {mode}: {n_bad} of {len(dirs)} directions differ; first: item {i}, direction {dirs[i].tolist()} "
                    f"(bits {S.bits(dirs[i]).tolist()}), u {u[0]!r} v {v[0]!r}\noracle {want[i].tolist()}\ndevice {got[i].tolist()}")


@pytest.mark.parametrize("width,height", S.FRAME_SIZES, ids=[f"{w}x{h}" for w, h in S.FRAME_SIZES])
def test_primary_rays_equal_the_oracle(rt, oracle, diag, width, height):
    """every ray of these (x, y, sample), not the image: corners, edge mid-points and random pixels of the frame, under six camera
    matrices (rotations, a sheared one, one translated by 1e5) and four focal lengths (0 among them)"""
    for k, ((cam, xys), want) in enumerate(zip(S.primary_items(width, height), S.primary_reference(width, height))):
        got = np.zeros_like(want)
        rc = diag.rt_test_primary_ray(C.byref(cam), width, height, len(xys), xys.ctypes.data, got.ctypes.data)
        assert rc == 0, rt.last_error(diag)
        n_bad, i = _first_bad(np.all(S.same_bits(want, got), axis=1))
        assert n_bad == 0, (f"{width}x{height}, call {k}: {n_bad} of {len(xys)} rays differ; first: (x, y, sample) {xys[i].tolist()}, "
                            f"focal_length {cam.focal_length!r}, view_matrix {np.array(cam.view_matrix.rows).tolist()}\n"
                            f"oracle {want[i].tolist()}\ndevice {got[i].tolist()}")
