"""Adaptive sampling without a GPU.

1. The restatement (tests/_adaptive.py) driven by the CPU oracle's sums per sample range, on the GPU tests' own scenes: the inputs
   can tell a wrong kernel -- several final sample counts occur, chunks stop at 2 x min and reach max, ragged chunks among both -- and
   four wrong merges each change `err` or the outcome on them.  These are CONDITIONS on the inputs, asserted here.
2. The exported names in all four libraries, the struct's layout against the C header, the Python mirror and entry points, and every
   refusal of the four entry points -- each reported before a device is touched, with the outputs untouched.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _adaptive as A

NAMES = ["rt_render_accumulate_chunks", "rt_adaptive_merge", "rt_resolve_adaptive", "rt_render_adaptive"]
FIELDS = ["min_samples", "max_samples", "threshold", "reserved"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

# the cases of tests/test_gpu_adaptive.py: (scene, width, height, min, max, bounces, seed, threshold)
W, H = 104, 72                      # 4 x 3 chunks, ragged both ways: the right column is 8 pixels wide, the bottom row 8 high
CASES = {"spheres": ("spheres", W, H, 2, 32, 4, 0x1234ABCD, 0.035), "helmet": ("helmet", W, H, 2, 32, 4, 0x1234ABCD, 0.035),
         # the second size: at 104 x 72 every ragged chunk is background and stops at 2 x min; at 40 x 56 (2 x 2 chunks, the right
         # column 8 wide, the bottom row 24 high) the ragged chunks hold the spheres, and one of them reaches max
         "spheres_ragged": ("spheres", 40, 56, 2, 32, 4, 0x1234ABCD, 0.035)}
MAIN = ("spheres", "helmet")

_scenes, _sums, _runs = {}, {}, {}


def scene(name):
    from raytracing_c_amd.configs import load_config
    if name not in _scenes:
        _scenes[name] = load_config(name)[0]
    return _scenes[name]


def oracle_sums(case, first, count):
    """The oracle's u64 sums (h, w, 3) of samples [first, first + count) of every pixel: once per range, read-only."""
    from tests import _oracle
    name, w, h, _, mx, bounces, seed, _ = CASES[case]
    key = (case, first, count)
    if key not in _sums:
        a = _oracle.render(scene(name), w, h, mx, bounces, seed=seed, sample_range=(first, count))["accum"]
        a.setflags(write=False)
        _sums[key] = a
    return _sums[key]


def oracle_run(case, mutation=None):
    _, w, h, mn, mx, _, _, thr = CASES[case]
    key = (case, mutation)
    if key not in _runs:
        _runs[key] = A.run(lambda first, count: oracle_sums(case, first, count), w, h, mn, mx, thr, mutation)
    return _runs[key]


# ---- 1. the inputs can tell a wrong kernel ----------------------------------------------------------------------------------------

def test_the_sample_ranges_add_up_to_the_plain_frame(oracle):
    """What the whole scheme rests on: the sums of [0, 2) + [2, 2) + [4, 4) are the sums of the plain 8-sample frame."""
    from tests import _oracle
    name, w, h, _, _, bounces, seed, _ = CASES["spheres"]
    parts = oracle_sums("spheres", 0, 2) + oracle_sums("spheres", 2, 2) + oracle_sums("spheres", 4, 4)
    assert np.array_equal(parts, _oracle.render(scene(name), w, h, 8, bounces, seed=seed)["accum"])


def test_the_cases_spread_over_the_sample_counts(oracle):
    """spheres: 4, 8, 16 and 32 all occur; helmet: 4, 16 and 32.  First-round chunk errors on both sides of the threshold."""
    want = {"spheres": {4, 8, 16, 32}, "helmet": {4, 16, 32}, "spheres_ragged": {16, 32}}
    assert set(A.ragged_chunks(W, H)) == {3, 7, 8, 9, 10, 11} and set(A.ragged_chunks(40, 56)) == {1, 2, 3}
    stopped_ragged, capped_ragged = False, False
    for case, (_, w, h, mn, mx, _, _, thr) in CASES.items():
        r = oracle_run(case)
        counts = r["chunk_samples"]
        ragged = A.ragged_chunks(w, h)
        print(case, "final counts", counts.tolist(), "first-round errors %.4f .. %.4f" % (min(r["first_errors"]), max(r["first_errors"])))
        assert set(counts.tolist()) == want[case], (case, counts.tolist())
        if case in MAIN:
            assert len(set(counts.tolist())) >= 3
            assert (counts == 2 * mn).any() and (counts == mx).any()
            assert min(r["first_errors"]) < thr < max(r["first_errors"])
        stopped_ragged |= any(counts[c] == 2 * mn for c in ragged)
        capped_ragged |= any(counts[c] == mx for c in ragged)
        # every chunk's sums are the plain frame's at its own count, and nothing is left in `fresh`
        assert not r["fresh"].any()
        for c in range(counts.size):
            x0, y0, x1, y1 = A.chunk_box(w, h, c)
            plain = sum(oracle_sums(case, f, n) for f, n in [(0, mn)] + [(k, k) for k in (2, 4, 8, 16) if k < counts[c]])
            assert np.array_equal(r["accum"][y0:y1, x0:x1], plain[y0:y1, x0:x1]), (case, c)
    assert stopped_ragged and capped_ragged


def test_the_first_round_errors_are_the_recorded_ones(oracle):
    for case, lo, hi in (("spheres", 0.0007, 0.097), ("helmet", 0.0009, 0.134)):
        e = oracle_run(case)["first_errors"]
        assert abs(min(e) - lo) < 1e-4 and abs(max(e) - hi) < 1e-3, (case, min(e), max(e))


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_a_wrong_merge_shows_on_these_inputs(oracle, mutation):
    """Each wrong merge changes an err entry, the sums or the final counts of at least one case."""
    shown = []
    for case in CASES:
        good, bad = oracle_run(case), oracle_run(case, mutation)
        differs = (not np.array_equal(good["chunk_samples"], bad["chunk_samples"]) or not np.array_equal(good["accum"], bad["accum"])
                   or not np.array_equal(good["fresh"], bad["fresh"])
                   or any(not np.array_equal(g[2], b[2]) for g, b in zip(good["rounds"], bad["rounds"])))
        shown.append(differs)
    assert any(shown), mutation
    if mutation == "ragged_1024":          # (it leaves the merge alone: it must change the OUTCOME)
        assert any(not np.array_equal(oracle_run(c)["chunk_samples"], oracle_run(c, mutation)["chunk_samples"]) for c in CASES)
    if mutation == "no_clamp":             # (there are means above 1 among the inputs: the clamp is exercised)
        assert any((A.accum_resolve(oracle_sums(c, 0, 2), 2) > 1.0).any() for c in CASES)


def test_the_restatement_on_hand_made_sums():
    """One chunk of 2 x 1 pixels: a pixel whose halves agree has q = 0; one whose halves are 0 and 1 has e = 3 / sqrt(3.0001)."""
    accum = np.zeros((1, 2, 3), np.uint64)
    fresh = np.zeros((1, 2, 3), np.uint64)
    accum[0, 0] = 5 << 30
    fresh[0, 0] = 5 << 30
    fresh[0, 1] = 7 << 32                                      # mean 3.5 with n = 2: clamped to 1
    a, f, err = A.merge(accum, fresh, 2, [0], np.array([99], np.uint64))
    e = np.float32(3.0) / np.sqrt(np.float32(3.0) + np.float32(1e-4))
    assert int(err[0]) == int(float(e) * 4294967296.0) and not f.any() and np.array_equal(a, accum + fresh)
    assert A.chunk_error(err[0], 2, 1, 0) == float(e) / 2.0 and A.chunk_error(err[0], 2, 1, 0, "ragged_1024") == float(e) / 1024.0
    assert A.stays_active(err[0], 2, 1, 0, 2, 8, 0.5) and not A.stays_active(err[0], 2, 1, 0, 2, 4, 0.5)
    assert not A.stays_active(err[0], 2, 1, 0, 2, 8, float(e) / 2.0)          # at the threshold: the chunk stops


# ---- 2. names, layout, refusals ---------------------------------------------------------------------------------------------------

def test_symbols_in_all_four_libraries_and_python_entry_points():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    for n in NAMES:
        assert n in abi.EXPORTED_SYMBOLS
        for lib in (rt.lib, rt.diag):
            assert getattr(lib, n) is not None
    for path in ("librt_hip_v1.so", "librt_hip_v2.so"):
        dll = C.CDLL(os.path.join(os.path.dirname(rt.native.LIB_PATH), path))
        for n in NAMES:
            assert getattr(dll, n) is not None
    for f in (rt.render_adaptive, rt.render_accumulate_chunks, rt.adaptive_merge, rt.resolve_adaptive):
        assert callable(f)


def test_the_struct_is_the_headers(tmp_path):
    from raytracing_c_amd import ctypes_abi as abi
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(RT_Adaptive_Params));\n'
                   + "".join(f'  printf(" %zu", offsetof(RT_Adaptive_Params, {n}));\n' for n in FIELDS) + '  return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    mirror = [C.sizeof(abi.RT_Adaptive_Params)] + [getattr(abi.RT_Adaptive_Params, n).offset for n in FIELDS]
    assert got == mirror == [16, 0, 4, 8, 12]
    assert [n for n, _ in abi.RT_Adaptive_Params._fields_] == FIELDS


def test_every_refusal_comes_before_the_device_and_leaves_the_outputs_untouched():
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    lib = rt.lib
    w, h = 104, 72                                             # 12 chunks
    A1 = 1 << 20                                               # device addresses that are never read

    def fails(call, who, *words):
        lib.rt_clear_error()
        assert call() == -1
        for word in (who + ":",) + words:
            assert word in rt.last_error(), (word, rt.last_error())

    def i32s(*v):
        return np.array(v, np.int32)

    bad_lists = [(i32s(0, 12), "chunks[1] = 12", "outside"), (i32s(-1, 3), "chunks[0] = -1", "outside"), (i32s(3, 3), "strictly ascending"),
                 (i32s(5, 2), "strictly ascending"), (i32s(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11), "strictly ascending"),
                 (i32s(1 << 30), "outside")]

    # ---- rt_render_accumulate_chunks: a scene handle that is never read
    fake = (C.c_uint8 * 4096)()
    good = abi.RT_Render_Params(width=w, height=h, samples=8, max_bounces=4, seed=1, rank=0, world=1, sample_first=3, sample_count=5)
    some = i32s(0, 5, 11)

    def launch(d=C.addressof(fake), p=good, n=3, chunks=some, accum=A1):
        return lib.rt_render_accumulate_chunks(d, None if p is None else C.byref(p), n, None if chunks is None else chunks.ctypes.data,
                                               accum, None)
    who = "rt_render_accumulate_chunks"
    fails(lambda: launch(d=None), who, "NULL scene")
    fails(lambda: launch(accum=None), who, "accumulation buffer")
    lib.rt_clear_error()
    assert launch(p=None) == -1 and "render params are NULL" in rt.last_error()
    for field, value, word in (("world", 2, "rank 0 of world 1"), ("width", 0, "invalid"), ("samples", 0, "samples"),
                               ("sample_count", 6, "sample range")):
        p = abi.RT_Render_Params.from_buffer_copy(good)
        setattr(p, field, value)
        lib.rt_clear_error()
        assert launch(p=p) == -1 and word in rt.last_error(), (field, rt.last_error())
    p = abi.RT_Render_Params.from_buffer_copy(good)
    p.rank, p.world = 1, 2
    fails(lambda: launch(p=p), who, "rank 0 of world 1")
    fails(lambda: launch(n=-1), who, "n_list")
    fails(lambda: launch(chunks=None), who, "chunks is NULL")
    for entry in bad_lists:
        fails(lambda: launch(n=entry[0].size, chunks=entry[0]), who, *entry[1:])

    # ---- rt_adaptive_merge
    def merge(width=w, height=h, n=2, n_list=3, chunks=some, accum=A1, fresh=2 * A1, err=3 * A1):
        return lib.rt_adaptive_merge(width, height, n, n_list, None if chunks is None else chunks.ctypes.data, accum, fresh, err, None)
    who = "rt_adaptive_merge"
    for width, height, word in ((0, 4, "invalid"), (4, -1, "invalid"), (1 << 15, (1 << 13) + 1, "too large")):
        fails(lambda: merge(width=width, height=height), who, word)
    fails(lambda: merge(n=0), who, "n must be >= 1")
    fails(lambda: merge(n=-4), who, "n must be >= 1")
    fails(lambda: merge(n_list=-1), who, "n_list")
    fails(lambda: merge(chunks=None), who, "chunks is NULL")
    for entry in bad_lists:
        fails(lambda: merge(n_list=entry[0].size, chunks=entry[0]), who, *entry[1:])
    fails(lambda: merge(width=33, height=31, n_list=1, chunks=i32s(2)), who, "outside [0, 2)")
    fails(lambda: merge(accum=None), who, "d_accum is NULL")
    fails(lambda: merge(fresh=None), who, "d_fresh is NULL")
    fails(lambda: merge(err=None), who, "d_err is NULL")
    fails(lambda: merge(fresh=A1), who, "one buffer")

    # ---- rt_resolve_adaptive
    def resolve(width=w, height=h, counts=A1, accum=2 * A1, image=3 * A1, linear=4 * A1, smap=5 * A1):
        return lib.rt_resolve_adaptive(width, height, counts, accum, image, linear, smap, None)
    who = "rt_resolve_adaptive"
    for width, height, word in ((0, 4, "invalid"), (4, 0, "invalid"), (1 << 15, (1 << 13) + 1, "too large")):
        fails(lambda: resolve(width=width, height=height), who, word)
    fails(lambda: resolve(counts=None), who, "d_chunk_samples is NULL")
    fails(lambda: resolve(accum=None), who, "d_accum is NULL")
    fails(lambda: resolve(image=None, linear=None, smap=None), who, "no output is wanted")

    # ---- rt_render_adaptive
    scene = abi.Scene()
    pixels = np.full((h, w, 3), 0x55, np.uint8)
    image = abi.Image()
    image.width, image.height, image.stride, image.components = w, h, w, 3
    image.pixels.data, image.pixels.len = pixels.ctypes.data, pixels.size
    linear, accum = np.full((h, w, 3), 7.0, np.float32), np.full((h, w, 3), 7, np.uint64)
    counts = np.full(12, 7, np.int32)
    ok = abi.RT_Adaptive_Params(2, 32, 0.035, 0)

    def frame(sc=scene, im=image, ap=ok, bounces=4, lin=linear.ctypes.data, acc=accum.ctypes.data, cs=counts.ctypes.data):
        return lib.rt_render_adaptive(None if sc is None else C.byref(sc), None if im is None else C.byref(im),
                                      None if ap is None else C.byref(ap), bounces, lin, acc, cs)
    who = "rt_render_adaptive"
    fails(lambda: frame(sc=None), who, "scene is NULL")
    fails(lambda: frame(im=None), who, "image is NULL")
    fails(lambda: frame(ap=None), who, "adaptive params are NULL")
    for mn, mx, thr, res, word in ((0, 32, 0.1, 0, "min_samples"), (-2, 32, 0.1, 0, "min_samples"), (2, 2, 0.1, 0, "max_samples"),
                                   (2, 1, 0.1, 0, "max_samples"), (2, 24, 0.1, 0, "max_samples"), (3, 32, 0.1, 0, "max_samples"),
                                   (2, 0, 0.1, 0, "max_samples"), (1 << 30, -(1 << 31), 0.1, 0, "max_samples"),
                                   (2, 32, -0.1, 0, "threshold"), (2, 32, NAN, 0, "threshold"), (2, 32, INF, 0, "threshold"),
                                   (2, 32, 0.1, 1, "reserved")):
        fails(lambda: frame(ap=abi.RT_Adaptive_Params(mn, mx, thr, res)), who, word)

    def sized(width, height):
        im = abi.Image()
        im.width, im.height, im.stride, im.components = width, height, max(width, 1), 3
        return im
    for width, height, word in ((0, 4, "invalid"), (8, -1, "invalid"), (1 << 32, 4, "invalid"), (1 << 15, (1 << 13) + 1, "too large")):
        fails(lambda: frame(im=sized(width, height)), who, word)
    fails(lambda: frame(bounces=-1), who, "max_bounces")
    fails(lambda: frame(im=sized(w, h), lin=None, acc=None, cs=None), who, "no output is wanted")
    narrow = sized(w, h)
    narrow.pixels.data = image.pixels.data
    narrow.stride = w - 1
    fails(lambda: frame(im=narrow), who, "stride")
    two = sized(w, h)
    two.pixels.data = image.pixels.data
    two.components = 2
    fails(lambda: frame(im=two), who, "components")

    assert (pixels == 0x55).all() and (linear == 7.0).all() and (accum == 7).all() and (counts == 7).all()
    lib.rt_clear_error()
