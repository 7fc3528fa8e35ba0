"""The input lists of tests/_shade_inputs.py through the ORACLE ALONE: every class of input that tests/test_gpu_shade.py is meant
to carry to the device is populated, so that test cannot pass vacuously.  The counts are conditions on the generator, not
measurements: a class the oracle does not reach is a reason to change the generator."""
import numpy as np
import pytest

from tests import _shade_inputs as S


def test_shade_level_classes_are_populated(oracle):
    classes = S.shade_classes()
    counts = {k: int(m.sum()) for k, m in classes.items()}
    print(counts)
    for name, least in S.SHADE_CLASS_MINIMUM.items():
        assert counts[name] >= least, (name, counts[name], least)
    sc = S.shade_scene()
    for v in range(len(sc.variant_slots)):                  # every device material
        assert counts[f"variant {v}"] >= 100, (v, counts[f"variant {v}"])
    ref = S.shade_reference()
    assert not (ref["draws"] == -1).any(), "an item drew a number of random numbers that is neither 0, 3 nor 5"
    assert np.all(ref["draws"][classes["debug material"]] == 0) and np.all(ref["terminate"][classes["debug material"]] == 1)


def test_shade_scene_is_what_the_lists_assume(oracle):
    sc = S.shade_scene()
    hs = sc.hs
    assert [(int(i.width), int(i.height)) for i in hs.images] == S.IMAGE_SIZES
    assert (int(hs.background_image.width), int(hs.background_image.height)) == S.BACKGROUND_SIZE
    assert len(sc.variant_slots) == 16 and int(sc.variant_debug.sum()) == 2 and int((sc.slot_variant >= 0).sum()) == 24
    combos = {tuple(t is not None for t in (m.texture_albedo, m.texture_normal, m.texture_metal_roughness, m.texture_emission))
              for m in sc.materials}
    for want in ((False,) * 4, (True,) * 4, (True, False, False, False), (False, True, False, False), (False, False, True, False),
                 (False, False, False, True)):
        assert want in combos, want
    it = S.shade_items()
    assert 8000 <= len(it["tri"]) <= 20000
    assert np.all(sc.slot_variant[it["tri"]] == it["variant"])
    uv = it["inp"][:, 12:14]
    assert np.all(np.isfinite(uv)) and np.abs(uv).max() <= 2.0 ** 20


def test_brdf_level_classes_are_populated(oracle):
    it, ref = S.brdf_items(), S.brdf_reference()
    assert 8000 <= len(it["seed"]) <= 20000
    d, p = it["in_dir"], it["params"]
    counts = {
        "in_dir == (0, 0, 1)": int(np.sum((d[:, 0] == 0) & (d[:, 1] == 0) & (d[:, 2] == 1))),
        "in_dir.z == 0": int(np.sum(d[:, 2] == 0)),
        "in_dir.z < 0": int(np.sum(d[:, 2] < 0)),
        "metalness 1": int(np.sum(p[:, 1] == 1)),
        "metalness 0": int(np.sum(p[:, 1] == 0)),
        "roughness 0.001": int(np.sum(p[:, 0] == np.float32(0.001))),
        "roughness 1": int(np.sum(p[:, 0] == 1)),
        "diffuse lobe": int(np.sum(ref["draws"] == 5)),
        "specular lobe": int(np.sum(ref["draws"] == 3)),
        "live": int(np.sum(ref["brdf"][:, 3] > 0)),
    }
    print(counts)
    assert counts["in_dir == (0, 0, 1)"] >= 100
    for name in ("in_dir.z == 0", "in_dir.z < 0"):
        assert counts[name] >= 50, (name, counts)
    for name in ("metalness 1", "metalness 0", "roughness 0.001", "roughness 1", "diffuse lobe", "specular lobe", "live"):
        assert counts[name] >= 100, (name, counts)
    for a in (0.0, 0.49, 1.0):
        assert np.sum(p[:, 4] == np.float32(a)) >= 100, a
    assert not (ref["draws"] == -1).any()


def test_background_classes_are_populated(oracle):
    dirs = S.background_dirs()
    assert 8000 <= len(dirs) <= 20000 and np.all(np.isfinite(dirs))
    u, v = S.background_uv(dirs)
    # The +y pole: v = fma(-asin(1), 1 / pi, 0.5) with asin(1) = RN(pi / 2) and RN(1 / pi) is 6.2572632e-09, not 0:
    # the product rounds below one half.  No direction gives less, so THAT value is the pole's "v exactly at 0"; the -y pole
    # gives exactly 1.
    v_top = S.background_uv(np.array([[0, 1, 0]], np.float32))[1][0]
    assert 0 < v_top < 1e-8 and v.min() == v_top and v.max() == 1
    counts = {"u at 0": int(np.sum(np.abs(u) <= 1e-6)), "u at 1": int(np.sum(np.abs(u - 1) <= 1e-6)),
              "u at 0.5": int(np.sum(np.abs(u - 0.5) <= 1e-6)), "v at the +y pole": int(np.sum(v == v_top)), "v == 1": int(np.sum(v == 1))}
    print(counts)
    for name, c in counts.items():
        assert c >= 10, (name, counts)
    assert np.sum(np.abs(dirs[:, 1]) > 1) >= 100                       # rt_asinf clamps
    want = S.background_reference()
    assert np.all(np.isfinite(want)) and len(np.unique(want, axis=0)) > 1000


@pytest.mark.parametrize("width,height", S.FRAME_SIZES, ids=[f"{w}x{h}" for w, h in S.FRAME_SIZES])
def test_primary_ray_lists_cover_the_frame(oracle, width, height):
    calls = S.primary_items(width, height)
    want = S.primary_reference(width, height)
    assert len(calls) == S.CALLS
    pixels = set()
    for (cam, xys), rays in zip(calls, want):
        assert np.all((xys[:, 0] >= 0) & (xys[:, 0] < width) & (xys[:, 1] >= 0) & (xys[:, 1] < height))
        assert set(xys[:, 2].tolist()) == set(S.SAMPLES)
        pixels |= set(map(tuple, xys[:, :2].tolist()))
        assert rays.shape == (len(xys), 6)
        assert np.array_equal(rays[:, 0:3], np.tile(np.array(cam.view_matrix.rows, np.float32)[:3, 3], (len(xys), 1)))
    for corner in ((0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, 0), (0, height // 2)):
        assert corner in pixels
    assert sum(len(x) for _, x in calls) // len(S.SAMPLES) >= 2000
    assert {round(float(c.focal_length), 3) for c, _ in calls} >= {0.0}
    assert len({bytes(c.view_matrix) for c, _ in calls}) == 6
