"""rt_materials_share_taps (include/rt_hip.h): may a shade block compute one set of bilinear taps for a material's four textures?
The predicate on crafted material tables; it touches no device, so it runs where the library loads."""
import numpy as np

from tests._taps_scene import material_table

A, B = (8, 8, 2), (5, 3, 2)


def _share(table):
    import raytracing_c_amd as rt
    t = np.ascontiguousarray(table, np.int32)
    return rt.lib.rt_materials_share_taps(t.ctypes.data if t.size else None, len(t))


def test_all_equal():
    assert _share(material_table([[A, A, A, A], [B, B, B, B], [None, A, None, A]])) == 1


def test_one_field_off():
    assert _share(material_table([[A, A, A, A], [B, B, B, (5, 3, 3)]])) == 0, "stride"
    assert _share(material_table([[A, (4, 8, 2), A, A]])) == 0, "width"
    assert _share(material_table([[A, A, (8, 4, 2), A]])) == 0, "height"
    assert _share(material_table([[A, A, A, A], [A, A, A, A], [None, None, A, (8, 8, 1)]])) == 0, "the last material, its last two slots"


def test_offsets_do_not_count():
    t = material_table([[A, A, A, A]])
    assert len({int(t[0, 20 + 4 * k]) for k in range(4)}) == 4 and _share(t) == 1


def test_empty_slots():
    assert _share(material_table([[None] * 4, [A, None, None, None], [None, None, None, B]])) == 1
    t = material_table([[A, None, None, B]])
    assert _share(t) == 0
    t[0, 15] = -1                                    # the emission slot named no more: its stale descriptor is not read
    assert _share(t) == 1
    t[0, 15], t[0, 12] = 3, -7                       # ... and any negative index is "none"
    assert _share(t) == 1


def test_zero_materials():
    assert _share(np.zeros((0, 36), np.int32)) == 1
    import raytracing_c_amd as rt
    assert rt.lib.rt_materials_share_taps(None, 0) == 1 and rt.lib.rt_materials_share_taps(None, 5) == 1


def test_a_texture_named_twice():
    t = material_table([[A, A, None, None]])
    t[0, 13], t[0, 24:28] = t[0, 12], t[0, 20:24]    # normal = the albedo's texture: same index, same descriptor, same offset
    assert _share(t) == 1
    t = material_table([[A, B, B, None]])            # the same texture twice beside one of another size
    t[0, 14], t[0, 28:32] = t[0, 13], t[0, 24:28]
    assert _share(t) == 0
