"""scene_refit / rt_scene_slot_map (include/rt_scene.h, csrc/rt_scene_refit.c): the BVH of a deformed mesh refitted in place on the
host.  No GPU: the library loads without one."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _refit
from tests._refit import BUILDERS, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.float32(0.0001)


def _lib():
    import raytracing_c_amd as rt
    return rt.lib


def _slot_map(hs, tri):
    from raytracing_c_amd import ctypes_abi as abi
    out = np.full(len(tri), -7, np.int32)
    rc = _lib().rt_scene_slot_map(C.byref(hs.scene), abi.Triangle_Slice(tri.ctypes.data, len(tri)), out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_tris", SHAPES)
def test_slot_map_is_a_bijection_onto_the_populated_slots(n_tris, builder):
    sp = _refit.soup(n_tris)
    hs = sp.build(builder)
    tri = hs.source_triangles
    rc, smap = _slot_map(hs, tri)
    assert rc == n_tris
    coords, aos, populated = _refit.slot_views(hs)
    assert np.array_equal(np.sort(smap), np.flatnonzero(populated))
    assert np.array_equal(smap, hs.slot_map())
    # every slot holds its source's bytes: positions (x0 x1 x2 y0 ... per slot), vertex normals, uvs, Shader
    want = tri["positions"].transpose(0, 2, 1).reshape(n_tris, 9)
    assert np.array_equal(coords[smap].view(np.uint32), want.view(np.uint32))
    assert aos[smap, 12:48].tobytes() == tri["normals"].tobytes()
    assert aos[smap, 72:96].tobytes() == tri["tex_coords"].tobytes()
    assert aos[smap, 96:104].tobytes() == tri["shader_data"].tobytes()
    # byte-identical duplicates: the k-th in source order has the k-th matching slot in slot order
    if n_tris >= 8:
        groups = {}
        for i in range(n_tris):
            groups.setdefault(tri[i].tobytes(), []).append(i)
        dups = [g for g in groups.values() if len(g) > 1]
        assert len(dups) >= sp.n_duplicates >= 2 and (n_tris < 64 or any(len(g) == 3 for g in dups))
        for g in dups:
            assert list(smap[g]) == sorted(smap[g])
    # one triangle altered: it has no slot of its own
    other = tri.copy()
    other["positions"][n_tris // 2, 1, 2] += np.float32(0.25)
    rc, out = _slot_map(hs, other)
    assert rc == -1 and (out == -7).all()
    rc, out = _slot_map(hs, tri[:-1].copy()) if n_tris > 1 else (-1, np.full(0, -7, np.int32))
    assert rc == -1 and (out == -7).all()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_tris", SHAPES)
def test_refit_with_unmoved_triangles_is_the_identity(n_tris, builder):
    hs = _refit.soup(n_tris).build(builder)
    before = _refit.scene_bytes(hs), _refit.raw_bytes(hs)
    hs.refit(device="cpu")
    assert (_refit.scene_bytes(hs), _refit.raw_bytes(hs)) == before


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_tris", SHAPES)
def test_refit_of_normals_and_uvs_equals_a_rebuild(n_tris, builder):
    """The positions decide the sort, so a rebuild of a source with other normals and uvs has the same slots: same topology by
    construction, and the refitted scene must be the rebuilt one byte for byte.  The byte-identical copies stay byte-identical
    here: which of them a builder puts in which slot is not the order rt_scene_slot_map gives them (the k-th copy to the k-th
    slot; the split's stack reverses halves), and neither order can be told from the other while the copies are equal."""
    sp = _refit.soup(n_tris)
    _, N, UV = sp.moved(seed=5)
    UV[0] = [[0.25, 0.5], [0.25 + 0.005, 0.5], [0.25, 0.5 + 0.005]]          # |du1 dv2 - du2 dv1| = 2.5e-5 < 1e-4
    sp.copy_duplicates(N), sp.copy_duplicates(UV)
    assert abs(float(np.float32(UV[0, 1, 0] - UV[0, 0, 0]) * np.float32(UV[0, 2, 1] - UV[0, 0, 1]))) < 1e-4
    assert (sp.P[sp.zero_area, 0] == sp.P[sp.zero_area, 1]).all() and (sp.P[sp.zero_area, 0] == sp.P[sp.zero_area, 2]).all()
    hs = sp.build(builder)
    hs.refit(normals=N, uvs=UV, device="cpu")
    rebuilt = sp.build(builder, N=N, UV=UV)
    assert np.array_equal(hs.slot_map(), rebuilt.slot_map())
    assert _refit.scene_bytes(hs) == _refit.scene_bytes(rebuilt)


def _expected_boxes(coords, populated, depth):
    """numpy float32 restatement: per level, per (node, child): min / max over the populated slots of the child's subtree of
    min3 - EPSILON / max3 + EPSILON, zero where the subtree holds nothing.  (n_nodes, 6, 8)."""
    n = len(coords)
    xyz = coords.reshape(n, 3, 3)                                             # [slot][axis][vertex]
    lo = (xyz.min(axis=2) - EPS).astype(np.float32)
    hi = (xyz.max(axis=2) + EPS).astype(np.float32)
    lo = np.where(populated[:, None], lo, np.float32(np.inf))
    hi = np.where(populated[:, None], hi, np.float32(-np.inf))
    out = []
    for level in range(depth):
        children = 8 ** (level + 1)
        any_ = populated.reshape(children, -1).any(axis=1)
        l = lo.reshape(children, -1, 3).min(axis=1)
        h = hi.reshape(children, -1, 3).max(axis=1)
        l = np.where(any_[:, None], l, np.float32(0)).reshape(-1, 8, 3)
        h = np.where(any_[:, None], h, np.float32(0)).reshape(-1, 8, 3)
        out.append(np.concatenate([l.transpose(0, 2, 1), h.transpose(0, 2, 1)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 6, 8), np.float32)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_tris", SHAPES)
def test_refit_of_moved_positions(n_tris, builder):
    from raytracing_c_amd import ctypes_abi as abi
    lib = _lib()
    sp = _refit.soup(n_tris)
    hs = sp.build(builder)
    original = _refit.scene_bytes(hs), _refit.raw_bytes(hs)
    smap = hs.slot_map().copy()
    P, N, UV = sp.moved()
    assert 0.02 < np.abs(P - sp.P).mean() < 0.08
    hs.refit(positions=P, normals=N, uvs=UV, device="cpu")
    coords, aos, populated = _refit.slot_views(hs)
    assert np.array_equal(np.flatnonzero(populated), np.sort(smap))
    # every child box
    want = _expected_boxes(coords, populated, hs.depth)
    got = hs.nodes_array()
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.isinf(got).any()
    # every populated slot: coordinates and AoS record are those of a depth-0 scene_init of the same (up to 8) source triangles,
    # which inserts in input order -- the builder's own triangles_insert
    tri = hs.source_triangles
    for i0 in range(0, n_tris, 8):
        part = np.ascontiguousarray(tri[i0:i0 + 8])
        sc = abi.Scene()
        lib.scene_init(C.byref(sc), abi.Triangle_Slice(part.ctypes.data, len(part)), abi.Allocator(None, None))
        assert int(sc.bvh.depth) == 0 and int(sc.triangles.len) == 8
        raw = np.frombuffer(C.string_at(C.cast(sc.triangles.x[0], C.c_void_p), 8 * 148), np.uint8).copy()
        lib.rt_scene_free(C.byref(sc))
        k = len(part)
        slots = smap[i0:i0 + k]
        assert np.array_equal(coords[slots].view(np.uint32), raw[:8 * 36].view(np.uint32).reshape(9, 8).T[:k])
        assert np.array_equal(aos[slots], raw[8 * 36:].reshape(8, 112)[:k])
    # padding slots stay all zero
    assert not coords[~populated].any() and not aos[~populated].any()
    # and back
    hs.refit(positions=sp.P, normals=sp.N, uvs=sp.UV, device="cpu")
    assert (_refit.scene_bytes(hs), _refit.raw_bytes(hs)) == original


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_tris", [9, 65, 513])
def test_refit_rejects_what_is_not_the_same_topology(n_tris, builder):
    import raytracing_c_amd as rt
    sp = _refit.soup(n_tris)
    hs = sp.build(builder)
    before = _refit.raw_bytes(hs)
    smap = hs.slot_map()
    P, N, UV = sp.moved()
    tri = hs.source_triangles.copy()
    tri["positions"], tri["normals"], tri["tex_coords"] = P, N, UV

    def rejected(t, m, what):
        rt.lib.rt_clear_error()
        assert _refit.call_refit(hs, t, m) == -1, what
        assert what in rt.last_error(), rt.last_error()
        assert _refit.raw_bytes(hs) == before, what

    repeated = smap.copy()
    same_material = np.flatnonzero(tri["shader_data"] == tri["shader_data"][3])
    repeated[same_material[same_material != 3][-1]] = repeated[3]                            # (same Shader: the one thing wrong is the repetition)
    rejected(tri, repeated, "twice")
    for bad in (-1, hs.n_slots, 2 ** 31 - 1):
        out_of_range = smap.copy()
        out_of_range[n_tris - 1] = bad
        rejected(tri, out_of_range, "outside")
    coords, aos, populated = _refit.slot_views(hs)
    padding = smap.copy()
    padding[0] = np.flatnonzero(~populated)[0]
    rejected(tri, padding, "padding")
    rejected(tri[:-1].copy(), smap[:-1].copy(), "src.len")
    rejected(np.concatenate([tri, tri[:1]]), np.concatenate([smap, smap[:1]]), "src.len")
    shader = tri.copy()
    others = np.unique(tri["shader_data"])
    shader["shader_data"][2] = others[others != tri["shader_data"][2]][0]
    rejected(shader, smap, "Shader")
    assert _refit.call_refit(hs, tri, smap) == 0                        # the same call with nothing wrong goes through
    assert _refit.raw_bytes(hs) != before


def test_refit_of_a_loaded_scene_file():
    """rt_scene_slot_map changes no builder: a Scene that aliases a .scene file's bytes is mapped and refitted like any other."""
    from raytracing_c_amd import ctypes_abi as abi
    lib = _lib()
    sp = _refit.soup(65)
    hs = sp.build("sah")
    size = lib.scene_file_size(C.byref(hs.scene))
    buf = np.zeros(size + 32, np.uint8)
    off = (-buf.ctypes.data) % 32
    assert lib.scene_save_bytes(C.byref(hs.scene), buf.ctypes.data + off, size) == size
    loaded = abi.Scene()
    assert lib.scene_load_bytes(abi.Byte_Slice(buf.ctypes.data + off, size), C.byref(loaded))
    tri = hs.source_triangles.copy()
    smap = np.zeros(len(tri), np.int32)
    assert lib.rt_scene_slot_map(C.byref(loaded), abi.Triangle_Slice(tri.ctypes.data, len(tri)), smap.ctypes.data) == len(tri)
    assert np.array_equal(smap, hs.slot_map())
    P, N, UV = sp.moved()
    tri["positions"], tri["normals"], tri["tex_coords"] = P, N, UV
    assert lib.scene_refit(C.byref(loaded), abi.Triangle_Slice(tri.ctypes.data, len(tri)), smap.ctypes.data) == 0
    hs.refit(positions=P, normals=N, uvs=UV, device="cpu")
    n_nodes, n = hs.n_nodes, hs.n_slots
    assert bytes(buf[off + 96:off + 96 + n_nodes * 192 + n * 148]) == b"".join(_refit.raw_bytes(hs))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_refit_host_code_is_clean_under_sanitizers(tmp_path):
    """AddressSanitizer + UndefinedBehaviorSanitizer over build -> map -> refit -> refit back -> the rejections, as a stand-alone
    program (tests/c/refit_host.c) linked with the two host units alone."""
    exe = str(tmp_path / "refit_host")
    csrc = os.path.join(ROOT, "raytracing_c_amd", "csrc")
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "c", "refit_host.c"), os.path.join(csrc, "rt_scene_build.c"),
           os.path.join(csrc, "rt_scene_refit.c"), "-o", exe, "-lpthread", "-lm"]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 8, r.stdout                        # n = 1, 9, 65, 513 with both builders
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_refit_on_the_gpu_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    sp = _refit.soup(9)
    hs = sp.build("reference")
    before = _refit.raw_bytes(hs), hs.source_triangles.copy()
    with pytest.raises(RuntimeError, match="scene_refit_gpu"):         # "... no HIP device available ...": there is no CPU fallback
        hs.refit(positions=sp.moved()[0], device="gpu")
    assert _refit.raw_bytes(hs) == before[0] and hs.source_triangles.tobytes() == before[1].tobytes()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n_tris", [9, 65, 513, 4097])
def test_refit_equals_a_rebuild_when_identical_copies_stop_being_identical(n_tris, builder):
    """The changed source as it is: normals and uvs of every triangle change on their own, so byte-identical copies stop being
    identical.  Their positions stay equal, so a rebuild may put them into each other's slots (the split's stack reverses halves;
    rt_scene_slot_map pairs the k-th copy with the k-th slot): the rebuilt scene has the same nodes, the same populated slots, and
    every source triangle's slot holds the same bytes in both scenes -- through each scene's own map."""
    sp = _refit.soup(n_tris)
    _, N, UV = sp.moved(seed=6)
    assert any((N[dst] != N[src]).any() for dst, src in sp.copies)
    hs = sp.build(builder)
    hs.refit(normals=N, uvs=UV, device="cpu")
    rebuilt = sp.build(builder, N=N, UV=UV)
    (head_a, nodes_a, _, _, pop_a), (head_b, nodes_b, _, _, pop_b) = _refit.scene_bytes(hs), _refit.scene_bytes(rebuilt)
    assert head_a == head_b and nodes_a == nodes_b and pop_a == pop_b
    map_a, map_b = hs.slot_map(), rebuilt.slot_map()
    moved = np.flatnonzero(map_a != map_b)
    copies = {i for pair in sp.copies for i in pair}
    assert set(moved.tolist()) <= copies                                # only copies can have changed places
    coords_a, aos_a, _ = _refit.slot_views(hs)
    coords_b, aos_b, _ = _refit.slot_views(rebuilt)
    assert np.array_equal(coords_a[map_a].view(np.uint32), coords_b[map_b].view(np.uint32))
    assert np.array_equal(aos_a[map_a][:, :96], aos_b[map_b][:, :96])     # (the Shader holds each HostScene's own pointers)
    base_a, base_b = C.addressof(hs.materials), C.addressof(rebuilt.materials)
    assert np.array_equal(aos_a[map_a][:, 96:104].copy().view(np.uint64) - base_a, aos_b[map_b][:, 96:104].copy().view(np.uint64) - base_b)
