#!/usr/bin/env python3
"""Records what the reference's own text computes (oracle/_ref/libref.so, `make -C oracle ref`) into tests/golden/ref/*.npz
for the machines that have no reference tree: tests/test_gpu_reference_pin.py replays them through librt_hip_v1.so.
DATA ONLY.  Per scene (quad, spheres, tower, soup513):

  triangles    the input Triangle records, shader words zeroed (positions, normals, tex_coords)
  material     material index per input triangle
  head         depth, last_row_offset, nodes, slots of the BUILT scene
  nodes        the populated node rows: `node_rows` (index) and `node_bits` (48 uint32 each)
  slot_input   per populated slot, in slot order: `slot_index` and the input triangle that lies there
  frames       per populated slot the 9 words the builder computes: face normal, tangent, bitangent
  rays, t, triangle, uv   about 4096 seeded rays with the hard cases and the reference's closest hit for each

Everything else of a built scene is a copy of its input triangle, so (slot_input, frames, nodes) ARE the built bytes
(tests/_refpin.expand_fixture rebuilds them).  The tree is the reference's scene_init where it builds one; where it stops
at its own assertion (deviation D7: soup513) or builds no node (deviation D3: quad) the tree is the library's and `builder`
says so; the hits are the reference's traversal in every case but depth 0, where there is nothing to traverse and `rays` is
empty.

usage: tools/make_reference_pin_fixtures.py [name ...]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ["quad", "spheres", "tower", "soup513"]
N_RAYS = 4096


def record(name, ref):
    from tests import _refpin as R
    ps = R.PinScene(name, ref)
    try:
        built_by_reference = ps.rs is not None
        sc = ps.rs if built_by_reference else ps.hs.scene
        head, nodes, soa, aos, mat, has_proc = R.scene_bytes(sc, C.addressof(ps.hs.materials))
        tri = ps.tri.copy()
        material = ((tri["shader_data"].astype(np.int64) - C.addressof(ps.hs.materials)) // 80).astype(np.int32)
        tri["shader_data"] = 0
        tri["shader_proc"] = 0
        slot_index = np.flatnonzero(has_proc).astype(np.int32)
        # which input triangle lies in a slot: match on (coordinates, vertex normals, UVs, material), first unused wins
        key_in = np.concatenate([tri["positions"].transpose(0, 2, 1).reshape(len(tri), 9).view(np.uint32),
                                 tri["normals"].reshape(len(tri), 9).view(np.uint32),
                                 tri["tex_coords"].reshape(len(tri), 6).view(np.uint32), material[:, None].view(np.uint32)], axis=1)
        key_slot = np.concatenate([soa.T, aos[:, 3:12], aos[:, 18:24], mat[:, None].view(np.uint32)], axis=1)[slot_index]
        pool = {}
        for i, k in enumerate(map(bytes, key_in)):
            pool.setdefault(k, []).append(i)
        slot_input = np.array([pool[bytes(k)].pop(0) for k in key_slot], np.int32)
        assert sorted(slot_input.tolist()) == list(range(len(tri)))
        node_rows = np.flatnonzero(np.any(nodes != 0, axis=1)).astype(np.int32)
        out = dict(triangles=tri.view(np.uint8).reshape(len(tri), 112)[:, :96].copy().view(np.uint32),
                   material=material, head=np.array(head, np.int64), node_rows=node_rows, node_bits=nodes[node_rows],
                   slot_index=slot_index, slot_input=slot_input,
                   frames=np.concatenate([aos[:, 0:3], aos[:, 12:18]], axis=1)[slot_index],
                   builder=np.array("reference" if built_by_reference else "library"))
        n = N_RAYS if head[2] else 0
        rays = R.seeded_rays(sc, n, 31) if n else np.zeros((0, 6), np.float32)
        t, tri_hit, uv = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
        if n:
            assert ref.ref_trace_rays(C.byref(sc), n, rays.ctypes.data, t.ctypes.data, tri_hit.ctypes.data, uv.ctypes.data) == 0
        out.update(rays=rays.view(np.uint32), t=t.view(np.uint32), triangle=tri_hit, uv=R.plus_zero(uv).view(np.uint32))
        return out
    finally:
        ps.free()


def main():
    from tests import _refpin as R
    if R.reference_state() != "ready":
        sys.exit("oracle/_ref/libref.so is not built: `make -C oracle ref` needs the reference tree")
    ref = R.load_ref()
    os.makedirs(R.FIXTURE_DIR, exist_ok=True)
    for name in sys.argv[1:] or NAMES:
        out = record(name, ref)
        path = os.path.join(R.FIXTURE_DIR, name + ".npz")
        np.savez_compressed(path, **out)
        hits = int((out["triangle"] >= 0).sum())
        print(f"{name}: {os.path.getsize(path)} bytes, built by {out['builder']}, head {out['head'].tolist()}, {hits} hits of {len(out['t'])} rays")


if __name__ == "__main__":
    main()
