#!/usr/bin/env python3
"""Worker of tests/test_gpu_reference_pin.py: runs in its OWN process with RT_LIB_PATH = librt_hip_v1.so (the product under
numeric contract v1) and replays the recorded reference results of tests/golden/ref/*.npz.  argv: fixture paths; stdout: one
JSON line per fixture."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import raytracing_c_amd as rt
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.query import closest_hits_device
    from tests import _refpin as R
    assert os.path.basename(rt.native.LIB_PATH) == "librt_hip_v1.so", rt.native.LIB_PATH
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    assert rt.lib.rt_math_contract() == 1
    proc = rt.native.symbol_address("disney_shader_proc")
    for path in sys.argv[1:]:
        out = {"fixture": os.path.basename(path), "error": None, "builder": None}
        try:
            g = dict(np.load(path))
            out["builder"] = str(g["builder"])
            materials = (abi.PBR_Shader_Data * (int(g["material"].max()) + 1))()
            for m in materials:
                m.base_color, m.roughness = abi.Vec3(0.8, 0.8, 0.8), 0.5
            base = C.addressof(materials)
            tri = R.fixture_triangles(g, base, proc)
            want = R.expand_fixture(g)

            # 1. the GPU builder on the recorded triangles -> the recorded bytes
            built = abi.Scene()
            if rt.lib.scene_init_gpu(C.byref(built), abi.Triangle_Slice(tri.ctypes.data, len(tri)), abi.Allocator(None, None)) != 0:
                raise RuntimeError("scene_init_gpu: " + rt.last_error())
            got = R.scene_bytes(built, base)
            out["head_equal"] = list(got[0]) == list(want[0])
            out["build_equal"] = [bool(np.array_equal(a, b)) for a, b in zip(got[1:], want[1:])]
            rt.lib.rt_scene_free(C.byref(built))

            # 2. rt_query_closest over the RECORDED tree -> the recorded hits
            n = len(g["t"])
            out["rays"] = n
            if n:
                sc = abi.Scene()
                assert rt.lib.rt_scene_alloc(C.byref(sc), len(tri), abi.Allocator(None, None))
                head, nodes, soa, aos, mat, populated = want
                assert (int(sc.bvh.depth), int(sc.bvh.last_row_offset), int(sc.bvh.nodes.len), int(sc.triangles.len)) == head
                np.ctypeslib.as_array(C.cast(sc.bvh.nodes.data, C.POINTER(C.c_uint32)), nodes.shape)[:] = nodes
                np.ctypeslib.as_array(C.cast(sc.triangles.x[0], C.POINTER(C.c_uint32)), soa.shape)[:] = soa
                rec = np.ctypeslib.as_array(C.cast(sc.triangles.aos, C.POINTER(C.c_uint32)), (head[3], 28))
                rec[:, :24] = aos
                ptr = np.zeros((head[3], 2), np.uint64)
                ptr[populated, 0] = base + mat[populated].astype(np.uint64) * 80
                ptr[populated, 1] = proc
                rec[:, 24:28] = ptr.view(np.uint32)
                sc.background.proc = rt.native.symbol_address("sample_background")
                bg = np.zeros((2, 4, 3), np.uint8)
                img = abi.Image()
                img.components, img.pixel_type, img.width, img.stride, img.height = 3, 0, 4, 4, 2
                img.pixels.data, img.pixels.len = bg.ctypes.data, bg.size
                sc.background.data = C.addressof(img)
                d = rt.lib.rt_scene_upload(C.byref(sc))
                if not d:
                    raise RuntimeError("rt_scene_upload: " + rt.last_error())
                rays = torch.from_numpy(g["rays"].view(np.float32).copy()).cuda()
                hits = closest_hits_device(d, rays)
                torch.cuda.synchronize()
                h = hits.cpu().numpy()
                t, tri_hit = h[:, 0].copy().view(np.uint32), h[:, 1].copy().view(np.int32)
                uv = R.plus_zero(h[:, 2:4]).view(np.uint32)
                out["t_equal"] = bool(np.array_equal(t, g["t"]))
                out["triangle_equal"] = bool(np.array_equal(tri_hit, g["triangle"]))
                out["uv_equal"] = bool(np.array_equal(uv, g["uv"]))
                out["mismatches"] = int(((t != g["t"]) | (tri_hit != g["triangle"]) | (uv != g["uv"]).any(axis=1)).sum())
                out["hits"] = int((g["triangle"] >= 0).sum())
                rt.lib.rt_scene_release(d)
                rt.lib.rt_scene_free(C.byref(sc))
        except Exception as e:           # noqa: BLE001 -- reported to the parent, which fails the test
            out["error"] = repr(e)
        print(json.dumps(out), flush=True)
        if out["error"] is not None:     # nothing more is started on the GPU after a failure; the parent fails the missing fixtures
            break


if __name__ == "__main__":
    main()
