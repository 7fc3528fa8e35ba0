#!/usr/bin/env python3
"""Worker of tests/test_gpu_lifecycle.py: in its OWN process, with the product library, uses every kind of device state once --
a frame, a view batch, two frames in flight, queries, a feature pass, then a frame and a frame in flight over two rehearsed device
slots, whose worker thread stays parked -- and returns from main.  The parent looks at the exit status and at stderr."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import raytracing_c_amd as rt
    from raytracing_c_amd.configs import load_config
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    hs, _ = load_config("spheres")
    w, h, s, b = 96, 64, 2, 2
    one = rt.render_frame(hs, w, h, s, b)["image"]
    views = rt.render_views(hs, [hs.scene.camera, hs.scene.camera], 32, 32, s, b, seeds=[1, 2])
    assert not np.array_equal(views[0]["image"], views[1]["image"])
    t0, out0, keep0 = rt.frame_begin(hs, w, h, s, b)
    t1, out1, keep1 = rt.frame_begin(hs, w, h, s, b)
    rt.frame_end(t0)
    rt.frame_end(t1)
    assert np.array_equal(out0, one) and np.array_equal(out1, one)
    rays = np.zeros((64, 6), np.float32)
    rays[:, 2], rays[:, 5] = 5.0, -1.0
    rt.closest_hits(hs, rays)
    rt.occluded(hs, rays)
    rt.render_features(hs, 8, 8, s, b)
    assert rt.lib.rt_set_devices(2, 1) == 0, rt.last_error()
    two = rt.render_frame(hs, w, h, s, b)["image"]                 # spread over two slots of this GPU
    t, out, keep = rt.frame_begin(hs, w, h, s, b)
    rt.frame_end(t)
    assert np.array_equal(two, one) and np.array_equal(out, one)
    rt.lib.rt_scene_invalidate(C.byref(hs.scene))
    assert np.array_equal(rt.render_frame(hs, w, h, s, b)["image"], one)      # (copies and workspaces stay: nothing is freed at exit)
    print("lifecycle ok", flush=True)


if __name__ == "__main__":
    main()
