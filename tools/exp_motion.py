#!/usr/bin/env python3
"""GPU experiment: what the motion channel of a deforming mesh costs, for config #3's shape -- helmet, 1920x1080, 16 samples, 8
bounces.  The helmet's geometry is kept, then refitted on the GPU to a per-vertex displacement of 0.01; on that device copy, device
level, buffers resident, HIP events on one stream:
  * the feature pass (rt_render_accumulate_features + rt_resolve_features) against the motion feature pass
    (rt_render_accumulate_features_motion + rt_resolve_features + rt_resolve_motion), clear included;
  * the accumulation (rt_temporal_accumulate) against rt_temporal_accumulate_motion, over those planes and a history of one frame;
  * rt_device_scene_keep_geometry alone (one device-to-device copy of the leaf tiles).
Everything is warmed up, then each pair is timed alternately, one launch each per step: median and min - max of `steps` launches.
Uses the diagnostic library, which names the cached copy a refit deforms (rt_diag_cached_scene); its kernels are the product's
objects.

    python tools/exp_motion.py [out.md] [steps]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                      # noqa: E402
import torch                                            # noqa: E402
import raytracing_c_amd as rt                           # noqa: E402
from raytracing_c_amd import ctypes_abi as abi          # noqa: E402
from raytracing_c_amd.configs import load_config        # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "motion_table.md")
steps = int(args[1]) if len(args) > 1 else 20
W, H, S, B = 1920, 1080, 16, 8
lib = rt.diag

assert lib.rt_init(0) == 0, rt.last_error(lib)
hs, _ = load_config("helmet")
scene = C.byref(hs.scene)
assert lib.rt_scene_keep_geometry(scene) == 0, rt.last_error(lib)
smap = hs.slot_map()
tri = hs.source_triangles.copy()
tri["positions"] += (np.random.default_rng(1).normal(size=tri["positions"].shape) * 0.01).astype(np.float32)
assert lib.scene_refit_gpu(scene, abi.Triangle_Slice(tri.ctypes.data, len(tri)), smap.ctypes.data) == 0, rt.last_error(lib)
d = lib.rt_diag_cached_scene(scene)
assert d and lib.rt_scene_has_kept_geometry(scene) == 1
assert lib.rt_set_camera(d, C.byref(hs.scene.camera)) == 0
p = abi.RT_Render_Params(width=W, height=H, samples=S, max_bounces=B, seed=0x1234ABCD, world=1)
dev = "cuda"
sums = torch.zeros((H, W, 10), dtype=torch.int64, device=dev)
msums = torch.zeros((H, W, 3), dtype=torch.int64, device=dev)
planes = [torch.zeros((H, W) if k == 0 else (H, W, 3), dtype=torch.float32, device=dev) for k in range(4)]
motion = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
color = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
hist = [torch.zeros((3, H, W, 4), dtype=torch.float32, device=dev) for _ in range(2)]
out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
stream = torch.cuda.current_stream()
sp = stream.cuda_stream
tp = abi.RT_Temporal_Params(alpha=0.05, max_history=64, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
cam = hs.scene.camera


def feature_pass():
    sums.zero_()
    assert lib.rt_render_accumulate_features(d, C.byref(p), sums.data_ptr(), sp) == 0, rt.last_error(lib)
    assert lib.rt_resolve_features(C.byref(p), sums.data_ptr(), *[t.data_ptr() for t in planes], sp) == 0, rt.last_error(lib)


def motion_feature_pass():
    sums.zero_()
    msums.zero_()
    assert lib.rt_render_accumulate_features_motion(d, C.byref(p), sums.data_ptr(), msums.data_ptr(), sp) == 0, rt.last_error(lib)
    assert lib.rt_resolve_features(C.byref(p), sums.data_ptr(), *[t.data_ptr() for t in planes], sp) == 0, rt.last_error(lib)
    assert lib.rt_resolve_motion(C.byref(p), msums.data_ptr(), motion.data_ptr(), sp) == 0, rt.last_error(lib)


def frame_args():
    return [color.data_ptr()] + [t.data_ptr() for t in planes]


def accumulation():
    assert lib.rt_temporal_accumulate(W, H, C.byref(tp), C.byref(cam), C.byref(cam), *frame_args(), hist[0].data_ptr(), hist[1].data_ptr(),
                                      out.data_ptr(), None, None, sp) == 0, rt.last_error(lib)


def motion_accumulation():
    assert lib.rt_temporal_accumulate_motion(W, H, C.byref(tp), C.byref(cam), C.byref(cam), *frame_args(), hist[0].data_ptr(),
                                             hist[1].data_ptr(), out.data_ptr(), None, None, None, None, None, None, sp,
                                             motion.data_ptr()) == 0, rt.last_error(lib)


def keep():
    assert lib.rt_device_scene_keep_geometry(d, sp) == 0, rt.last_error(lib)


motion_feature_pass()                                   # the planes and the motion the accumulations read
assert lib.rt_temporal_accumulate(W, H, C.byref(tp), C.byref(cam), None, *frame_args(), None, hist[0].data_ptr(), None, None, None,
                                  sp) == 0, rt.last_error(lib)
torch.cuda.synchronize()
moved = float((motion != 0).any(dim=2).float().mean())
pairs = [[("feature pass", feature_pass), ("motion feature pass", motion_feature_pass)],
         [("accumulation", accumulation), ("motion accumulation", motion_accumulation)]]
ms = {}
for pair in pairs:
    for _, fn in pair:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for name, _ in pair:
        ms[name] = []
    for _ in range(steps):
        for name, fn in pair:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
# (the keep after the timed passes: it replaces the snapshot the motion was measured against)
for _ in range(3):
    keep()
torch.cuda.synchronize()
ms["rt_device_scene_keep_geometry"] = []
for _ in range(steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    keep()
    e1.record(stream)
    e1.synchronize()
    ms["rt_device_scene_keep_geometry"].append(e0.elapsed_time(e1))
lib.rt_scene_invalidate(scene)

med = {k: statistics.median(v) for k, v in ms.items()}
lines = [f"helmet {W}x{H}, {S} spp, {B} bounces, {steps} launches each, pairs alternating; {hs.n_slots} triangle slots; "
         f"pixels with non-zero motion: {moved:.3f}", "", "| what | median ms | min - max ms |", "|---|---|---|"]
for name in ms:
    lines.append(f"| {name} | {med[name]:.3f} | {min(ms[name]):.3f} - {max(ms[name]):.3f} |")
lines.append(f"\nmotion feature pass / feature pass = {med['motion feature pass'] / med['feature pass']:.3f}; "
             f"motion accumulation / accumulation = {med['motion accumulation'] / med['accumulation']:.3f}")
print("\n".join(lines), flush=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
