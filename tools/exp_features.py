#!/usr/bin/env python3
"""GPU experiment: the first-hit feature pass (rt_render_accumulate_features + rt_resolve_features: coverage, albedo, normal,
position) against the only other route to a normal buffer, a frame of the same scene with every material on debug_shader_proc
(rt_render_accumulate + rt_resolve), for config #3's shape -- helmet, 1920x1080 -- at 16 samples and 8 bounces.  Both trace the
same camera rays.  Device level, buffers resident, HIP events around clear + kernel(s) + resolve on one stream; both are warmed
up, then timed alternately, one launch each per step: median and min - max of `steps` launches.

    python tools/exp_features.py [out.md] [steps] [--profile]     # --profile: 5 launches each and no timing, for a
                                                                  # rocprofv3 --kernel-trace --stats run of its own"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                            # noqa: E402
import raytracing_c_amd as rt                           # noqa: E402
from raytracing_c_amd import ctypes_abi as abi          # noqa: E402
from raytracing_c_amd.configs import load_config        # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
profile = "--profile" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "features_table.md")
steps = 5 if profile else (int(args[1]) if len(args) > 1 else 20)
W, H, S, B = 1920, 1080, 16, 8

assert rt.lib.rt_init(0) == 0, rt.last_error()
hs, _ = load_config("helmet")
hs_debug, _ = load_config("helmet", shader="debug")
d = rt.lib.rt_scene_upload(C.byref(hs.scene))
d_debug = rt.lib.rt_scene_upload(C.byref(hs_debug.scene))
assert d and d_debug, rt.last_error()
p = abi.RT_Render_Params(width=W, height=H, samples=S, max_bounces=B, seed=0x1234ABCD, world=1)
sums = torch.zeros((H, W, 10), dtype=torch.int64, device="cuda")
planes = [torch.zeros((H, W) if k == 0 else (H, W, 3), dtype=torch.float32, device="cuda") for k in range(4)]
accum = torch.zeros((H, W, 3), dtype=torch.int64, device="cuda")
linear = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream


def feature_pass():
    sums.zero_()
    assert rt.lib.rt_render_accumulate_features(d, C.byref(p), sums.data_ptr(), sp) == 0, rt.last_error()
    assert rt.lib.rt_resolve_features(C.byref(p), sums.data_ptr(), *[t.data_ptr() for t in planes], sp) == 0, rt.last_error()


def debug_frame():
    accum.zero_()
    assert rt.lib.rt_render_accumulate(d_debug, C.byref(p), accum.data_ptr(), sp) == 0, rt.last_error()
    assert rt.lib.rt_resolve(C.byref(p), accum.data_ptr(), None, None, linear.data_ptr(), sp) == 0, rt.last_error()


cases = [("feature pass (4 buffers)", feature_pass), ("debug frame (normal only)", debug_frame)]
for _, fn in cases:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
ms = {name: [] for name, _ in cases}
for _ in range(steps):
    for name, fn in cases:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms[name].append(e0.elapsed_time(e1))
# the two routes give the same normal wherever every sample of the pixel has a feature hit (elsewhere the frame adds the background)
full = planes[0] == 1.0
same = bool(full.any()) and torch.equal(planes[2][full], linear[full])
rt.lib.rt_scene_release(d)
rt.lib.rt_scene_release(d_debug)
if not profile:
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"helmet {W}x{H}, {S} spp, {B} bounces, {steps} launches each, alternating; normals of fully covered pixels equal: {same}", "",
             "| route | median ms | min - max ms |", "|---|---|---|"]
    for name, _ in cases:
        lines.append(f"| {name} | {med[name]:.3f} | {min(ms[name]):.3f} - {max(ms[name]):.3f} |")
    a, b = (med[name] for name, _ in cases)
    lines.append(f"\nfeature pass / debug frame = {a / b:.3f}")
    print("\n".join(lines), flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
