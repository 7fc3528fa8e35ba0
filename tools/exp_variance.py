#!/usr/bin/env python3
"""GPU experiment: the post stages of rt_render_svgf -- the moments pass (rt_temporal_moments_kernel), the variance launch
(rt_variance_kernel) and the variance-guided filter (rt_variance_pack_kernel + rt_variance_filter_kernel per iteration) -- beside the
stages of rt_render_temporal with the guided filter at the same iteration count (rt_temporal_kernel; rt_guided_pack_kernel +
rt_guided_filter_kernel), on config #3's shape: helmet, 1920x1080, 16 spp, 8 bounces.  Device level, buffers resident, HIP events
on one stream around BATCH calls back to back, divided by BATCH (a single launch is short beside what an event pair resolves);
5 warm-up rounds, then `steps` timed rounds with the stages interleaved; median and min - max.

Two histories of the same view under equal cameras: SHORT (one frame accumulated: every surface pixel has len' = 2 < 4 and takes the
7 x 7 estimate) and LONG (six frames: len' = 7 everywhere, so no workgroup stages a halo).  The variance launch is timed alone
as well: the moments call with a variance wanted minus the same call without.

    python tools/exp_variance.py [out.md] [steps]"""
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
from raytracing_c_amd.guided import default_sigma_position   # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "variance_table.md")
steps = int(args[1]) if len(args) > 1 else 20
W, H, S, B = 1920, 1080, 16, 8
BATCH = 20
ITERATIONS = 4

assert rt.lib.rt_init(0) == 0, rt.last_error()
lib = rt.lib
hs, _ = load_config("helmet")
cam = abi.Camera()
C.memmove(C.byref(cam), C.byref(hs.scene.camera), C.sizeof(abi.Camera))
frames = [rt.render_frame(hs, W, H, S, B, seed=100 + k, want_linear=True)["linear"] for k in range(7)]
feats = rt.render_features(hs, W, H, S, B)
sigma_p = default_sigma_position(feats["position"], feats["coverage"])
planes = [torch.from_numpy(feats[k]).cuda() for k in ("coverage", "albedo", "normal", "position")]
colors = [torch.from_numpy(f).cuda() for f in frames]
pp = [p.data_ptr() for p in planes]
stream = torch.cuda.current_stream()
sp = stream.cuda_stream


def buf(n_bytes):
    return torch.zeros((n_bytes,), dtype=torch.uint8, device="cuda")


n_hist, n_mom, n_work = lib.rt_temporal_history_bytes(W, H), lib.rt_temporal_moments_bytes(W, H), lib.rt_guided_variance_work_bytes(W, H)
assert n_work == lib.rt_guided_work_bytes(W, H)
out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
filtered = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
length = torch.empty((H, W), dtype=torch.float32, device="cuda")
var = torch.empty((H, W), dtype=torch.float32, device="cuda")
img = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
work = buf(n_work)
tp = abi.RT_Temporal_Params(alpha=0.05, max_history=64, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
vp = abi.RT_Variance_Params(0.2, sigma_p)
g_fixed = abi.RT_Guided_Params(ITERATIONS, 1.0, 0.2, sigma_p, 1)
g_var = abi.RT_Guided_Params(ITERATIONS, 4.0, 0.2, sigma_p, 1)


def moments(color, h_in, m_in, h_out, m_out, want_variance=True):
    assert lib.rt_temporal_accumulate_moments(W, H, C.byref(tp), C.byref(cam), C.byref(cam), color.data_ptr(), *pp,
                                              None if h_in is None else h_in.data_ptr(), h_out.data_ptr(), out.data_ptr(),
                                              length.data_ptr(), None, C.byref(vp), None if m_in is None else m_in.data_ptr(),
                                              m_out.data_ptr(), var.data_ptr() if want_variance else None, sp) == 0, rt.last_error()


def plain(color, h_in, h_out):
    assert lib.rt_temporal_accumulate(W, H, C.byref(tp), C.byref(cam), C.byref(cam), color.data_ptr(), *pp, h_in.data_ptr(),
                                      h_out.data_ptr(), out.data_ptr(), length.data_ptr(), None, sp) == 0, rt.last_error()


def filter_fixed():
    assert lib.rt_guided_denoise(W, H, C.byref(g_fixed), out.data_ptr(), *pp, filtered.data_ptr(), img.data_ptr(), work.data_ptr(),
                                 sp) == 0, rt.last_error()


def filter_variance():
    assert lib.rt_guided_denoise_variance(W, H, C.byref(g_var), out.data_ptr(), *pp, filtered.data_ptr(), img.data_ptr(),
                                          work.data_ptr(), sp, var.data_ptr(), None) == 0, rt.last_error()


# the two histories: after one frame (SHORT) and after six (LONG), with their moments
hist = {k: (buf(n_hist), buf(n_mom)) for k in ("short", "long")}
a, b = (buf(n_hist), buf(n_mom)), (buf(n_hist), buf(n_mom))
moments(colors[0], None, None, *hist["short"])
moments(colors[0], None, None, *a)
for k in range(1, 6):
    moments(colors[k], a[0], a[1], *(hist["long"] if k == 5 else b))
    a, b = b, a
scratch = (buf(n_hist), buf(n_mom))
torch.cuda.synchronize()
fractions = {}
for name in hist:
    moments(colors[6], *hist[name], *scratch)
    torch.cuda.synchronize()
    surface = planes[0] > 0
    fractions[name] = (float(surface.float().mean().item()), float(((length < 4) & surface).float().sum().item() / surface.sum().item()))

stages = []
for name in ("short", "long"):
    h, m = hist[name]
    stages += [(name, "rt_temporal_accumulate", lambda h=h: plain(colors[6], h, scratch[0])),
               (name, "rt_temporal_accumulate_moments, no variance wanted", lambda h=h, m=m: moments(colors[6], h, m, *scratch, False)),
               (name, "rt_temporal_accumulate_moments + variance launch", lambda h=h, m=m: moments(colors[6], h, m, *scratch, True)),
               (name, "rt_guided_denoise, %d iterations" % ITERATIONS, filter_fixed),
               (name, "rt_guided_denoise_variance, %d iterations" % ITERATIONS, filter_variance)]


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(BATCH):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / BATCH


for _ in range(5):
    for _, _, call in stages:
        call()
torch.cuda.synchronize()
ms = {(n, s): [] for n, s, _ in stages}
for _ in range(steps):
    for n, s, call in stages:
        if "denoise" in s:                                # the filters read `out` and `var` of this history's accumulation
            moments(colors[6], *hist[n], *scratch, True)
            torch.cuda.synchronize()
        ms[(n, s)].append(timed(call))

lines = [f"helmet {W}x{H}, {S} spp, {B} bounces; {steps} rounds of {BATCH} calls back to back per stage, stages interleaved; "
         f"{fractions['long'][0] * 100:.1f} % of the pixels see a surface; of those, len' < 4 in the SHORT history: "
         f"{fractions['short'][1] * 100:.1f} %, in the LONG history: {fractions['long'][1] * 100:.1f} %", "",
         "| history | stage | per call: median ms | min - max ms |", "|---|---|---|---|"]
for n, s, _ in stages:
    v = ms[(n, s)]
    lines.append(f"| {n} | {s} | {statistics.median(v):.4f} | {min(v):.4f} - {max(v):.4f} |")
lines += ["", "| history | the variance launch alone (with - without, of the medians) ms | post stages of rt_render_svgf ms | "
          "post stages of rt_render_temporal + filter ms |", "|---|---|---|---|"]
for n in ("short", "long"):
    med = {s: statistics.median(ms[(n, s)]) for nn, s, _ in stages if nn == n}
    keys = list(med)
    lines.append(f"| {n} | {med[keys[2]] - med[keys[1]]:.4f} | {med[keys[2]] + med[keys[4]]:.4f} | {med[keys[0]] + med[keys[3]]:.4f} |")
print("\n".join(lines), flush=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
