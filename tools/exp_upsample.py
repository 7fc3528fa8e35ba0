#!/usr/bin/env python3
"""GPU experiment: what a half-resolution frame costs -- rt_render_upsampled (the path frame at 960x540, its feature pass, the
full-resolution feature pass with guide_samples samples, the upsampling, optionally the guided filter) beside rt_render_denoised at
the full size, on config #3's shape: helmet, 1920x1080, 16 spp, 8 bounces.  One process; 3 warm-up rounds, then `steps` timed
rounds with the cases interleaved; median and min - max.

Two tables.  The upsampling alone: rt_guided_upsample on the device level, buffers resident, HIP events on one stream around BATCH
calls back to back, divided by BATCH; a call is the pack launch over the low frame and the upsampling launch, and the bytes per
full pixel are the least both must move.  The frames: the host clock around the whole call (the Image's 6 MB come back to the
host in every case, no f32 output is asked for), and rt_get_frame_timing()'s split of the GPU time -- gpu_path_ms is the path
kernel, gpu_resolve_ms + gpu_copy_ms everything behind it: resolve, feature passes, upsampling, filter, the image's copy.

    python tools/exp_upsample.py [out.md] [steps]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                      # noqa: E402
import torch                                            # noqa: E402
import raytracing_c_amd as rt                           # noqa: E402
from raytracing_c_amd import ctypes_abi as abi          # noqa: E402
from raytracing_c_amd.configs import load_config        # noqa: E402
from raytracing_c_amd.guided import default_sigma_position   # noqa: E402
from raytracing_c_amd.scene import make_image           # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "upsample_table.md")
steps = int(args[1]) if len(args) > 1 else 10
W, H, S, B = 1920, 1080, 16, 8
BATCH = 20
ITERATIONS = 4
ORDER = ("coverage", "albedo", "normal", "position")

assert rt.lib.rt_init(0) == 0, rt.last_error()
lib = rt.lib
hs, _ = load_config("helmet")
low_frame = rt.render_frame(hs, W // 2, H // 2, S, B, want_linear=True)["linear"]
low = rt.render_features(hs, W // 2, H // 2, S, B)
full = rt.render_features(hs, W, H, 4, B)
sigma_p = default_sigma_position(full["position"], full["coverage"])

# ---- the upsampling alone, device level -----------------------------------------------------------------------------------------
t_low = [torch.from_numpy(low_frame).cuda()] + [torch.from_numpy(low[k]).cuda() for k in ORDER]
t_full = [torch.from_numpy(full[k]).cuda() for k in ORDER]
out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
img = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
work = torch.empty((lib.rt_guided_upsample_work_bytes(W, H),), dtype=torch.uint8, device="cuda")
stream = torch.cuda.current_stream()
up = abi.RT_Upsample_Params(0.2, sigma_p, 1, 0)
ptrs = [t.data_ptr() for t in t_low + t_full]


def upsample_call(want_out, want_img):
    assert lib.rt_guided_upsample(W, H, C.byref(up), *ptrs, out.data_ptr() if want_out else None, img.data_ptr() if want_img else None,
                                  work.data_ptr(), stream.cuda_stream) == 0, rt.last_error()


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(BATCH):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / BATCH


# least bytes per FULL pixel: the pack launch reads 52 B and writes 48 B per low pixel (a quarter of that per full pixel); the
# upsampling launch reads the 48 B record once per low pixel and 40 B of full-resolution planes, and writes 12 B (f32) and / or 3 B
device_cases = [("f32 and u8", True, True, 25 + 12 + 40 + 15), ("f32 alone", True, False, 25 + 12 + 40 + 12),
                ("u8 alone", False, True, 25 + 12 + 40 + 3)]
for _ in range(3):
    for _, o, i, _ in device_cases:
        upsample_call(o, i)
torch.cuda.synchronize()
device_ms = {name: [] for name, *_ in device_cases}
for _ in range(steps):
    for name, o, i, _ in device_cases:
        device_ms[name].append(timed(lambda: upsample_call(o, i)))

# ---- the frames -----------------------------------------------------------------------------------------------------------------
pixels = np.zeros((H, W, 3), np.uint8)
image, _keep = make_image(pixels)
image.pixels.data = pixels.ctypes.data
gp = abi.RT_Guided_Params(ITERATIONS, 1.0, 0.2, sigma_p, 1)
timing = abi.RT_Frame_Timing()


def upsampled(guide_samples, filtered):
    p = abi.RT_Upsample_Params(0.2, sigma_p, 1, guide_samples)
    assert lib.rt_render_upsampled(C.byref(hs.scene), C.byref(image), S, B, C.byref(p), C.byref(gp) if filtered else None, None, None,
                                   None) == 0, rt.last_error()


def denoised():
    assert lib.rt_render_denoised(C.byref(hs.scene), C.byref(image), S, B, C.byref(gp), None, None) == 0, rt.last_error()


def plain():
    assert lib.rt_render_frame(C.byref(hs.scene), C.byref(image), S, B, None, None) == 0, rt.last_error()


frame_cases = [("rt_render_frame 1920x1080 (no post stage)", plain), ("rt_render_denoised 1920x1080", denoised)]
for gs in (16, 4, 1):
    frame_cases += [(f"rt_render_upsampled, guide_samples {gs}, no filter", lambda gs=gs: upsampled(gs, False)),
                    (f"rt_render_upsampled, guide_samples {gs}, filter", lambda gs=gs: upsampled(gs, True))]
for _ in range(3):
    for _, call in frame_cases:
        call()
frame_ms = {name: dict(wall=[], path=[], behind=[]) for name, _ in frame_cases}
for _ in range(steps):
    for name, call in frame_cases:
        t0 = time.perf_counter()
        call()
        frame_ms[name]["wall"].append((time.perf_counter() - t0) * 1e3)
        assert lib.rt_get_frame_timing(C.byref(timing)) == 0
        frame_ms[name]["path"].append(timing.gpu_path_ms)
        frame_ms[name]["behind"].append(timing.gpu_resolve_ms + timing.gpu_copy_ms)


def stat(v):
    return f"{statistics.median(v):.3f} | {min(v):.3f} - {max(v):.3f}"


lines = [f"helmet {W}x{H} (low frame {W // 2}x{H // 2}), {S} spp, {B} bounces, filter of {ITERATIONS} iterations; {steps} rounds, cases "
         "interleaved, one process", "",
         f"rt_guided_upsample, device level, buffers resident, {BATCH} calls back to back per round:", "",
         "| outputs | per call: median ms | min - max ms | least B per full pixel | implied GB/s at the median |", "|---|---|---|---|---|"]
for name, _, _, nbytes in device_cases:
    med = statistics.median(device_ms[name])
    lines.append(f"| {name} | {stat(device_ms[name])} | {nbytes} | {nbytes * W * H / (med * 1e-3) / 1e9:.0f} |")
lines += ["", "whole calls (host clock; the path kernel and what runs behind it from rt_get_frame_timing):", "",
          "| call | wall: median ms | min - max ms | path kernel: median ms | min - max ms | behind the path kernel: median ms | min - max ms |",
          "|---|---|---|---|---|---|---|"]
for name, _ in frame_cases:
    v = frame_ms[name]
    lines.append(f"| {name} | {stat(v['wall'])} | {stat(v['path'])} | {stat(v['behind'])} |")
print("\n".join(lines), flush=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
