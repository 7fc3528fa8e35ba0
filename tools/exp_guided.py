#!/usr/bin/env python3
"""GPU experiment: the guided denoiser (rt_guided_denoise: one pack launch + one filter launch per iteration) on config #3's
shape -- helmet, 1920x1080, 16 spp, 8 bounces -- with 5 iterations, beside the path-kernel time of the same frame and the byte
floor of the filter (64 B per pixel and iteration: three float4 records in, one out).  Device level, buffers resident, HIP events
around each call on one stream: 3 warm-up calls, then `steps` timed calls per iteration count k = 1 .. 5, interleaved; median and
min - max.  A call with k iterations is pack + k filter launches, so the k-th iteration costs about T(k) - T(k - 1) (the last
launch of every call is the one that stores f32 + u8 instead of a float4).

    python tools/exp_guided.py [out.md] [steps]"""
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
from raytracing_c_amd.guided import default_sigma_position   # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "guided_table.md")
steps = int(args[1]) if len(args) > 1 else 20
W, H, S, B, ITER = 1920, 1080, 16, 8, 5

assert rt.lib.rt_init(0) == 0, rt.last_error()
hs, _ = load_config("helmet")
frame = rt.render_frame(hs, W, H, S, B, want_linear=True)
path_ms = [float(rt.lib.rt_last_kernel_ms())]
for _ in range(4):
    rt.render_frame(hs, W, H, S, B)
    path_ms.append(float(rt.lib.rt_last_kernel_ms()))
feats = rt.render_features(hs, W, H, S, B)
sigma_p = default_sigma_position(feats["position"], feats["coverage"])
t = {k: torch.from_numpy(v).cuda() for k, v in
     dict(color=frame["linear"], coverage=feats["coverage"], albedo=feats["albedo"], normal=feats["normal"], position=feats["position"]).items()}
out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
img = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
work = torch.empty((rt.lib.rt_guided_work_bytes(W, H),), dtype=torch.uint8, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream


def denoise(k):
    p = abi.RT_Guided_Params(iterations=k, sigma_color=1.0, sigma_normal=0.2, sigma_position=sigma_p, demodulate=1)
    assert rt.lib.rt_guided_denoise(W, H, C.byref(p), t["color"].data_ptr(), t["coverage"].data_ptr(), t["albedo"].data_ptr(),
                                    t["normal"].data_ptr(), t["position"].data_ptr(), out.data_ptr(), img.data_ptr(), work.data_ptr(),
                                    sp) == 0, rt.last_error()


ks = list(range(1, ITER + 1))
for k in ks:
    for _ in range(3):
        denoise(k)
torch.cuda.synchronize()
ms = {k: [] for k in ks}
for _ in range(steps):
    for k in ks:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        denoise(k)
        e1.record(stream)
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1))
med = {k: statistics.median(v) for k, v in ms.items()}
floor_mb = 64 * W * H / 1e6
lines = [f"helmet {W}x{H}, {S} spp, {B} bounces; {steps} calls per iteration count, interleaved; sigma_position {sigma_p:.4f}", "",
         "| call | median ms | min - max ms | last iteration alone (difference of medians) ms | its 64 B / pixel floor as GB/s |",
         "|---|---|---|---|---|"]
for k in ks:
    d = med[k] - (med[k - 1] if k > 1 else 0.0)
    what = f"{d:.3f}" if k > 1 else f"{d:.3f} (with the pack launch)"
    lines.append(f"| pack + {k} iteration(s), step up to {1 << (k - 1)} | {med[k]:.3f} | {min(ms[k]):.3f} - {max(ms[k]):.3f} | {what} | "
                 f"{floor_mb / d:.0f} |")
lines += ["", f"whole filter ({ITER} iterations): {med[ITER]:.3f} ms; byte floor {ITER} x {floor_mb:.1f} MB = {ITER * floor_mb:.1f} MB "
          f"(+ {(13 * 4 + 48) * W * H / 1e6:.1f} MB for the pack launch)",
          f"path kernel of the same frame: median {statistics.median(path_ms):.3f} ms ({min(path_ms):.3f} - {max(path_ms):.3f}, {len(path_ms)} frames)"]
print("\n".join(lines), flush=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
