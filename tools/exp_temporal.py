#!/usr/bin/env python3
"""GPU experiment: temporal accumulation (rt_temporal_accumulate: ONE launch of rt_temporal_kernel) on config #3's shape -- helmet,
1920x1080, 16 spp, 8 bounces -- beside the path-kernel time of the same frame and the bytes the contract moves per pixel.  Device
level, buffers resident, HIP events around the launch alone on one stream: 5 warm-up launches, then `steps` timed launches per
case, the cases interleaved; median and min - max.  A launch is short beside what an event pair resolves, so a second column times
BATCH launches back to back between one event pair (every launch reads hist[0] and writes hist[1]) and divides.  Cases: no
history; equal cameras (every pixel fetches its own history pixel); a camera that moved sideways by about 3 pixels at the scene's
median depth (the gathers straddle pixels and rows).

Bytes per pixel, from the record sizes: 13 planar f32 read (52 B), three float4 of new history written (48 B), and the old history
read once where it is used at all (48 B: neighbouring pixels share their taps, so the unique read is one record set per pixel);
with the three optional outputs f32 x 3 + f32 + u8 x 3 = 19 B more.  Sky pixels read 52 B and write 48 B + outputs.

    python tools/exp_temporal.py [out.md] [steps]"""
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
out_path = args[0] if args else os.path.join(ROOT, "profiles", "temporal_table.md")
steps = int(args[1]) if len(args) > 1 else 20
W, H, S, B = 1920, 1080, 16, 8
BATCH = 50

assert rt.lib.rt_init(0) == 0, rt.last_error()
hs, _ = load_config("helmet")
cam = hs.scene.camera
rows = [[cam.view_matrix.rows[i][k] for k in range(4)] for i in range(4)]


def camera_moved(offset):
    c = abi.Camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(abi.Camera))
    for i in range(3):
        c.view_matrix.rows[i][3] = float(np.float32(rows[i][3] + offset * rows[i][0]))     # along the camera's own x axis
    return c


frame = rt.render_frame(hs, W, H, S, B, want_linear=True)
path_ms = [float(rt.lib.rt_last_kernel_ms())]
for _ in range(4):
    rt.render_frame(hs, W, H, S, B)
    path_ms.append(float(rt.lib.rt_last_kernel_ms()))
feats = rt.render_features(hs, W, H, S, B)
full = feats["coverage"] == 1.0
origin = np.array([rows[i][3] for i in range(3)])
depth = float(np.median(np.linalg.norm(feats["position"][full].astype(np.float64) - origin, axis=1)))
pixel = depth * (W / H) / (cam.focal_length * W * 0.5)                                     # world size of a pixel at that depth
t = {k: torch.from_numpy(v).cuda() for k, v in
     dict(color=frame["linear"], coverage=feats["coverage"], albedo=feats["albedo"], normal=feats["normal"], position=feats["position"]).items()}
n_hist = rt.lib.rt_temporal_history_bytes(W, H)
hist = [torch.zeros((n_hist,), dtype=torch.uint8, device="cuda") for _ in range(2)]
out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
length = torch.empty((H, W), dtype=torch.float32, device="cuda")
img = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream
params = abi.RT_Temporal_Params(alpha=0.05, max_history=64, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=1)
here = camera_moved(0.0)


def launch(previous, h_in, h_out):
    assert rt.lib.rt_temporal_accumulate(W, H, C.byref(params), C.byref(here), None if previous is None else C.byref(previous),
                                         t["color"].data_ptr(), t["coverage"].data_ptr(), t["albedo"].data_ptr(), t["normal"].data_ptr(),
                                         t["position"].data_ptr(), None if previous is None else h_in.data_ptr(), h_out.data_ptr(),
                                         out.data_ptr(), length.data_ptr(), img.data_ptr(), sp) == 0, rt.last_error()


launch(None, None, hist[0])                                                                # hist[0]: a real history of this view
torch.cuda.synchronize()
cases = [("no history", None), ("equal cameras", camera_moved(0.0)), ("camera moved 3.3 pixels sideways", camera_moved(-3.3 * pixel))]
for _ in range(5):
    for _, previous in cases:
        launch(previous, hist[0], hist[1])
torch.cuda.synchronize()
ms = {name: [] for name, _ in cases}
reused = {}
for _ in range(steps):
    for name, previous in cases:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch(previous, hist[0], hist[1])
        e1.record(stream)
        e1.synchronize()
        ms[name].append(e0.elapsed_time(e1))
        reused[name] = float((length > 1).float().mean().item())
batch_ms = {name: [] for name, _ in cases}
for _ in range(steps):
    for name, previous in cases:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _k in range(BATCH):
            launch(previous, hist[0], hist[1])
        e1.record(stream)
        e1.synchronize()
        batch_ms[name].append(e0.elapsed_time(e1) / BATCH)
hit = float((feats["coverage"] > 0).mean())
lines = [f"helmet {W}x{H}, {S} spp, {B} bounces; {steps} launches per case, interleaved; {hit * 100:.1f} % of the pixels see a surface; "
         f"median depth {depth:.3f}, a pixel there is {pixel:.5f} wide", "",
         f"| case | one launch: median ms | min - max ms | {BATCH} launches back to back, per launch: median ms | min - max ms | "
         "pixels that reused history | bytes per pixel | MB | GB/s at the back-to-back median |", "|---|---|---|---|---|---|---|---|---|"]
for name, previous in cases:
    med, bmed = statistics.median(ms[name]), statistics.median(batch_ms[name])
    per_pixel = 52 + 48 + 19 + (0 if previous is None else 48 * hit)
    mb = per_pixel * W * H / 1e6
    lines.append(f"| {name} | {med:.4f} | {min(ms[name]):.4f} - {max(ms[name]):.4f} | {bmed:.4f} | {min(batch_ms[name]):.4f} - "
                 f"{max(batch_ms[name]):.4f} | {reused[name] * 100:.1f} % | {per_pixel:.1f} | {mb:.1f} | {mb / bmed:.0f} |")
lines += ["", f"path kernel of the same frame: median {statistics.median(path_ms):.3f} ms ({min(path_ms):.3f} - {max(path_ms):.3f}, "
          f"{len(path_ms)} frames)"]
print("\n".join(lines), flush=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
