#!/usr/bin/env python3
"""GPU experiment: what a probe pass costs -- a 16 x 16 x 16 probe_grid over the helmet's bounding box grown by 10 %, 256 samples
per probe, 8 bounces (1 048 576 paths) through rt_probe_trace, rt_probe_project and rt_probe_resolve on the device level, buffers
resident, one HIP event pair around each of the three launches -- beside rt_render_frame on the same scene at the same path count
(512 x 512, 4 spp, 8 bounces), in one process, alternating.  3 warm-up rounds, then `steps` timed rounds; median and min - max.
Rays per second: rt_get_probe_counters().rays over the trace time, rt_get_counters().rays over rt_get_frame_timing().gpu_path_ms.

    python tools/exp_probes.py [out.md] [steps]"""
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
out_path = args[0] if args else os.path.join(ROOT, "profiles", "probes_table.md")
steps = int(args[1]) if len(args) > 1 else 20
GRID, SAMPLES, BOUNCES = (16, 16, 16), 256, 8
FW, FH, FS = 512, 512, 4
SEED = 0x1234ABCD

assert rt.lib.rt_init(0) == 0, rt.last_error()
lib = rt.lib
hs, _ = load_config("helmet")

# the bounding box of the triangles the scene holds (the builder's empty slots have no shader)
T = hs.scene.triangles
n_slots = int(T.len)
rows = np.zeros(n_slots, np.dtype([("head", "<f4", (24,)), ("shader_data", "<u8"), ("shader_proc", "<u8")]))
C.memmove(rows.ctypes.data, T.aos, n_slots * 112)
held = rows["shader_proc"] != 0
pts = np.stack([np.concatenate([np.ctypeslib.as_array(getattr(T, ax)[k], (n_slots,))[held] for k in range(3)]) for ax in "xyz"], 1)
lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
c, e = (lo + hi) / 2, (hi - lo) * 1.1 / 2
positions = rt.probe_grid(c - e, c + e, GRID)
n = len(positions)
assert n * SAMPLES == FW * FH * FS

d = lib.rt_scene_upload(C.byref(hs.scene))
assert d, rt.last_error()
pos = torch.from_numpy(positions).cuda()
records = torch.empty((n, SAMPLES, 8), dtype=torch.float32, device="cuda")
sums = torch.zeros((n, 9, 3), dtype=torch.int64, device="cuda")
coeffs = torch.empty((n, 9, 3), dtype=torch.float32, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream
p = abi.RT_Probe_Params(samples=SAMPLES, max_bounces=BOUNCES, seed=SEED)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]


def probe_pass():
    sums.zero_()
    ev[0].record(stream)
    assert lib.rt_probe_trace(d, C.byref(p), n, pos.data_ptr(), records.data_ptr(), sp) == 0, rt.last_error()
    ev[1].record(stream)
    assert lib.rt_probe_project(C.byref(p), n, records.data_ptr(), sums.data_ptr(), sp) == 0, rt.last_error()
    ev[2].record(stream)
    assert lib.rt_probe_resolve(C.byref(p), n, sums.data_ptr(), coeffs.data_ptr(), sp) == 0, rt.last_error()
    ev[3].record(stream)
    ev[3].synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(3)], rt.get_probe_counters()


def frame():
    f = rt.render_frame(hs, FW, FH, FS, BOUNCES, seed=SEED)
    t = abi.RT_Frame_Timing()
    assert lib.rt_get_frame_timing(C.byref(t)) == 0, rt.last_error()
    return t.gpu_path_ms, f["counters"]


for _ in range(3):
    probe_pass()
    frame()
rows_p, rows_f = [], []
for _ in range(steps):
    rows_p.append(probe_pass())
    rows_f.append(frame())
lib.rt_scene_release(d)


def stat(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"


pc, fc = rows_p[-1][1], rows_f[-1][1]
trace = [r[0][0] for r in rows_p]
path = [r[0] for r in rows_f]
grays_p = pc.rays / (statistics.median(trace) * 1e-3) / 1e9
grays_f = fc.rays / (statistics.median(path) * 1e-3) / 1e9
lines = [
    f"helmet, {GRID[0]} x {GRID[1]} x {GRID[2]} probes x {SAMPLES} samples, {BOUNCES} bounces = {n * SAMPLES} paths; "
    f"frame {FW} x {FH} x {FS} spp; 3 warm-ups, {steps} rounds, alternating; ms: median (min - max)",
    "",
    "| launch | ms | paths | rays | node visits | leaf visits | shades | backgrounds | G rays / s |",
    "|---|---|---|---|---|---|---|---|---|",
    f"| rt_probe_kernel (trace) | {stat(trace)} | {pc.paths} | {pc.rays} | {pc.node_visits} | {pc.leaf_visits} | {pc.shades} | {pc.backgrounds} | {grays_p:.3f} |",
    f"| rt_probe_project_kernel | {stat([r[0][1] for r in rows_p])} | | | | | | | |",
    f"| rt_probe_resolve_kernel | {stat([r[0][2] for r in rows_p])} | | | | | | | |",
    f"| path kernel of rt_render_frame | {stat(path)} | {fc.paths} | {fc.rays} | {fc.node_visits} | {fc.leaf_visits} | {fc.shades} | {fc.backgrounds} | {grays_f:.3f} |",
    "",
    f"probe kernel / frame kernel, rays per second: {grays_p / grays_f:.3f}",
]
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
