#!/usr/bin/env python3
"""GPU experiment: throughput of the batch ray queries (rt_query_closest, rt_query_occluded, closest hit + full records) in
Mray/s from HIP events, rays and results resident on the device, for helmet and tower, three kinds of ray list and three batch
sizes:
  (a) camera  -- the camera rays of the 1920x1080 frame in pixel order (repeated / cut to the batch size),
  (b) mix     -- the incoherent mix of the traversal's parity test: half from outside aimed into the scene box, half from inside,
  (c) shadow  -- from the hit points of (b) towards one point light, unnormalised, t_max = 1 (the light's distance).
Every case is warmed up (3 launches), then `reps` launches are timed one by one: median and min - max.  Also printed: the
any-hit visit ratio (node + leaf visits of the occlusion query / of the closest-hit query).

    python tools/exp_queries.py [out.md] [reps] [--quick]
    python tools/exp_queries.py --yardstick       # rt_test_trace_stream (diagnostic library) once per case and size, for a
                                                  # rocprofv3 --kernel-trace --stats run of its own: it has no event timing"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                      # noqa: E402
import torch                                            # noqa: E402
import raytracing_c_amd as rt                           # noqa: E402
from raytracing_c_amd.configs import load_config        # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
quick = "--quick" in sys.argv
yardstick = "--yardstick" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "queries_table.md")
reps = int(args[1]) if len(args) > 1 else 10
SIZES = [1 << 16, 1 << 20] if quick else [1 << 16, 1 << 20, 1 << 24]
SCENES = ["helmet", "tower"]


def bbox(hs):
    T = hs.scene.triangles
    n = int(T.len)
    pts = [np.concatenate([np.ctypeslib.as_array(getattr(T, ax)[k], (n,)) for k in range(3)]) for ax in "xyz"]
    return np.array([p.min() for p in pts]), np.array([p.max() for p in pts])


def camera_rays(hs, w=1920, h=1080):
    cam = hs.scene.camera
    m = np.array([[cam.view_matrix.rows[i][j] for j in range(4)] for i in range(3)], np.float64)
    y, x = np.mgrid[0:h, 0:w]
    uvx = (x + 0.5) * 2.0 / w - 1.0
    uvy = (y + 0.5) * 2.0 / h - 1.0
    d = np.stack([uvx * (w / h), -uvy, np.full_like(uvx, -float(cam.focal_length))], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.empty((w * h, 6), np.float32)
    rays[:, :3] = m[:, 3]
    rays[:, 3:] = d @ m[:, :3].T
    return rays


def mix_rays(hs, n, rng):
    lo, hi = bbox(hs)
    c, e = (lo + hi) / 2, np.maximum(hi - lo, 1e-3)
    rays = np.zeros((n, 6), np.float32)
    k = n // 2
    o = c + rng.normal(size=(k, 3)) * e * 1.5
    d = c + rng.uniform(-0.5, 0.5, (k, 3)) * e - o
    rays[:k, :3], rays[:k, 3:] = o, d / np.linalg.norm(d, axis=1, keepdims=True)
    d = rng.normal(size=(n - k, 3))
    rays[k:, :3], rays[k:, 3:] = c + rng.uniform(-0.5, 0.5, (n - k, 3)) * e, d / np.linalg.norm(d, axis=1, keepdims=True)
    return rays


def sized(rays, n):
    return np.ascontiguousarray(np.resize(rays, (n, 6)))


def timed(fn, stream):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


assert rt.lib.rt_init(0) == 0, rt.last_error()
lines = ["| scene | rays | n | closest Mray/s (min - max) | occluded Mray/s (min - max) | closest + full Mray/s (min - max) | any-hit visits / closest |",
         "|---|---|---|---|---|---|---|"]
for name in SCENES:
    hs, _ = load_config(name)
    rng = np.random.default_rng(11)
    lo, hi = bbox(hs)
    light = ((lo + hi) / 2 + (hi - lo) * np.array([0.8, 1.5, 0.6])).astype(np.float32)
    base = {"camera": camera_rays(hs), "mix": mix_rays(hs, 1 << 22, rng)}
    d = (rt.diag if yardstick else rt.lib).rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error()
    stream = torch.cuda.current_stream()
    # shadow rays: from the hit points of the mix towards the light
    if not yardstick:
        r = torch.from_numpy(base["mix"]).cuda()
        hits = rt.closest_hits_device(d, r).cpu().numpy()
        ok = hits[:, 1].view(np.int32) >= 0
        p = base["mix"][ok, :3] + base["mix"][ok, 3:] * hits[ok, 0:1]
        sh = np.empty((len(p), 6), np.float32)
        sh[:, :3], sh[:, 3:] = p, light - p
        base["shadow"] = sh
    for kind, rays0 in base.items():
        for n in SIZES:
            rays = sized(rays0, n)
            if yardstick:
                t, tri, uv = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
                visits = (C.c_uint64 * 2)()
                for _ in range(4):
                    assert rt.diag.rt_test_trace_stream(d, n, rays.ctypes.data, None, 48, 0, t.ctypes.data, tri.ctypes.data,
                                                        uv.ctypes.data, visits) == 0, rt.last_error(rt.diag)
                print(f"yardstick {name} {kind} n={n}: 4 launches of rt_test_trace_stream_kernel", flush=True)
                continue
            r = torch.from_numpy(rays).cuda()
            tm = torch.ones(n, dtype=torch.float32, device="cuda") if kind == "shadow" else None
            row = []
            for fn in (lambda: rt.closest_hits_device(d, r, tm), lambda: rt.occluded_device(d, r, tm),
                       lambda: rt.closest_hits_device(d, r, tm, full=True)):
                med, lo_ms, hi_ms = timed(fn, stream)
                row.append(f"{n / med / 1e3:.0f} ({n / hi_ms / 1e3:.0f} - {n / lo_ms / 1e3:.0f})")
            rt.closest_hits_device(d, r, tm)
            c = rt.get_query_counters()
            rt.occluded_device(d, r, tm)
            a = rt.get_query_counters()
            ratio = (a.node_visits + a.leaf_visits) / max(1, c.node_visits + c.leaf_visits)
            lines.append(f"| {name} | {kind} | 2^{n.bit_length() - 1} | {row[0]} | {row[1]} | {row[2]} | {ratio:.3f} |")
            print(lines[-1], flush=True)
            del r, tm
            torch.cuda.empty_cache()
    (rt.diag if yardstick else rt.lib).rt_scene_release(d)
if not yardstick:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
