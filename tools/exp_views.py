#!/usr/bin/env python3
"""GPU experiment: K views of one scene rendered three ways, host wall time per view, scene resident, every image copied to the
host on all three sides:
  (a) K blocking rt_render_frame() calls (camera and seed set before each),
  (b) the same K frames pipelined two at a time through rt_frame_begin() / rt_frame_end(),
  (c) one rt_render_views() -- one launch of the path kernel for all K views.
The outputs of (a), (b) and (c) are compared once per shape, bit for bit.  Every shape is warmed up first; then `reps`
repetitions in alternating order give the median and the min - max spread.  The kernel column is the library's own HIP-event
time of the path-kernel launches of ONE repetition (rt_kernel_timing_mean_ms x launches), per view; rocprofv3 kernel times
belong in a separate run (`--quick` and EXP_ONLY keep that run short).  Writes a markdown table.

    python tools/exp_views.py [out.md] [reps] [--quick]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                      # noqa: E402
import raytracing_c_amd as rt                           # noqa: E402
from raytracing_c_amd import ctypes_abi as abi          # noqa: E402
from raytracing_c_amd.configs import load_config        # noqa: E402
from raytracing_c_amd.render import make_views          # noqa: E402
from raytracing_c_amd.scene import set_camera           # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
quick = "--quick" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "views.md")
reps = int(args[1]) if len(args) > 1 else 7
KS = [1, 2, 6, 16]
SHAPES = [("BASELINE config #1 shape", "spheres", 256, 256, 16, 4),
          ("helmet 512^2", "helmet", 512, 512, 16, 8),
          ("driver default frame shape", "helmet", 1024, 1024, 16, 8)]
if quick:
    reps = 2
if os.environ.get("EXP_ONLY"):                # "shape:K[,shape:K ...]" (shape = index into SHAPES): e.g. for a rocprofv3 run
    only = [tuple(map(int, t.split(":"))) for t in os.environ["EXP_ONLY"].split(",")]
    SHAPES = [SHAPES[i] for i in sorted({i for i, _ in only})]
    KS = sorted({k for _, k in only})

assert rt.lib.rt_init(0) == 0, rt.last_error()


def orbit(hs, k):
    """k cameras on an orbit about the world's y axis through the file camera, distinct seeds"""
    m = np.array([[hs.scene.camera.view_matrix.rows[i][j] for j in range(4)] for i in range(4)], np.float32)
    fov = float(hs.scene.camera.fov)
    cams = []
    for v in range(k):
        a = np.deg2rad(360.0 * v / k)
        r = np.eye(4, dtype=np.float32)
        r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        cam = abi.Camera()
        set_camera(cam, r @ m, fov)
        cams.append(cam)
    return cams, [0x1234ABCD + 977 * v for v in range(k)]


class Target:
    def __init__(self, k, w, h):
        self.out = np.zeros((k, h, w, 3), np.uint8)
        self.images = (abi.Image * k)()
        for v in range(k):
            im = self.images[v]
            im.components, im.pixel_type, im.width, im.stride, im.height = 3, 0, w, w, h
            im.pixels.data, im.pixels.len = self.out[v].ctypes.data, self.out[v].size


def blocking(hs, cams, seeds, tg, s, b):
    saved = abi.Camera.from_buffer_copy(hs.scene.camera)
    t0 = time.perf_counter()
    for v, (cam, sd) in enumerate(zip(cams, seeds)):
        hs.scene.camera = cam
        rt.lib.rt_set_seed(sd)
        assert rt.lib.rt_render_frame(C.byref(hs.scene), C.byref(tg.images[v]), s, b, None, None) == 0, rt.last_error()
    dt = time.perf_counter() - t0
    hs.scene.camera = saved
    return dt


def pipelined(hs, cams, seeds, tg, s, b):
    saved = abi.Camera.from_buffer_copy(hs.scene.camera)
    t0 = time.perf_counter()
    pending = []
    for v, (cam, sd) in enumerate(zip(cams, seeds)):
        if len(pending) == 2:
            assert rt.lib.rt_frame_end(pending.pop(0)) == 0, rt.last_error()
        hs.scene.camera = cam                 # (camera and seed are read at begin)
        rt.lib.rt_set_seed(sd)
        t = rt.lib.rt_frame_begin(C.byref(hs.scene), C.byref(tg.images[v]), s, b)
        assert t >= 0, rt.last_error()
        pending.append(t)
    while pending:
        assert rt.lib.rt_frame_end(pending.pop(0)) == 0, rt.last_error()
    dt = time.perf_counter() - t0
    hs.scene.camera = saved
    return dt


def batched(hs, views, tg, s, b):
    t0 = time.perf_counter()
    assert rt.lib.rt_render_views(C.byref(hs.scene), len(views), views, tg.images, s, b, None, None) == 0, rt.last_error()
    return time.perf_counter() - t0


def kernel_ms(fn):
    """path-kernel GPU time of one call of fn (HIP events of the library), summed over its launches"""
    rt.lib.rt_kernel_timing_reset()
    fn()
    n = C.c_int32()
    mean = rt.lib.rt_kernel_timing_mean_ms(C.byref(n))
    return mean * n.value, n.value


rows = []
for label, cfg, w, h, s, b in SHAPES:
    hs, _ = load_config(cfg)
    for k in KS:
        cams, seeds = orbit(hs, k)
        views = make_views(cams, seeds)
        ta, tb, tc = Target(k, w, h), Target(k, w, h), Target(k, w, h)
        run = {"a": lambda: blocking(hs, cams, seeds, ta, s, b), "b": lambda: pipelined(hs, cams, seeds, tb, s, b),
               "c": lambda: batched(hs, views, tc, s, b)}
        for f in run.values():                # warm-up of this shape (uploads, buffers, schedule feedback)
            f()
            f()
        assert np.array_equal(ta.out, tb.out), "pipelined frames differ from the blocking ones"
        assert np.array_equal(ta.out, tc.out), "rt_render_views differs from the blocking frames"
        times = {m: [] for m in run}
        for r in range(reps):
            order = "abc" if r % 2 == 0 else "cba"
            for m in order:
                times[m].append(run[m]() * 1e3 / k)
        kern = {m: kernel_ms(run[m]) for m in run}
        rows.append((label, cfg, w, h, s, b, k, times, kern))
        med = {m: statistics.median(v) for m, v in times.items()}
        print(f"{cfg} {w}x{h} {s}spp {b}b K={k}: " + ", ".join(f"{m} {med[m]:.3f}" for m in "abc") +
              " ms/view; kernel/view " + ", ".join(f"{m} {kern[m][0] / k:.3f} ({kern[m][1]})" for m in "abc"), flush=True)
    rt.lib.rt_scene_invalidate(C.byref(hs.scene))


def cell(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"


lines = ["| shape | K | (a) K x rt_render_frame | (b) two frames in flight | (c) rt_render_views | (c) / (a) | (c) / (b) | "
         "path kernel per view (a) / (b) / (c), launches |",
         "|---|---|---|---|---|---|---|---|"]
for label, cfg, w, h, s, b, k, times, kern in rows:
    ma, mb, mc = (statistics.median(times[m]) for m in "abc")
    lines.append(f"| {label}: {cfg} {w}x{h}, {s} spp, {b} bounces | {k} | {cell(times['a'])} | {cell(times['b'])} | "
                 f"{cell(times['c'])} | {(mc / ma - 1) * 100:+.1f} % | {(mc / mb - 1) * 100:+.1f} % | "
                 f"{kern['a'][0] / k:.3f} / {kern['b'][0] / k:.3f} / {kern['c'][0] / k:.3f} ms, {kern['a'][1]} / {kern['b'][1]} / "
                 f"{kern['c'][1]} |")
table = "\n".join(lines)
print(table)
if out_path != "-":
    head = ["# K views of one scene: K frames, two frames in flight, or one rt_render_views launch", "",
            f"`python tools/exp_views.py` on one MI355X, {reps} repetitions per cell after a warm-up of every shape (alternating order "
            "a b c / c b a).  Host wall time per view in ms, median (min - max); scene resident and checked every call; every "
            "image copied to the host.  The K views are an orbit in K steps about the world's y axis through the file camera, one "
            "seed each; (a), (b) and (c) give the same images, bit for bit (checked per shape).  Last column: the path-kernel "
            "launches of one repetition, HIP-event GPU time per view and the number of launches.", "", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(head) + table + "\n")
