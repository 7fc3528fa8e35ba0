#!/usr/bin/env python3
"""GPU experiment: what an HDR lightmap bake costs beside the reference's entry point and beside the probe kernel.  Per scene -- a
soup of 40 000 small charts (tests/_lightmap.py: emissive_soup(9, 40000, chart=0.012, textured=True)) and the helmet on its own
UVs -- a 1024 x 1024 map at 8 bounces and `samples` samples per texel:
  (a) lightmap_bake (rt_lightmap_bake_kernel: one lane per texel, its samples in sequence), host call, wall clock around it minus
      nothing: uploads and the read-back of a 3 MB image are in; the kernel is unchanged since the parent commit (profiles/lightmap_hdr.md)
  (b) rt_lightmap_trace + rt_lightmap_resolve on the device level, buffers resident, one HIP event pair around each
  (c) rt_probe_trace at the same path count: one probe per list entry at the entry's origin, `samples` samples
plus rt_lightmap_texels and one dilation pass.  2 warm-up rounds, then `rounds` timed rounds, alternating (a) (b) (c); median and
min - max.  Rays per second from each call's own counters.

    python tools/exp_lightmap.py [out.md] [rounds] [samples,samples,...] [scene,scene] [rounds with (a)]
    python tools/exp_lightmap.py --trace-only ...     (b)'s trace alone: run once with the product and once with RT_LIB_PATH naming
                                                      a library whose rt_lightmap.hip was built with -DRT_LIGHTMAP_NO_ADDS"""
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

trace_only = "--trace-only" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "lightmap_hdr_table.md")
rounds = int(args[1]) if len(args) > 1 else 20
sample_counts = [int(v) for v in args[2].split(",")] if len(args) > 2 else [64, 256]
scenes = args[3].split(",") if len(args) > 3 else ["soup", "helmet"]
a_rounds = int(args[4]) if len(args) > 4 else rounds   # timed rounds in which (a) runs too (it is seconds long: the first ones only)
W = H = 1024
BOUNCES, SEED = 8, 0x1234ABCD

assert rt.lib.rt_init(0) == 0, rt.last_error()
lib = rt.lib
stream = torch.cuda.current_stream()
sp = stream.cuda_stream


def stat(v):
    if not v:
        return "not run"
    return f"{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


for name in scenes:
    if name == "soup":
        from tests._lightmap import emissive_soup
        hs = emissive_soup(9, 40000, chart=0.012, textured=True)
    else:
        hs, _ = load_config(name)
    d = lib.rt_scene_upload(C.byref(hs.scene))
    assert d, rt.last_error()
    verts = torch.from_numpy(rt.lightmap_vertices(hs)).cuda()
    owner = torch.empty(W * H + H, dtype=torch.int32, device="cuda")
    texels = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    image = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    work = torch.empty_like(image)

    def make_list():
        assert lib.rt_lightmap_texels(d, verts.data_ptr(), W, H, owner.data_ptr(), texels.data_ptr(), count.data_ptr(), sp) == 0, rt.last_error()
    t_list = [timed(make_list) for _ in range(rounds + 2)][2:]
    n = int(count.item())
    if n == 0:                                          # (the reference's rasteriser accepts no texel of this scene's UVs)
        emit(f"## {name}: {W} x {H}: no owned texel, nothing to trace; rt_lightmap_texels {stat(t_list)} ms")
        emit()
        lib.rt_scene_release(d)
        continue
    sums = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    positions = texels[:n, :3].contiguous()
    emit(f"## {name}: {W} x {H}, {n} owned texels ({n / (W * H):.3f}), {BOUNCES} bounces; 2 warm-ups, {rounds} rounds, alternating; ms: median (min - max)")
    emit()
    emit(f"rt_lightmap_texels (four kernels): {stat(t_list)} ms")
    for S in sample_counts:
        p = abi.RT_Lightmap_Params(width=W, height=H, samples=S, max_bounces=BOUNCES, seed=SEED, scale=1.0)
        pp = abi.RT_Probe_Params(samples=S, max_bounces=BOUNCES, seed=SEED)
        paths = n * S
        assert paths <= 1 << 30

        def trace():
            assert lib.rt_lightmap_trace(d, C.byref(p), texels.data_ptr(), 0, n, sums.data_ptr(), sp) == 0, rt.last_error()

        def resolve():
            assert lib.rt_lightmap_resolve(C.byref(p), n, texels.data_ptr(), sums.data_ptr(), image.data_ptr(), sp) == 0, rt.last_error()

        def hdr():
            sums.zero_()
            t = timed(trace)
            return t, timed(resolve), rt.get_lightmap_counters()

        if trace_only:
            rows = [hdr() for _ in range(rounds + 2)][2:]
            emit(f"{name}, {S} samples, library {os.environ.get('RT_LIB_PATH', 'product')}: rt_lightmap_kernel {stat([r[0] for r in rows])} ms")
            continue
        records = torch.empty((n, S, 8), dtype=torch.float32, device="cuda")

        def probes():
            t = timed(lambda: lib.rt_probe_trace(d, C.byref(pp), n, positions.data_ptr(), records.data_ptr(), sp))
            return t, rt.get_probe_counters()

        img = abi.Image()
        arr = np.zeros((H, W, 3), np.uint8)
        img.components, img.pixel_type, img.width, img.stride, img.height = 3, 0, W, W, H
        img.pixels.data, img.pixels.len = arr.ctypes.data, arr.size

        def reference():
            lib.rt_set_seed(SEED)
            t0 = time.perf_counter()
            lib.lightmap_bake(C.byref(img), C.byref(hs.scene), S)
            return (time.perf_counter() - t0) * 1e3

        ra, rb, rc = [], [], []
        for k in range(rounds + 2):
            a = reference() if k < a_rounds + 2 else None
            if a is not None:
                print(f"  {name} {S} round {k}: (a) {a:.1f} ms", flush=True)      # (a long (a) must not look like a hang)
            b = hdr()
            c = probes()
            print(f"  {name} {S} round {k}: (b) {b[0]:.3f} + {b[1]:.3f} ms, (c) {c[0]:.3f} ms", flush=True)
            if k >= 2:
                rb.append(b), rc.append(c)
                if a is not None:
                    ra.append(a)
        del records
        lc, pc = rb[-1][2], rc[-1][1]
        tb = [r[0] + r[1] for r in rb]
        tr = [r[0] for r in rb]
        tc = [r[0] for r in rc]
        g_b = lc.rays / (statistics.median(tr) * 1e-3) / 1e9
        g_c = pc.rays / (statistics.median(tc) * 1e-3) / 1e9
        emit()
        emit(f"### {name}, {S} samples: {paths} paths")
        emit()
        emit("| call | ms | paths | rays | node visits | leaf visits | shades | backgrounds | G rays / s |")
        emit("|---|---|---|---|---|---|---|---|---|")
        emit(f"| (a) lightmap_bake, host call, {len(ra)} rounds | {stat(ra)} | | | | | | | |")
        emit(f"| (b) rt_lightmap_trace + rt_lightmap_resolve | {stat(tb)} | | | | | | | |")
        emit(f"| (b) rt_lightmap_kernel alone | {stat(tr)} | {lc.paths} | {lc.rays} | {lc.node_visits} | {lc.leaf_visits} | {lc.shades} | {lc.backgrounds} | {g_b:.3f} |")
        emit(f"| (b) rt_lightmap_resolve alone | {stat([r[1] for r in rb])} | | | | | | | |")
        emit(f"| (c) rt_probe_trace, same origins | {stat(tc)} | {pc.paths} | {pc.rays} | {pc.node_visits} | {pc.leaf_visits} | {pc.shades} | {pc.backgrounds} | {g_c:.3f} |")
        emit()
        emit(f"(a) / (b): {(statistics.median(ra) if ra else float('nan')) / statistics.median(tb):.2f};  rays per second (b) / (c): {g_b / g_c:.3f};  "
             f"per path (b): {lc.rays / lc.paths:.2f} rays, {lc.node_visits / lc.paths:.1f} node visits, {lc.leaf_visits / lc.paths:.1f} leaf visits;  "
             f"(c): {pc.rays / pc.paths:.2f} rays, {pc.node_visits / pc.paths:.1f} node visits, {pc.leaf_visits / pc.paths:.1f} leaf visits")
    if not trace_only:
        t_dil = [timed(lambda: lib.rt_lightmap_dilate(W, H, 1, image.data_ptr(), work.data_ptr(), sp)) for _ in range(rounds + 2)][2:]
        emit()
        emit(f"rt_lightmap_dilate, one pass (one kernel and the copy back): {stat(t_dil)} ms")
        emit()
    del sums, texels, owner, image, work
    lib.rt_scene_release(d)
