#!/usr/bin/env python3
"""GPU experiment: the adaptive frame (rt_render_adaptive) against plain frames (rt_render_frame) of the same scene.

Setup: helmet 1920 x 1080, 8 bounces, min 16 / max 256 samples, three thresholds; scene resident, the u8 image copied to the host
on both sides (and, on the adaptive side, the chunks' sample counts: a few KB).  Per setting:
  * whole-call time by host clock, median and min - max of `reps` calls after a warm-up, the settings taken in turn within every
    repetition so that a drift of the machine hits all of them;
  * the share of paths traced: rt_get_counters().paths over width x height x 256, the launches of the frame, and the library's own
    HIP-event time of its path-kernel launches (rt_kernel_timing_mean_ms x launches) -- what is left of the call is the merges, the
    resolve, the copies, the host's decisions and the synchronisations between the rounds;
  * the RMS error of the linear frame, clamped at 1 as the output stage clamps it, against a plain frame of 4096 samples.
Beside them: rt_render_frame at 256 samples and, per threshold, at the plain sample count nearest to the adaptive frame's paths per
pixel and, once the times are known, at the plain sample count that takes the adaptive frame's TIME (256 x its median over the
256-sample frame's).  Every launch of the path kernel ends with its tail: the adaptive frame pays it once per
launch.
Writes a markdown table.

    python tools/exp_adaptive.py [out.md] [reps] [--quick]"""
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
from raytracing_c_amd.render import get_counters        # noqa: E402
from raytracing_c_amd.scene import make_image           # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
quick = "--quick" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "adaptive_table.md")
reps = int(args[1]) if len(args) > 1 else 9
W, H, BOUNCES, MIN, MAX, REF = 1920, 1080, 8, 16, 256, 4096
THRESHOLDS = [0.01, 0.02, 0.04]
if quick:
    W, H, REF, reps = 480, 270, 512, 2

assert rt.lib.rt_init(0) == 0, rt.last_error()
hs, _ = load_config("helmet")
rt.lib.rt_set_seed(0x1234ABCD)
pixels = np.zeros((H, W, 3), np.uint8)
image, _keep = make_image(pixels)
image.pixels.data = pixels.ctypes.data
n_chunks = rt.lib.rt_chunk_count(W, H)
counts = np.zeros(n_chunks, np.int32)


def plain(samples, linear=None):
    assert rt.lib.rt_render_frame(C.byref(hs.scene), C.byref(image), samples, BOUNCES, None if linear is None else linear.ctypes.data,
                                  None) == 0, rt.last_error()


def adaptive(threshold, linear=None):
    ap = abi.RT_Adaptive_Params(MIN, MAX, threshold, 0)
    assert rt.lib.rt_render_adaptive(C.byref(hs.scene), C.byref(image), C.byref(ap), BOUNCES,
                                     None if linear is None else linear.ctypes.data, None, counts.ctypes.data) == 0, rt.last_error()


def rms(linear, ref):
    d = np.minimum(linear, 1.0).astype(np.float64) - ref
    return float(np.sqrt(np.mean(d * d)))


lin = np.zeros((H, W, 3), np.float32)
plain(REF, lin)
ref = np.minimum(lin, 1.0).astype(np.float64)

def describe_plain(samples, label):
    plain(samples)
    rt.lib.rt_kernel_timing_reset()
    plain(samples, lin)
    n = C.c_int32(0)
    mean = rt.lib.rt_kernel_timing_mean_ms(C.byref(n))
    paths = get_counters().paths
    info = dict(paths=paths, share=paths / (W * H * MAX), launches=n.value, kernel_ms=mean * n.value, rms=rms(lin, ref), hist={samples: n_chunks})
    return (label % samples, (lambda s=samples: plain(s)), info)


def timed(group):
    out = [[] for _ in group]
    for rep in range(reps):
        for i, (_, call, _) in enumerate(group):
            t0 = time.perf_counter()
            call()                                       # (blocking: returns with the image on the host)
            out[i].append((time.perf_counter() - t0) * 1e3)
    return out


# what every setting is, once: paths, launches, kernel time of one call, error
settings = []                                            # (label, call, dict)
for thr in THRESHOLDS:
    adaptive(thr)                                        # (warm-up: buffers, code objects)
    rt.lib.rt_kernel_timing_reset()
    adaptive(thr, lin)
    n = C.c_int32(0)
    mean = rt.lib.rt_kernel_timing_mean_ms(C.byref(n))
    paths = get_counters().paths
    hist = {int(v): int((counts == v).sum()) for v in sorted(set(counts.tolist()))}
    info = dict(paths=paths, share=paths / (W * H * MAX), launches=n.value, kernel_ms=mean * n.value, rms=rms(lin, ref), hist=hist)
    settings.append(("adaptive %d / %d, threshold %g" % (MIN, MAX, thr), (lambda t=thr: adaptive(t)), info))
plain_counts = [MAX] + [max(1, round(s[2]["paths"] / (W * H))) for s in settings]
for samples in plain_counts:
    settings.append(describe_plain(samples, "rt_render_frame, %d samples"))
times = timed(settings)

# the plain frames of equal TIME, now that the times are known
t_full = statistics.median(times[len(THRESHOLDS)])
equal = [describe_plain(max(1, round(MAX * statistics.median(times[i]) / t_full)), "rt_render_frame, %%d samples (the time of threshold %g)" % thr)
         for i, thr in enumerate(THRESHOLDS)]
times += timed(equal)
settings += equal

lines = ["| setting | call ms, median (min - max) | path-kernel ms | launches | paths, share of %d spp | paths / pixel | RMS error vs %d spp | chunks per final count |" % (MAX, REF),
         "|---|---|---|---|---|---|---|---|"]
for (label, _, info), t in zip(settings, times):
    lines.append("| %s | %.2f (%.2f - %.2f) | %.2f | %d | %.1f %% | %.1f | %.5f | %s |" % (
        label, statistics.median(t), min(t), max(t), info["kernel_ms"], info["launches"], 100.0 * info["share"], info["paths"] / (W * H),
        info["rms"], ", ".join("%d: %d" % kv for kv in info["hist"].items())))
text = "helmet %d x %d, %d bounces, %d repetitions per setting, taken in turn\n\n" % (W, H, BOUNCES, reps) + "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
