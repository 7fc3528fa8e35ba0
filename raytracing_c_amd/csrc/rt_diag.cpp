// rt_diag.cpp -- the host side of what only librt_hip_diag.so has (-DRT_DIAG_VARIANTS, include/rt_hip_diag.h).

#include "rt_host.h"

#include <cmath>
#include <vector>

#include "../../include/rt_math.h"      // rt_dot3: the texture coordinates a hit interpolates, as the device computes them
#include "../../include/rt_hip_diag.h"

#ifndef RT_DIAG_VARIANTS
#error rt_diag.cpp belongs to the diagnostic library only (-DRT_DIAG_VARIANTS)
#endif

// unit-test kernels (rt_kernels_test.hip) and the wavefront pipeline (rt_wavefront.hip)
extern "C" {
int rt_launch_test_math(int op, int n, const float *x, const float *y, float *out, hipStream_t stream);
int rt_launch_test_rcp_sweep(unsigned long long *counts, hipStream_t stream);
int rt_launch_test_srgb_sweep(unsigned long long *counts, hipStream_t stream);
int rt_launch_test_env_sweep(int which, uint32_t seed, unsigned long long *counts, hipStream_t stream);
int rt_launch_test_quantize_sweep(unsigned long long *counts, hipStream_t stream);
int rt_launch_test_encode_sweep(unsigned long long *counts, hipStream_t stream);
int rt_launch_test_sky_add_group(void);
int rt_launch_test_group_sum(int group, int n_waves, const unsigned long long *in, const unsigned char *valid, unsigned long long *out,
                              hipStream_t stream);
int rt_launch_test_node_order(int n, const uint32_t *t_min, const unsigned char *cand, uint32_t *out, hipStream_t stream);
int rt_launch_test_trace(const RT_KParams *P, int n, const float *rays, float *out_t, int *out_tri, float *out_uv,
                         hipStream_t stream);
int rt_launch_test_trace_stream(const RT_KParams *P, int n, const float *rays, const float *pyr, int exit_lanes, int n_blocks,
                                int smem_bytes, float *out_t, int *out_tri, float *out_uv, unsigned long long *visits,
                                hipStream_t stream);
int rt_launch_test_texture(const RT_KParams *P, int tex, int n, const float *uv, float *out, hipStream_t stream);
int rt_launch_test_shade(const RT_KParams *P, int lds, int n, const int *tri, const float *in, const uint32_t *state_in, float *out,
                         uint32_t *state_out, int *terminate, int *textured, hipStream_t stream);
int rt_launch_test_shade_hit(const RT_KParams *P, int mode, int n, const int *tri, const float *hit, const float *ray, const float *carry,
                             const uint32_t *state_in, const int *bounce_in, float *out, uint32_t *iout, hipStream_t stream);
int rt_launch_test_feature_hit(const RT_KParams *P, int n, const int *tri, const float *hit, const float *ray, float *out, int *flag,
                               hipStream_t stream);
int rt_launch_test_brdf(int n, const float *params, const float *in_dir, const uint32_t *state_in, float *out_dir, float *brdf,
                        uint32_t *state_out, hipStream_t stream);
int rt_launch_test_background(const RT_KParams *P, int mode, int n, const float *dir, float *rgb, hipStream_t stream);
int rt_launch_test_primary_ray(const RT_KParams *P, int n, const int *xys, float *rays, hipStream_t stream);
int rt_wf_launch_camera(const RT_KParams *P, int n_blocks, int geometry, int smem_bytes, hipStream_t stream);
int rt_wf_launch_trace(const RT_KParams *P, int n_blocks, int geometry, int smem_bytes, hipStream_t stream);
int rt_wf_launch_shade(const RT_KParams *P, int n_blocks, int first, hipStream_t stream);
}

// 0 = tile-stream path kernel (the product's ONE kernel), 1 = wavefront pipeline (rt_wavefront.hip:
// same images and counters, measured slower on every BASELINE config -- profiles/r03_experiments.md -- kept for measurements)
std::atomic<int>            g_pipeline{0};
static std::atomic<int64_t> g_wf_cap_records{(int64_t)96 << 20};

extern "C" int rt_set_pipeline(i32 pipeline) {
  if (pipeline != 0 && pipeline != 1) return rt_fail("rt_set_pipeline: %d is not 0 (tile stream) or 1 (wavefront)", pipeline);
  g_pipeline.store(pipeline);
  return 0;
}
extern "C" i32 rt_get_pipeline(void) { return g_pipeline.load(); }
extern "C" void rt_set_wavefront_capacity(i64 records) {
  if (records >= 1024) g_wf_cap_records.store(records);
}

// A test process that has both libraries mapped builds its scenes with the product's token addresses (rt_host.cpp)
extern "C" void rt_diag_set_tokens(void *disney, void *debug, void *background) {
  if (disney) g_tok_disney = (Shader_Proc)disney;
  if (debug) g_tok_debug = (Shader_Proc)debug;
  if (background) g_tok_background = (Background_Proc)background;
}

// ---- wavefront pipeline (rt_wavefront.hip; diagnostic library only) --------------------------------------------------
// Camera kernel -> (shade, trace) per bounce, joined by record queues in HBM.  The queues are sized for `cap` camera-ray
// hits per pass (grown on demand, never beyond rt_set_wavefront_capacity() records); a frame with more first hits than
// that takes several passes: the camera kernel stops taking units when its hit queue is nearly full, the bounces run, and
// the host -- which reads one control word after every pass -- launches it again; tile_next / work_head keep the position.
static int wavefront_ensure_queues(RT_Device_Scene *d, int64_t paths, int cam_waves, int max_waves) {
  const int64_t cap = g_wf_cap_records.load();
  const int64_t want = paths < cap ? paths : cap;
  // chunks: a closed chunk holds at least WF_CHUNK - 63 records; every wave leaves one open chunk behind
  const int64_t fill = WF_CHUNK - 63;
  const int64_t soft = (want + fill - 1) / fill + cam_waves + 1;
  if (d->wf_ctl && d->wf_soft0 >= soft && d->wf_waves >= max_waves) return 0;
  d->wf_hit0.reset(); d->wf_hit.reset(); d->wf_ray[0].reset(); d->wf_ray[1].reset(); d->wf_cnt.reset(); d->wf_ctl.reset();
  d->wf_soft0 = 0;
  const int64_t hard = soft + 2 * (int64_t)cam_waves + 8;                      // a stopped wave closes at most two more chunks
  const int64_t ray_chunks = (hard * WF_CHUNK + fill - 1) / fill + max_waves + 8;   // rays <= hits
  const int64_t hit_chunks = (ray_chunks * WF_CHUNK + fill - 1) / fill + max_waves + 8;   // hits <= rays
  HIP_TRY(d->wf_hit0.grow((size_t)hard * WF_HIT0_FIELDS * WF_CHUNK));
  HIP_TRY(d->wf_hit.grow((size_t)hit_chunks * WF_HIT_FIELDS * WF_CHUNK));
  HIP_TRY(d->wf_ray[0].grow((size_t)ray_chunks * WF_RAY_FIELDS * WF_CHUNK));
  HIP_TRY(d->wf_ray[1].grow((size_t)ray_chunks * WF_RAY_FIELDS * WF_CHUNK));
  HIP_TRY(d->wf_cnt.grow((size_t)(hard + hit_chunks + 2 * ray_chunks)));
  HIP_TRY(d->wf_ctl.grow((size_t)WF_N_CTL * WF_CTL_STRIDE));
  HIP_TRY(d->wf_ctl_host.grow((size_t)WF_N_CTL * WF_CTL_STRIDE));
  d->wf_soft0 = soft; d->wf_hard0 = hard; d->wf_ray_chunks = ray_chunks; d->wf_hit_chunks = hit_chunks;
  d->wf_waves = max_waves;
  return 0;
}

// K: filled for the tile-stream kernel (units, tile counters, schedule feedback)
int launch_wavefront(Device &D, RT_Device_Scene *d, RT_KParams &K, hipStream_t stream) {
  if (K.width > 65535 || K.height > 65535) return rt_fail("the wavefront pipeline packs a pixel into 16 + 16 bits: %dx%d is too large", K.width, K.height);
  int geometry = knob_int("RT_WF_GEOMETRY", 0);
  if (geometry < 0 || geometry > 2) geometry = 0;
  int geometry_cam = knob_int("RT_WF_GEOMETRY_CAM", geometry);
  if (geometry_cam < 0 || geometry_cam > 2) geometry_cam = 0;
  static const int wpb_of[3] = {16, 12, 10}, bpc_of[3] = {1, 2, 2};
  const int wpb_cam = wpb_of[geometry_cam], bpc_cam = bpc_of[geometry_cam], wpb_tr = wpb_of[geometry], bpc_tr = bpc_of[geometry];
  const int cam_blocks = D.num_cus * bpc_cam, cam_waves = cam_blocks * wpb_cam;
  const int tr_blocks = D.num_cus * bpc_tr, tr_waves = tr_blocks * wpb_tr;
  int shade_blocks_per_cu = knob_int("RT_WF_SHADE_BLOCKS", 5);
  if (shade_blocks_per_cu < 1 || shade_blocks_per_cu > 8) shade_blocks_per_cu = 5;
  const int shade_blocks = D.num_cus * shade_blocks_per_cu, shade_waves = shade_blocks * 4;
  const int max_waves = std::max(std::max(cam_waves, tr_waves), shade_waves);
  // per wave the perm stack and the accumulator tile; the CU's whole LDS is shared out (these launches never counted the table)
  LdsSplit S_cam = lds_split(d, K.depth, wpb_cam, RT_LDS_ACC_TILE_BYTES, bpc_cam, false);
  LdsSplit S_trace = lds_split(d, K.depth, wpb_tr, RT_LDS_ACC_TILE_BYTES, bpc_tr, false);
  S_cam.cap(knob_int("RT_LDS_NODES", -1));
  S_trace.cap(knob_int("RT_LDS_NODES", -1));
  const int n_lds_cam = S_cam.n_lds_nodes, n_lds_trace = S_trace.n_lds_nodes, smem_cam = S_cam.smem, smem_trace = S_trace.smem;

  const int64_t paths = (int64_t)K.n_tiles * 64 * (K.sample_end - K.sample_first);
  if (wavefront_ensure_queues(d, paths, cam_waves, max_waves) != 0) return -1;
  K.wf_hit0 = d->wf_hit0; K.wf_hit = d->wf_hit; K.wf_ray[0] = d->wf_ray[0]; K.wf_ray[1] = d->wf_ray[1];
  K.wf_cnt_hit0 = d->wf_cnt;
  K.wf_cnt_hit = d->wf_cnt + d->wf_hard0;
  K.wf_cnt_ray[0] = K.wf_cnt_hit + d->wf_hit_chunks;
  K.wf_cnt_ray[1] = K.wf_cnt_ray[0] + d->wf_ray_chunks;
  K.wf_ctl = d->wf_ctl;
  K.wf_soft_chunks = (int32_t)(d->wf_soft0 > 0x7fffffff ? 0x7fffffff : d->wf_soft0);
  K.park = nullptr;
  HIP_TRY(hipMemsetAsync(d->wf_ctl, 0, (size_t)WF_N_CTL * WF_CTL_STRIDE * 4, stream));

  for (int pass = 0; pass < (1 << 20); pass++) {
    if (pass > 0) HIP_TRY(hipMemsetAsync(d->wf_ctl + WF_STOPPED * WF_CTL_STRIDE, 0, 4, stream));
    K.n_lds_nodes = n_lds_cam;
    K.pyr_nodes = knob_int("RT_PYRAMID", 1) ? n_lds_cam : 0;
    K.wf_n_waves = cam_waves;
    int rc = rt_wf_launch_camera(&K, cam_blocks, geometry_cam, smem_cam, stream);
    if (rc != 0) return rt_fail("camera kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    for (int b = 0; b < K.max_bounces; b++) {
      K.wf_bounce = b;
      K.wf_n_waves = shade_waves;
      rc = rt_wf_launch_shade(&K, shade_blocks, b == 0, stream);
      if (rc != 0) return rt_fail("shade kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
      if (b + 1 >= K.max_bounces) break;
      K.wf_bounce = b + 1;
      K.wf_n_waves = tr_waves;
      K.n_lds_nodes = n_lds_trace;
      rc = rt_wf_launch_trace(&K, tr_blocks, geometry, smem_trace, stream);
      if (rc != 0) return rt_fail("trace kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
      if (b >= 7 && (b & 3) == 3) {
        // long bounce limits: most paths have ended long before; every fourth bounce look at the hit queue the next shade
        // kernel would read and stop launching when a whole bounce produced no hit
        HIP_TRY(hipMemcpyAsync(d->wf_ctl_host, d->wf_ctl, (size_t)WF_N_CTL * WF_CTL_STRIDE * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (d->wf_ctl_host[WF_HIT_ALLOC * WF_CTL_STRIDE] == 0) break;
      }
    }
    HIP_TRY(hipMemcpyAsync(d->wf_ctl_host, d->wf_ctl, (size_t)WF_N_CTL * WF_CTL_STRIDE * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (d->wf_ctl_host[WF_STOPPED * WF_CTL_STRIDE] == 0) break;
  }
  return 0;
}

// fault injection for tests/test_gpu_multi_device.py (diagnostic library only): bit 0 = pretend no device has peer access
// to slot 0 (staged tile copies), bits 8.. = 1 + the slot whose frame fails
static std::atomic<int> g_multi_fault{0};
extern "C" void rt_diag_multi_fault(i32 no_peer, i32 failing_slot) {
  g_multi_fault.store((no_peer ? 1 : 0) | ((failing_slot >= 0 ? failing_slot + 1 : 0) << 8));
}
bool fault_no_peer() { return (g_multi_fault.load() & 1) != 0; }
bool fault_fails(int slot) { return (g_multi_fault.load() >> 8) == slot + 1; }

// Block ledger of a -DRT_LEDGER build of the tile-stream kernel (LG_* slots, rt_dev.hip.h): out[0 .. n) = counters[RT_CNT_LEDGER .. + n).
extern "C" int rt_get_ledger(u64 *out, i32 n) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0 || !out || n < 0 || n > RT_CNT_LEDGER_SLOTS) return -1;
  unsigned long long c[RT_N_COUNTERS];
  if (read_counters(D, c) != 0) return -1;
  for (int i = 0; i < n; i++) out[i] = c[RT_CNT_LEDGER + i];
  return 0;
}

// RT_WAVE_TIMES: per wave of the last launch its start time, end time (100 MHz ticks) and (time of its last grab - start) << 16 |
// tiles it owned.  Returns the number of waves written.
extern "C" int rt_get_wave_times(u64 *out, i32 max_waves) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0 || !out || !D.ws.wave_times) return -1;
  int n = D.ws.wave_times_n < max_waves ? D.ws.wave_times_n : max_waves;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, D.ws.wave_times, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
  return n;
}

// Device bytes the library's owners hold right now (rt_mem.h): what a test compares before and after to see a leak exactly.
extern "C" int64_t rt_diag_device_bytes_live(void) { return g_device_bytes_live.load(); }

// The staging part of a slot's teardown (remap_device_slots, rt_partition.cpp) on slot 0, which is never torn down.
extern "C" int rt_diag_release_staging(void) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  HIP_TRY(hipDeviceSynchronize());
  release_staging(D);
  return 0;
}

// The primary device's cached copy of `scene` (NULL: none) -- the copy scene_refit_gpu deforms and rt_scene_keep_geometry
// snapshots -- so that a test can run the device-level calls on it.  The cache still owns it.
extern "C" RT_Device_Scene *rt_diag_cached_scene(Scene const *scene) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  auto it = D.scene_cache.find(scene);
  return it == D.scene_cache.end() ? nullptr : it->second;
}

// ---------------------------------------------------------------------------------
// unit-level device entry points (include/rt_hip_diag.h; diagnostic library only)

extern "C" int rt_test_math(i32 op, i32 n, f32 const *x, f32 const *y, f32 *out) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (n <= 0 || !x || !out) return rt_fail("rt_test_math: bad arguments");
  DevMem<float> dx, dy, dout;
  size_t bytes = (size_t)n * sizeof(float);
  HIP_TRY(dx.grow((size_t)n));
  HIP_TRY(dout.grow((size_t)n));
  HIP_TRY(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
  if (y) {
    HIP_TRY(dy.grow((size_t)n));
    HIP_TRY(hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice));
  }
  int rc = rt_launch_test_math(op, n, dx, dy, dout, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_math failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

static int run_sweep(int (*launch)(unsigned long long *, hipStream_t), const char *name, u64 *out, int n_out) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (!out) return rt_fail("%s: NULL", name);
  DevMem<unsigned long long> b;
  HIP_TRY(b.grow((size_t)n_out));
  HIP_TRY(hipMemset(b, 0, (size_t)n_out * sizeof(unsigned long long)));
  int rc = launch(b, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, b, (size_t)n_out * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("%s failed: %s", name, hipGetErrorString((hipError_t)rc));
  return 0;
}

// rcp_exact() (the six-instruction reciprocal of the leaf blocks) against the IEEE quotient over all 2^32 bit patterns:
// out[0] differing patterns inside its domain (must be 0), out[1] patterns outside the domain, out[2] differing ones
// among those, out[3] first differing pattern inside the domain + 1; out[4], out[5]: the same for rcp_leaf() (rt_hip_diag.h).
extern "C" int rt_test_rcp_sweep(u64 out[6]) { return run_sweep(rt_launch_test_rcp_sweep, "rt_test_rcp_sweep", out, 6); }

// The kernels' sRGB decode of a texture sample (division by 1.055 as a corrected multiplication) against
// rt_srgb_to_linear1() for every float in [0, 2] (and 4 M negative ones): out[0] patterns compared, out[1] differing (0 expected),
// out[2] first differing pattern + 1.
extern "C" int rt_test_srgb_sweep(u64 out[3]) { return run_sweep(rt_launch_test_srgb_sweep, "rt_test_srgb_sweep", out, 3); }

// The short forms of the environment lookup and the normalisations (atan_pos_dev, asin_dev, inv_sqrt_exact, the background's
// coordinates without the negative wrap, sqrt_dev: which = 0 .. 5) against the rt_math.h functions over all 2^32 bit patterns, and
// atan2_dev against rt_atan2f on 2^26 pairs drawn from `seed` (which = 6): out[0] patterns or pairs compared, out[1] differing
// (0 expected), out[2] first differing pattern or pair index + 1, out[3] differing when a NaN must keep its bits (rt_hip_diag.h).
extern "C" int rt_test_env_sweep(i32 which, u32 seed, u64 out[4]) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (which < 0 || which > 6 || !out) return rt_fail("rt_test_env_sweep: bad arguments");
  DevMem<unsigned long long> b;
  HIP_TRY(b.grow(4));
  HIP_TRY(hipMemset(b, 0, 4 * sizeof(unsigned long long)));
  int rc = rt_launch_test_env_sweep(which, seed, b, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, b, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_env_sweep failed: %s", hipGetErrorString((hipError_t)rc));
  if (out[2]) out[2] = 0x100000000ull - out[2] + 1;          // the kernel keeps 2^32 - the lowest differing pattern
  return 0;
}

// The tile-stream kernel's shift-based fixed-point conversion of a sample against rt_accum_quantize() over all 2^32 bit
// patterns: out[0] differing patterns (0 expected), out[1] first differing pattern + 1.
extern "C" int rt_test_quantize_sweep(u64 out[2]) { return run_sweep(rt_launch_test_quantize_sweep, "rt_test_quantize_sweep", out, 2); }

// rt_encode_u8() on the device over all 2^32 bit patterns (rt_hip_diag.h): out[0 .. 255] the lowest pattern of [0, 0x3F800000] per
// byte (2^32: the byte does not occur), out[256] descents over that range, out[257 .. 259] patterns above 1.0 that do not give 255,
// negative ones and NaNs that do not give 0.
extern "C" int rt_test_encode_sweep(u64 out[260]) {
  if (int rc = run_sweep(rt_launch_test_encode_sweep, "rt_test_encode_sweep", out, 260)) return rc;
  for (int k = 0; k < 256; k++) out[k] = 0x100000000ull - out[k];       // the kernel keeps 2^32 - the lowest pattern, 0 = none
  return 0;
}

// The sky loop's sample reduction on crafted lanes (rt_hip_diag.h): three channels of n_waves x 64 values, out[c * n + i] = the sum of
// channel c over lane i's aligned group of `group` lanes.
extern "C" int rt_test_group_sum(i32 group, i32 n_waves, u64 const *in, u8 const *valid, u64 *out) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if ((group != 4 && group != 16 && group != 64) || n_waves <= 0 || n_waves > 65535 || !in || !valid || !out)
    return rt_fail("rt_test_group_sum: bad arguments");
  const size_t n = (size_t)n_waves * 64;
  DevMem<unsigned long long> din, dout;
  DevMem<unsigned char> dvalid;
  HIP_TRY(din.grow(3 * n));
  HIP_TRY(dout.grow(3 * n));
  HIP_TRY(dvalid.grow(n));
  HIP_TRY(hipMemcpy(din, in, 3 * n * sizeof(u64), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dvalid, valid, n, hipMemcpyHostToDevice));
  int rc = rt_launch_test_group_sum(group, n_waves, din, dvalid, dout, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, dout, 3 * n * sizeof(u64), hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_group_sum failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_test_sky_add_group(void) { return rt_launch_test_sky_add_group(); }

// The two orderings of a node block's children on crafted distances (rt_hip_diag.h): n cases of eight entry distances (bit patterns)
// and eight candidate flags; out[3 i ..] = the word from the keys, the word from the rank sort, 1 when the keys are not exact.
extern "C" int rt_test_node_order(i32 n, u32 const *t_min, u8 const *cand, u32 *out) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (n <= 0 || n > (1 << 24) || !t_min || !cand || !out) return rt_fail("rt_test_node_order: bad arguments");
  DevMem<uint32_t> dt, dout;
  DevMem<unsigned char> dcand;
  HIP_TRY(dt.grow((size_t)n * 8));
  HIP_TRY(dcand.grow((size_t)n * 8));
  HIP_TRY(dout.grow((size_t)n * 3));
  HIP_TRY(hipMemcpy(dt, t_min, (size_t)n * 8 * sizeof(u32), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dcand, cand, (size_t)n * 8, hipMemcpyHostToDevice));
  int rc = rt_launch_test_node_order(n, dt, dcand, dout, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, dout, (size_t)n * 3 * sizeof(u32), hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_node_order failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// The tile order the preparation kernel derives from per-tile costs (rays of the previous launch): order[] must be a
// permutation of 0 .. n_tiles - 1 with non-increasing cost buckets (rt_kernels.hip: cost_bucket, 4 per power of two).
extern "C" int rt_test_tile_order(i32 n_tiles, u32 const *cost, u32 *order) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (n_tiles <= 0 || !cost || !order) return rt_fail("rt_test_tile_order: bad arguments");
  DevMem<uint32_t> bc, bo, bn, bw, bz;
  DevMem<unsigned long long> bk;
  HIP_TRY(bc.grow((size_t)n_tiles));
  HIP_TRY(bo.grow((size_t)n_tiles));
  HIP_TRY(bn.grow((size_t)n_tiles + (size_t)(n_tiles + 63) / 64));
  HIP_TRY(bk.grow(RT_N_COUNTERS));
  HIP_TRY(bw.grow(16));
  HIP_TRY(bz.grow((size_t)n_tiles));
  HIP_TRY(hipMemcpy(bc, cost, (size_t)n_tiles * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(bo, 0xFF, (size_t)n_tiles * 4));
  int rc = rt_launch_prepare(n_tiles, bn, bn + n_tiles, bk, bw, bz, bc, bo, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(order, bo, (size_t)n_tiles * 4, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_tile_order failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_test_trace(RT_Device_Scene *d, i32 n, f32 const *rays, f32 *out_t, i32 *out_tri, f32 *out_uv) {
  if (!d || n <= 0 || !rays || !out_t || !out_tri || !out_uv) return rt_fail("rt_test_trace: bad arguments");
  Device &D = *d->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (ensure_device(D) != 0) return -1;
  RT_KParams K;
  scene_only_kparams(&K, d);
  DevMem<float> dr, dt, duv;
  DevMem<int>   dtri;
  HIP_TRY(dr.grow((size_t)n * 6));
  HIP_TRY(dt.grow((size_t)n));
  HIP_TRY(dtri.grow((size_t)n));
  HIP_TRY(duv.grow((size_t)n * 2));
  HIP_TRY(hipMemcpy(dr, rays, (size_t)n * 24, hipMemcpyHostToDevice));
  int rc = rt_launch_test_trace(&K, n, dr, dt, dtri, duv, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out_t, dt, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(out_tri, dtri, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(out_uv, duv, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_trace failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// n rays through traversal_blocks() -- the NODE / LEAF / pop code of the path kernels -- in the path kernel's launch geometry.
//   pyramid: NULL, or 19 floats (4 outward plane normals at [4 q .. 4 q + 2], the rays' common origin at [16 .. 18]): every
//            ray is then treated as a camera ray of one tile and node blocks take the pyramid-culled form where the path
//            kernel would; the caller guarantees that every ray starts at that origin and lies inside the four planes
//   exit_lanes: 1 .. 64, how many finished lanes end a round of blocks (the path kernel's `sched_thresh`, 48)
//   mode: 0 = the instance the path kernel would choose for this scene, 1 = force the IEEE division in the leaf blocks,
//         2 = nodes from L1 / L2 instead of the LDS copy
//   visits: [0] += ray_aabbs_hit_8 equivalents, [1] += ray_triangles_hit_8 equivalents
extern "C" int rt_test_trace_stream(RT_Device_Scene *d, i32 n, f32 const *rays, f32 const *pyramid, i32 exit_lanes, i32 mode,
                                    f32 *out_t, i32 *out_tri, f32 *out_uv, u64 visits[2]) {
  if (!d || n <= 0 || !rays || !out_t || !out_tri || !out_uv || !visits) return rt_fail("rt_test_trace_stream: bad arguments");
  if (exit_lanes < 1 || exit_lanes > 64) return rt_fail("rt_test_trace_stream: exit_lanes %d outside [1, 64]", exit_lanes);
  Device &D = *d->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (ensure_device(D) != 0) return -1;
  RT_KParams K;
  scene_only_kparams(&K, d);
  LdsSplit S = lds_split(d, K.depth, 16, RT_LDS_ACC_TILE_BYTES, 1, false);      // the path kernel's geometry, without its table
  if (mode == 2) S.cap(0);
  K.n_lds_nodes = S.n_lds_nodes;
  K.pyr_nodes = K.n_lds_nodes;
  // the short reciprocal is valid while |det| < 2^102: edges <= 2^38 (as for frames) and, here, ray directions <= 2^16
  float dir_max = 0.0f;
  for (i32 i = 0; i < n; i++)
    for (int k = 3; k < 6; k++) {
      float m = fabsf(rays[(size_t)i * 6 + k]);
      if (!(m <= dir_max)) dir_max = m;
    }
  K.short_div = (mode != 1 && d->max_edge <= 0x1p38f && dir_max <= 0x1p16f) ? 1 : 0;
  int n_blocks = (n + 16 * 64 * 4 - 1) / (16 * 64 * 4);                 // ~4 rays per lane
  if (n_blocks > D.num_cus) n_blocks = D.num_cus;
  if (n_blocks < 1) n_blocks = 1;
  DevMem<float> br, bp, bt, buv;
  DevMem<int>   btri;
  DevMem<unsigned long long> bv;
  HIP_TRY(br.grow((size_t)n * 6));
  HIP_TRY(bp.grow(19));
  HIP_TRY(bt.grow((size_t)n));
  HIP_TRY(btri.grow((size_t)n));
  HIP_TRY(buv.grow((size_t)n * 2));
  HIP_TRY(bv.grow(2));
  HIP_TRY(hipMemcpy(br, rays, (size_t)n * 24, hipMemcpyHostToDevice));
  if (pyramid) HIP_TRY(hipMemcpy(bp, pyramid, 19 * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(bv, 0, 16));
  int rc = rt_launch_test_trace_stream(&K, n, br, pyramid ? bp.get() : nullptr, exit_lanes, n_blocks, S.smem, bt, btri, buv, bv, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out_t, bt, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(out_tri, btri, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(out_uv, buv, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(visits, bv, 16, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_trace_stream failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_test_texture(RT_Device_Scene *d, i32 tex, i32 n, f32 const *uv, f32 *out_rgb) {
  if (!d || n <= 0 || !uv || !out_rgb) return rt_fail("rt_test_texture: bad arguments");
  Device &D = *d->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (ensure_device(D) != 0) return -1;
  if (tex < 0) tex = d->bg_texture;
  if (tex >= d->n_textures) return rt_fail("rt_test_texture: texture %d of %d", tex, d->n_textures);
  RT_KParams K;
  scene_only_kparams(&K, d);
  DevMem<float> duv, dout;
  HIP_TRY(duv.grow((size_t)n * 2));
  HIP_TRY(dout.grow((size_t)n * 3));
  HIP_TRY(hipMemcpy(duv, uv, (size_t)n * 8, hipMemcpyHostToDevice));
  int rc = rt_launch_test_texture(&K, tex, n, duv, dout, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out_rgb, dout, (size_t)n * 12, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_texture failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- the shade block, the BRDF sampler, the environment lookup and the camera rays on inputs a test chooses ----------
// (include/rt_hip_diag.h; compared with the oracle's unit functions by tests/test_gpu_shade.py)

static bool all_finite(f32 const *v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

extern "C" int rt_test_shade(RT_Device_Scene *d, i32 mode, i32 n, i32 const *tri, f32 const *in, u32 const *state_in, f32 *out,
                             u32 *state_out, i32 *terminate, i32 *textured) {
  if (!d || n <= 0 || !tri || !in || !state_in || !out || !state_out || !terminate || !textured) return rt_fail("rt_test_shade: bad arguments");
  if ((mode & ~RT_TEST_SHARED_TAPS) != 0 && (mode & ~RT_TEST_SHARED_TAPS) != 1)
    return rt_fail("rt_test_shade: mode %d is not 0 (ShadeParams) or 1 (ShadeParamsLds), with or without RT_TEST_SHARED_TAPS", mode);
  if ((mode & RT_TEST_SHARED_TAPS) && !rt_materials_share_taps(d->mats_host.data(), d->n_materials))
    return rt_fail("rt_test_shade: RT_TEST_SHARED_TAPS on a scene with a material whose textures differ in size");
  for (i32 i = 0; i < n; i++) {
    if (tri[i] < 0 || tri[i] >= d->n_triangles) return rt_fail("rt_test_shade: item %d names triangle slot %d of %d", i, tri[i], d->n_triangles);
    // texture coordinates index texels: finite only (a NaN converts to an index differently on the two sides)
    if (!all_finite(in + (size_t)i * 14 + 12, 2)) return rt_fail("rt_test_shade: item %d has non-finite texture coordinates", i);
  }
  Device &D = *d->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (ensure_device(D) != 0) return -1;
  RT_KParams K;
  scene_only_kparams(&K, d);
  DevMem<int> dtri, dterm, dtex;
  DevMem<float> din, dout;
  DevMem<uint32_t> ds0, ds1;
  HIP_TRY(dtri.grow((size_t)n));
  HIP_TRY(dterm.grow((size_t)n));
  HIP_TRY(dtex.grow((size_t)n));
  HIP_TRY(din.grow((size_t)n * 14));
  HIP_TRY(dout.grow((size_t)n * 9));
  HIP_TRY(ds0.grow((size_t)n));
  HIP_TRY(ds1.grow((size_t)n));
  HIP_TRY(hipMemcpy(dtri, tri, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(din, in, (size_t)n * 56, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ds0, state_in, (size_t)n * 4, hipMemcpyHostToDevice));
  int rc = rt_launch_test_shade(&K, mode, n, dtri, din, ds0, dout, ds1, dterm, dtex, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, dout, (size_t)n * 36, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(state_out, ds1, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(terminate, dterm, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(textured, dtex, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_shade failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- one path step / one feature hit on hits a test chooses (shade_hit, feature_hit; tests/test_gpu_shade_hit.py) ----------

// What both refuse, as rt_test_shade does: a slot outside the scene or without a material, vertex texture coordinates that are
// not finite, and barycentrics that carry them to a texture coordinate that is not finite (a NaN converts to a texel index
// differently on the two sides).  `rec`: the device scene's 28-float triangle records, read back.
static int check_hit_items(const char *who, RT_Device_Scene *d, const std::vector<float> &rec, i32 n, i32 const *tri, f32 const *hit) {
  for (i32 i = 0; i < n; i++) {
    if (tri[i] < 0 || tri[i] >= d->n_triangles) return rt_fail("%s: item %d names triangle slot %d of %d", who, i, tri[i], d->n_triangles);
    const float *r = &rec[(size_t)tri[i] * 28];
    int32_t mat;
    memcpy(&mat, r + 3, 4);
    if (mat < 0 || mat >= d->n_materials) return rt_fail("%s: item %d triangle slot %d names no material of the scene", who, i, tri[i]);
    const f32 ux[3] = {r[7], r[15], r[23]}, uy[3] = {r[11], r[19], r[24]};      // Surface::uvx / uvy (rt_dev.hip.h)
    if (!all_finite(ux, 3) || !all_finite(uy, 3)) return rt_fail("%s: item %d: triangle slot %d has non-finite texture coordinates", who, i, tri[i]);
    const f32 t1 = hit[(size_t)i * 3 + 1], t2 = hit[(size_t)i * 3 + 2], t0 = 1.0f - t1 - t2;
    const f32 uv[2] = {rt_dot3(ux[0], t0, ux[1], t1, ux[2], t2), rt_dot3(uy[0], t0, uy[1], t1, uy[2], t2)};
    if (!all_finite(uv, 2)) return rt_fail("%s: item %d: barycentrics (%g, %g) give non-finite texture coordinates", who, i, (double)t1, (double)t2);
  }
  return 0;
}

extern "C" int rt_test_shade_hit(RT_Device_Scene *d, i32 mode, i32 max_bounces, i32 n, i32 const *tri, f32 const *hit, f32 const *ray,
                                 f32 const *carry, u32 const *state_in, i32 const *bounce_in, f32 *out, u32 *out_words) {
  if (!d || n <= 0 || !tri || !hit || !ray || !carry || !state_in || !bounce_in || !out || !out_words) return rt_fail("rt_test_shade_hit: bad arguments");
  if ((mode < 0 || mode > 2) && mode != (0 | RT_TEST_SHARED_TAPS) && mode != (1 | RT_TEST_SHARED_TAPS))
    return rt_fail("rt_test_shade_hit: mode %d is not 0 (ShadeParams), 1 (ShadeParamsLds) or 2 (RT_KParams), nor one of the first two with RT_TEST_SHARED_TAPS", mode);
  if ((mode & RT_TEST_SHARED_TAPS) && !rt_materials_share_taps(d->mats_host.data(), d->n_materials))
    return rt_fail("rt_test_shade_hit: RT_TEST_SHARED_TAPS on a scene with a material whose textures differ in size");
  Device &D = *d->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (ensure_device(D) != 0) return -1;
  std::vector<float> rec((size_t)d->n_triangles * 28);
  HIP_TRY(hipMemcpy(rec.data(), d->tris, rec.size() * 4, hipMemcpyDeviceToHost));
  if (check_hit_items("rt_test_shade_hit", d, rec, n, tri, hit) != 0) return -1;
  RT_KParams K;
  scene_only_kparams(&K, d);
  K.max_bounces = max_bounces;
  DevMem<int> dtri, dbounce;
  DevMem<float> dhit, dray, dcarry, dout;
  DevMem<uint32_t> ds0, dwords;
  HIP_TRY(dtri.grow((size_t)n));
  HIP_TRY(dbounce.grow((size_t)n));
  HIP_TRY(dhit.grow((size_t)n * 3));
  HIP_TRY(dray.grow((size_t)n * 6));
  HIP_TRY(dcarry.grow((size_t)n * 6));
  HIP_TRY(dout.grow((size_t)n * 15));
  HIP_TRY(ds0.grow((size_t)n));
  HIP_TRY(dwords.grow((size_t)n * 5));
  HIP_TRY(hipMemcpy(dtri, tri, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dbounce, bounce_in, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dhit, hit, (size_t)n * 12, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dray, ray, (size_t)n * 24, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dcarry, carry, (size_t)n * 24, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ds0, state_in, (size_t)n * 4, hipMemcpyHostToDevice));
  int rc = rt_launch_test_shade_hit(&K, mode, n, dtri, dhit, dray, dcarry, ds0, dbounce, dout, dwords, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, dout, (size_t)n * 60, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(out_words, dwords, (size_t)n * 20, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_shade_hit failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_test_feature_hit(RT_Device_Scene *d, i32 n, i32 const *tri, f32 const *hit, f32 const *ray, f32 *out, i32 *flag) {
  if (!d || n <= 0 || !tri || !hit || !ray || !out || !flag) return rt_fail("rt_test_feature_hit: bad arguments");
  Device &D = *d->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (ensure_device(D) != 0) return -1;
  std::vector<float> rec((size_t)d->n_triangles * 28);
  HIP_TRY(hipMemcpy(rec.data(), d->tris, rec.size() * 4, hipMemcpyDeviceToHost));
  if (check_hit_items("rt_test_feature_hit", d, rec, n, tri, hit) != 0) return -1;
  RT_KParams K;
  scene_only_kparams(&K, d);
  DevMem<int> dtri, dflag;
  DevMem<float> dhit, dray, dout;
  HIP_TRY(dtri.grow((size_t)n));
  HIP_TRY(dflag.grow((size_t)n));
  HIP_TRY(dhit.grow((size_t)n * 3));
  HIP_TRY(dray.grow((size_t)n * 6));
  HIP_TRY(dout.grow((size_t)n * 12));
  HIP_TRY(hipMemcpy(dtri, tri, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dhit, hit, (size_t)n * 12, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dray, ray, (size_t)n * 24, hipMemcpyHostToDevice));
  int rc = rt_launch_test_feature_hit(&K, n, dtri, dhit, dray, dout, dflag, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out, dout, (size_t)n * 48, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(flag, dflag, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_feature_hit failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_test_brdf(i32 n, f32 const *params, f32 const *in_dir, u32 const *state_in, f32 *out_dir, f32 *brdf, u32 *state_out) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (n <= 0 || !params || !in_dir || !state_in || !out_dir || !brdf || !state_out) return rt_fail("rt_test_brdf: bad arguments");
  DevMem<float> dp, di, dout, db;
  DevMem<uint32_t> ds0, ds1;
  HIP_TRY(dp.grow((size_t)n * 8));
  HIP_TRY(di.grow((size_t)n * 3));
  HIP_TRY(dout.grow((size_t)n * 3));
  HIP_TRY(db.grow((size_t)n * 4));
  HIP_TRY(ds0.grow((size_t)n));
  HIP_TRY(ds1.grow((size_t)n));
  HIP_TRY(hipMemcpy(dp, params, (size_t)n * 32, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(di, in_dir, (size_t)n * 12, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ds0, state_in, (size_t)n * 4, hipMemcpyHostToDevice));
  int rc = rt_launch_test_brdf(n, dp, di, ds0, dout, db, ds1, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(out_dir, dout, (size_t)n * 12, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(brdf, db, (size_t)n * 16, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(state_out, ds1, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_brdf failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_test_background(RT_Device_Scene *d, i32 mode, i32 n, f32 const *dir, f32 *rgb) {
  if (!d || n <= 0 || !dir || !rgb) return rt_fail("rt_test_background: bad arguments");
  if ((mode & ~RT_TEST_BG_IMAGE) != 0 && (mode & ~RT_TEST_BG_IMAGE) != 1)
    return rt_fail("rt_test_background: mode %d is not 0 (ShadeParams) or 1 (ShadeParamsLds), with or without RT_TEST_BG_IMAGE", mode);
  Device &D = *d->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (ensure_device(D) != 0) return -1;
  RT_KParams K;
  scene_only_kparams(&K, d);
  DevMem<float> dd, dout;
  HIP_TRY(dd.grow((size_t)n * 3));
  HIP_TRY(dout.grow((size_t)n * 3));
  HIP_TRY(hipMemcpy(dd, dir, (size_t)n * 12, hipMemcpyHostToDevice));
  int rc = rt_launch_test_background(&K, mode, n, dd, dout, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(rgb, dout, (size_t)n * 12, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_background failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_test_primary_ray(Camera const *camera, i32 width, i32 height, i32 n, i32 const *xys, f32 *rays) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (!camera || width < 1 || height < 1 || n <= 0 || !xys || !rays) return rt_fail("rt_test_primary_ray: bad arguments");
  RT_KParams K;
  memset(&K, 0, sizeof K);
  RT_Render_Params p;
  memset(&p, 0, sizeof p);
  p.width = width; p.height = height; p.samples = 1; p.max_bounces = 1;
  camera_frame_kparams(&K, camera, &p);          // the host's own three divisions, not a copy of them
  DevMem<int> dx;
  DevMem<float> dr;
  HIP_TRY(dx.grow((size_t)n * 3));
  HIP_TRY(dr.grow((size_t)n * 6));
  HIP_TRY(hipMemcpy(dx, xys, (size_t)n * 12, hipMemcpyHostToDevice));
  int rc = rt_launch_test_primary_ray(&K, n, dx, dr, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(rays, dr, (size_t)n * 24, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("rt_test_primary_ray failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}
