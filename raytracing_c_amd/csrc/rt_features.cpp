// rt_features.cpp -- first-hit feature buffers (include/rt_hip.h): coverage, albedo, shading normal and world position of what the
// camera sees, on the device level (device pointers, one launch on the caller's stream) and on the host level (host arrays, the
// cached device copy of a Scene through scene_checked, rt_residency.cpp).  The work is rt_features_kernel and
// rt_features_resolve_kernel (rt_features.hip), and with THE MOTION rt_features_motion_kernel and rt_motion_resolve_kernel; nothing
// here computes a feature on the CPU.

#include "rt_host.h"

static_assert(RT_FEATURE_CHANNELS == 10, "coverage, albedo rgb, normal xyz, position xyz");
static_assert(RT_MOTION_CHANNELS == 3, "THE MOTION xyz");

// What can be checked without the device.  `who` prefixes the messages.
static int check_feature_params(const char *who, RT_Render_Params const *p) {
  if (!p) return rt_fail("%s: render params are NULL", who);
  if (check_image_size(who, p->width, p->height) != 0) return -1;
  if (p->samples <= 0) return rt_fail("%s: samples must be positive (got %d)", who, p->samples);
  if (p->max_bounces < 0) return rt_fail("%s: max_bounces must be >= 0 (got %d)", who, p->max_bounces);
  if (p->rank != 0 || p->world != 1) return rt_fail("%s: rank %d / world %d: a feature pass renders the whole image on one device (0 / 1)", who, p->rank, p->world);
  if (p->sample_first < 0 || p->sample_count < 0 || p->sample_first + p->sample_count > p->samples)
    return rt_fail("%s: sample range [%d, +%d) outside [0, %d)", who, p->sample_first, p->sample_count, p->samples);
  return 0;
}

// Enqueues one launch of the feature kernel on `stream` (d_motion_sums given: of the motion kernel, against d's kept geometry).
// D.mutex held, D's GPU current, every pointer on D.
static int enqueue_features(Device &D, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p, void *d_sums, hipStream_t stream,
                            void *d_motion_sums) {
  RT_KParams K;
  scene_only_kparams(&K, d);
  camera_frame_kparams(&K, cam, p);
  const int n_samples = K.sample_end - K.sample_first;
  if (n_samples <= 0 || K.max_bounces == 0) return 0;             // nothing to trace: every sample of the range is 0

  // units: 64 paths of one 8x8 tile = (64 >> shift) pixels x (1 << shift) samples (RT_FParams, rt_device.h)
  RT_FParams F;
  memset(&F, 0, sizeof F);
  int shift = 0;
  while (shift < 6 && (1 << shift) < n_samples) shift++;
  F.shift = shift;
  F.n_sample_blocks = (n_samples + (1 << shift) - 1) >> shift;
  F.units_per_tile = F.n_sample_blocks << shift;
  F.tiles_x = (p->width + RT_TILE - 1) / RT_TILE;
  const int64_t n_units = (int64_t)F.tiles_x * ((p->height + RT_TILE - 1) / RT_TILE) * F.units_per_tile;
  // (the kernel's 32-bit work counter ends at n_units plus one grab per wave)
  if (n_units > (int64_t)0x7fff0000) return rt_fail("feature pass: too many work items (%lld)", (long long)n_units);
  F.n_units = (int)n_units;
  F.sums = (unsigned long long *)d_sums;

  // launch geometry: the query kernel's (rt_query.cpp) -- one workgroup of 16 waves per CU, the tree fills the LDS beside the waves'
  // perm stacks and the kernel's static sRGB scale table
  const int wg_waves = 16;
  const LdsSplit S = lds_split(d, K.depth, wg_waves, 0, 1, true);
  K.n_lds_nodes = S.n_lds_nodes;
  int64_t blocks = (n_units + wg_waves - 1) / wg_waves;
  if (blocks > D.num_cus) blocks = D.num_cus;
  // units per grab: an eighth of a wave's mean share, within [1, 8] -- what is left when the counter runs out is one grab per wave
  int64_t grab = n_units / (blocks * wg_waves * 8);
  F.grab = grab < 1 ? 1 : (grab > 8 ? 8 : (int)grab);

  int slot = 0;
  if (ensure_query_state(D) != 0 || acquire_slot(D, &slot, false) != 0) return -1;
  uint8_t *sl = D.query.slots + (size_t)slot * 64;
  F.head = (uint32_t *)(sl + 32);
  HIP_TRY(hipMemsetAsync(F.head, 0, 4, stream));                  // (the slot's query counters stay: rt_get_query_counters)
  // (without kept geometry the current tiles serve as the kept ones: the first frame of a sequence has motion 0)
  const float *kept = d->has_kept ? d->kept_leaves.get() : d->leaves.get();
  int rc = d_motion_sums ? rt_launch_features_motion(&K, &F, kept, (unsigned long long *)d_motion_sums, (int)blocks, S.smem, stream)
                         : rt_launch_features(&K, &F, (int)blocks, S.smem, stream);
  if (rc != 0) return rt_fail("feature kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  HIP_TRY(hipEventRecord(D.query.done[slot], stream));
  return 0;
}

static int enqueue_resolve(RT_Render_Params const *p, void const *d_sums, void *d_coverage, void *d_albedo, void *d_normal,
                           void *d_position, hipStream_t stream) {
  int rc = rt_launch_features_resolve(p->width * p->height, p->samples, (const unsigned long long *)d_sums, (float *)d_coverage,
                                      (float *)d_albedo, (float *)d_normal, (float *)d_position, stream);
  if (rc != 0) return rt_fail("feature resolve kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

static int enqueue_resolve_motion(RT_Render_Params const *p, void const *d_motion_sums, void *d_motion, hipStream_t stream) {
  int rc = rt_launch_motion_resolve(p->width * p->height, p->samples, (const unsigned long long *)d_motion_sums, (float *)d_motion, stream);
  if (rc != 0) return rt_fail("motion resolve kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// THE FEATURE PASS of one frame on `stream` (rt_host.h): the sums zeroed, the one launch, the resolves that are wanted.
int enqueue_feature_pass(Device &D, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p, void *d_sums, RT_Features const &to,
                         hipStream_t stream, void *d_motion_sums, void *d_motion) {
  const size_t pixels = (size_t)p->width * p->height;
  HIP_TRY(hipMemsetAsync(d_sums, 0, pixels * RT_FEATURE_CHANNELS * sizeof(unsigned long long), stream));
  if (d_motion_sums) HIP_TRY(hipMemsetAsync(d_motion_sums, 0, pixels * RT_MOTION_CHANNELS * sizeof(unsigned long long), stream));
  if (enqueue_features(D, d, cam, p, d_sums, stream, d_motion_sums) != 0) return -1;
  if ((to.coverage || to.albedo || to.normal || to.position) &&
      enqueue_resolve(p, d_sums, to.coverage, to.albedo, to.normal, to.position, stream) != 0)
    return -1;
  return d_motion ? enqueue_resolve_motion(p, d_motion_sums, d_motion, stream) : 0;
}

// ---- device level -------------------------------------------------------------------------------------------------------------
// rt_render_accumulate_features and rt_render_accumulate_features_motion (with_motion: d_motion_sums is required)
static int accumulate_device(const char *who, bool with_motion, RT_Device_Scene *dscene, RT_Render_Params const *params, void *d_sums,
                             void *d_motion_sums, hipStream_t stream) {
  // (everything that can be checked without the device is checked before it is touched)
  if (!dscene) return rt_fail("%s: device scene is NULL", who);
  if (check_feature_params(who, params) != 0) return -1;
  if (!d_sums) return rt_fail("%s: d_sums is NULL", who);
  if (with_motion && !d_motion_sums) return rt_fail("%s: d_motion_sums is NULL", who);
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  auto it = D.cameras.find(dscene);
  if (it == D.cameras.end()) return rt_fail("%s: no camera set for this scene (rt_set_camera)", who);
  return enqueue_features(D, dscene, &it->second, params, d_sums, stream, d_motion_sums);
}

extern "C" int rt_render_accumulate_features(RT_Device_Scene *dscene, RT_Render_Params const *params, void *d_sums, void *stream) {
  return accumulate_device("rt_render_accumulate_features", false, dscene, params, d_sums, nullptr, (hipStream_t)stream);
}

extern "C" int rt_render_accumulate_features_motion(RT_Device_Scene *dscene, RT_Render_Params const *params, void *d_sums,
                                                    void *d_motion_sums, void *stream) {
  return accumulate_device("rt_render_accumulate_features_motion", true, dscene, params, d_sums, d_motion_sums, (hipStream_t)stream);
}

extern "C" int rt_resolve_motion(RT_Render_Params const *params, void const *d_motion_sums, void *d_motion, void *stream) {
  const char *who = "rt_resolve_motion";
  if (check_feature_params(who, params) != 0) return -1;
  if (!d_motion_sums) return rt_fail("%s: d_motion_sums is NULL", who);
  if (!d_motion) return rt_fail("%s: d_motion is NULL", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_resolve_motion(params, d_motion_sums, d_motion, (hipStream_t)stream);
}

extern "C" int rt_resolve_features(RT_Render_Params const *params, void const *d_sums, void *d_coverage, void *d_albedo,
                                   void *d_normal, void *d_position, void *stream) {
  const char *who = "rt_resolve_features";
  if (check_feature_params(who, params) != 0) return -1;
  if (!d_sums) return rt_fail("%s: d_sums is NULL", who);
  if (!d_coverage && !d_albedo && !d_normal && !d_position) return rt_fail("%s: no output is wanted", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_resolve(params, d_sums, d_coverage, d_albedo, d_normal, d_position, (hipStream_t)stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
// rt_render_features and rt_render_features_motion (with_motion: motion and motion_sums are two more optional outputs, and the
// pass is the motion kernel's)
static int features_host(const char *who, bool with_motion, Scene const *scene, i32 width, i32 height, isize samples, isize max_bounces,
                         RT_Features const *out, u64 *sums, f32 *motion, u64 *motion_sums) {
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (samples > 0x7fffffff || max_bounces > 0x7fffffff) return rt_fail("%s: samples / max_bounces do not fit 32 bits", who);
  RT_Render_Params p;
  memset(&p, 0, sizeof p);
  p.width = width;
  p.height = height;
  p.samples = samples < 0 ? -1 : (i32)samples;
  p.max_bounces = max_bounces < 0 ? -1 : (i32)max_bounces;
  p.world = 1;
  if (check_feature_params(who, &p) != 0) return -1;
  const bool planes = out && (out->coverage || out->albedo || out->normal || out->position);
  if (!planes && !sums && !motion && !motion_sums)
    return rt_fail(with_motion ? "%s: no output is wanted (every plane of `out`, `sums`, `motion` and `motion_sums` are NULL)"
                               : "%s: no output is wanted (every plane of `out` and `sums` are NULL)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (rt_device_count() > 1)
    return rt_fail("%s: a feature pass renders on one device, and %d are set (rt_set_devices)", who, rt_device_count());
  FeatureState &S = D.features;
  const size_t pixels = (size_t)width * height;
  HIP_TRY(S.sums.grow(pixels * RT_FEATURE_CHANNELS));
  HIP_TRY(S.planes.grow(pixels * RT_FEATURE_CHANNELS));
  if (with_motion) {
    HIP_TRY(S.motion_sums.grow(pixels * RT_MOTION_CHANNELS));
    if (motion) HIP_TRY(S.motion.grow(pixels * RT_MOTION_CHANNELS));
  }
  const RT_Features f = split_feature_planes(S.planes, pixels);
  // (only the planes the caller asked for are resolved)
  const RT_Features to = planes ? RT_Features{out->coverage ? f.coverage : nullptr, out->albedo ? f.albedo : nullptr,
                                              out->normal ? f.normal : nullptr, out->position ? f.position : nullptr}
                                : RT_Features{};
  hipStream_t stream = nullptr;                                 // (does not wait for the lane streams of frames in flight)
  auto pass = [&](RT_Device_Scene *d) -> int {
    return enqueue_feature_pass(D, d, &scene->camera, &p, S.sums, to, stream, with_motion ? S.motion_sums.get() : nullptr,
                                motion ? S.motion.get() : nullptr);
  };
  if (!scene_checked(D, scene, stream, nullptr, pass)) return -1;      // (a scene edited since the copy: uploaded and traced again)
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  if (planes) {
    if (out->coverage) HIP_TRY(hipMemcpy(out->coverage, f.coverage, pixels * sizeof(float), hipMemcpyDeviceToHost));
    if (out->albedo) HIP_TRY(hipMemcpy(out->albedo, f.albedo, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->normal) HIP_TRY(hipMemcpy(out->normal, f.normal, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->position) HIP_TRY(hipMemcpy(out->position, f.position, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (sums) HIP_TRY(hipMemcpy(sums, S.sums, pixels * RT_FEATURE_CHANNELS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (motion) HIP_TRY(hipMemcpy(motion, S.motion, pixels * RT_MOTION_CHANNELS * sizeof(float), hipMemcpyDeviceToHost));
  if (motion_sums)
    HIP_TRY(hipMemcpy(motion_sums, S.motion_sums, pixels * RT_MOTION_CHANNELS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rt_render_features(Scene const *scene, i32 width, i32 height, isize samples, isize max_bounces, RT_Features const *out,
                                  u64 *sums) {
  return features_host("rt_render_features", false, scene, width, height, samples, max_bounces, out, sums, nullptr, nullptr);
}

extern "C" int rt_render_features_motion(Scene const *scene, i32 width, i32 height, isize samples, isize max_bounces,
                                         RT_Features const *out, u64 *sums, f32 *motion, u64 *motion_sums) {
  return features_host("rt_render_features_motion", true, scene, width, height, samples, max_bounces, out, sums, motion, motion_sums);
}
