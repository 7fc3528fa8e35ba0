// rt_extras.cpp -- the reference's other entry points on the GPU: lightmap bake, scene_init and scene_refit (scene_init_gpu,
// scene_refit_gpu), the u8 denoiser (rt_denoise, denoise_image).

#include "rt_host.h"

// raytracer.c:722-784 on the GPU; semantics and the three documented choices
// (last triangle wins, texels outside the image skipped, per-texel seeding) are in oracle/oracle.h.
static int lightmap_bake_locked(Device &D, Image const *lightmap, Scene const *scene, isize samples) {
  if (ensure_device(D) != 0) return -1;
  if (!lightmap || !scene || !lightmap->pixels.data) return rt_fail("lightmap_bake: NULL argument");
  if (lightmap->pixel_type != PT_u8 || lightmap->components < 3) return rt_fail("lightmap_bake: need a u8 image with >= 3 components");
  if (samples <= 0 || lightmap->width <= 0 || lightmap->height <= 0 || lightmap->stride < lightmap->width)
    return rt_fail("lightmap_bake: bad size or sample count");
  RT_Device_Scene *d = cached_scene_locked(D, scene, nullptr, nullptr);
  if (!d) return -1;
  RT_KParams K;
  scene_only_kparams(&K, d);
  K.max_bounces = 8;            // cast_ray(scene, r, 8), raytracer.c:774
  K.seed = g_seed.load();
  const Triangles &T = scene->triangles;
  std::vector<float> verts((size_t)T.len * 9);
  for (int i = 0; i < T.len; i++)
    for (int k = 0; k < 3; k++) {
      verts[(size_t)i * 9 + 0 + k] = T.x[k][i];
      verts[(size_t)i * 9 + 3 + k] = T.y[k][i];
      verts[(size_t)i * 9 + 6 + k] = T.z[k][i];
    }
  size_t pb = (size_t)lightmap->stride * lightmap->height * lightmap->components;
  size_t ob = (size_t)lightmap->width * lightmap->height * sizeof(int);
  DevMem<float>   dv;
  DevMem<int>     dow;
  DevMem<uint8_t> dp;
  HIP_TRY(dv.grow(verts.size()));
  HIP_TRY(dow.grow((size_t)lightmap->width * lightmap->height));
  HIP_TRY(dp.grow(pb));
  HIP_TRY(hipMemcpy(dv, verts.data(), verts.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(dow, 0xFF, ob));                                        // owner = -1
  HIP_TRY(hipMemcpy(dp, lightmap->pixels.data, pb, hipMemcpyHostToDevice));   // untouched texels keep their value
  int rc = rt_launch_lightmap(&K, dv, T.len, (int)lightmap->width, (int)lightmap->height, (int)lightmap->stride,
                              (int)lightmap->components, (int)samples, dow, dp, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(lightmap->pixels.data, dp, pb, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("lightmap_bake failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" void lightmap_bake(Image const *lightmap, Scene const *scene, isize samples) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  forget_multi_counters();
  lightmap_bake_locked(D, lightmap, scene, samples);
}

// ==== HDR lightmaps (include/rt_hip.h, "HDR lightmaps") ========================================================================
// The baker a user runs: the texel list of a UV layout, path-traced 32.32 sums per list entry that can be filled by sample and texel
// ranges, a float image and seam padding -- on the device level (device pointers, launches on the caller's stream) and on the host
// level (the cached device copy of a Scene through scene_checked, slices of RT_LIGHTMAP_SLICE paths).  The work is the kernels of
// rt_lightmap.hip; nothing here rasterises, traces or filters on the CPU.  lightmap_bake above stays the reference's entry point.

static_assert(sizeof(RT_Lightmap_Texel) == 32 && sizeof(RT_Lightmap_Texel) == RT_LIGHTMAP_TEXEL_F4 * 16, "RT_Lightmap_Texel is two 16-byte stores");
static_assert(sizeof(RT_Lightmap_Params) == 32, "RT_Lightmap_Params");
static_assert(RT_CNT_TEXTURED < 8, "the lightmap counters fit the slot's eight words");

static std::atomic<Device *> g_lightmap_dev{nullptr};   // the device of the most recent lightmap trace (rt_get_lightmap_counters)

static int check_lightmap_size(const char *who, i32 width, i32 height) {
  if (width <= 0 || height <= 0) return rt_fail("%s: width and height must be positive (got %d x %d)", who, width, height);
  if ((i64)width * height > RT_LIGHTMAP_MAX_TEXELS) return rt_fail("%s: the map is too large (%d x %d > 2^28 texels)", who, width, height);
  return 0;
}

// What can be checked without the device.  *count = the sample range's length (0 = all resolved).
static int check_lightmap_params(const char *who, RT_Lightmap_Params const *p, i32 *count) {
  if (!p) return rt_fail("%s: lightmap params are NULL", who);
  if (check_lightmap_size(who, p->width, p->height) != 0) return -1;
  if (p->samples <= 0) return rt_fail("%s: samples must be positive (got %d)", who, p->samples);
  if (p->sample_first < 0 || p->sample_count < 0 || (i64)p->sample_first + p->sample_count > p->samples)
    return rt_fail("%s: sample range [%d, +%d) outside [0, %d]", who, p->sample_first, p->sample_count, p->samples);
  if (p->max_bounces < 0) return rt_fail("%s: max_bounces must be >= 0 (got %d)", who, p->max_bounces);
  *count = p->sample_count ? p->sample_count : p->samples - p->sample_first;
  return 0;
}

static int check_lightmap_passes(const char *who, i32 passes) {
  if (passes < 0 || passes > RT_LIGHTMAP_MAX_PASSES) return rt_fail("%s: passes must be within [0, 254] (got %d)", who, passes);
  return 0;
}

void release_lightmap_state(Device &D) {
  D.lightmap = LightmapState();
  Device *self = &D;
  g_lightmap_dev.compare_exchange_strong(self, nullptr);
}

// The ring slot of a new lightmap call: the query ring's next slot (its event orders the reuse) and this ring's words of it.
static int acquire_lightmap_slot(Device &D, int *slot) {
  if (ensure_query_state(D) != 0) return -1;
  HIP_TRY(D.lightmap.slots.grow(RT_QUERY_SLOTS * RT_PROBE_SLOT_BYTES));
  if (acquire_slot(D, slot, false) != 0) return -1;
  D.lightmap.last = *slot;
  g_lightmap_dev.store(&D);
  return 0;
}

// Enqueues the four kernels of the texel list on `stream`.  D.mutex held, D's GPU current, every pointer on D.
static int enqueue_lightmap_texels(RT_Device_Scene *d, const float *verts, i32 width, i32 height, int *owner, float *texels,
                                   long long *count, hipStream_t stream) {
  const size_t pixels = (size_t)width * (size_t)height;
  HIP_TRY(hipMemsetAsync(owner, 0xFF, pixels * sizeof(int), stream));                      // owner = -1
  int rc = rt_launch_lightmap_texels(d->tris, verts, d->n_triangles, width, height, owner, owner + pixels, texels, count, stream);
  if (rc != 0) return rt_fail("lightmap texel kernels launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// Enqueues one launch of the lightmap kernel on `stream`: list entries [j0, j0 + m) x samples [s0, s0 + c).  `fresh`: the slot's
// counters start at zero (the first launch of a call); its work counter always does.  D.mutex held, D's GPU current.
static int enqueue_lightmap_trace(Device &D, RT_Device_Scene *d, RT_Lightmap_Params const *q, i32 s0, i32 c, const float *texels, i64 j0,
                                  i64 m, unsigned long long *sums, hipStream_t stream, int slot, bool fresh) {
  uint8_t *sl = D.lightmap.slots + (size_t)slot * RT_PROBE_SLOT_BYTES;
  if (fresh) HIP_TRY(hipMemsetAsync(sl, 0, RT_PROBE_SLOT_BYTES, stream));
  else HIP_TRY(hipMemsetAsync(sl + 64, 0, 4, stream));
  RT_KParams K;
  scene_only_kparams(&K, d);
  K.max_bounces = q->max_bounces;
  K.seed = q->seed;
  RT_LParams R;
  memset(&R, 0, sizeof R);
  R.texels = texels;
  R.sums = sums;
  R.counters = (unsigned long long *)sl;
  R.head = (uint32_t *)(sl + 64);
  const int64_t n_paths = m * (int64_t)c;
  R.n_paths = (int32_t)n_paths;
  R.m = (int32_t)m;
  R.texel_first = (int32_t)j0;
  R.sample_first = s0;

  // launch geometry: the probe kernel's (rt_query.cpp) -- one workgroup of 16 waves per CU, the tree fills the LDS beside the waves'
  // perm stacks and the kernel's static sRGB scale table
  const int wg_waves = 16, wg_lanes = wg_waves * 64;
  const LdsSplit S = lds_split(d, K.depth, wg_waves, 0, 1, true);
  K.n_lds_nodes = S.n_lds_nodes;
  int64_t blocks = (n_paths + wg_lanes - 1) / wg_lanes;
  if (blocks > D.num_cus) blocks = D.num_cus;
  if (blocks < 1) blocks = 1;
  // paths per grab: an eighth of a wave's mean share, in whole wave-fulls, within [64, 512] (why: rt_query_kernel)
  const int64_t grab = n_paths / (blocks * wg_waves * 8) / 64 * 64;
  R.grab = grab < 64 ? 64 : (grab > 512 ? 512 : (int)grab);
  R.exit_lanes = knob_int("RT_LIGHTMAP_EXIT", 48);                // (the probe kernel's: the S block behind it is the same)
  if (R.exit_lanes < 1 || R.exit_lanes > 64) R.exit_lanes = 48;
  int rc = rt_launch_lightmap_trace(&K, &R, (int)blocks, S.smem, stream);
  if (rc != 0) return rt_fail("lightmap kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  HIP_TRY(hipEventRecord(D.query.done[slot], stream));
  return 0;
}

static int enqueue_lightmap_resolve(RT_Lightmap_Params const *p, i64 n, const void *texels, const void *sums, void *image, hipStream_t stream) {
  const size_t pixels = (size_t)p->width * (size_t)p->height;
  HIP_TRY(hipMemsetAsync(image, 0, pixels * 16, stream));                                  // a texel nobody owns: {0, 0, 0, 0}
  if (n == 0) return 0;
  int rc = rt_launch_lightmap_resolve((long long)n, (long long)pixels, p->samples, p->scale, (const float *)texels,
                                      (const unsigned long long *)sums, (float *)image, stream);
  if (rc != 0) return rt_fail("lightmap resolve kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// `passes` launches, ping-pong between image and work; an odd number ends with one copy back into image
static int enqueue_lightmap_dilate(i32 width, i32 height, i32 passes, void *image, void *work, hipStream_t stream) {
  float *src = (float *)image, *dst = (float *)work;
  for (i32 k = 1; k <= passes; k++) {
    int rc = rt_launch_lightmap_dilate(width, height, k, src, dst, stream);
    if (rc != 0) return rt_fail("lightmap dilation kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    std::swap(src, dst);
  }
  if (src != (float *)image) HIP_TRY(hipMemcpyAsync(image, src, (size_t)width * (size_t)height * 16, hipMemcpyDeviceToDevice, stream));
  return 0;
}

// ---- device level -------------------------------------------------------------------------------------------------------------
extern "C" int rt_lightmap_texels(RT_Device_Scene *dscene, void const *d_vertices, i32 width, i32 height, void *d_owner, void *d_texels,
                                  void *d_count, void *stream) {
  const char *who = "rt_lightmap_texels";
  // (everything that can be checked without the device is checked before it is touched)
  if (!dscene) return rt_fail("%s: device scene is NULL", who);
  if (check_lightmap_size(who, width, height) != 0) return -1;
  if (!d_vertices) return rt_fail("%s: d_vertices is NULL", who);
  if (!d_owner) return rt_fail("%s: d_owner is NULL", who);
  if (!d_texels) return rt_fail("%s: d_texels is NULL", who);
  if (!d_count) return rt_fail("%s: d_count is NULL", who);
  if ((uintptr_t)d_texels & 15) return rt_fail("%s: d_texels is not 16-byte aligned", who);
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  return enqueue_lightmap_texels(dscene, (const float *)d_vertices, width, height, (int *)d_owner, (float *)d_texels, (long long *)d_count,
                                 (hipStream_t)stream);
}

extern "C" int rt_lightmap_trace(RT_Device_Scene *dscene, RT_Lightmap_Params const *params, void const *d_texels, i64 texel_first,
                                 i64 texel_count, void *d_sums, void *stream) {
  const char *who = "rt_lightmap_trace";
  if (!dscene) return rt_fail("%s: device scene is NULL", who);
  i32 count = 0;
  if (check_lightmap_params(who, params, &count) != 0) return -1;
  if (!d_texels) return rt_fail("%s: d_texels is NULL", who);
  if (!d_sums) return rt_fail("%s: d_sums is NULL", who);
  if ((uintptr_t)d_texels & 15) return rt_fail("%s: d_texels is not 16-byte aligned", who);
  if (texel_first < 0 || texel_count <= 0 || texel_first + texel_count > (i64)params->width * params->height)
    return rt_fail("%s: texel range [%lld, +%lld) outside the list (at most %d x %d entries)", who, (long long)texel_first,
                   (long long)texel_count, params->width, params->height);
  if (texel_count * (i64)count > RT_LIGHTMAP_MAX_PATHS)
    return rt_fail("%s: too many paths (%lld texels x %d samples > 2^30 per call)", who, (long long)texel_count, count);
  if (count == 0) return 0;                                     // (an empty range at the end of the samples: nothing to trace)
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  int slot = 0;
  if (acquire_lightmap_slot(D, &slot) != 0) return -1;
  return enqueue_lightmap_trace(D, dscene, params, params->sample_first, count, (const float *)d_texels, texel_first, texel_count,
                                (unsigned long long *)d_sums, (hipStream_t)stream, slot, true);
}

extern "C" int rt_lightmap_resolve(RT_Lightmap_Params const *params, i64 n_texels, void const *d_texels, void const *d_sums, void *d_image,
                                   void *stream) {
  const char *who = "rt_lightmap_resolve";
  i32 count = 0;
  if (check_lightmap_params(who, params, &count) != 0) return -1;
  if (n_texels < 0 || n_texels > (i64)params->width * params->height)
    return rt_fail("%s: n_texels %lld outside [0, %d x %d]", who, (long long)n_texels, params->width, params->height);
  if (!d_image) return rt_fail("%s: d_image is NULL", who);
  if (n_texels > 0 && !d_texels) return rt_fail("%s: d_texels is NULL", who);
  if (n_texels > 0 && !d_sums) return rt_fail("%s: d_sums is NULL", who);
  if (((uintptr_t)d_texels | (uintptr_t)d_image) & 15) return rt_fail("%s: d_texels or d_image is not 16-byte aligned", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_lightmap_resolve(params, n_texels, d_texels, d_sums, d_image, (hipStream_t)stream);
}

extern "C" i64 rt_lightmap_work_bytes(i32 width, i32 height) {
  if (check_lightmap_size("rt_lightmap_work_bytes", width, height) != 0) return -1;
  return (i64)width * height * 16;
}

extern "C" int rt_lightmap_dilate(i32 width, i32 height, i32 passes, void *d_image, void *d_work, void *stream) {
  const char *who = "rt_lightmap_dilate";
  if (check_lightmap_size(who, width, height) != 0 || check_lightmap_passes(who, passes) != 0) return -1;
  if (!d_image) return rt_fail("%s: d_image is NULL", who);
  if (!d_work) return rt_fail("%s: d_work is NULL", who);
  if (d_image == d_work) return rt_fail("%s: d_image and d_work must differ", who);
  if (((uintptr_t)d_image | (uintptr_t)d_work) & 15) return rt_fail("%s: d_image or d_work is not 16-byte aligned", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_lightmap_dilate(width, height, passes, d_image, d_work, (hipStream_t)stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
// The list goes through the device in launches of at most RT_LIGHTMAP_SLICE paths: sample ranges of the whole list, or -- where one
// sample of the list exceeds a slice -- texel ranges of one sample.  Launch k of a call, from the list's length n:
static void lightmap_slice(i64 n, i32 count, i64 k, i64 *j0, i64 *m, i32 *s, i32 *c) {
  if (n <= RT_LIGHTMAP_SLICE) {
    const i64 per = RT_LIGHTMAP_SLICE / n;
    *j0 = 0, *m = n, *s = (i32)(k * per), *c = (i32)(count - *s < per ? count - *s : per);
  } else {
    const i64 parts = (n + RT_LIGHTMAP_SLICE - 1) / RT_LIGHTMAP_SLICE;
    *j0 = (k % parts) * RT_LIGHTMAP_SLICE, *m = n - *j0 < RT_LIGHTMAP_SLICE ? n - *j0 : RT_LIGHTMAP_SLICE, *s = (i32)(k / parts), *c = 1;
  }
}
static i64 lightmap_slices(i64 n, i32 count) {
  if (n <= 0 || count <= 0) return 0;
  if (n <= RT_LIGHTMAP_SLICE) { const i64 per = RT_LIGHTMAP_SLICE / n; return (count + per - 1) / per; }
  return (i64)count * ((n + RT_LIGHTMAP_SLICE - 1) / RT_LIGHTMAP_SLICE);
}

extern "C" int rt_scene_lightmap(Scene const *scene, RT_Lightmap_Params const *params, i32 dilate_passes, f32 *image, u64 *sums,
                                 RT_Lightmap_Texel *texels, i64 *n_texels) {
  const char *who = "rt_scene_lightmap";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  i32 count = 0;
  if (check_lightmap_params(who, params, &count) != 0 || check_lightmap_passes(who, dilate_passes) != 0) return -1;
  if (!image) return rt_fail("%s: image is NULL", who);

  Device &D = dev0();                                            // (the primary device only, whatever rt_device_count() says)
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  LightmapState &S = D.lightmap;
  const i32 width = params->width, height = params->height;
  const size_t pixels = (size_t)width * (size_t)height;
  HIP_TRY(S.owner.grow(pixels + (size_t)height));
  HIP_TRY(S.texels.grow(pixels * 8));
  HIP_TRY(S.count.grow(1));
  HIP_TRY(S.image.grow(pixels * 4));
  if (dilate_passes > 0) HIP_TRY(S.work.grow(pixels * 4));
  int slot = 0;
  if (acquire_lightmap_slot(D, &slot) != 0) return -1;
  hipStream_t stream = nullptr;
  long long n = 0;
  auto trace_slice = [&](RT_Device_Scene *ds, i64 k) -> int {
    i64 j0, m;
    i32 s, c;
    lightmap_slice(n, count, k, &j0, &m, &s, &c);
    return enqueue_lightmap_trace(D, ds, params, params->sample_first + s, c, S.texels, j0, m, S.sums, stream, slot, k == 0);
  };
  // the first launch's enqueue: the vertices as lightmap_bake uploads them, the list, its length, sums from zero -- so that a scene
  // check that traces again starts from zero, on the list of the scene as it is
  auto first_slice = [&](RT_Device_Scene *ds) -> int {
    const Triangles &T = scene->triangles;
    std::vector<float> verts((size_t)T.len * 9);
    for (int i = 0; i < T.len; i++)
      for (int v = 0; v < 3; v++) {
        verts[(size_t)i * 9 + 0 + v] = T.x[v][i];
        verts[(size_t)i * 9 + 3 + v] = T.y[v][i];
        verts[(size_t)i * 9 + 6 + v] = T.z[v][i];
      }
    if (ds->n_triangles != (int)T.len) return rt_fail("%s: the device copy has another shape", who);
    HIP_TRY(S.verts.grow(verts.size()));
    HIP_TRY(hipMemcpy(S.verts, verts.data(), verts.size() * sizeof(float), hipMemcpyHostToDevice));
    if (enqueue_lightmap_texels(ds, S.verts, width, height, S.owner, S.texels, S.count, stream) != 0) return -1;
    HIP_TRY(hipMemcpy(&n, S.count, sizeof n, hipMemcpyDeviceToHost));
    HIP_TRY(S.sums.grow((size_t)(n > 0 ? n : 1) * 3));
    HIP_TRY(hipMemsetAsync(S.slots + (size_t)slot * RT_PROBE_SLOT_BYTES, 0, RT_PROBE_SLOT_BYTES, stream));      // (a call without a launch counts nothing)
    HIP_TRY(hipMemsetAsync(S.sums, 0, (size_t)(n > 0 ? n : 1) * 24, stream));
    return lightmap_slices(n, count) > 0 ? trace_slice(ds, 0) : 0;
  };
  RT_Device_Scene *d = scene_checked(D, scene, stream, nullptr, first_slice);
  if (!d) return -1;
  for (i64 k = 1, kn = lightmap_slices(n, count); k < kn; k++)
    if (trace_slice(d, k) != 0) return -1;
  if (enqueue_lightmap_resolve(params, n, S.texels, S.sums, S.image, stream) != 0) return -1;
  if (enqueue_lightmap_dilate(width, height, dilate_passes, S.image, S.work, stream) != 0) return -1;
  HIP_TRY(hipMemcpy(image, S.image, pixels * 16, hipMemcpyDeviceToHost));
  if (sums && n > 0) HIP_TRY(hipMemcpy(sums, S.sums, (size_t)n * 24, hipMemcpyDeviceToHost));
  if (texels && n > 0) HIP_TRY(hipMemcpy(texels, S.texels, (size_t)n * sizeof(RT_Lightmap_Texel), hipMemcpyDeviceToHost));
  if (n_texels) *n_texels = n;
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int rt_get_lightmap_counters(RT_Counters *out) {
  if (!out) return rt_fail("rt_get_lightmap_counters: NULL");
  memset(out, 0, sizeof *out);
  Device *Dp = g_lightmap_dev.load();
  if (!Dp) return 0;                                           // no lightmap trace yet: zeros
  Device &D = *Dp;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (D.lightmap.last < 0 || !D.lightmap.slots) return 0;
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long c[8];
  HIP_TRY(hipMemcpy(c, D.lightmap.slots + (size_t)D.lightmap.last * RT_PROBE_SLOT_BYTES, sizeof c, hipMemcpyDeviceToHost));
  out->paths = c[RT_CNT_PATHS];
  out->rays = c[RT_CNT_RAYS];
  out->node_visits = c[RT_CNT_NODES];
  out->leaf_visits = c[RT_CNT_LEAVES];
  out->shades = c[RT_CNT_SHADES];
  out->backgrounds = c[RT_CNT_BG];
  out->textured = c[RT_CNT_TEXTURED];
  return 0;
}

// ---------------------------------------------------------------------------------
// scene_init on the GPU (csrc/rt_build.hip): same Scene, byte for byte, as scene_init()

extern "C" int rt_gpu_build(const Triangle *h_tris, long n_in, long depth, BVH_Node *h_nodes, long n_internal, float *h_block,
                            long block_len, char *err, int err_len);

extern "C" int scene_init_gpu(Scene *scene, Triangle_Slice src, Allocator allocator) {
  if (!scene) return rt_fail("scene_init_gpu: scene is NULL");
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  if (src.len < 0 || (src.len > 0 && !src.data)) return rt_fail("scene_init_gpu: bad triangle slice");
  if (src.len > (isize)1 << 27) return rt_fail("scene_init_gpu: %ld triangles are too many", (long)src.len);
  // The GPU build orders centroid keys with a radix sort of their bit patterns, which equals the `<` order of scene_init's
  // merge sort for every number including the infinities -- but not for NaN (`<` leaves a NaN where it stands, the radix
  // order puts it behind +inf).  A soup with a NaN coordinate is therefore built by scene_init itself: same Scene by definition.
  for (isize i = 0; i < src.len; i++)
    for (int v = 0; v < 3; v++) {
      const Vec3 &q = src.data[i].positions[v];
      if (q.x != q.x || q.y != q.y || q.z != q.z) {
        scene_init(scene, src, allocator);
        return 0;
      }
    }
  if (!rt_scene_alloc(scene, src.len, allocator)) return rt_fail("scene_init_gpu: the allocator failed");   // (drops a stale device copy)
  char err[256] = "";
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  int rc = rt_gpu_build(src.data, (long)src.len, (long)scene->bvh.depth, scene->bvh.nodes.data, (long)scene->bvh.nodes.len,
                        scene->triangles.x[0], (long)scene->triangles.len, err, (int)sizeof err);
  if (rc != 0) return rt_fail("scene_init_gpu: %s", err);
  return 0;
}

// ---------------------------------------------------------------------------------
// scene_refit on the GPU (csrc/rt_refit.hip): same bytes as scene_refit() in the host Scene, and the primary device's copy of
// the scene updated in place -- nothing is uploaded by the next frame

// 0 = refitted in place, 1 = the copy may not be kept (the caller refits on the host, which drops it), -1 = error
static int refit_gpu_locked(Device &D, Scene *scene, Triangle_Slice src, const std::vector<i32> &source_of_slot) {
  auto cached = D.scene_cache.find(scene);
  RT_Device_Scene *d = cached != D.scene_cache.end() ? cached->second
                                                     : cached_scene_locked(D, scene, nullptr, nullptr);   // (the ordinary upload, then the one path)
  if (!d) return -1;
  // The refit rewrites nodes and triangle block on both sides and then takes the host bytes as the copy's reference.  That is only
  // sound while everything ELSE of the host scene -- materials, texels, background -- still is what the copy was made from: an edit
  // nobody reported (rt_scene_touch) would otherwise be absorbed into the reference and never be seen again.  (The full blocks are
  // compared, not the sampled stamp of a frame: an existing copy is either kept as it is or dropped, never uploaded again in here.)
  std::vector<FpBlock> now;
  if (!refit_may_keep_copy(d, scene, now)) return 1;
  const Triangles &T = scene->triangles;
  const int len = (int)T.len, depth = (int)scene->bvh.depth, n_internal = (int)scene->bvh.nodes.len;
  if (d->n_triangles != len || d->depth != depth || d->n_nodes != n_internal) return rt_fail("scene_refit_gpu: the device copy has another shape");
  const size_t block_bytes = (size_t)TRIANGLES_ALLOCATION_SIZE(len), src_bytes = (size_t)src.len * sizeof(Triangle);
  RefitState &R = D.refit;
  HIP_TRY(R.src.grow(src_bytes));
  HIP_TRY(R.source_of_slot.grow((size_t)len));
  HIP_TRY(R.block.grow(block_bytes / 4));
  HIP_TRY(R.populated.grow((size_t)n_internal + (size_t)len / 8));
  HIP_TRY(R.max_edge_bits.grow(1));
  HIP_TRY(hipDeviceSynchronize());                          // whatever still reads the copy finishes before the kernels write it
  HIP_TRY(hipMemcpy(R.src, src.data, src_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(R.source_of_slot, source_of_slot.data(), (size_t)len * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(R.max_edge_bits, 0, 4));
  int rc = rt_launch_refit(len, depth, n_internal, R.src, R.source_of_slot, R.block, d->nodes, d->leaves, d->tris, R.populated,
                           R.max_edge_bits, nullptr);
  // one copy of the nodes and one of the staging block: the host Scene stays the truth for the oracle and the per-frame check
  uint32_t edge_bits = 0;
  if (rc == 0 && n_internal > 0) rc = (int)hipMemcpy(scene->bvh.nodes.data, d->nodes, (size_t)n_internal * sizeof(BVH_Node), hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(T.x[0], R.block, block_bytes, hipMemcpyDeviceToHost);
  if (rc == 0) rc = (int)hipMemcpy(&edge_bits, R.max_edge_bits, 4, hipMemcpyDeviceToHost);
  if (rc != 0) {
    // the copy (and perhaps part of the host Scene) is half refitted: drop the copy, the caller rebuilds or refits again
    rt_fail("scene_refit_gpu failed: %s", hipGetErrorString((hipError_t)rc));
    free_device_scene(d);
    D.scene_cache.erase(scene);
    return -1;
  }
  memcpy(&d->max_edge, &edge_bits, 4);                      // exact, not "can only grow"
  d->boxes_ordered = n_internal == 0 || node_boxes_ordered((const float *)scene->bvh.nodes.data, (size_t)n_internal);
  rehash_geometry_blocks(scene, now);
  adopt_scene_stamps(d, scene, now);
  return 0;
}

extern "C" int scene_refit_gpu(Scene *scene, Triangle_Slice src, i32 const *slot_of_source) {
  if (!scene) return rt_fail("scene_refit_gpu: scene is NULL");
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  std::vector<i32> source_of_slot((size_t)(scene->triangles.len > 0 ? scene->triangles.len : 0));
  if (rt_refit_check(scene, src, slot_of_source, source_of_slot.data()) != 0) return -1;
  // scene_init_gpu's rule: the kernels reduce bounds in another order than the host, which gives the same boxes for numbers
  // only.  A soup with a NaN position is refitted by scene_refit itself (which drops the device copies).
  for (isize i = 0; i < src.len; i++)
    for (int v = 0; v < 3; v++) {
      const Vec3 &q = src.data[i].positions[v];
      if (q.x != q.x || q.y != q.y || q.z != q.z) return scene_refit(scene, src, slot_of_source);
    }
  int rc;
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    DeviceGuard guard(D);
    rc = refit_gpu_locked(D, scene, src, source_of_slot);
    // the other device slots hold the old geometry: they upload on their next frame (lock order: slot 0, then slot r)
    for (int i = 1; i < RT_MAX_DEVICES; i++) {
      Device &O = g_devs[i];
      std::lock_guard<std::mutex> other(O.mutex);
      auto it = O.scene_cache.find(scene);
      if (it == O.scene_cache.end()) continue;
      DeviceGuard og(O);
      (void)hipDeviceSynchronize();
      free_device_scene(it->second);
      O.scene_cache.erase(it);
    }
  }
  // an unreported edit outside the geometry: scene_refit drops every copy, and the next frame uploads the scene as it is
  return rc == 1 ? scene_refit(scene, src, slot_of_source) : rc;
}

// ---------------------------------------------------------------------------------
// denoiser (reference denoiser.h / denoiser.c:131-153), SURVEY.md section 8f #3

extern "C" int rt_denoise(i32 width, i32 height, void const *d_src, void *d_dst, void *stream) {
  {
    Device &D = dev0();
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  if (width <= 0 || height <= 0 || !d_src || !d_dst || d_src == d_dst) return rt_fail("rt_denoise: bad arguments");
  int rc = rt_launch_denoise(width, height, width, 3, width, 3, (const uint8_t *)d_src, (uint8_t *)d_dst, (hipStream_t)stream);
  if (rc != 0) return rt_fail("denoise kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

static int denoise_host(Image const *src, Image const *dst) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (!src || !dst || !src->pixels.data || !dst->pixels.data) return rt_fail("denoise_image: NULL image");
  if (src->pixels.data == dst->pixels.data) return rt_fail("denoise_image: src and dst must differ (denoiser.c:134)");
  if (src->width != dst->width || src->height != dst->height) return rt_fail("denoise_image: size mismatch");
  if (src->components < 1 || dst->components < 1 || src->stride < src->width || dst->stride < dst->width)
    return rt_fail("denoise_image: bad layout");
  size_t sb = (size_t)src->stride * src->height * src->components;
  size_t db = (size_t)dst->stride * dst->height * dst->components;
  DevMem<uint8_t> ds, dd;
  HIP_TRY(ds.grow(sb));
  HIP_TRY(dd.grow(db));
  HIP_TRY(hipMemcpy(ds, src->pixels.data, sb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dd, dst->pixels.data, db, hipMemcpyHostToDevice));     // components beyond 3 keep their values
  int rc = rt_launch_denoise((int)src->width, (int)src->height, (int)src->stride, (int)src->components,
                             (int)dst->stride, (int)dst->components, ds, dd, nullptr);
  if (rc == 0) rc = (int)hipMemcpy(dst->pixels.data, dd, db, hipMemcpyDeviceToHost);
  if (rc != 0) return rt_fail("denoise_image failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" void denoise_image(Image const *src, Image const *dst, isize n_threads) {
  (void)n_threads;      // the reference's CPU thread count (denoiser.c:131); one kernel launch here
  denoise_host(src, dst);
}
