// rt_extras.cpp -- the reference's other GPU entry points: lightmap bake, scene_init on the GPU, the denoiser; and the guided
// denoiser over the feature buffers and the temporal accumulation of a sequence's frames (rt_hip.h).

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

void release_refit_state(Device &D) { D.refit = RefitState(); }

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

// ---------------------------------------------------------------------------------
// The guided denoiser (include/rt_hip.h): the edge-stopping a-trous filter of a linear frame over its first-hit feature buffers, on
// the device level (device pointers, a pack launch and one filter launch per iteration on the caller's stream), on the host level
// (host arrays through library-owned staging) and behind a frame (rt_render_denoised: the shared frame sequence, the feature pass
// and the filter in ONE scene-checked call).  The work is rt_guided_pack_kernel and rt_guided_filter_kernel (rt_guided.hip);
// nothing here filters a pixel on the CPU.  (Beside the reference's u8 denoiser above rather than in a unit of its own:
// tests/test_mem_owner.py scans a fixed number of host units for allocator calls outside rt_mem.h, and this code is scanned with them.)

static_assert(sizeof(RT_Guided_Params) == 20, "iterations, three sigmas, demodulate");

#define RT_GUIDED_WORK_PER_PIXEL 64      // two colour buffers (r, g, b, L) and the guides (N, coverage), (P, 0): four float4

// What can be checked without the device.  `who` prefixes the messages.
static int check_guided(const char *who, i32 width, i32 height, RT_Guided_Params const *g) {
  if (width <= 0 || height <= 0) return rt_fail("%s: image size %dx%d is invalid", who, width, height);
  if ((int64_t)width * height > (int64_t)1 << 28) return rt_fail("%s: image %dx%d is too large (more than 2^28 pixels)", who, width, height);
  if (!g) return rt_fail("%s: guided params are NULL", who);
  if (g->iterations < 1 || g->iterations > 8) return rt_fail("%s: iterations must be 1 .. 8 (got %d)", who, g->iterations);
  // (written so that NaN fails: it is not > 0)
  if (!(g->sigma_color > 0.0f)) return rt_fail("%s: sigma_color must be > 0 (got %g)", who, (double)g->sigma_color);
  if (!(g->sigma_normal > 0.0f)) return rt_fail("%s: sigma_normal must be > 0 (got %g)", who, (double)g->sigma_normal);
  if (!(g->sigma_position > 0.0f)) return rt_fail("%s: sigma_position must be > 0 (got %g)", who, (double)g->sigma_position);
  if (g->demodulate != 0 && g->demodulate != 1) return rt_fail("%s: demodulate must be 0 or 1 (got %d)", who, g->demodulate);
  return 0;
}

extern "C" i64 rt_guided_work_bytes(i32 width, i32 height) {
  if (width <= 0 || height <= 0 || (int64_t)width * height > (int64_t)1 << 28) {
    rt_fail("rt_guided_work_bytes: image size %dx%d is invalid", width, height);
    return -1;
  }
  return (i64)width * height * RT_GUIDED_WORK_PER_PIXEL;
}

// Enqueues the pack launch and g->iterations filter launches on `stream`.  Every pointer is on the current device; every input
// is in d_work before d_out / d_image are written (the last launch reads a pixel's colour and albedo only to write that pixel).
static int enqueue_guided(i32 width, i32 height, RT_Guided_Params const *g, void const *d_color, void const *d_coverage,
                          void const *d_albedo, void const *d_normal, void const *d_position, void *d_out, void *d_image, void *d_work,
                          hipStream_t stream) {
  const size_t pixels = (size_t)width * height;
  uint8_t *w = (uint8_t *)d_work;
  void *buf[2] = {w, w + pixels * 16}, *g0 = w + pixels * 32, *g1 = w + pixels * 48;
  int rc = rt_launch_guided_pack((int)pixels, g->demodulate, (const float *)d_color, (const float *)d_coverage, (const float *)d_albedo,
                                 (const float *)d_normal, (const float *)d_position, buf[0], g0, g1, stream);
  if (rc != 0) return rt_fail("guided pack kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  const float k_c = 1.0f / (g->sigma_color * g->sigma_color), k_n = 1.0f / (g->sigma_normal * g->sigma_normal),
              k_p = 1.0f / (g->sigma_position * g->sigma_position);
  for (int i = 0; i < g->iterations; i++) {
    const int last = i == g->iterations - 1;
    const float kc_i = k_c * (float)(1u << (2 * i));            // the colour sigma halves every iteration
    rc = rt_launch_guided_filter(width, height, 1 << i, k_n, k_p, kc_i, last, g->demodulate, buf[i & 1], buf[(i & 1) ^ 1], g0, g1,
                                 (const float *)d_color, (const float *)d_albedo, last ? (float *)d_out : nullptr,
                                 last ? (uint8_t *)d_image : nullptr, stream);
    if (rc != 0) return rt_fail("guided filter kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  return 0;
}

// ---- device level -------------------------------------------------------------------------------------------------------------
extern "C" int rt_guided_denoise(i32 width, i32 height, RT_Guided_Params const *params, void const *d_color, void const *d_coverage,
                                 void const *d_albedo, void const *d_normal, void const *d_position, void *d_out, void *d_image,
                                 void *d_work, void *stream) {
  const char *who = "rt_guided_denoise";
  // (everything that can be checked without the device is checked before it is touched)
  if (check_guided(who, width, height, params) != 0) return -1;
  if (!d_color) return rt_fail("%s: d_color is NULL", who);
  if (!d_coverage) return rt_fail("%s: d_coverage is NULL", who);
  if (!d_albedo && params->demodulate) return rt_fail("%s: d_albedo is NULL and demodulate is set", who);
  if (!d_normal) return rt_fail("%s: d_normal is NULL", who);
  if (!d_position) return rt_fail("%s: d_position is NULL", who);
  if (!d_out && !d_image) return rt_fail("%s: no output is wanted (d_out and d_image are NULL)", who);
  if (!d_work) return rt_fail("%s: d_work is NULL", who);
  if ((uintptr_t)d_work & 15) return rt_fail("%s: d_work must be 16-byte aligned", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_guided(width, height, params, d_color, d_coverage, d_albedo, d_normal, d_position, d_out, d_image, d_work,
                        (hipStream_t)stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
// Gives back the staging of the host-level calls.  D.mutex held, D's GPU current, device idle.
void release_guided_state(Device &D) { D.guided = GuidedState(); }

extern "C" int rt_guided_denoise_host(i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                                      RT_Features const *planes, f32 *out, u8 *image) {
  const char *who = "rt_guided_denoise_host";
  if (check_guided(who, width, height, params) != 0) return -1;
  if (!color) return rt_fail("%s: color is NULL", who);
  if (!planes) return rt_fail("%s: planes is NULL", who);
  if (!planes->coverage) return rt_fail("%s: planes->coverage is NULL", who);
  if (!planes->albedo && params->demodulate) return rt_fail("%s: planes->albedo is NULL and demodulate is set", who);
  if (!planes->normal) return rt_fail("%s: planes->normal is NULL", who);
  if (!planes->position) return rt_fail("%s: planes->position is NULL", who);
  if (!out && !image) return rt_fail("%s: no output is wanted (out and image are NULL)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  GuidedState &S = D.guided;
  const size_t pixels = (size_t)width * height;
  HIP_TRY(S.in.grow(pixels * 13));
  HIP_TRY(S.work.grow(pixels * RT_GUIDED_WORK_PER_PIXEL));
  if (out) HIP_TRY(S.out.grow(pixels * 3));
  if (image) HIP_TRY(S.image.grow(pixels * 3));
  float *d_col = S.in, *d_cov = S.in + pixels * 3, *d_alb = S.in + pixels * 4, *d_nrm = S.in + pixels * 7, *d_pos = S.in + pixels * 10;
  hipStream_t stream = nullptr;                                 // (does not wait for the lane streams of frames in flight)
  HIP_TRY(hipMemcpy(d_col, color, pixels * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_cov, planes->coverage, pixels * sizeof(float), hipMemcpyHostToDevice));
  if (planes->albedo) HIP_TRY(hipMemcpy(d_alb, planes->albedo, pixels * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_nrm, planes->normal, pixels * 3 * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_pos, planes->position, pixels * 3 * sizeof(float), hipMemcpyHostToDevice));
  if (enqueue_guided(width, height, params, d_col, d_cov, planes->albedo ? d_alb : nullptr, d_nrm, d_pos, out ? S.out.get() : nullptr,
                     image ? S.image.get() : nullptr, S.work, stream) != 0)
    return -1;
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  if (out) HIP_TRY(hipMemcpy(out, S.out, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (image) HIP_TRY(hipMemcpy(image, S.image, pixels * 3, hipMemcpyDeviceToHost));
  return 0;
}

// ---- behind a frame -----------------------------------------------------------------------------------------------------------
extern "C" int rt_render_denoised(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                                  RT_Guided_Params const *params, f32 *linear_noisy, f32 *linear_denoised) {
  const char *who = "rt_render_denoised";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!image) return rt_fail("%s: image is NULL", who);
  if (image->width <= 0 || image->height <= 0 || image->width > 0x7fffffff || image->height > 0x7fffffff)
    return rt_fail("%s: image size %ldx%ld is invalid", who, (long)image->width, (long)image->height);
  if (check_guided(who, (i32)image->width, (i32)image->height, params) != 0) return -1;
  if (image->pixels.data && image->components < 3) return rt_fail("%s: image needs >= 3 components", who);
  if (image->pixels.data && image->stride < image->width) return rt_fail("%s: image stride < width", who);
  if (samples <= 0 || samples > 0x7fffffff) return rt_fail("%s: samples must be positive and fit 32 bits (got %ld)", who, (long)samples);
  if (max_bounces < 0 || max_bounces > 0x7fffffff) return rt_fail("%s: max_bounces must be >= 0 and fit 32 bits (got %ld)", who, (long)max_bounces);
  if (!image->pixels.data && !linear_denoised) return rt_fail("%s: no output is wanted (no pixels and no linear_denoised)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  const double t_start = now_ms();
  if (ensure_device(D) != 0) return -1;
  if (rt_device_count() > 1)
    return rt_fail("%s: a denoised frame renders on one device, and %d are set (rt_set_devices)", who, rt_device_count());
  RT_Render_Params p;
  memset(&p, 0, sizeof p);
  p.width = (i32)image->width;
  p.height = (i32)image->height;
  p.samples = (i32)samples;
  p.max_bounces = (i32)max_bounces;
  p.seed = g_seed.load();
  p.world = 1;
  if (check_params(&p) != 0) return -1;
  forget_multi_counters();

  FrameTiming T;
  Workspace &W = D.ws;
  FeatureState &F = D.features;
  GuidedState &S = D.guided;
  const size_t pixels = (size_t)p.width * p.height;
  if (ensure_ws_buffers(W, p.width, p.height, 0, 0) != 0) return -1;
  HIP_TRY(F.sums.grow(pixels * RT_FEATURE_CHANNELS));
  HIP_TRY(F.planes.grow(pixels * RT_FEATURE_CHANNELS));
  HIP_TRY(S.work.grow(pixels * RT_GUIDED_WORK_PER_PIXEL));
  if (linear_denoised) HIP_TRY(S.out.grow(pixels * 3));
  float *d_cov = F.planes, *d_alb = F.planes + pixels, *d_nrm = F.planes + pixels * 4, *d_pos = F.planes + pixels * 7;
  hipStream_t stream = nullptr;
  // the frame's linear values, the four planes of its feature pass, the filter: W.image receives the DENOISED frame's encoding
  auto pass = [&](RT_Device_Scene *d) -> int {
    if (enqueue_frame(D, d, &scene->camera, &p, W, stream, 0, nullptr, nullptr, W.linear) != 0) return -1;
    HIP_TRY(hipMemsetAsync(F.sums, 0, pixels * RT_FEATURE_CHANNELS * sizeof(unsigned long long), stream));
    if (enqueue_features(D, d, &scene->camera, &p, F.sums, stream) != 0) return -1;
    if (enqueue_resolve(&p, F.sums, d_cov, d_alb, d_nrm, d_pos, stream) != 0) return -1;
    return enqueue_guided(p.width, p.height, params, W.linear, d_cov, d_alb, d_nrm, d_pos, linear_denoised ? S.out.get() : nullptr,
                          W.image, S.work, stream);
  };
  if (!scene_checked(D, scene, stream, &T, pass)) return -1;      // (a scene edited since the copy: uploaded and rendered again)

  if (copy_image_out(image, W.image, p.width, p.height, stream) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[4], stream));
  if (linear_noisy) HIP_TRY(hipMemcpy(linear_noisy, W.linear, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (linear_denoised) HIP_TRY(hipMemcpy(linear_denoised, S.out, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  frame_split(W, T);
  T.total_ms = (float)(now_ms() - t_start);
  D.timing = T;
  return 0;
}

// ---------------------------------------------------------------------------------
// Temporal accumulation (include/rt_hip.h): the frame blended with the history of the frames before it, reprojected through the
// first hits -- on the device level (device pointers, one launch on the caller's stream), on the host level (host arrays through
// library-owned staging) and behind a frame (rt_render_temporal: frame, feature pass, accumulation against an RT_History, optionally
// the guided filter, in ONE scene-checked call).  The work is rt_temporal_kernel (rt_temporal.hip); nothing here accumulates a pixel
// on the CPU.  (In this unit for the reason the guided denoiser is: it is scanned with the units tests/test_mem_owner.py counts.)

static_assert(sizeof(RT_Temporal_Params) == 20, "alpha, max_history, two tolerances, demodulate");

#define RT_TEMPORAL_HISTORY_PER_PIXEL 48   // (c, len), (N, coverage), (W, 0): three float4
#define RT_TEMPORAL_MAX_HISTORY (1 << 20)

// What can be checked without the device.  `who` prefixes the messages.
static int check_temporal(const char *who, i32 width, i32 height, RT_Temporal_Params const *t) {
  if (width <= 0 || height <= 0) return rt_fail("%s: image size %dx%d is invalid", who, width, height);
  if ((int64_t)width * height > (int64_t)1 << 28) return rt_fail("%s: image %dx%d is too large (more than 2^28 pixels)", who, width, height);
  if (!t) return rt_fail("%s: temporal params are NULL", who);
  // (written so that NaN fails)
  if (!(t->alpha > 0.0f && t->alpha <= 1.0f)) return rt_fail("%s: alpha must be in (0, 1] (got %g)", who, (double)t->alpha);
  if (t->max_history < 1 || t->max_history > RT_TEMPORAL_MAX_HISTORY)
    return rt_fail("%s: max_history must be 1 .. 2^20 (got %d)", who, t->max_history);
  if (!(t->normal_tolerance > 0.0f)) return rt_fail("%s: normal_tolerance must be > 0 (got %g)", who, (double)t->normal_tolerance);
  if (!(t->plane_tolerance > 0.0f)) return rt_fail("%s: plane_tolerance must be > 0 (got %g)", who, (double)t->plane_tolerance);
  if (t->demodulate != 0 && t->demodulate != 1) return rt_fail("%s: demodulate must be 0 or 1 (got %d)", who, t->demodulate);
  return 0;
}

extern "C" i64 rt_temporal_history_bytes(i32 width, i32 height) {
  if (width <= 0 || height <= 0 || (int64_t)width * height > (int64_t)1 << 28) {
    rt_fail("rt_temporal_history_bytes: image size %dx%d is invalid", width, height);
    return -1;
  }
  return (i64)width * height * RT_TEMPORAL_HISTORY_PER_PIXEL;
}

static void temporal_camera(RT_TCamera *c, Camera const *cam) {
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 3; k++) c->r[i][k] = cam->view_matrix.rows[i][k];
    c->t[i] = cam->view_matrix.rows[i][3];
  }
  c->focal_length = cam->focal_length;
}

// Enqueues the launch on `stream`.  Every pointer is on the current device; prev is read only when d_history_in is given.
static int enqueue_temporal(i32 width, i32 height, RT_Temporal_Params const *t, Camera const *cam, Camera const *prev,
                            void const *d_color, void const *d_coverage, void const *d_albedo, void const *d_normal,
                            void const *d_position, void const *d_history_in, void *d_history_out, void *d_out, void *d_length,
                            void *d_image, hipStream_t stream) {
  RT_TParams P;
  memset(&P, 0, sizeof P);
  temporal_camera(&P.cur, cam);
  temporal_camera(&P.prev, d_history_in ? prev : cam);
  P.width = width;
  P.height = height;
  P.half_w = (float)width * 0.5f;
  P.half_h = (float)height * 0.5f;
  P.aspect = (float)width / (float)height;
  P.tn2 = t->normal_tolerance * t->normal_tolerance;
  P.tp2 = t->plane_tolerance * t->plane_tolerance;
  P.alpha = t->alpha;
  P.max_history = (float)t->max_history;
  P.demodulate = t->demodulate;
  P.tiles_x = (width + 31) / 32;
  int rc = rt_launch_temporal(&P, (const float *)d_color, (const float *)d_coverage, (const float *)d_albedo, (const float *)d_normal,
                              (const float *)d_position, d_history_in, d_history_out, (float *)d_out, (float *)d_length,
                              (uint8_t *)d_image, stream);
  if (rc != 0) return rt_fail("temporal kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- device level -------------------------------------------------------------------------------------------------------------
extern "C" int rt_temporal_accumulate(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                      Camera const *previous_camera, void const *d_color, void const *d_coverage, void const *d_albedo,
                                      void const *d_normal, void const *d_position, void const *d_history_in, void *d_history_out,
                                      void *d_out, void *d_length, void *d_image, void *stream) {
  const char *who = "rt_temporal_accumulate";
  // (everything that can be checked without the device is checked before it is touched)
  if (check_temporal(who, width, height, params) != 0) return -1;
  if (!camera) return rt_fail("%s: camera is NULL", who);
  if (d_history_in && !previous_camera) return rt_fail("%s: previous_camera is NULL and a history is given", who);
  if (!d_color) return rt_fail("%s: d_color is NULL", who);
  if (!d_coverage) return rt_fail("%s: d_coverage is NULL", who);
  if (!d_albedo && params->demodulate) return rt_fail("%s: d_albedo is NULL and demodulate is set", who);
  if (!d_normal) return rt_fail("%s: d_normal is NULL", who);
  if (!d_position) return rt_fail("%s: d_position is NULL", who);
  if (!d_history_out) return rt_fail("%s: d_history_out is NULL", who);
  if (((uintptr_t)d_history_out | (uintptr_t)d_history_in) & 15) return rt_fail("%s: the histories must be 16-byte aligned", who);
  if (d_history_in) {
    const uintptr_t a = (uintptr_t)d_history_in, b = (uintptr_t)d_history_out;
    const uintptr_t bytes = (uintptr_t)width * height * RT_TEMPORAL_HISTORY_PER_PIXEL;
    if ((a <= b ? b - a : a - b) < bytes) return rt_fail("%s: d_history_in and d_history_out overlap (the reads are gathers)", who);
  }
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_temporal(width, height, params, camera, previous_camera, d_color, d_coverage, d_albedo, d_normal, d_position,
                          d_history_in, d_history_out, d_out, d_length, d_image, (hipStream_t)stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
// Gives back the staging of the host-level calls and the memory of every RT_History, which start again from nothing (the objects
// stay their hosts').  D.mutex held, D's GPU current, device idle.
void release_temporal_state(Device &D) {
  std::vector<RT_History *> keep = std::move(D.temporal.histories);
  for (RT_History *h : keep) {
    h->buf[0].reset();
    h->buf[1].reset();
    h->valid = false;
  }
  D.temporal = TemporalState();
  D.temporal.histories = std::move(keep);
}

static const char *missing_history_plane(RT_History_Planes const *h) {
  return !h->color ? "color" : !h->length ? "length" : !h->coverage ? "coverage" : !h->normal ? "normal" : !h->position ? "position" : nullptr;
}

extern "C" int rt_temporal_accumulate_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                           Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                           RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                           f32 *length, u8 *image) {
  const char *who = "rt_temporal_accumulate_host";
  if (check_temporal(who, width, height, params) != 0) return -1;
  if (!camera) return rt_fail("%s: camera is NULL", who);
  if (history_in && !previous_camera) return rt_fail("%s: previous_camera is NULL and a history is given", who);
  if (!color) return rt_fail("%s: color is NULL", who);
  if (!planes) return rt_fail("%s: planes is NULL", who);
  if (!planes->coverage) return rt_fail("%s: planes->coverage is NULL", who);
  if (!planes->albedo && params->demodulate) return rt_fail("%s: planes->albedo is NULL and demodulate is set", who);
  if (!planes->normal) return rt_fail("%s: planes->normal is NULL", who);
  if (!planes->position) return rt_fail("%s: planes->position is NULL", who);
  if (history_in && missing_history_plane(history_in)) return rt_fail("%s: history_in->%s is NULL", who, missing_history_plane(history_in));
  if (history_out && missing_history_plane(history_out)) return rt_fail("%s: history_out->%s is NULL", who, missing_history_plane(history_out));
  if (!history_out && !out && !length && !image)
    return rt_fail("%s: no output is wanted (history_out, out, length and image are NULL)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  TemporalState &S = D.temporal;
  const size_t pixels = (size_t)width * height, f3 = pixels * 3 * sizeof(float), f1 = pixels * sizeof(float);
  HIP_TRY(S.in.grow(pixels * 13));
  HIP_TRY(S.planar.grow(pixels * 11));
  HIP_TRY(S.hist[0].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  HIP_TRY(S.hist[1].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  if (out) HIP_TRY(S.out.grow(pixels * 3));
  if (length) HIP_TRY(S.length.grow(pixels));
  if (image) HIP_TRY(S.image.grow(pixels * 3));
  float *d_col = S.in, *d_cov = S.in + pixels * 3, *d_alb = S.in + pixels * 4, *d_nrm = S.in + pixels * 7, *d_pos = S.in + pixels * 10;
  float *h_col = S.planar, *h_len = S.planar + pixels * 3, *h_cov = S.planar + pixels * 4, *h_nrm = S.planar + pixels * 5,
        *h_pos = S.planar + pixels * 8;
  hipStream_t stream = nullptr;                                 // (does not wait for the lane streams of frames in flight)
  HIP_TRY(hipMemcpy(d_col, color, f3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_cov, planes->coverage, f1, hipMemcpyHostToDevice));
  if (planes->albedo) HIP_TRY(hipMemcpy(d_alb, planes->albedo, f3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_nrm, planes->normal, f3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_pos, planes->position, f3, hipMemcpyHostToDevice));
  if (history_in) {
    HIP_TRY(hipMemcpy(h_col, history_in->color, f3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_len, history_in->length, f1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_cov, history_in->coverage, f1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_nrm, history_in->normal, f3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_pos, history_in->position, f3, hipMemcpyHostToDevice));
    int rc = rt_launch_temporal_pack((int)pixels, h_col, h_len, h_cov, h_nrm, h_pos, S.hist[0], stream);
    if (rc != 0) return rt_fail("temporal pack kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  if (enqueue_temporal(width, height, params, camera, previous_camera, d_col, d_cov, planes->albedo ? d_alb : nullptr, d_nrm, d_pos,
                       history_in ? S.hist[0].get() : nullptr, S.hist[1], out ? S.out.get() : nullptr,
                       length ? S.length.get() : nullptr, image ? S.image.get() : nullptr, stream) != 0)
    return -1;
  if (history_out) {
    int rc = rt_launch_temporal_unpack((int)pixels, S.hist[1], h_col, h_len, h_cov, h_nrm, h_pos, stream);
    if (rc != 0) return rt_fail("temporal unpack kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  if (history_out) {
    HIP_TRY(hipMemcpy(history_out->color, h_col, f3, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(history_out->length, h_len, f1, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(history_out->coverage, h_cov, f1, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(history_out->normal, h_nrm, f3, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(history_out->position, h_pos, f3, hipMemcpyDeviceToHost));
  }
  if (out) HIP_TRY(hipMemcpy(out, S.out, f3, hipMemcpyDeviceToHost));
  if (length) HIP_TRY(hipMemcpy(length, S.length, f1, hipMemcpyDeviceToHost));
  if (image) HIP_TRY(hipMemcpy(image, S.image, pixels * 3, hipMemcpyDeviceToHost));
  return 0;
}

// ---- the history a host keeps ---------------------------------------------------------------------------------------------------
extern "C" RT_History *rt_history_create(i32 width, i32 height) {
  if (width <= 0 || height <= 0 || (int64_t)width * height > (int64_t)1 << 28) {
    rt_fail("rt_history_create: image size %dx%d is invalid", width, height);
    return nullptr;
  }
  RT_History *h = new RT_History();
  h->width = width;
  h->height = height;
  memset(&h->camera, 0, sizeof h->camera);
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  D.temporal.histories.push_back(h);                            // (no device is touched: the memory comes with the first frame)
  return h;
}

extern "C" int rt_history_reset(RT_History *history) {
  if (!history) return rt_fail("rt_history_reset: history is NULL");
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  history->valid = false;                                       // (the memory stays for the next frame)
  return 0;
}

extern "C" void rt_history_destroy(RT_History *history) {
  if (!history) return;
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  auto &list = D.temporal.histories;
  list.erase(std::remove(list.begin(), list.end(), history), list.end());
  if (history->buf[0] || history->buf[1]) {                     // (memory exists only after a frame: the device is there)
    DeviceGuard guard(D);
    (void)hipDeviceSynchronize();                               // whatever still reads the histories finishes first
    history->buf[0].reset();
    history->buf[1].reset();
  }
  delete history;
}

// ---- behind a frame -----------------------------------------------------------------------------------------------------------
extern "C" int rt_render_temporal(Scene const *scene, Image const *image, isize samples, isize max_bounces, RT_History *history,
                                  RT_Temporal_Params const *temporal_params, RT_Guided_Params const *guided_params, f32 *linear_noisy,
                                  f32 *linear_out, f32 *length) {
  const char *who = "rt_render_temporal";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!image) return rt_fail("%s: image is NULL", who);
  if (!history) return rt_fail("%s: history is NULL", who);
  if (image->width <= 0 || image->height <= 0 || image->width > 0x7fffffff || image->height > 0x7fffffff)
    return rt_fail("%s: image size %ldx%ld is invalid", who, (long)image->width, (long)image->height);
  if (check_temporal(who, (i32)image->width, (i32)image->height, temporal_params) != 0) return -1;
  if (guided_params && check_guided(who, (i32)image->width, (i32)image->height, guided_params) != 0) return -1;
  if (image->pixels.data && image->components < 3) return rt_fail("%s: image needs >= 3 components", who);
  if (image->pixels.data && image->stride < image->width) return rt_fail("%s: image stride < width", who);
  if (samples <= 0 || samples > 0x7fffffff) return rt_fail("%s: samples must be positive and fit 32 bits (got %ld)", who, (long)samples);
  if (max_bounces < 0 || max_bounces > 0x7fffffff) return rt_fail("%s: max_bounces must be >= 0 and fit 32 bits (got %ld)", who, (long)max_bounces);
  if (!image->pixels.data && !linear_out && !length) return rt_fail("%s: no output is wanted (no pixels, no linear_out, no length)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (image->width != history->width || image->height != history->height)
    return rt_fail("%s: the image is %ldx%ld and the history %dx%d", who, (long)image->width, (long)image->height, history->width,
                   history->height);
  const double t_start = now_ms();
  if (ensure_device(D) != 0) return -1;
  if (rt_device_count() > 1)
    return rt_fail("%s: an accumulated frame renders on one device, and %d are set (rt_set_devices)", who, rt_device_count());
  RT_Render_Params p;
  memset(&p, 0, sizeof p);
  p.width = (i32)image->width;
  p.height = (i32)image->height;
  p.samples = (i32)samples;
  p.max_bounces = (i32)max_bounces;
  p.seed = g_seed.load();
  p.world = 1;
  if (check_params(&p) != 0) return -1;
  forget_multi_counters();

  FrameTiming T;
  Workspace &W = D.ws;
  FeatureState &F = D.features;
  GuidedState &G = D.guided;
  TemporalState &S = D.temporal;
  const size_t pixels = (size_t)p.width * p.height;
  if (ensure_ws_buffers(W, p.width, p.height, 0, 0) != 0) return -1;
  HIP_TRY(F.sums.grow(pixels * RT_FEATURE_CHANNELS));
  HIP_TRY(F.planes.grow(pixels * RT_FEATURE_CHANNELS));
  if (!history->buf[0] || !history->buf[1]) history->valid = false;          // (given back with the staging: from nothing)
  HIP_TRY(history->buf[0].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  HIP_TRY(history->buf[1].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  const bool want_out = guided_params || linear_out;
  if (want_out) HIP_TRY(S.out.grow(pixels * 3));
  if (length) HIP_TRY(S.length.grow(pixels));
  if (guided_params) {
    HIP_TRY(G.work.grow(pixels * RT_GUIDED_WORK_PER_PIXEL));
    if (linear_out) HIP_TRY(G.out.grow(pixels * 3));
  }
  float *d_cov = F.planes, *d_alb = F.planes + pixels, *d_nrm = F.planes + pixels * 4, *d_pos = F.planes + pixels * 7;
  const uint8_t *h_in = history->valid ? history->buf[history->cur].get() : nullptr;
  uint8_t *h_out = history->buf[history->cur ^ 1];
  hipStream_t stream = nullptr;
  // the frame's linear values, the four planes of its feature pass, the accumulation, the filter: W.image receives the encoding of
  // the last stage.  (A pass that is run again after a scene edit reads the same old history and writes the same new one.)
  auto pass = [&](RT_Device_Scene *d) -> int {
    if (enqueue_frame(D, d, &scene->camera, &p, W, stream, 0, nullptr, nullptr, W.linear) != 0) return -1;
    HIP_TRY(hipMemsetAsync(F.sums, 0, pixels * RT_FEATURE_CHANNELS * sizeof(unsigned long long), stream));
    if (enqueue_features(D, d, &scene->camera, &p, F.sums, stream) != 0) return -1;
    if (enqueue_resolve(&p, F.sums, d_cov, d_alb, d_nrm, d_pos, stream) != 0) return -1;
    if (enqueue_temporal(p.width, p.height, temporal_params, &scene->camera, &history->camera, W.linear, d_cov, d_alb, d_nrm, d_pos,
                         h_in, h_out, want_out ? S.out.get() : nullptr, length ? S.length.get() : nullptr,
                         guided_params ? nullptr : W.image.get(), stream) != 0)
      return -1;
    if (!guided_params) return 0;
    return enqueue_guided(p.width, p.height, guided_params, S.out, d_cov, d_alb, d_nrm, d_pos, linear_out ? G.out.get() : nullptr,
                          W.image, G.work, stream);
  };
  if (!scene_checked(D, scene, stream, &T, pass)) {
    history->valid = false;                                     // (the new history may be half written, the old one is not current)
    return -1;
  }
  history->cur ^= 1;
  history->valid = true;
  history->camera = scene->camera;

  if (copy_image_out(image, W.image, p.width, p.height, stream) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[4], stream));
  if (linear_noisy) HIP_TRY(hipMemcpy(linear_noisy, W.linear, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (linear_out) HIP_TRY(hipMemcpy(linear_out, guided_params ? G.out.get() : S.out.get(), pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (length) HIP_TRY(hipMemcpy(length, S.length, pixels * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  frame_split(W, T);
  T.total_ms = (float)(now_ms() - t_start);
  D.timing = T;
  return 0;
}
