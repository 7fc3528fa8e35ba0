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
