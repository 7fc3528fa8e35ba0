// rt_query.cpp -- batch ray queries (include/rt_hip.h): closest hit, occlusion and full hit records for rays the host supplies,
// on the device level (device pointers, one launch on the caller's stream) and on the host level (host arrays, the cached device
// copy of a Scene through scene_checked, rt_residency.cpp, slices of RT_QUERY_SLICE rays).  The work is rt_query_kernel and
// rt_hit_attributes_kernel (rt_kernels.hip); nothing here computes a hit on the CPU.

#include "rt_host.h"

#include <stddef.h>

static_assert(sizeof(RT_Ray_Hit) == 16, "RT_Ray_Hit is one 16-byte store");
static_assert(sizeof(RT_Device_Hit) == sizeof(Hit) && sizeof(RT_Device_Hit) == RT_HIT_DWORDS * 4, "RT_Device_Hit is Hit-sized");
static_assert(offsetof(RT_Device_Hit, tex_coords) == offsetof(Hit, tex_coords) && offsetof(RT_Device_Hit, triangle) == offsetof(Hit, shader),
              "RT_Device_Hit is Hit with the Shader pair replaced");
static_assert(sizeof(Ray) == 24, "Ray is f32[6]");

static std::atomic<Device *> g_query_dev{nullptr};      // the device of the most recent query call (rt_get_query_counters)

// ---- launch geometry: waves per workgroup, workgroups, BVH nodes in LDS, rays per grab --------------------------------------
static void query_geometry(const Device &D, const RT_Device_Scene *d, int n, RT_KParams &K, RT_QParams &Q, int *wg_waves, int *n_blocks,
                           int *smem) {
  // One workgroup per CU as in the path kernel (the tree fills the LDS).  A batch that gives every ray a lane of its own even with
  // 8 waves per CU runs with 8: nothing is refilled, the launch is the tail the path kernel's small launches are (rt_launch.cpp,
  // launch_geometry), and two waves per SIMD issue faster than four.  Every other batch takes all 16.
  *wg_waves = (int64_t)n <= (int64_t)D.num_cus * 8 * 64 ? 8 : 16;
  int v = knob_int("RT_QUERY_WG_WAVES", 0);
  if (v == 8 || v == 16) *wg_waves = v;
  const LdsSplit S = lds_split(d, K.depth, *wg_waves, 0, 1, false);      // nodes beside the waves' perm stacks; no static table
  K.n_lds_nodes = S.n_lds_nodes;
  *smem = S.smem;
  const int wg_lanes = *wg_waves * 64;
  int blocks = (n + wg_lanes - 1) / wg_lanes;
  if (blocks > D.num_cus) blocks = D.num_cus;
  if (blocks < 1) blocks = 1;
  *n_blocks = blocks;
  // Rays per grab: an eighth of a wave's mean share, in whole wave-fulls, within [64, 512] (why: rt_query_kernel)
  int grab = n / (blocks * *wg_waves * 8) / 64 * 64;
  Q.grab = grab < 64 ? 64 : (grab > 512 ? 512 : grab);
  // Finished lanes that end a traversal call while rays are left: a refill here is a 24-byte read and three divisions -- cheap
  // beside the path kernel's shade block, whose threshold is 48 -- so lanes are refilled once a quarter of the wave waits.
  Q.exit_lanes = knob_int("RT_QUERY_EXIT", 16);
  if (Q.exit_lanes < 1 || Q.exit_lanes > 64) Q.exit_lanes = 16;
}

int ensure_query_state(Device &D) {                     // D.mutex held, D's GPU current
  HIP_TRY(D.query.slots.grow(RT_QUERY_SLOTS * 64));
  return 0;
}

// The ring slot of a new launch (`query`: of a query call; a feature pass only borrows the slot's work counter and leaves what
// rt_get_query_counters() reports alone).  D.mutex held, D's GPU current.
int acquire_slot(Device &D, int *slot, bool query) {
  QueryState &S = D.query;
  const int s = (int)(S.next++ % RT_QUERY_SLOTS);
  HIP_TRY(S.done[s].ensure(hipEventDisableTiming));
  if (S.used[s]) HIP_TRY(hipEventSynchronize(S.done[s]));      // (its launch of RT_QUERY_SLOTS calls ago, long over)
  S.used[s] = true;
  if (query) {
    S.last = s;
    g_query_dev.store(&D);
  }
  *slot = s;
  return 0;
}

// Enqueues one query launch (+ the attribute kernel when `full`) on `stream`.  `fresh`: the slot's counters start at zero (the
// first launch of a call); its work counter always does.  D.mutex held, D's GPU current, every pointer on D.
static int enqueue_query(Device &D, RT_Device_Scene *d, int n, const float *rays, const float *t_max, float *hits, float *full,
                         uint8_t *flags, hipStream_t stream, int slot, bool fresh) {
  QueryState &S = D.query;
  uint8_t *sl = S.slots + (size_t)slot * 64;
  if (fresh) HIP_TRY(hipMemsetAsync(sl, 0, 64, stream));
  else HIP_TRY(hipMemsetAsync(sl + 32, 0, 4, stream));
  RT_KParams K;
  scene_only_kparams(&K, d);
  RT_QParams Q;
  memset(&Q, 0, sizeof Q);
  Q.rays = rays;
  Q.t_max = t_max;
  Q.hits = hits;
  Q.flags = flags;
  Q.counters = (unsigned long long *)sl;
  Q.head = (uint32_t *)(sl + 32);
  Q.n = n;
  int wg_waves, n_blocks, smem;
  query_geometry(D, d, n, K, Q, &wg_waves, &n_blocks, &smem);
  int rc = rt_launch_query(&K, &Q, flags != nullptr, wg_waves, n_blocks, smem, stream);
  if (rc != 0) return rt_fail("query kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  if (full) {
    rc = rt_launch_hit_attributes(&K, n, rays, hits, full, stream);
    if (rc != 0) return rt_fail("hit attribute kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  HIP_TRY(hipEventRecord(S.done[slot], stream));
  return 0;
}

static int check_count(i64 n, const char *who) {
  if (n <= 0) return rt_fail("%s: n must be positive (got %lld)", who, (long long)n);
  if (n > RT_QUERY_MAX_RAYS) return rt_fail("%s: too many rays (%lld > 2^30 per call)", who, (long long)n);
  return 0;
}

// ---- device level -------------------------------------------------------------------------------------------------------------
static int query_device(const char *who, RT_Device_Scene *dscene, i64 n, void const *d_rays, void const *d_t_max, void *d_hits,
                        void *d_full, void *d_flags, bool any, void *stream) {
  // (everything that can be checked without the device is checked before it is touched)
  if (!dscene) return rt_fail("%s: device scene is NULL", who);
  if (check_count(n, who) != 0) return -1;
  if (!d_rays) return rt_fail("%s: d_rays is NULL", who);
  if (any && !d_flags) return rt_fail("%s: d_flags is NULL", who);
  if (!any && !d_hits) return rt_fail("%s: d_hits is NULL", who);
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  int slot = 0;
  if (ensure_query_state(D) != 0 || acquire_slot(D, &slot) != 0) return -1;
  return enqueue_query(D, dscene, (int)n, (const float *)d_rays, (const float *)d_t_max, (float *)d_hits, (float *)d_full,
                       (uint8_t *)d_flags, (hipStream_t)stream, slot, true);
}

extern "C" int rt_query_closest(RT_Device_Scene *dscene, i64 n, void const *d_rays, void const *d_t_max, void *d_hits, void *d_full,
                                void *stream) {
  return query_device("rt_query_closest", dscene, n, d_rays, d_t_max, d_hits, d_full, nullptr, false, stream);
}

extern "C" int rt_query_occluded(RT_Device_Scene *dscene, i64 n, void const *d_rays, void const *d_t_max, void *d_flags, void *stream) {
  return query_device("rt_query_occluded", dscene, n, d_rays, d_t_max, nullptr, nullptr, d_flags, true, stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
template void std::vector<f32>::resize(size_t);      // (in the library's export list, like unordered_map::erase in rt_residency.cpp)

// Gives back what a device's query state holds (ring, events, staging).  D.mutex held, D's GPU current, device idle.
void release_query_state(Device &D) {
  D.query = QueryState();
  Device *self = &D;
  g_query_dev.compare_exchange_strong(self, nullptr);
}

// The three host-level forms: rt_scene_hits (hits), rt_scene_closest (records), rt_scene_occluded (flags); exactly one of the
// three outputs is not NULL.  Arguments are checked by the callers.  They run on the NULL stream, like rt_render_frame(): it does
// not wait for the non-blocking streams of frames in flight (rt_frame_begin), so a query overlaps such a frame.
static int query_host(Scene const *scene, i64 n, Ray const *rays, f32 const *t_max, Hit *hits, i32 *triangles, RT_Ray_Hit *records_out,
                      u8 *flags) {
  Device &D = dev0();                                          // (the primary device only, whatever rt_device_count() says)
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  if (ensure_query_state(D) != 0) return -1;
  QueryState &S = D.query;
  const bool any = flags != nullptr;
  const size_t slice = (size_t)(n < RT_QUERY_SLICE ? n : RT_QUERY_SLICE);
  // staging on the device, kept for the next call: rays 24 + t_max 4 B per ray of a slice, then flags 1, or hit records 16 and --
  // rt_scene_hits only -- full records 88
  HIP_TRY(S.rays.grow(slice * 6));
  HIP_TRY(S.t_max.grow(slice));
  if (any) HIP_TRY(S.flags.grow(slice));
  if (!any) HIP_TRY(S.hits.grow(slice * 4));
  if (hits) HIP_TRY(S.full.grow(slice * RT_HIT_DWORDS));
  int slot = 0;
  if (acquire_slot(D, &slot) != 0) return -1;
  hipStream_t stream = nullptr;
  std::vector<f32> bounds;
  std::vector<RT_Device_Hit> records;
  RT_Device_Scene *d = nullptr;
  for (i64 base = 0; base < n; base += RT_QUERY_SLICE) {
    const int m = (int)(n - base < RT_QUERY_SLICE ? n - base : RT_QUERY_SLICE);
    const f32 *bound = t_max ? t_max + base : nullptr;
    if (hits) {                                                // the reference's protocol: hit.distance on entry is the bound
      bounds.resize((size_t)m);
      for (int i = 0; i < m; i++) bounds[(size_t)i] = hits[base + i].distance;
      bound = bounds.data();
    }
    auto trace_slice = [&](RT_Device_Scene *ds) -> int {
      HIP_TRY(hipMemcpy(S.rays, rays + base, (size_t)m * 24, hipMemcpyHostToDevice));
      if (bound) HIP_TRY(hipMemcpy(S.t_max, bound, (size_t)m * 4, hipMemcpyHostToDevice));
      return enqueue_query(D, ds, m, S.rays, bound ? S.t_max : nullptr, any ? nullptr : S.hits, hits ? S.full : nullptr,
                           any ? S.flags : nullptr, stream, slot, base == 0);
    };
    // the scene is checked behind the first slice (edited since the copy: uploaded, traced again); later slices use that slice's copy
    if (base == 0) d = scene_checked(D, scene, stream, nullptr, trace_slice);
    if (!d || (base != 0 && trace_slice(d) != 0)) return -1;
    if (any) {
      HIP_TRY(hipMemcpy(flags + base, S.flags, (size_t)m, hipMemcpyDeviceToHost));
    } else if (records_out) {
      HIP_TRY(hipMemcpy(records_out + base, S.hits, (size_t)m * sizeof(RT_Ray_Hit), hipMemcpyDeviceToHost));
    } else {
      records.resize((size_t)m);
      HIP_TRY(hipMemcpy(records.data(), S.full, (size_t)m * sizeof(RT_Device_Hit), hipMemcpyDeviceToHost));
      for (int i = 0; i < m; i++) {
        const RT_Device_Hit &r = records[(size_t)i];
        if (r.triangle >= 0) {
          Hit &h = hits[base + i];
          memcpy(&h, &r, offsetof(Hit, shader));
          h.shader = scene->triangles.aos[r.triangle].shader;
        }
        if (triangles) triangles[base + i] = r.triangle;
      }
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

static int check_host(const char *who, Scene const *scene, i64 n, Ray const *rays, const void *out, const char *out_name) {
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (check_count(n, who) != 0) return -1;
  if (!rays) return rt_fail("%s: rays is NULL", who);
  if (!out) return rt_fail("%s: %s is NULL", who, out_name);
  return 0;
}

extern "C" int rt_scene_hits(Scene const *scene, i64 n, Ray const *rays, Hit *hits, i32 *triangles) {
  if (check_host("rt_scene_hits", scene, n, rays, hits, "hits") != 0) return -1;
  return query_host(scene, n, rays, nullptr, hits, triangles, nullptr, nullptr);
}

extern "C" int rt_scene_closest(Scene const *scene, i64 n, Ray const *rays, f32 const *t_max, RT_Ray_Hit *hits) {
  if (check_host("rt_scene_closest", scene, n, rays, hits, "hits") != 0) return -1;
  return query_host(scene, n, rays, t_max, nullptr, nullptr, hits, nullptr);
}

extern "C" int rt_scene_occluded(Scene const *scene, i64 n, Ray const *rays, f32 const *t_max, u8 *flags) {
  if (check_host("rt_scene_occluded", scene, n, rays, flags, "flags") != 0) return -1;
  return query_host(scene, n, rays, t_max, nullptr, nullptr, nullptr, flags);
}

extern "C" int rt_get_query_counters(RT_Query_Counters *out) {
  if (!out) return rt_fail("rt_get_query_counters: NULL");
  memset(out, 0, sizeof *out);
  Device *Dp = g_query_dev.load();
  if (!Dp) return 0;                                           // no query yet: zeros
  Device &D = *Dp;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (D.query.last < 0 || !D.query.slots) return 0;
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long c[RT_QUERY_COUNTERS];
  HIP_TRY(hipMemcpy(c, D.query.slots + (size_t)D.query.last * 64, sizeof c, hipMemcpyDeviceToHost));
  out->rays = c[RT_QCNT_RAYS];
  out->hits = c[RT_QCNT_HITS];
  out->node_visits = c[RT_QCNT_NODES];
  out->leaf_visits = c[RT_QCNT_LEAVES];
  return 0;
}
