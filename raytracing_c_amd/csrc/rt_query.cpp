// rt_query.cpp -- batch ray queries (include/rt_hip.h): closest hit, occlusion and full hit records for rays the host supplies,
// on the device level (device pointers, one launch on the caller's stream) and on the host level (host arrays, the cached device
// copy of a Scene through scene_checked, rt_residency.cpp, slices of RT_QUERY_SLICE rays).  The work is rt_query_kernel and
// rt_hit_attributes_kernel (rt_kernels.hip); nothing here computes a hit on the CPU.  Behind them, the light probes (below).

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

// ==== light probes (include/rt_hip.h, "light probes") ==========================================================================
// Path-traced samples of the incoming radiance at points the host supplies and their projection onto nine spherical harmonics, on
// the device level (device pointers, launches on the caller's stream) and on the host level (host arrays, the cached device copy of
// a Scene through scene_checked, slices of RT_PROBE_SLICE paths).  They live in this unit because they are the queries' shape -- a
// list the host supplies, one persistent kernel with one work counter, a ring slot per call, staged slices -- and take their ring
// slot from the ring above.  The work is rt_probe_kernel, rt_probe_project_kernel and rt_probe_resolve_kernel (rt_probes.hip);
// nothing here traces a path or forms a sum on the CPU.

static_assert(sizeof(RT_Probe_Sample) == 32 && sizeof(RT_Probe_Sample) == RT_PROBE_RECORD_F4 * 16, "RT_Probe_Sample is two 16-byte stores");
static_assert(sizeof(RT_Probe_Params) == 24, "RT_Probe_Params");
static_assert(RT_PROBE_COEFFS * 3 == RT_PROBE_SUMS, "nine coefficients x rgb");
static_assert(sizeof(Vec3) == 12, "a position is f32[3]");
static_assert(RT_CNT_TEXTURED < 8, "the probe counters fit the slot's eight words");

static std::atomic<Device *> g_probe_dev{nullptr};      // the device of the most recent probe call (rt_get_probe_counters)

// What can be checked without the device.  `who` prefixes the messages; *count = the sample range's length (0 = all resolved).
static int check_probe_params(const char *who, RT_Probe_Params const *p, i64 n, i32 *count) {
  if (!p) return rt_fail("%s: probe params are NULL", who);
  if (n <= 0) return rt_fail("%s: n must be positive (got %lld)", who, (long long)n);
  if (p->samples <= 0) return rt_fail("%s: samples must be positive (got %d)", who, p->samples);
  if (p->sample_first < 0 || p->sample_count < 0 || (i64)p->sample_first + p->sample_count > p->samples)
    return rt_fail("%s: sample range [%d, +%d) outside [0, %d]", who, p->sample_first, p->sample_count, p->samples);
  if (p->max_bounces < 0) return rt_fail("%s: max_bounces must be >= 0 (got %d)", who, p->max_bounces);
  if ((u64)p->probe_first + (u64)n > ((u64)1 << 32))
    return rt_fail("%s: probe_first %u + n %lld exceeds the 32-bit probe index", who, p->probe_first, (long long)n);
  *count = p->sample_count ? p->sample_count : p->samples - p->sample_first;
  return 0;
}

// ... and of a device-level call: one launch holds every path
static int check_probe_paths(const char *who, i64 n, i32 count) {
  if (n * (i64)count > RT_PROBE_MAX_PATHS)
    return rt_fail("%s: too many paths (%lld probes x %d samples > 2^30 per call)", who, (long long)n, count);
  return 0;
}

static int ensure_probe_state(Device &D) {              // D.mutex held, D's GPU current
  if (ensure_query_state(D) != 0) return -1;
  HIP_TRY(D.probes.slots.grow(RT_QUERY_SLOTS * RT_PROBE_SLOT_BYTES));
  return 0;
}

// The ring slot of a new probe call: the query ring's next slot (its event orders the reuse) and the probe ring's words of it.
static int acquire_probe_slot(Device &D, int *slot) {
  if (ensure_probe_state(D) != 0 || acquire_slot(D, slot, false) != 0) return -1;
  D.probes.last = *slot;
  g_probe_dev.store(&D);
  return 0;
}

void release_probe_state(Device &D) {
  D.probes = ProbeState();
  Device *self = &D;
  g_probe_dev.compare_exchange_strong(self, nullptr);
}

// Enqueues one launch of the probe kernel on `stream`: n probes x count samples from q->sample_first.  `fresh`: the slot's counters
// start at zero (the first launch of a call); its work counter always does.  D.mutex held, D's GPU current, every pointer on D.
static int enqueue_trace(Device &D, RT_Device_Scene *d, RT_Probe_Params const *q, i32 count, i64 n, const float *positions,
                         float *records, hipStream_t stream, int slot, bool fresh) {
  uint8_t *sl = D.probes.slots + (size_t)slot * RT_PROBE_SLOT_BYTES;
  if (fresh) HIP_TRY(hipMemsetAsync(sl, 0, RT_PROBE_SLOT_BYTES, stream));
  else HIP_TRY(hipMemsetAsync(sl + 64, 0, 4, stream));
  RT_KParams K;
  scene_only_kparams(&K, d);
  K.max_bounces = q->max_bounces;
  K.seed = q->seed;
  RT_PParams R;
  memset(&R, 0, sizeof R);
  R.positions = positions;
  R.records = records;
  R.counters = (unsigned long long *)sl;
  R.head = (uint32_t *)(sl + 64);
  const int64_t n_paths = n * (int64_t)count;
  R.n_paths = (int32_t)n_paths;
  R.sample_count = count;
  R.sample_first = q->sample_first;
  R.probe_first = q->probe_first;

  // launch geometry: the query kernel's (rt_query.cpp) -- one workgroup of 16 waves per CU, the tree fills the LDS beside the waves'
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
  // finished lanes that end a traversal call while paths are left: what follows is the path kernel's S block, whose threshold it is
  R.exit_lanes = knob_int("RT_PROBE_EXIT", 48);
  if (R.exit_lanes < 1 || R.exit_lanes > 64) R.exit_lanes = 48;
  int rc = rt_launch_probes(&K, &R, (int)blocks, S.smem, stream);
  if (rc != 0) return rt_fail("probe kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  HIP_TRY(hipEventRecord(D.query.done[slot], stream));
  return 0;
}

static int enqueue_project(i64 n, i32 count, const void *records, void *sums, hipStream_t stream) {
  int rc = rt_launch_probe_project((int)n, count, (const float *)records, (unsigned long long *)sums, stream);
  if (rc != 0) return rt_fail("probe projection kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

static int enqueue_resolve(i64 n, i32 samples, const void *sums, void *coeffs, hipStream_t stream) {
  int rc = rt_launch_probe_resolve((long long)n * RT_PROBE_SUMS, samples, (const unsigned long long *)sums, (float *)coeffs, stream);
  if (rc != 0) return rt_fail("probe resolve kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- device level -------------------------------------------------------------------------------------------------------------
extern "C" int rt_probe_trace(RT_Device_Scene *dscene, RT_Probe_Params const *params, i64 n, void const *d_positions, void *d_samples,
                              void *stream) {
  const char *who = "rt_probe_trace";
  // (everything that can be checked without the device is checked before it is touched)
  if (!dscene) return rt_fail("%s: device scene is NULL", who);
  i32 count = 0;
  if (check_probe_params(who, params, n, &count) != 0 || check_probe_paths(who, n, count) != 0) return -1;
  if (!d_positions) return rt_fail("%s: d_positions is NULL", who);
  if (!d_samples) return rt_fail("%s: d_samples is NULL", who);
  if ((uintptr_t)d_samples & 15) return rt_fail("%s: d_samples is not 16-byte aligned", who);
  if (count == 0) return 0;                                     // (an empty range at the end of the samples: nothing to trace)
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  int slot = 0;
  if (acquire_probe_slot(D, &slot) != 0) return -1;
  return enqueue_trace(D, dscene, params, count, n, (const float *)d_positions, (float *)d_samples, (hipStream_t)stream, slot, true);
}

extern "C" int rt_probe_project(RT_Probe_Params const *params, i64 n, void const *d_samples, void *d_sums, void *stream) {
  const char *who = "rt_probe_project";
  i32 count = 0;
  if (check_probe_params(who, params, n, &count) != 0 || check_probe_paths(who, n, count) != 0) return -1;
  if (!d_samples) return rt_fail("%s: d_samples is NULL", who);
  if (!d_sums) return rt_fail("%s: d_sums is NULL", who);
  if ((uintptr_t)d_samples & 15) return rt_fail("%s: d_samples is not 16-byte aligned", who);
  if (count == 0) return 0;
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_project(n, count, d_samples, d_sums, (hipStream_t)stream);
}

extern "C" int rt_probe_resolve(RT_Probe_Params const *params, i64 n, void const *d_sums, void *d_coeffs, void *stream) {
  const char *who = "rt_probe_resolve";
  i32 count = 0;
  if (check_probe_params(who, params, n, &count) != 0) return -1;
  if (n > RT_PROBE_MAX_PATHS) return rt_fail("%s: too many probes (%lld > 2^30 per call)", who, (long long)n);
  if (!d_sums) return rt_fail("%s: d_sums is NULL", who);
  if (!d_coeffs) return rt_fail("%s: d_coeffs is NULL", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_resolve(n, params->samples, d_sums, d_coeffs, (hipStream_t)stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
// Probes go through the device in GROUPS of as many whole probes as one slice holds; a probe whose sample range is longer than a
// slice is a group of its own, traced in several launches by sample range.  The group's 27 sums per probe are zeroed in front of
// its first launch, added to by every launch's projection, and resolved and copied out behind its last.
extern "C" int rt_scene_probes(Scene const *scene, RT_Probe_Params const *params, i64 n, Vec3 const *positions, f32 *coeffs, u64 *sums,
                               RT_Probe_Sample *samples) {
  const char *who = "rt_scene_probes";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  i32 count = 0;
  if (check_probe_params(who, params, n, &count) != 0) return -1;
  if (!positions) return rt_fail("%s: positions is NULL", who);
  if (!coeffs && !sums && !samples) return rt_fail("%s: no output is wanted (coeffs, sums and samples are NULL)", who);

  Device &D = dev0();                                            // (the primary device only, whatever rt_device_count() says)
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  ProbeState &S = D.probes;
  const i64 per = count > 0 && count <= RT_PROBE_SLICE ? RT_PROBE_SLICE / count : 1;      // probes of a group
  const i32 chunk = count <= RT_PROBE_SLICE ? count : (i32)RT_PROBE_SLICE;                  // samples of a launch
  const i64 group = n < per ? n : per;
  HIP_TRY(S.positions.grow((size_t)group * 3));
  HIP_TRY(S.records.grow((size_t)group * (size_t)(chunk > 0 ? chunk : 1) * 8));
  HIP_TRY(S.sums.grow((size_t)group * RT_PROBE_SUMS));
  if (coeffs) HIP_TRY(S.coeffs.grow((size_t)group * RT_PROBE_SUMS));
  int slot = 0;
  if (acquire_probe_slot(D, &slot) != 0) return -1;
  hipStream_t stream = nullptr;
  RT_Device_Scene *d = nullptr;
  bool first = true;
  for (i64 b = 0; b < n; b += per) {
    const i64 m = n - b < per ? n - b : per;
    if (count == 0) HIP_TRY(hipMemsetAsync(S.sums, 0, (size_t)m * RT_PROBE_SUMS * 8, stream));      // (an empty range: zero sums)
    for (i32 f = 0; f < count; f += chunk) {
      RT_Probe_Params q = *params;
      q.sample_first = params->sample_first + f;
      q.sample_count = count - f < chunk ? count - f : chunk;
      q.probe_first = params->probe_first + (u32)b;
      auto trace_slice = [&](RT_Device_Scene *ds) -> int {
        if (f == 0) {
          HIP_TRY(hipMemcpy(S.positions, positions + b, (size_t)m * 12, hipMemcpyHostToDevice));
          HIP_TRY(hipMemsetAsync(S.sums, 0, (size_t)m * RT_PROBE_SUMS * 8, stream));
        }
        if (enqueue_trace(D, ds, &q, q.sample_count, m, S.positions, S.records, stream, slot, first) != 0) return -1;
        return (coeffs || sums) ? enqueue_project(m, q.sample_count, S.records, S.sums, stream) : 0;
      };
      // the scene is checked behind the first launch (edited since the copy: uploaded, traced again); later ones use that copy
      if (first) d = scene_checked(D, scene, stream, nullptr, trace_slice);
      if (!d || (!first && trace_slice(d) != 0)) return -1;
      first = false;
      if (samples)      // (m whole probes from sample 0 of the range, or one probe's samples from f: contiguous either way)
        HIP_TRY(hipMemcpy(samples + (size_t)b * (size_t)count + f, S.records, (size_t)m * (size_t)q.sample_count * sizeof(RT_Probe_Sample),
                          hipMemcpyDeviceToHost));
    }
    if (coeffs) {
      if (enqueue_resolve(m, params->samples, S.sums, S.coeffs, stream) != 0) return -1;
      HIP_TRY(hipMemcpy(coeffs + (size_t)b * RT_PROBE_SUMS, S.coeffs, (size_t)m * RT_PROBE_SUMS * 4, hipMemcpyDeviceToHost));
    }
    if (sums) HIP_TRY(hipMemcpy(sums + (size_t)b * RT_PROBE_SUMS, S.sums, (size_t)m * RT_PROBE_SUMS * 8, hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int rt_get_probe_counters(RT_Counters *out) {
  if (!out) return rt_fail("rt_get_probe_counters: NULL");
  memset(out, 0, sizeof *out);
  Device *Dp = g_probe_dev.load();
  if (!Dp) return 0;                                           // no probe call yet: zeros
  Device &D = *Dp;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  if (D.probes.last < 0 || !D.probes.slots) return 0;
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long c[8];
  HIP_TRY(hipMemcpy(c, D.probes.slots + (size_t)D.probes.last * RT_PROBE_SLOT_BYTES, sizeof c, hipMemcpyDeviceToHost));
  out->paths = c[RT_CNT_PATHS];
  out->rays = c[RT_CNT_RAYS];
  out->node_visits = c[RT_CNT_NODES];
  out->leaf_visits = c[RT_CNT_LEAVES];
  out->shades = c[RT_CNT_SHADES];
  out->backgrounds = c[RT_CNT_BG];
  out->textured = c[RT_CNT_TEXTURED];
  return 0;
}
