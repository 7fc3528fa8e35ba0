// rt_launch.cpp -- one launch of the path tracer, resolve and untile, workspace buffers, counters and kernel timing.

#include "rt_host.h"

static std::atomic<int> g_taps_form{-1};      // rt_get_shade_taps_form(): the texture stage of the last path-kernel launch

int check_params(RT_Render_Params const *p) {
  if (!p) return rt_fail("render params are NULL");
  if (p->width <= 0 || p->height <= 0) return rt_fail("image size %dx%d is invalid", p->width, p->height);
  if ((int64_t)p->width * p->height > (int64_t)1 << 28) return rt_fail("image %dx%d is too large", p->width, p->height);
  if (p->samples <= 0) return rt_fail("samples must be positive (got %d)", p->samples);
  if (p->max_bounces < 0) return rt_fail("max_bounces must be >= 0 (got %d)", p->max_bounces);
  if (p->world <= 0 || p->rank < 0 || p->rank >= p->world) return rt_fail("rank %d / world %d is invalid", p->rank, p->world);
  if (p->sample_first < 0 || p->sample_count < 0 || p->sample_first + p->sample_count > p->samples)
    return rt_fail("sample range [%d, +%d) outside [0, %d)", p->sample_first, p->sample_count, p->samples);
  return 0;
}

int check_image_size(const char *who, i32 width, i32 height) {
  if (width <= 0 || height <= 0) return rt_fail("%s: image size %dx%d is invalid", who, width, height);
  if ((int64_t)width * height > RT_MAX_PIXELS) return rt_fail("%s: image %dx%d is too large (more than 2^28 pixels)", who, width, height);
  return 0;
}

int check_views(i32 n_views, RT_View const *views, i32 width, i32 height, const char *who) {
  if (n_views <= 0) return rt_fail("%s: n_views must be positive (got %d)", who, n_views);
  if (!views) return rt_fail("%s: views is NULL", who);
  if (width <= 0 || height <= 0) return rt_fail("%s: image size %dx%d is invalid", who, width, height);
  // (the kernel's pixel and tile indices are 32-bit: the bound check_params puts on one frame, over the whole batch)
  if ((int64_t)n_views * width * height > (int64_t)1 << 28)
    return rt_fail("%s: %d views of %dx%d are too many pixels (more than 2^28)", who, n_views, width, height);
  if ((int64_t)n_views * rt_chunk_count(width, height) * 16 > (int64_t)0x7fffffff)
    return rt_fail("%s: %d views of %dx%d are too many tiles (2^31 or more)", who, n_views, width, height);
  return 0;
}

int check_chunk_list(const char *who, i32 width, i32 height, i32 n_list, i32 const *chunks) {
  if (n_list < 0) return rt_fail("%s: n_list must be >= 0 (got %d)", who, n_list);
  if (n_list > 0 && !chunks) return rt_fail("%s: chunks is NULL", who);
  const i32 n_chunks = rt_chunk_count(width, height);
  for (i32 k = 0; k < n_list; k++) {
    if (chunks[k] < 0 || chunks[k] >= n_chunks)
      return rt_fail("%s: chunks[%d] = %d is outside [0, %d), the chunks of a %dx%d image", who, k, chunks[k], n_chunks, width, height);
    if (k > 0 && chunks[k] <= chunks[k - 1])
      return rt_fail("%s: chunks[%d] = %d after chunks[%d] = %d: the list must be strictly ascending", who, k, chunks[k], k - 1,
                     chunks[k - 1]);
  }
  return 0;
}

// The size limit of one launch, unchanged since a launch was cut into (tile x block of samples) items counted in 32 bits: blocks
// of p->slab samples, or by default the largest of 32 / 16 / 8 that leaves 24 items per wave of a full grid.  No kernel counts
// such items any more, but the limit still decides which launches are refused: check_params / check_views bound pixels and
// tiles, not samples (1024 x 1024 pixels at 2^23 samples pass them and are refused here).
static int check_launch_size(const Device &D, int tiles_per_view, int n_views, int n_samples, int slab) {
  if (slab <= 0) {
    slab = 8;
    for (int cand = 32; cand > 8; cand >>= 1)
      if ((int64_t)tiles_per_view * ((n_samples + cand - 1) / cand) >= (int64_t)24 * D.num_cus * 16) { slab = cand; break; }
  }
  int shift = 0;
  while ((1 << shift) < slab && (1 << shift) < n_samples) shift++;
  const int64_t items = (int64_t)tiles_per_view * ((n_samples + (1 << shift) - 1) >> shift) * n_views;
  if (items > 0x7fffffff) return rt_fail("too many work items (%lld)", (long long)items);
  return 0;
}

void camera_rows(float dst[3][4], Camera const *cam) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) dst[i][j] = cam->view_matrix.rows[i][j];
}

void camera_frame_kparams(RT_KParams *K, Camera const *cam, RT_Render_Params const *p) {
  camera_rows(K->cam, cam);
  K->focal_length = cam->focal_length;
  {
    volatile float fw = (float)p->width, fh = (float)p->height;      // plain IEEE fp32 divisions (raytracer.c:615-617), as the kernel used to do
    volatile float iw = 1.0f / fw, ih = 1.0f / fh, asp = fw / fh;
    K->inv_width = iw;
    K->inv_height = ih;
    K->aspect = asp;
  }
  K->width = p->width;
  K->height = p->height;
  K->samples = p->samples;
  K->max_bounces = p->max_bounces;
  K->sample_first = p->sample_first;
  K->sample_end = p->sample_count > 0 ? p->sample_first + p->sample_count : p->samples;
}

LdsSplit lds_split(const RT_Device_Scene *d, int depth, int wg_waves, int wave_extra_bytes, int wgs_per_cu, bool static_table) {
  const int per_wave = (depth > 0 ? depth : 1) * RT_LDS_PERM_LEVEL_BYTES + wave_extra_bytes;
  const int budget = (RT_LDS_BYTES - (static_table ? RT_LDS_TABLE_BYTES : 0)) / wgs_per_cu;
  int room = (budget - wg_waves * per_wave) / RT_LDS_NODE_BYTES;
  if (room < 0) room = 0;
  int n = d->n_nodes < room ? d->n_nodes : room;
  if (!d->boxes_ordered) n = 0;
  return {n, n * RT_LDS_NODE_BYTES + wg_waves * per_wave};
}

// Scene, camera, frame, partition and sample range of the launch; what depends on the launch state comes later.
static int fill_kparams(Device &D, RT_KParams *K, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p,
                        void *d_accum, ViewBatch const *batch, ChunkList const *list) {
  const int nv = batch ? batch->n : 1;
  if (batch) cam = &batch->views[0].camera;      // (the kernel reads every view's camera from the view table)
  scene_only_kparams(K, d);
  camera_frame_kparams(K, cam, p);
  K->seed = p->seed;
  K->chunks_x = (p->width + RT_CHUNK_SIZE - 1) / RT_CHUNK_SIZE;
  K->n_chunks = rt_chunk_count(p->width, p->height);
  K->rank = p->rank;
  K->world = p->world;
  if (list) {
    K->local_chunks = nullptr;       // (the caller's table: staged once the launch state is known)
    K->n_local_chunks = list->n;
  } else {
    int n_local = 0;
    if (device_chunk_list(D, p->width, p->height, p->rank, p->world, &K->local_chunks, &n_local) != 0) return -1;
    K->n_local_chunks = n_local;
  }
  K->n_tiles = K->n_local_chunks * 16 * nv;      // (a batch: the tiles of view v are [v * tiles_per_view, (v + 1) * tiles_per_view))
  if (check_launch_size(D, K->n_local_chunks * 16, nv, K->sample_end - K->sample_first, p->slab) != 0) return -1;
  K->accum = (unsigned long long *)d_accum;
  if (batch) {
    K->n_views = nv;
    K->tiles_per_view = K->n_local_chunks * 16;
    K->pixels_per_view = p->width * p->height;
  }
  return 0;
}

// ---- launch geometry: waves per workgroup, BVH nodes in LDS, dynamic LDS per workgroup ----
static void launch_geometry(const Device &D, const RT_Device_Scene *d, RT_KParams &K, int *wg_waves, int *smem) {
  // Workgroup size by the size of the launch (round 5, profiles/r05_small_launch.md section 3).  A launch ends with every wave
  // running the bounce chains of its last paths on thinning lanes, and at four waves per SIMD those thin waves are ISSUE-bound:
  // with two waves per SIMD a bounce of such a chain takes half the time.  A launch with little work per wave slot is mostly
  // that tail -- config #1: 0.58 ms with 16-wave workgroups, 0.41 with 8 -- one with much work needs all four waves per SIMD
  // for its body (the driver's default frame: 2.60 / 2.89 / 3.48 ms with 16 / 12 / 8).  One workgroup per CU either way (the
  // tree fills the LDS).  Measured crossovers, in wave-fulls of paths per slot of the 16-wave grid: tower 640x360x16 (14) 0.91 /
  // 0.76 / 0.69 ms, spheres 512^2 x 16 (16) 0.83 / 0.74 / 0.75, helmet 512^2 x 16 (16) 1.23 / 1.17 / 1.41, 64 and more: 16 wins.
  const int64_t paths = (int64_t)K.n_tiles * 64 * (int64_t)(K.sample_end - K.sample_first);
  int64_t per_slot = paths / ((int64_t)D.num_cus * 16 * 64);
  // (a depth-0 scene -- one leaf group, no node blocks -- traces a ray in a quarter of the instructions: its launches are as
  //  short as launches a quarter their size; quad 256^2 / 512^2 / 768^2 / 1024^2 x 64 spp: best with 8 / 12 / 12 / 16 waves,
  //  0.43 / 0.90 / 1.62 / 2.43 ms against 0.59 / 0.99 / 1.67 / 2.43 with 16)
  if (K.depth == 0) per_slot /= 4;
  *wg_waves = per_slot < 12 ? 8 : (per_slot < 40 ? 12 : 16);
  int v = knob_int("RT_WG_WAVES", 0);
  if (v == 8 || v == 12 || v == 16) *wg_waves = v;
  // dynamic LDS: per wave the perm stack and the accumulator tile, the leading BVH nodes that fit beside them and the static sRGB table
  LdsSplit S = lds_split(d, K.depth, *wg_waves, RT_LDS_ACC_TILE_BYTES, 1, true);
  S.cap(knob_int("RT_LDS_NODES", -1));
  K.n_lds_nodes = S.n_lds_nodes;
  *smem = S.smem;
}

// ---- schedule feedback: visit expensive tiles first (costs = rays per tile of the previous launch of this view) ----
// Sets K.order / K.tile_cost; *cost_prev = the costs the preparation kernel sorts into L.order (NULL: none that fit this launch).
static int schedule_feedback(LaunchState &L, RT_KParams &K, const uint32_t **cost_prev) {
  K.order = nullptr;
  K.tile_cost = nullptr;
  *cost_prev = nullptr;
  if (knob_is("RT_ORDER", "identity") || K.n_tiles <= 0) return 0;
  const int n_tiles = K.n_tiles;
  // the costs of a launch are reusable by a launch of the same frame shape, partition and bounce limit -- NOT only of the same
  // view: for a camera that moves between frames the previous view's costs are still a better guide than none (helmet, a rotation
  // of 0.5 / 2 / 10 degrees per frame: -0.7 / -0.8 / -0.2 % kernel time at 256 spp, -2.3 % at 1024^2 x 64 spp against the identity
  // order, tools/exp_moving.py, profiles/r05_experiments.md section 4), and an order is only ever a schedule, never a pixel
  uint64_t key = 1469598103934665603ull;
  auto mix = [&key](const void *ptr, size_t n) {
    const unsigned char *b = (const unsigned char *)ptr;
    for (size_t i = 0; i < n; i++) { key ^= b[i]; key *= 1099511628211ull; }
  };
  int32_t ids[6] = {K.width, K.height, K.rank, K.world, K.max_bounces, n_tiles};
  mix(ids, sizeof ids);
  if (L.sched_tiles != n_tiles) {      // (another size, not only a larger one: the costs kept are those of n_tiles tiles)
    L.cost[0].reset(); L.cost[1].reset(); L.order.reset();
    L.sched_tiles = 0;
    L.sched_valid = false;
    HIP_TRY(L.cost[0].grow((size_t)n_tiles));
    HIP_TRY(L.cost[1].grow((size_t)n_tiles));
    HIP_TRY(L.order.grow((size_t)n_tiles));
    L.sched_tiles = n_tiles;
  }
  if (L.sched_valid && L.sched_key == key) {
    *cost_prev = L.cost[L.sched_cur ^ 1];
    K.order = L.order;
  }
  K.tile_cost = L.cost[L.sched_cur];
  L.sched_cur ^= 1;                // after this launch, cost[sched_cur ^ 1] is the buffer just written
  L.sched_key = key;
  L.sched_valid = true;
  return 0;
}

// ---- a batch: the view table, on the launch's stream.  The pinned copy is rewritten only once the previous table's copy is done
// (which waits for the launches queued before it on that stream, at most one launch ahead of this one) ----
static int upload_view_table(LaunchState &L, RT_KParams &K, ViewBatch const *batch, hipStream_t stream) {
  const int nv = batch->n;
  HIP_TRY(L.views.grow((size_t)nv));
  HIP_TRY(L.views_host.grow((size_t)nv));
  if (!L.views_copied) HIP_TRY(L.views_copied.ensure(hipEventDisableTiming));
  else HIP_TRY(hipEventSynchronize(L.views_copied));
  for (int v = 0; v < nv; v++) {
    RT_KView &r = L.views_host[v];
    memset(&r, 0, sizeof r);
    camera_rows(r.cam, &batch->views[v].camera);
    r.focal_length = batch->views[v].camera.focal_length;
    r.seed = batch->views[v].seed;
  }
  HIP_TRY(hipMemcpyAsync(L.views, L.views_host, (size_t)nv * sizeof(RT_KView), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(L.views_copied, stream));
  K.views = L.views;
  return 0;
}

// ---- a chunk list: like the view table, through a pinned copy that is rewritten only once the previous list's copy is done ----
int stage_chunk_list(ChunkListStage &S, ChunkList const &list, hipStream_t stream, const int32_t **d_list) {
  if (!S.copied) HIP_TRY(S.copied.ensure(hipEventDisableTiming));
  else HIP_TRY(hipEventSynchronize(S.copied));
  // (a list that outgrows the device copy frees it: what was queued from the old block must be done first)
  if (S.dev && S.dev.cap < (size_t)list.n) HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(S.dev.grow((size_t)list.n));
  HIP_TRY(S.host.grow((size_t)list.n));
  if (list.n > 0) {
    memcpy(S.host.get(), list.chunks, (size_t)list.n * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(S.dev, S.host, (size_t)list.n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(S.copied, stream));
  }
  *d_list = S.dev;
  return 0;
}

// Enqueues one launch of the path tracer for p's rank / sample range.  D.mutex held, D's GPU current.
// ev_prep (optional): recorded between the per-launch preparation and the path kernel.
int render_accumulate_locked(Device &D, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p, void *d_accum,
                             hipStream_t stream, hipEvent_t ev_prep, int launch_state, ViewBatch const *batch, ChunkList const *list) {
  if (ensure_device(D) != 0) return -1;
  if (check_params(p) != 0) return -1;
  if (!d || !d_accum) return rt_fail("rt_render_accumulate: NULL scene or accumulation buffer");
  if (d->dev != &D) return rt_fail("rt_render_accumulate: the scene was uploaded to another device");
  if (batch && check_views(batch->n, batch->views, p->width, p->height, "view batch") != 0) return -1;
  if (list && (batch || launch_state != RT_ADAPTIVE_STATE || p->rank != 0 || p->world != 1 ||
               check_chunk_list("chunk list", p->width, p->height, list->n, list->chunks) != 0))
    return rt_fail("rt_render_accumulate: a chunk list needs rank 0 of 1, no view batch, its own launch state and a valid list");
  const int nv = batch ? batch->n : 1;
  RT_KParams K;
  if (fill_kparams(D, &K, d, cam, p, d_accum, batch, list) != 0) return -1;
  if (launch_state < 0 || launch_state > RT_ADAPTIVE_STATE) return rt_fail("rt_render_accumulate: launch state %d out of range", launch_state);
  if (!list && launch_state == RT_ADAPTIVE_STATE) return rt_fail("rt_render_accumulate: launch state %d serves chunk lists only", launch_state);
  LaunchState &L = d->ls[launch_state];
  HIP_TRY(L.counters.grow(RT_N_COUNTERS));
  HIP_TRY(L.work_head.grow(16));
  K.counters = L.counters;
  K.work_head = L.work_head;
  D.last_counters = L.counters;
  bool wavefront = false;
#ifdef RT_DIAG_VARIANTS
  wavefront = g_pipeline.load() == 1 || knob_is("RT_PIPELINE", "wf");
#endif
  if (batch && wavefront) return rt_fail("view batch: a batch of views needs the tile-stream path kernel (the wavefront pipeline is set)");

  // persistent grid, one workgroup of wg_waves waves per CU (RT_WAVES_PER_CU: another number of waves per CU)
  int wg_waves, smem;
  launch_geometry(D, d, K, &wg_waves, &smem);
  int waves_per_cu = knob_int("RT_WAVES_PER_CU", 0);
  if (waves_per_cu <= 0) waves_per_cu = wg_waves;
  K.sched_thresh = knob_int("RT_SCHED_THRESH", 48);
  if (K.sched_thresh < 1 || K.sched_thresh > 64) K.sched_thresh = 48;
  K.drain_thresh = knob_int("RT_DRAIN_THRESH", K.sched_thresh);
  if (K.drain_thresh < 1 || K.drain_thresh > 64) K.drain_thresh = K.sched_thresh;

  // (a chunk list: identity order and no costs -- the list has another length every time, and schedule_feedback gives its buffers
  //  back whenever the number of tiles changes)
  const uint32_t *cost_prev = nullptr;
  K.order = nullptr;
  K.tile_cost = nullptr;
  if (!list && schedule_feedback(L, K, &cost_prev) != 0) return -1;

  // unit = 2 neighbouring pixels x `slab` samples, default 64 (128 paths, pixel-major: the 64 lanes of a wave sit on one
  // pixel, then on its neighbour); it is also the granularity at which waves share a tile at the end of a launch.
  // Measured, helmet frame / rank 0 of 8: 32 samples 36.9 / 5.39 ms, 64 36.15 / 5.31, 128 36.6.
  const int n_samples = K.sample_end - K.sample_first;
  const int cs = p->slab > 0 ? p->slab : 64;
  int cshift = 0;
  while ((1 << cshift) < cs && (1 << cshift) < n_samples) cshift++;
  K.chunk_shift = cshift;
  K.n_sample_blocks = (n_samples + (1 << cshift) - 1) >> cshift;
  K.n_chunks_tile = 32 * K.n_sample_blocks;          // units: 8 rows x sample blocks x 4 pixel pairs
  // (a chunk list: sized once for every chunk of the image, whatever the list's length)
  const int tiles_room = list ? K.n_chunks * 16 : K.n_tiles;
  if (L.tile_next_n < tiles_room) {
    L.tile_next_n = 0;
    // [n_tiles] chunk counters, then [ceil(n_tiles / 64)] open-tile counts of the groups
    HIP_TRY(L.tile_next.grow((size_t)tiles_room + (size_t)((tiles_room + 63) / 64)));
    L.tile_next_n = tiles_room;
  }
  K.tile_next = L.tile_next;
  K.open_groups = L.tile_next + L.tile_next_n;
  // never more waves than units
  const int64_t n_units = (int64_t)K.n_tiles * K.n_chunks_tile;
  int n_waves = D.num_cus * waves_per_cu;
  if ((int64_t)n_waves > n_units) n_waves = (int)n_units;
  // units per atomic: 1 unit of 128 paths (what a wave still holds when the launch runs dry is its tail); smaller
  // units (few samples) are taken in pairs.  Measured with units of 128 paths: frame 1 -> 36.25 ms, 2 -> 36.4, 4 -> 37.2.
  K.grab_max = (cshift >= 6 || (int64_t)K.n_tiles < (int64_t)2 * n_waves) ? 1 : 2;
  {
    int v = knob_int("RT_GRAB", 0);
    if (v == 1 || v == 2 || v == 4) K.grab_max = v;
  }
  // ... of the tiles that take the batch loop (sky, leafless and triangle-less tiles): they hold no bounce chains, so what a wave
  // still holds at the end of the launch is batches of 64 paths; the taper towards the tile's end is the same.  Every grab is a
  // returning atomic the wave waits for, once per two batches at 1.  Measured, one process, arms interleaved, 1 / 2 / 4 / 8 / 16:
  // config #3 25.80 / 25.66 / 25.58 / 25.58 / 25.62 ms, tower 23.42 / 23.03 / 22.85 / 22.81 / 22.85 (profiles/r17_batch_lanes.md).
  K.grab_batch = 8;
  {
    int v = knob_int("RT_GRAB_BATCH", 0);
    if (v >= 1 && v <= 16) K.grab_batch = v;
  }
  // The owner's FIRST grab is grab_batch as it stands, so the taper is applied to the whole tile here: a tile of fewer than
  // 8 * grab_batch units -- the 32 units of a 16-spp frame -- never reaches grab_batch under the kernel's rule (it grabs 2 while 8
  // units are left, then 1), and with the constant set to that value its first grab follows the rule as well.  Same grabs otherwise.
  if (K.n_chunks_tile < 8 * K.grab_batch) K.grab_batch = (K.n_chunks_tile >= 8 && K.grab_batch >= 2) ? 2 : 1;
  K.pyr_nodes = knob_int("RT_PYRAMID", 1) ? K.n_lds_nodes : 0;
  // Leaf blocks with the short reciprocal (rcp_exact, rt_dev.hip.h): equal to the IEEE division while every triangle
  // determinant |e1 . (d x e2)| <= 6 D E^2 stays below 2^102.  E = largest edge component of the scene; D = largest
  // component of a ray direction: <= 3 max|view matrix entry| for camera rays (the direction is normalised before the
  // matrix is applied), < 2 for the normalised directions that shading emits.  E <= 2^38 and matrix entries <= 2^16
  // give 6 D E^2 < 2^97.  Anything else -- or a NaN -- renders with the kernel that divides.
  float cam_max = 0.0f;
  for (int v = 0; v < nv; v++)                 // (a batch: over the cameras of all views)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        float m = fabsf(batch ? batch->views[v].camera.view_matrix.rows[i][j] : K.cam[i][j]);
        if (!(m <= cam_max)) cam_max = m;
      }
  K.short_div = (d->max_edge <= 0x1p38f && cam_max <= 0x1p16f) ? 1 : 0;
  if (knob_int("RT_SHORT_DIV", 1) == 0) K.short_div = 0;
  // The shade block with one set of bilinear taps per hit (SharedTaps, rt_dev.hip.h): where every material's textures agree in
  // width, height and stride -- a property of the resident copy, kept current by rt_residency.cpp.  Same frames.
  K.shared_taps = (d->shared_taps && knob_int("RT_SHARED_TAPS", 1) != 0) ? 1 : 0;
  // hits parked until a dense shade block can be made of them: RT_PARK_RECORD_DWORDS = 18 fields x 128 records per wave
  K.park = nullptr;
  if (!wavefront && knob_int("RT_PARK", 1) != 0 && K.max_bounces < (1 << 26)) {      // (a parked record keeps the bounce count in 26 bits)
    const int grid_waves = (n_waves + wg_waves - 1) / wg_waves * wg_waves;         // whole workgroups are launched
    const size_t slice_dwords = RT_PARK_RECORD_DWORDS;                            // a wave's slice: 18 fields x 128 records (rt_device.h)
    HIP_TRY(L.park.grow((size_t)grid_waves * slice_dwords));
    K.park = L.park;
  }

  K.views = nullptr;
  if (batch && upload_view_table(L, K, batch, stream) != 0) return -1;
  if (list && stage_chunk_list(L.list, *list, stream, &K.local_chunks) != 0) return -1;

  // ---- ONE preparation launch: counters, work head, tile / unit counters, this launch's cost buffer, tile order ----
  {
    int rc2 = rt_launch_prepare(K.n_tiles, K.tile_next, K.open_groups, L.counters, L.work_head, K.tile_cost, cost_prev,
                                cost_prev ? L.order : nullptr, stream);
    if (rc2 != 0) return rt_fail("prepare kernel launch failed: %s", hipGetErrorString((hipError_t)rc2));
  }
  if (ev_prep) HIP_TRY(hipEventRecord(ev_prep, stream));
  if (n_units == 0) return 0;      // nothing to render: this rank owns no chunk, or the sample range is empty

  K.wave_times = nullptr;
  if (knob_set("RT_WAVE_TIMES")) {      // wave timeline (tools/exp_waves.py)
    HIP_TRY(D.ws.wave_times.grow((size_t)65536 * 3));
    HIP_TRY(hipMemsetAsync(D.ws.wave_times, 0, (size_t)65536 * 3 * 8, stream));
    K.wave_times = D.ws.wave_times;
    if (n_waves > 65536) n_waves = 65536;          // the diagnostic buffer holds that many waves
    D.ws.wave_times_n = n_waves;
  }

  size_t slot = D.ws.n_timed % RT_MAX_TIMED;
  if (slot >= D.ws.ev0.size()) {
    D.ws.ev0.emplace_back();
    D.ws.ev1.emplace_back();
  }
  HIP_TRY(D.ws.ev0[slot].ensure());
  HIP_TRY(D.ws.ev1[slot].ensure());
  HIP_TRY(hipEventRecord(D.ws.ev0[slot], stream));
#ifdef RT_DIAG_VARIANTS
  if (wavefront) {
    if (launch_wavefront(D, d, K, stream) != 0) return -1;
  } else
#endif
  {
    int rc = rt_launch_path_kernel(&K, n_waves, smem, wg_waves, stream);
    if (rc != 0) return rt_fail("path kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    g_taps_form.store(K.shared_taps);
  }
  HIP_TRY(hipEventRecord(D.ws.ev1[slot], stream));
  D.ws.n_timed += 1;
  return 0;
}

extern "C" int rt_set_camera(RT_Device_Scene *dscene, Camera const *camera) {
  if (!dscene || !camera) return rt_fail("rt_set_camera: NULL argument");
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  D.cameras[dscene] = *camera;
  return 0;
}

extern "C" int rt_render_accumulate(RT_Device_Scene *dscene, RT_Render_Params const *params, void *d_accum,
                                    void *stream) {
  if (!dscene) return rt_fail("rt_render_accumulate: NULL scene or accumulation buffer");
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  auto it = D.cameras.find(dscene);
  if (it == D.cameras.end()) return rt_fail("rt_render_accumulate: no camera set for this scene (rt_set_camera)");
  forget_multi_counters();             // rt_get_counters() now means THIS launch, not an older multi-device frame
  return render_accumulate_locked(D, dscene, &it->second, params, d_accum, (hipStream_t)stream);
}

// rt_render_accumulate with the caller's chunk table (rt_hip.h).  Everything that can be checked without the device is checked
// before dscene is read: a wrong index would be a write outside the accumulation buffer.
extern "C" int rt_render_accumulate_chunks(RT_Device_Scene *dscene, RT_Render_Params const *params, i32 n_list, i32 const *chunks,
                                           void *d_accum, void *stream) {
  const char *who = "rt_render_accumulate_chunks";
  if (!dscene || !d_accum) return rt_fail("%s: NULL scene or accumulation buffer", who);
  if (check_params(params) != 0) return -1;
  if (params->world != 1 || params->rank != 0)
    return rt_fail("%s: a chunk list replaces the partition: rank 0 of world 1 only (got %d of %d)", who, params->rank, params->world);
  if (check_chunk_list(who, params->width, params->height, n_list, chunks) != 0) return -1;
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  auto it = D.cameras.find(dscene);
  if (it == D.cameras.end()) return rt_fail("%s: no camera set for this scene (rt_set_camera)", who);
  forget_multi_counters();
  ChunkList list;
  list.n = n_list;
  list.chunks = chunks;
  return render_accumulate_locked(D, dscene, &it->second, params, d_accum, (hipStream_t)stream, nullptr, RT_ADAPTIVE_STATE, nullptr, &list);
}

extern "C" int rt_render_accumulate_views(RT_Device_Scene *dscene, RT_Render_Params const *params, i32 n_views,
                                          RT_View const *views, void *d_accum, void *stream) {
  // (everything that can be checked without the device is checked before it is touched)
  if (!dscene || !d_accum) return rt_fail("rt_render_accumulate_views: NULL scene or accumulation buffer");
  if (check_params(params) != 0) return -1;
  if (check_views(n_views, views, params->width, params->height, "rt_render_accumulate_views") != 0) return -1;
  Device &D = *dscene->dev;
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  forget_multi_counters();
  ViewBatch batch;
  batch.n = n_views;
  batch.views = views;
  return render_accumulate_locked(D, dscene, &views[0].camera, params, d_accum, (hipStream_t)stream, nullptr, RT_VIEWS_STATE, &batch);
}

int resolve_on(Device &D, RT_Render_Params const *p, void const *d_accum, void *d_tiles, void *d_image, void *d_linear,
               hipStream_t stream) {
  if (check_params(p) != 0) return -1;
  if (!d_accum) return rt_fail("rt_resolve: NULL accumulation buffer");
  int chunks_x = (p->width + RT_CHUNK_SIZE - 1) / RT_CHUNK_SIZE;
  const int32_t *d_list = nullptr;
  int n_local = 0;
  if (device_chunk_list(D, p->width, p->height, p->rank, p->world, &d_list, &n_local) != 0) return -1;
  int rc = rt_launch_resolve(p->width, p->height, p->samples, chunks_x, d_list, n_local,
                             (const unsigned long long *)d_accum, (uint8_t *)d_tiles, (uint8_t *)d_image,
                             (float *)d_linear, stream);
  if (rc != 0) return rt_fail("resolve kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_resolve(RT_Render_Params const *p, void const *d_accum, void *d_tiles, void *d_image,
                          void *d_linear, void *stream) {
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return resolve_on(D, p, d_accum, d_tiles, d_image, d_linear, (hipStream_t)stream);
}

int untile_on(Device &D, i32 width, i32 height, i32 world, void const *d_all_tiles, void *d_image, hipStream_t stream) {
  if (width <= 0 || height <= 0 || world <= 0 || !d_all_tiles || !d_image) return rt_fail("rt_untile: bad arguments");
  int chunks_x = (width + RT_CHUNK_SIZE - 1) / RT_CHUNK_SIZE;
  const int32_t *d_table = nullptr;
  int n_chunks = 0;
  if (!partition_args_ok(width, height, world)) return rt_fail("rt_untile: bad arguments");
  if (device_owner_table(D, width, height, world, &d_table, &n_chunks) != 0) return -1;
  int rc = rt_launch_untile(width, height, chunks_x, n_chunks, d_table, (const uint8_t *)d_all_tiles,
                            (uint8_t *)d_image, stream);
  if (rc != 0) return rt_fail("untile kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_untile(i32 width, i32 height, i32 world, void const *d_all_tiles, void *d_image, void *stream) {
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return untile_on(D, width, height, world, d_all_tiles, d_image, (hipStream_t)stream);
}

int ensure_ws_buffers(Workspace &W, int width, int height, size_t tiles_bytes, size_t all_tiles_bytes, bool want_linear) {
  const size_t pixels = (size_t)width * height;
  HIP_TRY(W.accum.grow(pixels * 3));
  HIP_TRY(W.image.grow(pixels * 3));
  if (want_linear) HIP_TRY(W.linear.grow(pixels * 3));                  // (a frame lane has no fp32 output)
  if (tiles_bytes) HIP_TRY(W.tiles.grow(tiles_bytes));                  // (multi-device frames only: a request for none would yield a pointer)
  if (all_tiles_bytes) HIP_TRY(W.all_tiles.grow(all_tiles_bytes));
  for (DevEvent &e : W.ev_frame) HIP_TRY(e.ensure());
  return 0;
}

int copy_image_out(Image const *image, const uint8_t *d_image, int width, int height, hipStream_t stream) {
  size_t pixels = (size_t)width * height;
  if (!image->pixels.data) return 0;
  if (image->components == 3 && image->stride == image->width) {
    HIP_TRY(hipMemcpyAsync(image->pixels.data, d_image, pixels * 3, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  } else {
    std::vector<uint8_t> tmp(pixels * 3);
    HIP_TRY(hipMemcpy(tmp.data(), d_image, pixels * 3, hipMemcpyDeviceToHost));
    for (isize y = 0; y < image->height; y++)
      for (isize x = 0; x < image->width; x++)
        for (int c = 0; c < 3; c++)
          image->pixels.data[image->components * (x + y * image->stride) + c] = tmp[((size_t)y * width + x) * 3 + c];
  }
  return 0;
}

// One counter of the last rt_render_accumulate launch.
static int get_counter(const char *who, int index, u64 *out) {
  if (!out) return rt_fail("%s: NULL", who);
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  unsigned long long c[RT_N_COUNTERS];
  if (read_counters(D, c) != 0) return -1;
  *out = c[index];
  return 0;
}

// Of the node visits of the last rt_render_accumulate launch: how many were COUNTED but not executed -- the one root visit of
// every camera path whose tile's pixel pyramid misses every child of the root (the reference, and the oracle, spend and count
// it; the kernel proves its outcome per tile and skips it).  bench.py's roofline carries it as a footnote.
extern "C" int rt_get_skipped_root_visits(u64 *out) { return get_counter("rt_get_skipped_root_visits", RT_CNT_SKIPPED_ROOT, out); }

// Camera paths of the last rt_render_accumulate launch that the leafless loop of the path kernel served (rt_kernels.hip).
extern "C" int rt_get_leafless_paths(u64 *out) { return get_counter("rt_get_leafless_paths", RT_CNT_LEAFLESS, out); }

// Of those: the paths of triangle-less tiles, whose pyramid reaches leaf groups but no triangle of them.
extern "C" int rt_get_triangleless_paths(u64 *out) { return get_counter("rt_get_triangleless_paths", RT_CNT_TRIANGLELESS, out); }

// Rays of the last rt_render_accumulate launch whose root visit ran at the top of a traversal call, in front of the traversal
// rounds (rt_kernels.hip): every NaN-free ray that the sky / leafless loop does not serve, when the root has at most four populated
// children.
extern "C" int rt_get_fused_root_visits(u64 *out) { return get_counter("rt_get_fused_root_visits", RT_CNT_FUSED_ROOT, out); }

// The texture stage of the last path-kernel launch: 1 = shared taps, 0 = general, -1 = none yet (include/rt_hip.h).
extern "C" int rt_get_shade_taps_form(void) { return g_taps_form.load(); }

int read_counters(Device &D, unsigned long long c[RT_N_COUNTERS]) {
  HIP_TRY(hipDeviceSynchronize());
  if (!D.last_counters) { memset(c, 0, RT_N_COUNTERS * sizeof(unsigned long long)); return 0; }
  HIP_TRY(hipMemcpy(c, D.last_counters, RT_N_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rt_get_counters(RT_Counters *out) {
  if (!out) return rt_fail("rt_get_counters: NULL");
  {
    std::lock_guard<std::mutex> lk(g_multi_mutex);
    if (g_multi_counters_valid) { *out = g_multi_counters; return 0; }
  }
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  unsigned long long c[RT_N_COUNTERS];
  if (read_counters(D, c) != 0) return -1;
  out->paths = c[RT_CNT_PATHS];
  out->rays = c[RT_CNT_RAYS];
  out->node_visits = c[RT_CNT_NODES];
  out->leaf_visits = c[RT_CNT_LEAVES];
  out->shades = c[RT_CNT_SHADES];
  out->backgrounds = c[RT_CNT_BG];
  out->textured = c[RT_CNT_TEXTURED];
  return 0;
}

static float timed_slot_ms(Workspace &W, size_t slot) {
  if (hipEventSynchronize(W.ev1[slot]) != hipSuccess) return -1.0f;
  return event_ms(W.ev0[slot], W.ev1[slot]);
}

extern "C" f32 rt_last_kernel_ms(void) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (!D.ready || D.ws.n_timed == 0) return -1.0f;
  DeviceGuard guard(D);
  return timed_slot_ms(D.ws, (D.ws.n_timed - 1) % RT_MAX_TIMED);
}

extern "C" void rt_kernel_timing_reset(void) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  D.ws.n_timed = 0;
}

extern "C" f32 rt_kernel_timing_mean_ms(i32 *n_launches) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  size_t n = D.ws.n_timed < RT_MAX_TIMED ? D.ws.n_timed : RT_MAX_TIMED;
  if (n_launches) *n_launches = (i32)n;
  if (!D.ready || n == 0) return -1.0f;
  DeviceGuard guard(D);
  double sum = 0.0;
  for (size_t i = 0; i < n; i++) {
    float ms = timed_slot_ms(D.ws, i);
    if (ms < 0.0f) return -1.0f;
    sum += ms;
  }
  return (float)(sum / (double)n);
}
