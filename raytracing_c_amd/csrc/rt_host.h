// rt_host.h -- internal header of the host side of librt_hip.so: the reference's render entry points
// (raytracer.h:51-56) and the device-control calls of include/rt_hip.h, in one unit per concern:
//   rt_host.cpp       errors, configuration, device slots, seed, material / background tokens
//   rt_residency.cpp  scene upload, fingerprints and stamps, rt_scene_touch / verify / invalidate / set_static, the per-device cache,
//                     the scene-checked call every host-level entry point runs its work through (scene_checked)
//   rt_partition.cpp  chunk counts and owners, partition tables, device chunk lists
//   rt_launch.cpp     launch set-up (fill_kparams, render_accumulate_locked), the LDS split and the camera / frame fields every
//                     kernel on traversal_blocks() is launched with (lds_split, camera_frame_kparams), resolve / untile, workspace
//                     buffers, counters, kernel timing
//   rt_frames.cpp     the one-device frame sequence, blocking frames, frame lanes (rt_frame_begin / rt_frame_end), completion helpers;
//                     adaptive sampling: the merge and the per-chunk resolve on the device level, the frame whose chunks double their
//                     samples until their error settles (rt_render_adaptive)
//   rt_multi.cpp      a frame spread over N devices, with one persistent host thread per device slot
//   rt_extras.cpp     lightmap bake, HDR lightmaps (texel list, trace, resolve, dilation: device level and host level), GPU BVH build and
//                     refit, the u8 denoiser
//   rt_post.cpp       what runs on a frame and its feature planes: guided denoiser (the a-trous filter), temporal accumulation (the
//                     reprojected history) and the moments, variance and variance-guided filter on top of them, each on the device level, on the host level and behind a frame (one pipeline);
//                     a stage reads one RT_Frame (rt_device.h) and is launched in one place, which chooses its plain or variance / moments kernel;
//                     and feature-guided upsampling of a half-resolution frame, on the same three levels (rt_render_upsampled)
//   rt_query.cpp      batch ray queries: closest hit, occlusion, full hit records (device level and host level); light probes: path-traced
//                     samples at points a host supplies and their SH projection, on the queries' ring and slicing (device level and host level)
//   rt_features.cpp   first-hit feature buffers: coverage, albedo, normal, position (device level and host level)
//   rt_diag.cpp       the diagnostic library only (-DRT_DIAG_VARIANTS): wavefront pipeline, unit-test entry points, fault hooks
//   rt_mem.h          the owners of device memory, pinned memory and events (DevMem, PinnedMem, DevEvent): what a struct below
//                     holds is given back when the struct is destroyed or assigned over, never by a hand-kept list
//
// Nothing on the host side computes a pixel on the CPU: every entry point either
// drives the gfx950 kernels of rt_kernels.hip (one object, shared by both libraries) / rt_wavefront.hip and rt_kernels_test.hip
// (diagnostic library only) or fails with rt_last_error().
//
// State is kept PER DEVICE (struct Device): HIP context, workspace, scene cache, launch timing.  Slot 0 is the
// process's primary device (rt_init); slots 1 .. N-1 exist when a frame behind render_thread_proc / render() is spread
// over N GPUs (RT_DEVICES, rt_set_devices).  The product library reads its configuration ONCE (config()); the RT_*
// experiment knobs exist only in the host units of the diagnostic build (-DRT_DIAG_VARIANTS, librt_hip_diag.so).
//
// Lock order everywhere: slot 0's Device::mutex -> slot r's -> g_partition_mutex (rt_partition.cpp).
//
// No HIP call from static destruction: at process exit the HIP runtime may be gone already and the device threads of rt_multi.cpp
// are still parked.  So NO object of static storage duration has an owner of rt_mem.h as a member, at any depth: the device slots
// (g_devs), the retired partition tables (rt_partition.cpp) and the workers (rt_multi.cpp) are allocated once with `new` and never
// destroyed.  Nothing is freed at exit.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_device.h"
#include "rt_mem.h"

// launchers in rt_kernels.hip, rt_denoise.hip
extern "C" {
int rt_launch_path_kernel(const RT_KParams *P, int n_waves, int smem_bytes, int wg_waves, hipStream_t stream);
int rt_launch_prepare(int n_tiles, uint32_t *tile_next, uint32_t *open_groups, unsigned long long *counters, uint32_t *work_head,
                      uint32_t *cost_cur, const uint32_t *cost_prev, uint32_t *order, hipStream_t stream);
int rt_launch_resolve(int width, int height, int samples, int chunks_x, const int32_t *local_chunks, int n_local_chunks,
                      const unsigned long long *accum, uint8_t *tiles, uint8_t *image, float *linear,
                      hipStream_t stream);
int rt_launch_untile(int width, int height, int chunks_x, int n_chunks, const int32_t *owner_slot,
                     const uint8_t *all_tiles, uint8_t *image, hipStream_t stream);
int rt_launch_lightmap(const RT_KParams *P, const float *verts, int n_tris, int lw, int lh, int stride, int comp,
                       int samples, int *owner, uint8_t *pixels, hipStream_t stream);
int rt_launch_denoise(int width, int height, int src_stride, int src_comp, int dst_stride, int dst_comp,
                      const uint8_t *src, uint8_t *dst, hipStream_t stream);
int rt_launch_pack_texture(const uint8_t *raw, int width, int rows, int y0, int stride, int comp, uint32_t *out,
                           hipStream_t stream);
int rt_launch_pack_bg_image(const uint8_t *raw, int width, int height, int rows, int y0, int stride, int comp, float *out,
                            hipStream_t stream);
int rt_launch_query(const RT_KParams *P, const RT_QParams *Q, int any, int wg_waves, int n_blocks, int smem_bytes, hipStream_t stream);
int rt_launch_hit_attributes(const RT_KParams *P, int n, const float *rays, const float *hits, float *out, hipStream_t stream);
// ... in rt_features.hip
int rt_launch_features(const RT_KParams *P, const RT_FParams *F, int n_blocks, int smem_bytes, hipStream_t stream);
int rt_launch_features_resolve(int n_pixels, int samples, const unsigned long long *sums, float *coverage, float *albedo, float *normal,
                               float *position, hipStream_t stream);
int rt_launch_features_motion(const RT_KParams *P, const RT_FParams *F, const float *kept, unsigned long long *motion_sums, int n_blocks,
                              int smem_bytes, hipStream_t stream);
int rt_launch_motion_resolve(int n_pixels, int samples, const unsigned long long *sums, float *motion, hipStream_t stream);
// ... in rt_probes.hip
int rt_launch_probes(const RT_KParams *P, const RT_PParams *R, int n_blocks, int smem_bytes, hipStream_t stream);
int rt_launch_probe_project(int n_probes, int sample_count, const float *records, unsigned long long *sums, hipStream_t stream);
int rt_launch_probe_resolve(long long n_coeffs, int samples, const unsigned long long *sums, float *coeffs, hipStream_t stream);
// ... in rt_lightmap.hip
int rt_launch_lightmap_texels(const float *tris, const float *verts, int n_tris, int lw, int lh, int *owner, int *rows, float *texels,
                              long long *count, hipStream_t stream);
int rt_launch_lightmap_trace(const RT_KParams *P, const RT_LParams *R, int n_blocks, int smem_bytes, hipStream_t stream);
int rt_launch_lightmap_resolve(long long n, long long n_pixels, int samples, float scale, const float *texels,
                               const unsigned long long *sums, float *image, hipStream_t stream);
int rt_launch_lightmap_dilate(int width, int height, int pass, const float *src, float *dst, hipStream_t stream);
// ... in rt_refit.hip
int rt_launch_refit(int len, int depth, int n_internal, const void *d_src, const int *d_source_of_slot, float *d_block, float *d_nodes,
                    float *d_leaves, float *d_tris, unsigned char *d_populated, unsigned int *d_max_edge_bits, hipStream_t stream);
// ... in rt_scene_refit.c: scene_refit's validation alone; source_of_slot (optional, triangles.len entries) receives the inverse map
int rt_refit_check(Scene const *scene, Triangle_Slice src, i32 const *slot_of_source, i32 *source_of_slot);
// ... in rt_guided.hip (RT_Frame, rt_device.h: the frame a post pass reads)
int rt_launch_guided_pack(int n_pixels, int demodulate, RT_Frame frame, void *c0, void *g0, void *g1, hipStream_t stream);
int rt_launch_guided_filter(int width, int height, int step, float k_n, float k_p, float k_c, int last, int demodulate, const void *src,
                            void *dst, const void *g0, const void *g1, RT_Frame frame, float *out, uint8_t *image, hipStream_t stream);
// ... in rt_temporal.hip
int rt_launch_temporal(const RT_TParams *P, RT_Frame frame, const void *hist_in, void *hist_out, float *out, float *length,
                       uint8_t *image, hipStream_t stream);
int rt_launch_temporal_motion(const RT_TParams *P, RT_Frame frame, const float *motion, const void *hist_in, void *hist_out, float *out,
                              float *length, uint8_t *image, hipStream_t stream);
int rt_launch_temporal_pack(int n_pixels, const float *c, const float *len, const float *cov, const float *n, const float *w, void *hist,
                            hipStream_t stream);
int rt_launch_temporal_unpack(int n_pixels, const void *hist, float *c, float *len, float *cov, float *n, float *w, hipStream_t stream);
// ... in rt_variance.hip
int rt_launch_temporal_moments(const RT_TParams *P, RT_Frame frame, const void *hist_in, void *hist_out, float *out, float *length,
                               uint8_t *image, const void *mom_in, void *mom_out, hipStream_t stream);
int rt_launch_temporal_moments_motion(const RT_TParams *P, RT_Frame frame, const float *motion, const void *hist_in, void *hist_out,
                                      float *out, float *length, uint8_t *image, const void *mom_in, void *mom_out, hipStream_t stream);
int rt_launch_variance(int width, int height, float k_n, float k_p, const void *hist, const void *mom, float *variance,
                       hipStream_t stream);
int rt_launch_variance_pack(int n_pixels, int demodulate, RT_Frame frame, const float *variance, void *c0, void *g0, void *g1,
                            hipStream_t stream);
int rt_launch_variance_filter(int width, int height, int step, float k_n, float k_p, float k_c, int last, int demodulate,
                              const void *src, void *dst, const void *g0, const void *g1, RT_Frame frame, float *out, uint8_t *image,
                              float *var_out, hipStream_t stream);
int rt_launch_moments_pack(int n_pixels, const float *planar, void *mom, hipStream_t stream);
int rt_launch_moments_unpack(int n_pixels, const void *mom, float *planar, hipStream_t stream);
// ... in rt_upsample.hip (c0, g0, g1: the low frame as rt_launch_guided_pack packs it; full: the full-resolution planes, no colour)
int rt_launch_upsample(int width, int height, float k_n, float k_p, int demodulate, const void *c0, const void *g0, const void *g1,
                       RT_Frame full, float *out, uint8_t *image, hipStream_t stream);
// ... in rt_adaptive.hip (chunks: n_list global chunk indices on the device, every one inside the image's chunk grid)
int rt_launch_adaptive_merge(int width, int height, int samples, int n_list, const int32_t *chunks, unsigned long long *accum,
                             unsigned long long *fresh, unsigned long long *err, hipStream_t stream);
int rt_launch_resolve_adaptive(int width, int height, const int32_t *chunk_samples, const unsigned long long *accum, uint8_t *image,
                               float *linear, int32_t *sample_map, hipStream_t stream);
}

// ---------------------------------------------------------------------------------
// errors

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return rt_fail("%s failed: %s", #expr, hipGetErrorString(e_));      \
  } while (0)

static inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static inline float event_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.0f;
  return ms;
}

// ---------------------------------------------------------------------------------
// configuration: read once, never per launch
//
// Product library: RT_DEVICES (GPUs a frame behind render_thread_proc / render() is spread over, default 1) and
// RT_DEVICES_REHEARSE (=1: the N logical devices all map onto the primary GPU -- what a one-GPU box can run of the
// N-GPU path), overridable by rt_set_devices().  Nothing else in the environment changes what the library does.
// Diagnostic library (-DRT_DIAG_VARIANTS): the experiment knobs (RT_SCHED_THRESH, RT_WG_WAVES, RT_PIPELINE, ...),
// read at every launch so that one process can A/B them (tools/exp_kernels.py, tests/test_gpu_diag.py).

#ifdef RT_DIAG_VARIANTS
static inline int knob_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
static inline bool knob_is(const char *name, const char *value) {
  const char *e = getenv(name);
  return e && strcmp(e, value) == 0;
}
static inline bool knob_set(const char *name) { return getenv(name) != nullptr; }
#else
static inline int knob_int(const char *, int dflt) { return dflt; }
static inline bool knob_is(const char *, const char *) { return false; }
static inline bool knob_set(const char *) { return false; }
#endif

#define RT_MAX_DEVICES 16

struct Config {
  int  devices = 1;
  bool rehearse = false;
};

// ---------------------------------------------------------------------------------
// per-device state

struct Partition;
struct RT_Device_Scene;

struct FrameTiming {          // the most recent frame through render_thread_proc / render / rt_render_frame
  float stamp_ms = 0, upload_ms = 0, enqueue_ms = 0, gpu_prep_ms = 0, gpu_path_ms = 0, gpu_resolve_ms = 0, gpu_copy_ms = 0,
        total_ms = 0, verify_ms = 0, gather_ms = 0;
  int   n_devices = 1, slowest_device = 0;
};

#ifndef RT_FRAME_LANES
#define RT_FRAME_LANES   2                       // frames in flight behind rt_frame_begin / rt_frame_end
#endif
#define RT_LAUNCH_STATES (1 + RT_FRAME_LANES)
#define RT_VIEWS_STATE   RT_LAUNCH_STATES        // the launch state of view batches (rt_render_views, rt_render_accumulate_views)
#define RT_ADAPTIVE_STATE (RT_VIEWS_STATE + 1)   // the launch state of chunk-list launches (rt_render_accumulate_chunks, rt_render_adaptive)

// K views of one frame (rt_render_views): one launch, the tiles of every view in one work queue.
struct ViewBatch {
  int            n = 0;
  RT_View const *views = nullptr;
};

// The chunks of one launch, chosen by the caller (rt_render_accumulate_chunks): a HOST array of global chunk indices that
// check_chunk_list() has passed.
struct ChunkList {
  int        n = 0;
  i32 const *chunks = nullptr;
};

// (hidden, here and at LaunchState: the structs made of owners have destructors and move assignments now, and none of them joins
//  the libraries' export lists)
#pragma GCC visibility push(hidden)
struct Workspace {
  DevMem<unsigned long long>    accum;        // [pixels][3]
  DevMem<uint8_t>               image;        // [pixels][3]
  DevMem<float>                 linear;       // [pixels][3] (a frame lane has none)
  DevMem<uint8_t>               tiles;        // multi-device frames: this device's compact tiles
  DevMem<uint8_t>               all_tiles;    // slot 0: the tiles of every device, rank-major
  PinnedMem<uint8_t>            tiles_host;   // a device without peer access to slot 0 stages its tiles here
  PinnedMem<unsigned long long> counters_host;   // ray counters of a multi-device frame, copied asynchronously
  // HIP event pairs around every path-kernel launch since the last timing reset
  std::vector<DevEvent>         ev0, ev1;
  size_t                        n_timed = 0;
  DevEvent                      ev_frame[5];  // frame start, prep done, path done, resolve done, copy done
  DevMem<unsigned long long>    wave_times;   // RT_WAVE_TIMES (diagnostic library): the wave timeline of the last launch
  int                           wave_times_n = 0;
};
#define RT_MAX_TIMED 256

struct DevPartition {
  const Partition        *host = nullptr;
  std::vector<DevMem<int32_t>> d_lists;       // device copies of the ranks' chunk lists, uploaded on first use
  DevMem<int32_t>         d_owner_slot;
};

// A frame in flight behind rt_frame_begin() / rt_frame_end() (slot 0): its own stream, accumulators and image buffer, and launch
// state 1 + lane of the device scene it renders from -- two frames overlap on the GPU, the second fills the CUs the first one's
// thinning bounce chains leave idle (profiles/r05_small_launch.md: a launch ends 0.6 - 1.0 ms after its last unit is handed out).
struct FrameLane {
  bool        busy = false;                   // begun, not yet ended
  bool        finished = false;               // rendered synchronously inside rt_frame_begin (a multi-device frame): nothing to wait for
  bool        ending = false;                 // a thread is inside rt_frame_end for this lane, waiting without the mutex
  int         rc = 0;
  hipStream_t stream = nullptr;
  Workspace   ws;
  Scene const *scene = nullptr;
  Image       image;                          // the caller's Image header (the pixels stay the caller's)
  RT_Render_Params p;
  Camera      camera;                         // scene->camera when the frame began
  RT_Device_Scene *d = nullptr;               // the copy the frame renders from; nullptr once that copy was dropped (free_device_scene waits first)
  uint64_t    fp = 0;                         // full fingerprint of that copy when the frame began
  bool        verify = false;
  FrameTiming timing;
  double      t_begin = 0.0;
};

// Batch ray queries (rt_query.cpp).  What a query launch writes besides its results -- the work counter and the four counters -- is
// one 64-byte slot of a ring, so that query calls on several streams can be in flight at once; a slot is taken again only after
// the event recorded behind its last launch has completed.  The staging buffers serve the host-level calls, one slice at a time;
// they are kept between calls (at most 133 B x RT_QUERY_SLICE) and given back with the rest when the slot is torn down
// (release_staging).  The staging buffers are counted in f32 (a ray is 6, a hit record 4, a full record RT_HIT_DWORDS).
#define RT_QUERY_SLOTS 64
struct QueryState {
  DevMem<uint8_t> slots;                      // [RT_QUERY_SLOTS][64]: counters u64[4] at +0, work counter u32 at +32
  DevEvent   done[RT_QUERY_SLOTS];
  bool       used[RT_QUERY_SLOTS] = {};
  unsigned   next = 0;
  int        last = -1;                       // slot of the most recent query call (rt_get_query_counters)
  DevMem<float>   rays, t_max, hits, full;
  DevMem<uint8_t> flags;
};

// First-hit feature buffers (rt_features.cpp): the device staging of the host-level call -- the sums and the ten f32 planes of one
// frame -- kept between calls, given back with the device slot (release_staging).  A launch's work counter is a slot of the
// query ring above.
struct FeatureState {
  DevMem<unsigned long long> sums;            // [pixels][RT_FEATURE_CHANNELS]
  DevMem<float>              planes;          // coverage [pixels], then albedo, normal, position [pixels][3] each
  // the motion feature pass alone (rt_render_features_motion, a history with motion on) grows these:
  DevMem<unsigned long long> motion_sums;     // [pixels][RT_MOTION_CHANNELS]
  DevMem<float>              motion;          // [pixels][RT_MOTION_CHANNELS]
};

// Light probes (rt_query.cpp).  What a probe launch writes besides its records -- the seven counters and the work counter -- is one
// 128-byte slot of a ring of its own, indexed like the query ring and taken with it (acquire_slot: the slot's event orders its
// reuse), so that rt_get_query_counters() and rt_get_probe_counters() never share a word.  The staging buffers serve the host-level
// call, one slice of at most RT_PROBE_SLICE paths at a time; they are kept between calls and given back with the device slot
// (release_staging).
#define RT_PROBE_SLOT_BYTES 128
struct ProbeState {
  DevMem<uint8_t>            slots;           // [RT_QUERY_SLOTS][128]: counters u64[8] at +0 (RT_CNT_PATHS .. RT_CNT_TEXTURED), work counter u32 at +64
  int                        last = -1;       // slot of the most recent probe call (rt_get_probe_counters)
  DevMem<float>              positions;       // [probes of a slice][3]
  DevMem<float>              records;         // [paths of a slice][8]
  DevMem<unsigned long long> sums;            // [probes of a slice][27]
  DevMem<float>              coeffs;          // [probes of a slice][27]
};

// HDR lightmaps (rt_extras.cpp).  Like ProbeState: a ring of 128-byte slots of its own for what a lightmap launch writes besides
// its sums, indexed like the query ring and taken with it, so that rt_get_lightmap_counters() shares no word with the queries' or
// the probes' counters.  The other buffers serve the host-level call; they are kept between calls and given back with the device
// slot (release_staging).
struct LightmapState {
  DevMem<uint8_t>            slots;           // [RT_QUERY_SLOTS][128]: counters u64[8] at +0 (RT_CNT_PATHS .. RT_CNT_TEXTURED), work counter u32 at +64
  int                        last = -1;       // slot of the most recent lightmap trace (rt_get_lightmap_counters)
  DevMem<float>              verts;           // [slots][9] original vertices
  DevMem<int>                owner;           // [width x height + height]: owners, then the rows' list offsets
  DevMem<float>              texels;          // [width x height][8]
  DevMem<long long>          count;           // the list's length
  DevMem<unsigned long long> sums;            // [list entries][3]
  DevMem<float>              image, work;     // [height][width][4] each
};

// The four planes of such a buffer, to write (the resolve) ...
static inline RT_Features split_feature_planes(float *planes, size_t pixels) {
  return {planes, planes + pixels, planes + pixels * 4, planes + pixels * 7};
}
// ... and, with a colour, as the frame the post passes read (RT_Frame, rt_device.h)
static inline RT_Frame device_frame(const float *color, RT_Features const &planes) {
  return {color, planes.coverage, planes.albedo, planes.normal, planes.position};
}

// Guided denoiser (rt_post.cpp): the device staging of the host-level calls, kept between calls, given back with the device slot
// (release_staging).  Behind a frame (rt_post.cpp's render_post) the filter is the optional last stage over FeatureState's planes
// -- of the workspace's linear frame (rt_render_denoised), of TemporalState's out or of UpsampleState's out (one RT_Frame each):
// it uses work and out.
struct GuidedState {
  DevMem<float>   in;                         // the host-level calls' RT_Frame: color [pixels][3], then planes as FeatureState's
  DevMem<float>   out;                        // [pixels][3]
  DevMem<uint8_t> image;                      // [pixels][3]
  DevMem<uint8_t> work;                       // rt_guided_work_bytes()
  DevMem<float>   variance;                   // rt_guided_denoise_variance_host: the variance plane [pixels] in ...
  DevMem<float>   variance_out;               // ... and out (grown by that call alone)
};

// Temporal accumulation (rt_post.cpp): the device staging of rt_temporal_accumulate_host -- the 13 planar f32 of the frame (one
// RT_Frame), a history as 11 planar f32 (staged in, later staged out: rt_post.cpp's HISTORY_PLANES is their one description), the
// two histories as records -- and the f32 output of rt_render_temporal, kept between calls; and the histories hosts keep
// (rt_history_create), whose device memory is part of this slot's staging: giving the staging back (release_temporal_state) empties
// every one of them (RT_History::release), so that none points at memory of a slot that was torn down.
struct TemporalState {
  DevMem<float>   in;                         // the host-level calls' RT_Frame: color [pixels][3], then planes as FeatureState's
  DevMem<float>   planar;                     // a history as planes, HISTORY_PLANES: colour [pixels][3], length, coverage [pixels], N, W [pixels][3]
  DevMem<uint8_t> hist[2];                    // rt_temporal_history_bytes() each: read, written
  DevMem<float>   out;                        // [pixels][3]
  DevMem<float>   length;                     // [pixels]
  DevMem<uint8_t> image;                      // [pixels][3]
  // rt_temporal_accumulate_moments_host and rt_render_svgf alone grow these:
  DevMem<uint8_t> mom[2];                     // rt_temporal_moments_bytes() each: read, written
  DevMem<float>   mom_planar;                 // moments as the host has them, [pixels][2]
  DevMem<float>   variance;                   // [pixels]: the variance launch's output, the variance-guided filter's input
  DevMem<float>   motion;                     // rt_temporal_accumulate_motion_host alone: the staged motion plane [pixels][3]
  std::vector<RT_History *> histories;        // every live RT_History (slot 0 only)
};

// Feature-guided upsampling (rt_post.cpp): the device staging of rt_guided_upsample_host -- the low frame and the full-resolution
// planes (two RT_Frames through the one upload, the second without a colour) -- kept between calls, given back with the device slot
// (release_staging).  Behind a frame the upsampling is a stage of render_post (rt_render_upsampled): the workspace's linear frame,
// rendered at the low size, and low_planes, the planes of its feature pass, are upsampled over FeatureState's planes at full size:
// it uses low_planes, work and out.
struct UpsampleState {
  DevMem<float>   in_low;                     // the host-level call's low RT_Frame: color [low pixels][3], then planes as FeatureState's
  DevMem<float>   in_full;                    // ... and its full-resolution planes, as FeatureState's
  DevMem<float>   low_planes;                 // render_post: the low frame's planes, as FeatureState's
  DevMem<uint8_t> work;                       // rt_guided_upsample_work_bytes()
  DevMem<float>   out;                        // [pixels][3]
  DevMem<uint8_t> image;                      // [pixels][3]
};

// scene_refit_gpu (rt_extras.cpp): the device staging of a refit, kept between calls -- a deforming mesh is refitted every frame --
// and given back with the device slot (release_staging).
struct RefitState {
  DevMem<uint8_t>  src;                       // the source triangles, 112 B each
  DevMem<int32_t>  source_of_slot;            // [slots]
  DevMem<float>    block;                     // the host-layout triangle block: nine f32 arrays, then the Triangle_AOS records
  DevMem<uint8_t>  populated;                 // [nodes + leaf groups], indexed like the implicit tree
  DevMem<uint32_t> max_edge_bits;             // one word
};

// A chunk list on its way to the device: the pinned copy is rewritten only once the copy queued from it is done (as the view table
// of a batch is, rt_launch.cpp).
struct ChunkListStage {
  DevMem<int32_t>    dev;
  PinnedMem<int32_t> host;
  DevEvent           copied;                  // recorded after the list's copy: `host` may be rewritten once it completed
};

// Adaptive sampling (rt_frames.cpp): the chunk list of rt_adaptive_merge, and what rt_render_adaptive keeps between calls -- the
// second sum buffer, the chunks' errors and sample counts, the sample map, the counters of the frame's launches -- given back with
// the device slot (release_staging).
struct AdaptiveState {
  ChunkListStage                merge_list;
  DevMem<unsigned long long>    fresh;        // [pixels][3]
  DevMem<unsigned long long>    err;          // [chunks]
  PinnedMem<unsigned long long> err_host;     // [chunks]
  DevMem<int32_t>               chunk_samples;   // [chunks]
  DevMem<int32_t>               sample_map;   // [pixels]
  PinnedMem<unsigned long long> counters_host;   // [RT_ADAPTIVE_MAX_LAUNCHES][RT_N_COUNTERS]
};
#define RT_ADAPTIVE_MAX_LAUNCHES 32           // the first launch and at most 30 doublings of min_samples >= 1 within 2^31

#pragma GCC visibility pop

struct Device {
  int        slot = 0, phys = 0;
  bool       ready = false;
  bool       peer_ok = true;                  // slots >= 1: direct copies into slot 0's memory are possible (xGMI peer access)
  hipStream_t mstream = nullptr;              // multi-device frames: this slot's own stream (slots rehearsed on ONE GPU overlap on it)
  int        num_cus = 0;
  std::mutex mutex;                           // serialises frames, the scene cache and the workspace of this device
  Workspace  ws;
  unsigned long long *last_counters = nullptr;   // counters of the most recent path-kernel launch
  std::unordered_map<const Scene *, RT_Device_Scene *> scene_cache;
  std::unordered_map<RT_Device_Scene *, Camera>        cameras;
  std::vector<DevPartition>                            parts;   // guarded by g_partition_mutex
  FrameTiming timing;
  FrameLane  lanes[RT_FRAME_LANES];           // slot 0 only
  QueryState query;
  FeatureState features;
  ProbeState probes;
  LightmapState lightmap;
  GuidedState guided;
  RefitState refit;
  TemporalState temporal;
  UpsampleState upsample;
  AdaptiveState adaptive;
};

// rt_history_create's object.  Guarded by slot 0's mutex like the staging it belongs to.
#pragma GCC visibility push(hidden)
struct RT_History {
  i32             width = 0, height = 0;
  DevMem<uint8_t> buf[2];                     // the two histories; [cur] is the one the last frame wrote
  int             cur = 0;
  bool            valid = false;              // buf[cur] holds a history and `camera` its camera
  DevMem<uint8_t> mom[2];                     // the moments of the two histories (rt_render_svgf allocates them), ping-ponged with buf
  bool            moments_valid = false;      // mom[cur] holds the moments of buf[cur]: the last frame was rt_render_svgf's
  bool            motion = false;             // rt_history_set_motion: the motion feature pass and THE ACCUMULATION WITH MOTION
  Camera          camera;
  // Gives the device memory back: the history is empty, as after rt_history_reset().  Slot 0's GPU current.
  void release() {
    buf[0].reset();
    buf[1].reset();
    mom[0].reset();
    mom[1].reset();
    valid = moments_valid = false;
  }
};
#pragma GCC visibility pop

// Makes `D`'s GPU the calling thread's current HIP device for the guard's lifetime.
struct DeviceGuard {
  int  prev = -1;
  bool switched = false;
  explicit DeviceGuard(const Device &D) {
    if (hipGetDevice(&prev) == hipSuccess && prev != D.phys) switched = hipSetDevice(D.phys) == hipSuccess;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// ---------------------------------------------------------------------------------
// scene residency

struct FpBlock {            // one block of a host scene's full fingerprint (scene_fingerprint_blocks)
  const void *begin;
  size_t      bytes;
  uint64_t    h;
};

#pragma GCC visibility push(hidden)
// What ONE launch of the path kernel writes besides the accumulators: counters, work head, the tiles' unit counters, parked hits,
// the schedule feedback.  A device scene owns several (RT_Device_Scene::ls), allocated on first use.
struct LaunchState {
  DevMem<unsigned long long> counters;         // RT_N_COUNTERS
  DevMem<uint32_t>    work_head;               // one 64-byte line
  DevMem<uint32_t>    tile_next;               // tile-stream kernel: chunks handed out per tile, then the groups' open-tile counts
  int32_t             tile_next_n = 0;         // tiles it was sized for: the groups' counts begin at tile_next + tile_next_n
  DevMem<uint32_t>    park;                    // tile-stream kernel: parked hits, [waves][18][128]
  // schedule feedback: rays per 8x8 tile of the previous launch of the same frame shape -> visiting order of the next
  DevMem<uint32_t>    cost[2];                 // [cur] is written by the running launch, [cur^1] is last launch's
  DevMem<uint32_t>    order;
  int32_t      sched_tiles = 0, sched_cur = 0;
  bool         sched_valid = false;            // cost[cur^1] holds the costs of a launch with sched_key
  uint64_t     sched_key = 0;
  // view batches: the device view table of the launch, filled from a pinned copy on the launch's stream
  DevMem<RT_KView>    views;
  PinnedMem<RT_KView> views_host;
  DevEvent            views_copied;            // recorded after the table's copy: views_host may be rewritten once it completed
  // chunk-list launches ([RT_ADAPTIVE_STATE] only): the device copy of the caller's list
  ChunkListStage      list;
};

#pragma GCC visibility pop

struct RT_Device_Scene {
  Device      *dev = nullptr;
  DevMem<float>       nodes, leaves, tris, mats;
  // the KEPT GEOMETRY (rt_device_scene_keep_geometry): `leaves` as one device-to-device copy left them, what THE MOTION of a later
  // feature pass is measured against; it goes with the copy
  DevMem<float>       kept_leaves;
  bool                has_kept = false;
  DevMem<RT_DTexture> textures;
  DevMem<uint32_t>    texels;
  DevMem<float>       bg_image;                // the background as padded floats (rt_device.h), made from the rows that fill `texels`
  int32_t      depth = 0, last_row_offset = 0, bg_texture = -1, n_nodes = 0;
  int32_t      n_triangles = 0, n_materials = 0, n_textures = 0;
  int64_t      bytes = 0;
  float        max_edge = 0.0f;   // largest |component| of an edge b - a, c - a in the leaf tiles (NaN if one is NaN)
  bool         boxes_ordered = true;      // every child box of every node has min <= max on every axis (no NaN either)
  // the material table as uploaded and patched since (rt_scene_touch), and what it says about the textures: every material's agree
  // in width, height and stride (rt_materials_share_taps) and one names a texture -> the path kernel's shared-taps instance
  std::vector<float> mats_host;
  bool         shared_taps = false;
  // what the host Scene looked like at upload: the per-frame stamp (scene_stamp) re-reads exactly this much of it
  uint64_t     stamp = 0;
  std::vector<const void *> mat_ptrs;     // distinct shader.data pointers, upload order
  std::vector<int32_t>      mat_first_tri;   // a triangle that uses mat_ptrs[k]
  // the FULL fingerprint of the host scene this copy was made from (scene_fingerprint_blocks), refreshed by rt_scene_touch:
  // every device slot checks a frame against ITS OWN copy's value
  std::vector<FpBlock>      fp_blocks;
  uint64_t                  full_fp = 0;
  // what rt_scene_touch() needs to patch the copy in place
  std::unordered_map<uint64_t, int> mat_map;            // (shader.data, kind) -> material id
  std::vector<const Image *>        tex_sources;        // Image of texture k (pool order; the background is one of them)
  std::vector<RT_DTexture>          tex_descs;          // its slot in the texel pool
  // launch state: RT_LAUNCH_STATES + 2 of them, so that launches of ONE device scene can be in flight on several streams at once
  // ([0]: the blocking entry points and rt_render_accumulate; [1 + k]: frame lane k of rt_frame_begin / rt_frame_end;
  // [RT_VIEWS_STATE]: view batches -- their tile list is K times as long, and a state of their own keeps the schedule feedback
  // of single frames and of batches from replacing each other; [RT_ADAPTIVE_STATE]: chunk-list launches -- their tile list has
  // another length every time, they run in identity order and keep no schedule feedback at all)
  LaunchState ls[RT_LAUNCH_STATES + 2];
  // wavefront pipeline (rt_wavefront.hip): record queues between the camera / shade / trace kernels
  DevMem<uint32_t>    wf_hit0, wf_hit, wf_ray[2];
  DevMem<uint32_t>    wf_cnt;                  // records per chunk: hit0 | hit | ray[0] | ray[1]
  DevMem<uint32_t>    wf_ctl;                  // WF_N_CTL control words, one per 64-byte line
  PinnedMem<uint32_t> wf_ctl_host;             // the copy the host reads after a pass
  int64_t             wf_soft0 = 0, wf_hard0 = 0, wf_ray_chunks = 0, wf_hit_chunks = 0;   // capacities in chunks
  int32_t             wf_waves = 0;            // waves the capacities were sized for
};

// ---------------------------------------------------------------------------------
// what one unit defines and another calls.  Hidden: none of it is exported from the library (the types above keep default
// visibility, the structs made of owners aside, so the library's export list is what it was).

#pragma GCC visibility push(hidden)

// rt_host.cpp
int    rt_fail(const char *fmt, ...);                   // sets rt_last_error(), returns -1
Config config();
int    ensure_device(Device &D);                        // D.mutex held (or single-threaded start-up); makes D's GPU current
extern Device *const    g_devs;                         // [RT_MAX_DEVICES], allocated once and never destroyed (see the top)
extern int              g_primary;                      // physical device of slot 0
extern std::atomic<u32> g_seed;
extern std::mutex       g_multi_mutex;                  // counters of the last multi-device frame
extern RT_Counters      g_multi_counters;
extern bool             g_multi_counters_valid;
extern Shader_Proc      g_tok_disney, g_tok_debug;      // what rt_scene_upload recognises as the device materials ...
extern Background_Proc  g_tok_background;               // ... and the device background (rt_diag_set_tokens may change them)
static inline Device &dev0() { return g_devs[0]; }

// rt_residency.cpp
void             free_device_scene(RT_Device_Scene *d);            // d->dev->mutex held, d's device current; waits for the lanes that render from d
uint64_t         scene_fingerprint(Scene const *scene);
bool             scene_is_static(Scene const *scene);               // takes g_static_mutex
int              drop_stale_copies(Scene const *scene, uint64_t now, int first_slot);   // takes each slot's mutex; returns copies dropped
void             scene_only_kparams(RT_KParams *K, RT_Device_Scene *d);
RT_Device_Scene *cached_scene_locked(Device &D, Scene const *scene, float *stamp_ms, float *upload_ms);   // D.mutex held
// After the host scene and the copy `d` were changed together (rt_scene_touch, scene_refit_gpu): d's stamp and full fingerprint
// become those of `now`, the host scene's blocks -- every one of which the caller knows the copy to match.
void             adopt_scene_stamps(RT_Device_Scene *d, Scene const *scene, const std::vector<FpBlock> &now);
// scene_refit_gpu's guard against an edit nobody reported: `now` = the host scene's blocks with the geometry (nodes, coordinates,
// AoS records: what the refit rewrites on both sides) unhashed; true when the list has the shape of d's and every other block has
// the hash d was made from.  rehash_geometry_blocks() completes `now` once the host Scene holds the refitted bytes.
bool             refit_may_keep_copy(const RT_Device_Scene *d, Scene const *scene, std::vector<FpBlock> &now);
void             rehash_geometry_blocks(Scene const *scene, std::vector<FpBlock> &now);
bool             node_boxes_ordered(const float *nodes, size_t n_nodes);      // every child box has min <= max on every axis
// What lets a host edit a Scene in place: take the cached copy (sampled stamp; uploads when it differs), run enqueue(ctx, copy) on
// `stream`, fingerprint the whole host scene on this thread while the GPU works; when it differs from the copy, wait for the stream,
// drop the copy and do it all once more.  Returns the copy the work finally ran from, nullptr after a failure.  T (optional):
// stamp_ms and upload_ms are added to, enqueue_ms (the last attempt) and verify_ms set.  D.mutex held, D's GPU current.
RT_Device_Scene *scene_checked_call(Device &D, Scene const *scene, hipStream_t stream, FrameTiming *T,
                                    int (*enqueue)(void *ctx, RT_Device_Scene *d), void *ctx);
// ... with any callable `int enqueue(RT_Device_Scene *)`, called in place: nothing is allocated per call
template <typename F>
static inline RT_Device_Scene *scene_checked(Device &D, Scene const *scene, hipStream_t stream, FrameTiming *T, F &enqueue) {
  return scene_checked_call(D, scene, stream, T, [](void *f, RT_Device_Scene *d) { return (*static_cast<F *>(f))(d); }, &enqueue);
}

// rt_partition.cpp
void remap_device_slots();                                                          // takes slot 0's mutex, then each slot's
void release_staging(Device &D);                                                    // D.mutex held, D's GPU current, device idle
bool partition_args_ok(i32 width, i32 height, i32 world);
int  device_chunk_list(Device &D, int width, int height, int rank, int world, const int32_t **d_list, int *n_local);   // D's GPU current; takes g_partition_mutex
int  device_owner_table(Device &D, int width, int height, int world, const int32_t **d_table, int *n_chunks);      // D's GPU current; takes g_partition_mutex

// rt_launch.cpp
#define RT_MAX_PIXELS ((int64_t)1 << 28)                                            // of one image: pixel and tile indices are 32-bit
int check_params(RT_Render_Params const *p);
int check_image_size(const char *who, i32 width, i32 height);                       // `who`: not positive / more than RT_MAX_PIXELS
int check_views(i32 n_views, RT_View const *views, i32 width, i32 height, const char *who);   // the batch's sizes; no device needed
// A caller's chunk list for a width x height image: n_list >= 0, a list when n_list > 0, every index in [0, rt_chunk_count), strictly
// ascending.  No device needed.
int check_chunk_list(const char *who, i32 width, i32 height, i32 n_list, i32 const *chunks);
// The list's device copy, enqueued on `stream` through S's pinned copy; *d_list stays valid for what is enqueued behind it on that
// stream.  The owning device's mutex held, its GPU current.
int stage_chunk_list(ChunkListStage &S, ChunkList const &list, hipStream_t stream, const int32_t **d_list);
// How a workgroup's LDS is split (rt_device.h): as many leading BVH nodes as fit beside `wg_waves` perm stacks of `depth` levels and
// `wave_extra_bytes` more per wave, when `wgs_per_cu` workgroups share a CU and -- `static_table` -- the kernel's sRGB table takes
// RT_LDS_TABLE_BYTES of it (launches that never counted the table say false).  No node when a child box has min > max (the LDS
// node blocks assume min <= max).  smem = the launch's dynamic LDS in bytes.  cap(n): at most n nodes (n < 0: as many as fit).
struct LdsSplit {
  int n_lds_nodes, smem;
  void cap(int n) { if (n >= 0 && n < n_lds_nodes) { smem -= (n_lds_nodes - n) * RT_LDS_NODE_BYTES; n_lds_nodes = n; } }
};
LdsSplit lds_split(const RT_Device_Scene *d, int depth, int wg_waves, int wave_extra_bytes, int wgs_per_cu, bool static_table);
void camera_rows(float dst[3][4], Camera const *cam);                                // rows 0..2 of the view matrix
void camera_frame_kparams(RT_KParams *K, Camera const *cam, RT_Render_Params const *p);   // the camera and frame fields of K
// Enqueues one launch of the path tracer for p's rank / sample range.  D.mutex held, D's GPU current.
// ev_prep (optional): recorded between the per-launch preparation and the path kernel.  batch (optional): K views in one launch
// (cam and p->seed are ignored; d_accum holds K images).  list (optional, launch state RT_ADAPTIVE_STATE, rank 0 of 1, no batch): the
// launch renders the list's chunks in place of the partition's, in identity order, and keeps no schedule feedback.
int render_accumulate_locked(Device &D, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p, void *d_accum,
                             hipStream_t stream, hipEvent_t ev_prep = nullptr, int launch_state = 0,
                             ViewBatch const *batch = nullptr, ChunkList const *list = nullptr);
int resolve_on(Device &D, RT_Render_Params const *p, void const *d_accum, void *d_tiles, void *d_image, void *d_linear,
               hipStream_t stream);                                                 // D's GPU current
int untile_on(Device &D, i32 width, i32 height, i32 world, void const *d_all_tiles, void *d_image, hipStream_t stream);   // D's GPU current
int ensure_ws_buffers(Workspace &W, int width, int height, size_t tiles_bytes, size_t all_tiles_bytes, bool want_linear = true);
int copy_image_out(Image const *image, const uint8_t *d_image, int width, int height, hipStream_t stream);
int read_counters(Device &D, unsigned long long c[RT_N_COUNTERS]);                  // D.mutex held, D's GPU current

// rt_frames.cpp
void forget_multi_counters();                                                       // takes g_multi_mutex
// The one-device frame sequence on `stream`: event 0, accumulator clear, path tracer (launch state `launch_state`), event 2,
// resolve into tiles / image / linear, event 3.  D.mutex held, D's GPU current.  batch (optional): K views, W.accum / image /
// linear hold K images one after the other, one resolve per view (tiles must be NULL).
int  enqueue_frame(Device &D, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p, Workspace &W, hipStream_t stream,
                   int launch_state, uint8_t *tiles, uint8_t *image, float *linear, ViewBatch const *batch = nullptr);
void frame_split(Workspace &W, FrameTiming &T);                                     // the four GPU spans between W's frame events
// The end of a blocking frame whose event 4 is recorded and whose copies are issued on `stream`: waits for it, and T -- with
// frame_split and total_ms since t_start -- becomes D's timing.
int  finish_frame(Device &D, Workspace &W, hipStream_t stream, FrameTiming &T, double t_start);
// The halves of a one-device frame's parameters (rank 0 of 1) into `image`: the Image's layout, refused with `who` in front; p
// filled and through check_params.
int  check_image_layout(Image const *image, const char *who);
int  fill_frame_params(RT_Render_Params *p, Image const *image, isize samples, isize max_bounces, u32 seed);

// rt_multi.cpp
int render_frame_multi(Scene const *scene, Image const *image, RT_Render_Params base, int world);   // slot 0's mutex held

// rt_query.cpp
void release_query_state(Device &D);                                                // release_staging()'s part here
int  ensure_query_state(Device &D);                                                 // D.mutex held, D's GPU current
// The ring slot of a new launch.  `query`: a query call, the one rt_get_query_counters() reports.  D.mutex held, D's GPU current.
int  acquire_slot(Device &D, int *slot, bool query = true);

// rt_features.cpp
// THE FEATURE PASS of one frame on `stream` (what rt_render_features runs; rt_post.cpp runs it behind a frame): d_sums zeroed, one
// launch of the feature kernel over p's image, and the resolve into the planes of `to` that are given (none: no resolve).
// d_motion_sums (optional): zeroed too, and the motion kernel in place of the plain one -- one launch -- against d's kept geometry
// (none: the current tiles, every motion sum 0); d_motion (optional, with d_motion_sums): they are resolved into it.
// D.mutex held, D's GPU current, every pointer on D.
int  enqueue_feature_pass(Device &D, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p, void *d_sums, RT_Features const &to,
                          hipStream_t stream, void *d_motion_sums = nullptr, void *d_motion = nullptr);

// rt_query.cpp, light probes
void release_probe_state(Device &D);                                                // release_staging()'s part here

// rt_extras.cpp, HDR lightmaps
void release_lightmap_state(Device &D);                                             // release_staging()'s part here

// rt_post.cpp
void release_temporal_state(Device &D);                                             // release_staging()'s part here

// rt_diag.cpp (diagnostic library only); the product's fault hooks are constant
#ifdef RT_DIAG_VARIANTS
extern std::atomic<int> g_pipeline;                     // 0 = tile-stream path kernel, 1 = wavefront pipeline
int  launch_wavefront(Device &D, RT_Device_Scene *d, RT_KParams &K, hipStream_t stream);   // D.mutex held, D's GPU current
bool fault_no_peer();
bool fault_fails(int slot);
#else
static inline bool fault_no_peer() { return false; }
static inline bool fault_fails(int) { return false; }
#endif

#pragma GCC visibility pop
