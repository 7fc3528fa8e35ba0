// rt_frames.cpp -- the one-device frame sequence, blocking frames, frames in flight, frame timing, completion protocol, the adaptive
// frame and its two device-level calls.

#include "rt_host.h"

#include <cmath>

void forget_multi_counters() {
  std::lock_guard<std::mutex> lk(g_multi_mutex);
  g_multi_counters_valid = false;
}

int check_image_layout(Image const *image, const char *who) {
  if (image->pixels.data && image->components < 3) return rt_fail("%s: image needs >= 3 components", who);
  if (image->pixels.data && image->stride < image->width) return rt_fail("%s: image stride < width", who);
  return 0;
}

int fill_frame_params(RT_Render_Params *p, Image const *image, isize samples, isize max_bounces, u32 seed) {
  memset(p, 0, sizeof *p);
  p->width = (i32)image->width;
  p->height = (i32)image->height;
  p->samples = (i32)samples;
  p->max_bounces = (i32)max_bounces;
  p->seed = seed;
  p->rank = 0;
  p->world = 1;
  return check_params(p);
}

// The parameters of a one-device frame into `image` (rank 0 of 1), validated; `who` prefixes the error messages.
static int frame_params(Image const *image, isize samples, isize max_bounces, u32 seed, const char *who, RT_Render_Params *p) {
  if (check_image_layout(image, who) != 0) return -1;
  return fill_frame_params(p, image, samples, max_bounces, seed);
}

int enqueue_frame(Device &D, RT_Device_Scene *d, Camera const *cam, RT_Render_Params const *p, Workspace &W, hipStream_t stream,
                  int launch_state, uint8_t *tiles, uint8_t *image, float *linear, ViewBatch const *batch) {
  const int nv = batch ? batch->n : 1;
  const size_t view3 = (size_t)p->width * p->height * 3;      // elements of one view's accumulator / image / linear values
  HIP_TRY(hipEventRecord(W.ev_frame[0], stream));
  HIP_TRY(hipMemsetAsync(W.accum, 0, view3 * nv * sizeof(unsigned long long), stream));
  if (render_accumulate_locked(D, d, cam, p, W.accum, stream, W.ev_frame[1], launch_state, batch) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[2], stream));
  for (int v = 0; v < nv; v++)
    if (resolve_on(D, p, W.accum + v * view3, tiles, image ? image + v * view3 : nullptr, linear ? linear + v * view3 : nullptr,
                   stream) != 0)
      return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[3], stream));
  return 0;
}

void frame_split(Workspace &W, FrameTiming &T) {
  T.gpu_prep_ms = event_ms(W.ev_frame[0], W.ev_frame[1]);
  T.gpu_path_ms = event_ms(W.ev_frame[1], W.ev_frame[2]);
  T.gpu_resolve_ms = event_ms(W.ev_frame[2], W.ev_frame[3]);
  T.gpu_copy_ms = event_ms(W.ev_frame[3], W.ev_frame[4]);
}

int finish_frame(Device &D, Workspace &W, hipStream_t stream, FrameTiming &T, double t_start) {
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  frame_split(W, T);
  T.total_ms = (float)(now_ms() - t_start);
  D.timing = T;
  return 0;
}

// batch (rt_render_views): `image` points to batch->n images of one size, linear / accum hold batch->n views one after the other.
static int render_frame_locked(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                               f32 *linear, u64 *accum, Camera const *camera = nullptr, u32 const *seed = nullptr,
                               ViewBatch const *batch = nullptr) {
  Device &D = dev0();
  const double t_start = now_ms();
  if (ensure_device(D) != 0) return -1;
  if (!scene || !image) return rt_fail("render: NULL scene or image");
  RT_Render_Params p;
  // (camera / seed given: a frame of rt_frame_begin rendered again, as it was begun)
  if (frame_params(image, samples, max_bounces, seed ? *seed : g_seed.load(), "render", &p) != 0) return -1;
  forget_multi_counters();
  const int world = rt_device_count();
  if (batch && world > 1)
    return rt_fail("rt_render_views: a batch of views renders on one device, and %d are set (rt_set_devices)", world);
  if (world > 1 && !linear && !accum && rt_chunk_count(p.width, p.height) >= world)
    return render_frame_multi(scene, image, p, world);

  FrameTiming T;
  const int nv = batch ? batch->n : 1;
  if (ensure_ws_buffers(D.ws, p.width, p.height * nv, 0, 0) != 0) return -1;      // (a batch: nv images one after the other)
  Workspace &W = D.ws;
  size_t pixels = (size_t)p.width * p.height;
  hipStream_t stream = nullptr;
  auto frame = [&](RT_Device_Scene *d) -> int {
    return enqueue_frame(D, d, camera ? camera : &scene->camera, &p, W, stream, batch ? RT_VIEWS_STATE : 0, nullptr, W.image,
                         linear ? W.linear : nullptr, batch);
  };
  if (!scene_checked(D, scene, stream, &T, frame)) return -1;      // (a scene edited since the copy: uploaded and rendered again)

  for (int v = 0; v < nv; v++)
    if (copy_image_out(&image[v], W.image + v * pixels * 3, p.width, p.height, stream) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[4], stream));
  if (linear) HIP_TRY(hipMemcpy(linear, W.linear, nv * pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (accum) HIP_TRY(hipMemcpy(accum, W.accum, nv * pixels * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return finish_frame(D, W, stream, T, t_start);
}

extern "C" int rt_render_frame(Scene const *scene, Image const *image, isize samples, isize max_bounces, f32 *linear,
                               u64 *accum) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  return render_frame_locked(scene, image, samples, max_bounces, linear, accum);
}

// K views of one scene in one launch: the frame sequence above with a view table (rt_hip.h).  Every argument is checked before the
// device is touched.
extern "C" int rt_render_views(Scene const *scene, i32 n_views, RT_View const *views, Image const *images, isize samples,
                               isize max_bounces, f32 *linear, u64 *accum) {
  const char *who = "rt_render_views";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!views) return rt_fail("%s: views is NULL", who);
  if (!images) return rt_fail("%s: images is NULL", who);
  if (n_views <= 0) return rt_fail("%s: n_views must be positive (got %d)", who, n_views);
  RT_Render_Params p;
  if (frame_params(&images[0], samples, max_bounces, 0, who, &p) != 0) return -1;
  if (check_views(n_views, views, p.width, p.height, who) != 0) return -1;      // (before images[1 ..] are read)
  for (i32 v = 1; v < n_views; v++) {
    Image const &im = images[v];
    if (im.width != images[0].width || im.height != images[0].height)
      return rt_fail("%s: image %d is %ldx%ld, image 0 is %ldx%ld: every view must have the same size", who, v, (long)im.width,
                     (long)im.height, (long)images[0].width, (long)images[0].height);
    if (im.pixels.data && im.components < 3) return rt_fail("%s: image %d needs >= 3 components", who, v);
    if (im.pixels.data && im.stride < im.width) return rt_fail("%s: image %d stride < width", who, v);
  }
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  ViewBatch batch;
  batch.n = n_views;
  batch.views = views;
  return render_frame_locked(scene, images, samples, max_bounces, linear, accum, &views[0].camera, &views[0].seed, &batch);
}

extern "C" int render(Scene *scene, Image *image, isize samples, isize max_bounces) {
  return rt_render_frame(scene, image, samples, max_bounces, nullptr, nullptr);
}

// A lane's stream must not share a HARDWARE queue with the other lane's: the runtime multiplexes its streams onto a few HSA queues
// (GPU_MAX_HW_QUEUES, 4 by default), and two streams on one queue run their kernels one after the other -- measured: with ONE more
// stream in the process (a torch side stream) two plain non-blocking streams landed on one queue and the overlap was gone (2.67
// instead of 2.23 ms per default frame, gpurun_out/r05fl).  The runtime pools its queues per stream priority, so the lanes take
// different priorities: never the same queue, whatever else the process creates.  (A stream with an all-ones CU mask owns its queue
// too and measures the same, but it is a blocking stream: it would wait for every null-stream operation of the host.)
static hipError_t create_lane_stream(hipStream_t *s, int lane) {
  int lo = 0, hi = 0;
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, lane == 0 ? 0 : hi);
}

// ---- frames in flight (rt_hip.h) ---------------------------------------------------------------------------------------------
extern "C" int rt_frame_begin(Scene const *scene, Image const *image, isize samples, isize max_bounces) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  const double t_start = now_ms();
  if (ensure_device(D) != 0) return -1;
  if (!scene || !image) return rt_fail("rt_frame_begin: NULL scene or image");
  RT_Render_Params p;
  if (frame_params(image, samples, max_bounces, g_seed.load(), "rt_frame_begin", &p) != 0) return -1;
  int ticket = -1;
  for (int k = 0; k < RT_FRAME_LANES; k++)
    if (!D.lanes[k].busy) { ticket = k; break; }
  if (ticket < 0) return rt_fail("rt_frame_begin: %d frames are in flight already (rt_frame_end one of them first)", RT_FRAME_LANES);
  FrameLane &F = D.lanes[ticket];
  F.scene = scene; F.image = *image; F.p = p; F.camera = scene->camera; F.d = nullptr; F.fp = 0; F.rc = 0; F.finished = false; F.timing = FrameTiming();
  F.t_begin = t_start;
  if (rt_device_count() > 1) {
    // a frame over N devices has its own pipeline (render_frame_multi): rendered here and now, rt_frame_end() reports how it went
    F.rc = render_frame_locked(scene, image, samples, max_bounces, nullptr, nullptr);
    F.finished = true;
    F.busy = true;
    return ticket;
  }
  forget_multi_counters();
  if (!F.stream) HIP_TRY(create_lane_stream(&F.stream, ticket));
  if (ensure_ws_buffers(F.ws, p.width, p.height, 0, 0, false) != 0) return -1;
  RT_Device_Scene *d = cached_scene_locked(D, scene, &F.timing.stamp_ms, &F.timing.upload_ms);
  if (!d) return -1;
  const double t_enq = now_ms();
  if (enqueue_frame(D, d, &F.camera, &p, F.ws, F.stream, 1 + ticket, nullptr, F.ws.image, nullptr) != 0) return -1;
  F.timing.enqueue_ms = (float)(now_ms() - t_enq);
  F.d = d;
  F.fp = d->full_fp;
  F.verify = !scene_is_static(scene) && F.timing.upload_ms == 0.0f;      // (a copy made for this frame IS the host scene)
  F.busy = true;
  return ticket;
}

extern "C" int rt_frame_end(int ticket) {
  Device &D = dev0();
  std::unique_lock<std::mutex> lock(D.mutex);
  if (ticket < 0 || ticket >= RT_FRAME_LANES || !D.lanes[ticket].busy || D.lanes[ticket].ending)
    return rt_fail("rt_frame_end: no frame in flight with ticket %d", ticket);
  FrameLane &F = D.lanes[ticket];
  if (F.finished) { F.busy = false; return F.rc; }
  if (ensure_device(D) != 0) { F.busy = false; return -1; }
  Workspace &W = F.ws;
  // The wait happens WITHOUT the device's mutex: another host thread can begin (or end) the other lane's frame, or render a
  // blocking one, meanwhile.  The lane stays busy -- nobody else touches it -- and `ending` refuses a second end of this ticket.
  F.ending = true;
  hipStream_t stream = F.stream;
  const bool verify = F.verify;
  Scene const *scene = F.scene;
  lock.unlock();
  // the full content check of the blocking path (render_frame_locked), on this thread, while the GPU renders: the frame came from
  // a copy with fingerprint F.fp; a host scene that no longer has it is rendered again, like there
  uint64_t now = 0;
  float verify_ms = 0.0f;
  if (verify) {
    const double t_v = now_ms();
    now = scene_fingerprint(scene);
    verify_ms = (float)(now_ms() - t_v);
  }
  hipError_t e = hipStreamSynchronize(stream);
  lock.lock();
  F.ending = false;
  F.timing.verify_ms = verify_ms;
  if (ensure_device(D) != 0) { F.busy = false; return -1; }
  if (verify && now != F.fp) {
    auto it = D.scene_cache.find(F.scene);
    if (it != D.scene_cache.end() && it->second->full_fp != now) {
      free_device_scene(it->second);        // (waits for the other lane if that renders from it)
      D.scene_cache.erase(it);
    }
    F.busy = false;
    F.d = nullptr;
    return render_frame_locked(F.scene, &F.image, F.p.samples, F.p.max_bounces, nullptr, nullptr, &F.camera, &F.p.seed);
  }
  F.busy = false;
  if (e != hipSuccess) return rt_fail("rt_frame_end: %s", hipGetErrorString(e));
  if (copy_image_out(&F.image, W.image, F.p.width, F.p.height, F.stream) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[4], F.stream));
  FrameTiming T = F.timing;
  if (finish_frame(D, W, F.stream, T, F.t_begin) != 0) return -1;
  D.last_counters = F.d ? F.d->ls[1 + ticket].counters : nullptr;       // rt_get_counters() = this frame's
  F.d = nullptr;
  return 0;
}

// Where the time of the last frame behind render_thread_proc / render / rt_render_frame went (one-device frames; a
// multi-device frame reports total_ms only).  Host: stamp = the per-frame scene check, upload = scene upload when it
// happened, enqueue = launching the frame; GPU (HIP events on the frame's stream): prep = accumulator clear + the
// preparation kernel, path = the path kernel, resolve, copy = device-to-host copy of the image; total = wall clock of the call.
extern "C" int rt_get_frame_timing(RT_Frame_Timing *out) {
  if (!out) return rt_fail("rt_get_frame_timing: NULL");
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  out->stamp_ms = D.timing.stamp_ms; out->upload_ms = D.timing.upload_ms; out->enqueue_ms = D.timing.enqueue_ms;
  out->gpu_prep_ms = D.timing.gpu_prep_ms; out->gpu_path_ms = D.timing.gpu_path_ms; out->gpu_resolve_ms = D.timing.gpu_resolve_ms;
  out->gpu_copy_ms = D.timing.gpu_copy_ms; out->total_ms = D.timing.total_ms;
  out->verify_ms = D.timing.verify_ms; out->gather_ms = D.timing.gather_ms;
  out->n_devices = D.timing.n_devices; out->slowest_device = D.timing.slowest_device;
  return 0;
}

// ---------------------------------------------------------------------------------
// the reference's entry points

extern "C" void render_thread_proc(Rendering_Context *ctx) {
  if (!ctx) return;
  i32 c = __atomic_fetch_add(&ctx->_current_chunk, 1, __ATOMIC_SEQ_CST);
  if (c == 0) {
    // this entrant owns the frame (all rt_device_count() GPUs of it: render_frame_multi)
    int rc;
    {
      Device &D = dev0();
      std::lock_guard<std::mutex> lock(D.mutex);
      rc = render_frame_locked(ctx->scene, &ctx->image, ctx->samples, ctx->max_bounces, nullptr, nullptr);
    }
    (void)rc;   // failure text is in rt_last_error(); the context still completes
    i32 n_chunks = rt_chunk_count((i32)ctx->image.width, (i32)ctx->image.height);
    __atomic_store_n(&ctx->_current_chunk, n_chunks > 0 ? n_chunks : 1, __ATOMIC_SEQ_CST);
  }
  __atomic_fetch_add(&ctx->n_threads, -1, __ATOMIC_SEQ_CST);
}

extern "C" bool rendering_context_is_finished(Rendering_Context *context) {
  return __atomic_load_n(&context->n_threads, __ATOMIC_SEQ_CST) == 0;
}

extern "C" void rendering_context_finish(Rendering_Context *context) {
  while (__atomic_load_n(&context->n_threads, __ATOMIC_SEQ_CST) > 0) std::this_thread::yield();
}

// ---------------------------------------------------------------------------------
// adaptive sampling (include/rt_hip.h): the merge of two equal halves of a chunk's samples and the per-chunk resolve on the device
// level, and the blocking frame whose chunks double their samples until their error settles (rt_render_adaptive): one launch of the
// path kernel per round over a shrinking chunk list (rt_launch.cpp: a launch with the caller's chunk table).

// ---- the device level -------------------------------------------------------------------------------------------------------------

// The merge of `list` on `stream`, the list staged through D.adaptive.merge_list.  D.mutex held, D's GPU current, list checked.
static int enqueue_merge(Device &D, i32 width, i32 height, i32 n, ChunkList const &list, void *d_accum, void *d_fresh, void *d_err,
                         hipStream_t stream) {
  const int32_t *d_list = nullptr;
  if (stage_chunk_list(D.adaptive.merge_list, list, stream, &d_list) != 0) return -1;
  int rc = rt_launch_adaptive_merge(width, height, n, list.n, d_list, (unsigned long long *)d_accum, (unsigned long long *)d_fresh,
                                    (unsigned long long *)d_err, stream);
  if (rc != 0) return rt_fail("adaptive merge kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int rt_adaptive_merge(i32 width, i32 height, i32 n, i32 n_list, i32 const *chunks, void *d_accum, void *d_fresh, void *d_err,
                                 void *stream) {
  const char *who = "rt_adaptive_merge";
  if (check_image_size(who, width, height) != 0) return -1;
  if (n < 1) return rt_fail("%s: n must be >= 1, the samples each buffer holds per pixel (got %d)", who, n);
  if (check_chunk_list(who, width, height, n_list, chunks) != 0) return -1;
  if (!d_accum) return rt_fail("%s: d_accum is NULL", who);
  if (!d_fresh) return rt_fail("%s: d_fresh is NULL", who);
  if (!d_err) return rt_fail("%s: d_err is NULL", who);
  if (d_accum == d_fresh) return rt_fail("%s: d_accum and d_fresh are one buffer", who);
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  DeviceGuard guard(D);
  ChunkList list;
  list.n = n_list;
  list.chunks = chunks;
  return enqueue_merge(D, width, height, n, list, d_accum, d_fresh, d_err, (hipStream_t)stream);
}

extern "C" int rt_resolve_adaptive(i32 width, i32 height, void const *d_chunk_samples, void const *d_accum, void *d_image, void *d_linear,
                                   void *d_sample_map, void *stream) {
  const char *who = "rt_resolve_adaptive";
  if (check_image_size(who, width, height) != 0) return -1;
  if (!d_chunk_samples) return rt_fail("%s: d_chunk_samples is NULL", who);
  if (!d_accum) return rt_fail("%s: d_accum is NULL", who);
  if (!d_image && !d_linear && !d_sample_map) return rt_fail("%s: no output is wanted (no d_image, no d_linear, no d_sample_map)", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  DeviceGuard guard(D);
  int rc = rt_launch_resolve_adaptive(width, height, (const int32_t *)d_chunk_samples, (const unsigned long long *)d_accum,
                                      (uint8_t *)d_image, (float *)d_linear, (int32_t *)d_sample_map, (hipStream_t)stream);
  if (rc != 0) return rt_fail("adaptive resolve kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- the frame --------------------------------------------------------------------------------------------------------------------

static int check_adaptive(const char *who, RT_Adaptive_Params const *ap) {
  if (!ap) return rt_fail("%s: adaptive params are NULL", who);
  if (ap->min_samples < 1) return rt_fail("%s: min_samples must be >= 1 (got %d)", who, ap->min_samples);
  bool doubled = false;
  for (int64_t m = (int64_t)ap->min_samples * 2; m <= (int64_t)0x7fffffff; m *= 2)
    if (m == ap->max_samples) doubled = true;
  if (!doubled)
    return rt_fail("%s: max_samples must be min_samples * 2^k with k >= 1 (got %d and min_samples %d)", who, ap->max_samples, ap->min_samples);
  if (!(ap->threshold >= 0.0f) || std::isinf(ap->threshold))
    return rt_fail("%s: threshold must be finite and >= 0 (got %g)", who, (double)ap->threshold);
  if (ap->reserved != 0) return rt_fail("%s: reserved must be 0 (got %d)", who, ap->reserved);
  return 0;
}

// The host's decision after a round (rt_hip.h): the chunk's mean per-pixel error, in double, over its pixels inside the image.
static double chunk_error(unsigned long long sum, i32 width, i32 height, i32 chunk) {
  const int chunks_x = (width + RT_CHUNK_SIZE - 1) / RT_CHUNK_SIZE;
  const int x0 = (chunk % chunks_x) * RT_CHUNK_SIZE, y0 = (chunk / chunks_x) * RT_CHUNK_SIZE;
  const int w = width - x0 < RT_CHUNK_SIZE ? width - x0 : RT_CHUNK_SIZE, h = height - y0 < RT_CHUNK_SIZE ? height - y0 : RT_CHUNK_SIZE;
  return (double)sum / 4294967296.0 / (double)(w * h);
}

extern "C" int rt_render_adaptive(Scene const *scene, Image const *image, RT_Adaptive_Params const *ap, isize max_bounces, f32 *linear,
                                  u64 *accum, i32 *chunk_samples) {
  const char *who = "rt_render_adaptive";
  // before the device lock: everything the arguments alone decide
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!image) return rt_fail("%s: image is NULL", who);
  if (check_adaptive(who, ap) != 0) return -1;
  if (image->width <= 0 || image->height <= 0 || image->width > 0x7fffffff || image->height > 0x7fffffff)
    return rt_fail("%s: image size %ldx%ld is invalid", who, (long)image->width, (long)image->height);
  if (check_image_size(who, (i32)image->width, (i32)image->height) != 0) return -1;
  if (check_image_layout(image, who) != 0) return -1;
  if (max_bounces < 0 || max_bounces > 0x7fffffff) return rt_fail("%s: max_bounces must be >= 0 and fit 32 bits (got %ld)", who, (long)max_bounces);
  if (!image->pixels.data && !linear && !accum && !chunk_samples)
    return rt_fail("%s: no output is wanted (no pixels, no linear, no accum, no chunk_samples)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  const double t_start = now_ms();
  if (ensure_device(D) != 0) return -1;
  if (rt_device_count() > 1)
    return rt_fail("%s: an adaptive frame renders on one device, and %d are set (rt_set_devices)", who, rt_device_count());
  RT_Render_Params p;      // (samples: the cap -- every launch traces a sample range inside [0, max_samples))
  if (fill_frame_params(&p, image, ap->max_samples, max_bounces, g_seed.load()) != 0) return -1;
  forget_multi_counters();

  FrameTiming T;
  Workspace &W = D.ws;
  AdaptiveState &A = D.adaptive;
  const i32 width = p.width, height = p.height, n_chunks = rt_chunk_count(width, height);
  const size_t pixels = (size_t)width * height;
  if (ensure_ws_buffers(W, width, height, 0, 0, linear != nullptr) != 0) return -1;
  HIP_TRY(A.fresh.grow(pixels * 3));
  HIP_TRY(A.err.grow((size_t)n_chunks));
  HIP_TRY(A.err_host.grow((size_t)n_chunks));
  HIP_TRY(A.chunk_samples.grow((size_t)n_chunks));
  HIP_TRY(A.counters_host.grow((size_t)RT_ADAPTIVE_MAX_LAUNCHES * RT_N_COUNTERS));

  hipStream_t stream = nullptr;
  std::vector<i32> active, counts((size_t)n_chunks, 0);
  int n_launches = 0;
  // one launch of the path kernel over the active chunks, samples [first, first + count) into `dst`; its counters go to the host
  // behind it (the next launch's preparation clears them)
  auto launch = [&](RT_Device_Scene *d, i32 first, i32 count, void *dst, hipEvent_t ev_prep) -> int {
    if (n_launches >= RT_ADAPTIVE_MAX_LAUNCHES) return rt_fail("%s: more than %d launches", who, RT_ADAPTIVE_MAX_LAUNCHES);
    RT_Render_Params q = p;
    q.sample_first = first;
    q.sample_count = count;
    ChunkList list;
    list.n = (int)active.size();
    list.chunks = active.data();
    if (render_accumulate_locked(D, d, &scene->camera, &q, dst, stream, ev_prep, RT_ADAPTIVE_STATE, nullptr, &list) != 0) return -1;
    HIP_TRY(hipMemcpyAsync(A.counters_host + (size_t)n_launches * RT_N_COUNTERS, d->ls[RT_ADAPTIVE_STATE].counters,
                           RT_N_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    n_launches++;
    return 0;
  };
  // a round: the active chunks hold n samples; samples [n, 2n) into `fresh`, the merge, the errors on their way to the host
  auto round = [&](RT_Device_Scene *d, i32 n) -> int {
    if (launch(d, n, n, A.fresh, nullptr) != 0) return -1;
    ChunkList list;
    list.n = (int)active.size();
    list.chunks = active.data();
    if (enqueue_merge(D, width, height, n, list, W.accum, A.fresh, A.err, stream) != 0) return -1;
    HIP_TRY(hipMemcpyAsync(A.err_host, A.err, (size_t)n_chunks * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(W.ev_frame[2], stream));
    return 0;
  };
  // what every frame needs -- samples [0, min) and the first round, over all chunks -- is enqueued inside the scene-checked call:
  // the full content check of the host scene runs while the GPU traces them (a scene edited since the copy: all of it once more)
  auto begin = [&](RT_Device_Scene *d) -> int {
    n_launches = 0;
    active.resize((size_t)n_chunks);
    for (i32 c = 0; c < n_chunks; c++) active[(size_t)c] = c;
    HIP_TRY(hipEventRecord(W.ev_frame[0], stream));
    HIP_TRY(hipMemsetAsync(W.accum, 0, pixels * 3 * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(A.fresh, 0, pixels * 3 * sizeof(unsigned long long), stream));      // (once: the merge re-zeroes what it consumed)
    if (launch(d, 0, ap->min_samples, W.accum, W.ev_frame[1]) != 0) return -1;
    return round(d, ap->min_samples);
  };
  RT_Device_Scene *d = scene_checked(D, scene, stream, &T, begin);
  if (!d) return -1;

  for (i32 n = ap->min_samples;; n *= 2) {
    HIP_TRY(hipStreamSynchronize(stream));            // the round's errors are on the host
    std::vector<i32> next;
    for (i32 c : active) {
      counts[(size_t)c] = 2 * n;
      if (chunk_error(A.err_host[c], width, height, c) > (double)ap->threshold && (int64_t)2 * n < ap->max_samples) next.push_back(c);
    }
    active.swap(next);
    if (active.empty()) break;
    if (round(d, 2 * n) != 0) return -1;
  }

  HIP_TRY(hipMemcpyAsync(A.chunk_samples, counts.data(), (size_t)n_chunks * sizeof(i32), hipMemcpyHostToDevice, stream));
  {
    int rc = rt_launch_resolve_adaptive(width, height, A.chunk_samples, W.accum, W.image, linear ? W.linear.get() : nullptr, nullptr, stream);
    if (rc != 0) return rt_fail("adaptive resolve kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  HIP_TRY(hipEventRecord(W.ev_frame[3], stream));
  if (copy_image_out(image, W.image, width, height, stream) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[4], stream));
  if (linear) HIP_TRY(hipMemcpy(linear, W.linear, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (accum) HIP_TRY(hipMemcpy(accum, W.accum, pixels * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (finish_frame(D, W, stream, T, t_start) != 0) return -1;
  if (chunk_samples) memcpy(chunk_samples, counts.data(), (size_t)n_chunks * sizeof(i32));

  // rt_get_counters(): the sum over the frame's launches, kept where a multi-device frame keeps its sum
  unsigned long long c[RT_N_COUNTERS] = {};
  for (int l = 0; l < n_launches; l++)
    for (int k = 0; k < RT_N_COUNTERS; k++) c[k] += A.counters_host[(size_t)l * RT_N_COUNTERS + k];
  std::lock_guard<std::mutex> lk(g_multi_mutex);
  g_multi_counters.paths = c[RT_CNT_PATHS];
  g_multi_counters.rays = c[RT_CNT_RAYS];
  g_multi_counters.node_visits = c[RT_CNT_NODES];
  g_multi_counters.leaf_visits = c[RT_CNT_LEAVES];
  g_multi_counters.shades = c[RT_CNT_SHADES];
  g_multi_counters.backgrounds = c[RT_CNT_BG];
  g_multi_counters.textured = c[RT_CNT_TEXTURED];
  g_multi_counters_valid = true;
  return 0;
}
