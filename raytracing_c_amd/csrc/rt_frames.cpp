// rt_frames.cpp -- the one-device frame sequence, blocking frames, frames in flight, frame timing, completion protocol.

#include "rt_host.h"

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
