// rt_multi.cpp -- a frame spread over the N GPUs of this node, behind the reference's own entry points.
//
// driver.c:793-803 starts `-T n` threads on render_thread_proc; the one that claims the frame drives N devices (N =
// rt_device_count()): every device holds its own copy of the scene, renders the chunks rt_chunk_owner() gives its rank and
// resolves them to compact u8 tiles; the tiles travel to device 0 with ONE peer copy per device over xGMI
// (hipMemcpyPeerAsync; 0.78 MB each at 1080p), device 0 untiles into the row-major image and copies it to the caller's
// pixels.  Devices are driven by one internal host thread each (uploads and launches proceed in parallel; the calling
// application's other threads return at once, as in the one-GPU case).  Per-path seeds depend on (pixel, sample) only, so
// the image does not depend on N (tests/test_gpu_multi_device.py: byte-equal to the one-device frame).
// How the N devices are driven (round 4):
//  * one PERSISTENT internal host thread per device slot >= 1, started the first time the slot is used and parked on a
//    condition variable between frames (round 3 created and joined N - 1 threads per frame);
//  * a device thread only ENQUEUES -- clear, preparation, path kernel, resolve to compact tiles, the tile copy towards slot 0,
//    an asynchronous copy of its ray counters into pinned host memory, an event -- and returns; nothing on it waits for the GPU;
//  * slot 0's stream waits for the other devices' events (hipStreamWaitEvent), untiles, copies the image out: ONE host
//    synchronisation per frame, at the end;
//  * a device without peer access to slot 0 (hipDeviceCanAccessPeer refused) stages its tiles through pinned host memory;
//  * the full content check of the host scene (rt_scene_touch) runs on the calling thread while all of that is in flight;
//  * rt_get_frame_timing() reports the slowest device's prep / path / resolve / copy times, the gather + untile + copy-out
//    time after it, and which device it was.

#include "rt_host.h"

struct MultiFrame {
  Scene const      *scene = nullptr;
  RT_Render_Params  base;
  int               world = 0, w = 0, h = 0;
  size_t            tiles_bytes = 0;
  int               rcs[RT_MAX_DEVICES];
  bool              staged[RT_MAX_DEVICES];
  float             stamp_ms[RT_MAX_DEVICES], upload_ms[RT_MAX_DEVICES], enqueue_ms[RT_MAX_DEVICES];
  uint64_t          full_fp[RT_MAX_DEVICES];       // the full fingerprint of the copy each slot rendered from
  char              err[RT_MAX_DEVICES][256];
  std::mutex              m;
  std::condition_variable cv;
  int                     pending = 0;
};

struct DevWorker {
  std::mutex              m;
  std::condition_variable cv;
  MultiFrame             *job = nullptr;
  bool                    started = false;
};
static DevWorker *g_workers = new DevWorker[RT_MAX_DEVICES];     // never destroyed: the parked threads outlive static destructors

static void device_fail(MultiFrame &J, int r, const char *what) {
  Device &D = g_devs[r];
  snprintf(J.err[r], sizeof J.err[r], "device %d (slot %d of %d): %s", D.phys, r, J.world, what);
}

// Everything device slot `r` contributes to the frame, enqueued on its null stream; returns without waiting for the GPU.
static void enqueue_device_frame(MultiFrame &J, int r) {
  Device &D = g_devs[r];
  Device &D0 = dev0();
  std::unique_lock<std::mutex> lock(D.mutex, std::defer_lock);
  if (r != 0) lock.lock();                                   // (slot 0's mutex is held by the frame's owner)
  J.rcs[r] = -1;
  J.staged[r] = false;
  J.err[r][0] = 0;
  J.full_fp[r] = 0;
  D.slot = r;
  if (ensure_device(D) != 0) { device_fail(J, r, rt_last_error()); return; }       // assigns D.phys and makes it this thread's device
  if (fault_fails(r)) { device_fail(J, r, "injected failure (rt_diag_multi_fault)"); return; }
  RT_Device_Scene *d = cached_scene_locked(D, J.scene, &J.stamp_ms[r], &J.upload_ms[r]);
  if (!d) { device_fail(J, r, rt_last_error()); return; }
  J.full_fp[r] = d->full_fp;                                 // what THIS slot's copy was made from
  const double t_enq = now_ms();
  Workspace &W = D.ws;
  if (ensure_ws_buffers(W, J.w, J.h, J.tiles_bytes, r == 0 ? J.tiles_bytes * (size_t)J.world : 0) != 0) { device_fail(J, r, rt_last_error()); return; }
  if (W.counters_host.grow(RT_N_COUNTERS) != hipSuccess) { device_fail(J, r, "pinned counter buffer"); return; }
  const bool same_gpu = D.phys == D0.phys;
  const bool direct = same_gpu || (D.peer_ok && !fault_no_peer());
  if (!direct && W.tiles_host.grow(J.tiles_bytes) != hipSuccess) { device_fail(J, r, "pinned tile buffer"); return; }
  RT_Render_Params p = J.base;
  p.rank = r;
  p.world = J.world;
  // every slot works on a stream of its own: on N GPUs that changes nothing; N slots rehearsed on ONE GPU overlap -- the
  // next slot's workgroups take the CUs the previous slot's last paths leave idle -- instead of queueing N launch tails
  hipStream_t stream = D.mstream;
  if (enqueue_frame(D, d, &J.scene->camera, &p, W, stream, 0, W.tiles, nullptr, nullptr) != 0) { device_fail(J, r, rt_last_error()); return; }
  uint8_t *dst = D0.ws.all_tiles + (size_t)r * J.tiles_bytes;
  hipError_t e;
  if (same_gpu) e = hipMemcpyAsync(dst, W.tiles, J.tiles_bytes, hipMemcpyDeviceToDevice, stream);
  else if (direct) e = hipMemcpyPeerAsync(dst, D0.phys, W.tiles, D.phys, J.tiles_bytes, stream);      // one xGMI link per device
  else { e = hipMemcpyAsync(W.tiles_host, W.tiles, J.tiles_bytes, hipMemcpyDeviceToHost, stream); J.staged[r] = true; }
  if (e == hipSuccess) e = hipMemcpyAsync(W.counters_host, d->ls[0].counters, RT_N_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipEventRecord(W.ev_frame[4], stream);
  if (e != hipSuccess) { device_fail(J, r, hipGetErrorString(e)); return; }
  J.enqueue_ms[r] = (float)(now_ms() - t_enq);
  J.rcs[r] = 0;
}

static void worker_loop(int r) {
  DevWorker &Wk = g_workers[r];
  for (;;) {
    MultiFrame *J;
    {
      std::unique_lock<std::mutex> lk(Wk.m);
      Wk.cv.wait(lk, [&] { return Wk.job != nullptr; });
      J = Wk.job;
      Wk.job = nullptr;
    }
    enqueue_device_frame(*J, r);
    {
      std::lock_guard<std::mutex> lk(J->m);
      J->pending -= 1;
    }
    J->cv.notify_all();
  }
}

int render_frame_multi(Scene const *scene, Image const *image, RT_Render_Params base, int world) {
  Device &D0 = dev0();                               // D0.mutex held by the caller
  const double t0 = now_ms();
  const int w = base.width, h = base.height;
  const size_t max_local = (size_t)rt_max_local_chunk_count(w, h, world);
  const size_t tiles_bytes = max_local * 1024 * 3;
  if (ensure_ws_buffers(D0.ws, w, h, tiles_bytes, tiles_bytes * (size_t)world) != 0) return -1;
  const bool verify = !scene_is_static(scene);
  FrameTiming T;
  T.n_devices = world;
  static MultiFrame J;                               // (one multi-device frame at a time: D0.mutex)
  for (int attempt = 0;; attempt++) {
    J.scene = scene; J.base = base; J.world = world; J.w = w; J.h = h; J.tiles_bytes = tiles_bytes;
    for (int r = 0; r < world; r++) { J.stamp_ms[r] = J.upload_ms[r] = J.enqueue_ms[r] = 0.0f; J.rcs[r] = -1; }
    {
      std::lock_guard<std::mutex> lk(J.m);
      J.pending = world - 1;
    }
    for (int r = 1; r < world; r++) {
      DevWorker &Wk = g_workers[r];
      {
        std::lock_guard<std::mutex> lk(Wk.m);
        if (!Wk.started) { std::thread(worker_loop, r).detach(); Wk.started = true; }
        Wk.job = &J;
      }
      Wk.cv.notify_one();
    }
    enqueue_device_frame(J, 0);
    // the full content check of the host scene while every device renders (see rt_scene_touch)
    bool stale = false;
    uint64_t fp_now = 0;
    if (verify && attempt == 0) {
      const double t_v = now_ms();
      fp_now = scene_fingerprint(scene);
      T.verify_ms = (float)(now_ms() - t_v);
    }
    {
      std::unique_lock<std::mutex> lk(J.m);
      J.cv.wait(lk, [&] { return J.pending == 0; });
    }
    int failed = -1;
    for (int r = 0; r < world; r++)
      if (J.rcs[r] != 0 && failed < 0) failed = r;
    // every slot against the fingerprint of ITS OWN copy: slot r >= 1 may hold a copy made before an in-place edit that
    // slot 0 has long re-uploaded (one fingerprint per Scene* let such a copy through)
    if (verify && attempt == 0)
      for (int r = 0; r < world; r++)
        if (J.rcs[r] == 0 && J.full_fp[r] != fp_now) stale = true;
    if (failed >= 0 || stale) {
      // nothing may still be writing into slot 0's tile buffer, or reading a scene copy, when we leave or start over
      for (int r = 0; r < world; r++)
        if (J.rcs[r] == 0) (void)hipEventSynchronize(g_devs[r].ws.ev_frame[4]);
      if (failed >= 0) return rt_fail("multi-device frame failed: %s", J.err[failed][0] ? J.err[failed] : "unknown error");
      {                                               // drop the copies that do not match the host scene as it is now
        auto it = D0.scene_cache.find(scene);
        if (it != D0.scene_cache.end() && it->second->full_fp != fp_now) { free_device_scene(it->second); D0.scene_cache.erase(it); }
        drop_stale_copies(scene, fp_now, 1);
      }
      continue;                                       // the host scene changed under the cached copies: upload and render again
    }
    break;
  }
  DeviceGuard guard(D0);
  hipStream_t s0 = D0.mstream;
  const double t_g = now_ms();
  for (int r = 1; r < world; r++) {
    Workspace &W = g_devs[r].ws;
    if (J.staged[r]) {                                // no peer access: pinned host memory -> slot 0
      HIP_TRY(hipEventSynchronize(W.ev_frame[4]));
      HIP_TRY(hipMemcpyAsync(D0.ws.all_tiles + (size_t)r * tiles_bytes, W.tiles_host, tiles_bytes, hipMemcpyHostToDevice, s0));
    } else {
      HIP_TRY(hipStreamWaitEvent(s0, W.ev_frame[4], 0));
    }
  }
  if (untile_on(D0, w, h, world, D0.ws.all_tiles, D0.ws.image, s0) != 0) return -1;
  if (copy_image_out(image, D0.ws.image, w, h, s0) != 0) return -1;
  HIP_TRY(hipStreamSynchronize(s0));
  // the slowest device's split, the ray counters of all
  float worst = -1.0f;
  RT_Counters sum;
  memset(&sum, 0, sizeof sum);
  for (int r = 0; r < world; r++) {
    Workspace &W = g_devs[r].ws;
    const float span = event_ms(W.ev_frame[0], W.ev_frame[4]);
    if (span > worst) {
      worst = span;
      T.slowest_device = r;
      frame_split(W, T);                              // (copy: its tiles to slot 0, + counters)
    }
    T.stamp_ms = J.stamp_ms[r] > T.stamp_ms ? J.stamp_ms[r] : T.stamp_ms;
    T.upload_ms = J.upload_ms[r] > T.upload_ms ? J.upload_ms[r] : T.upload_ms;
    T.enqueue_ms = J.enqueue_ms[r] > T.enqueue_ms ? J.enqueue_ms[r] : T.enqueue_ms;
    const unsigned long long *c = W.counters_host;
    sum.paths += c[RT_CNT_PATHS]; sum.rays += c[RT_CNT_RAYS]; sum.node_visits += c[RT_CNT_NODES]; sum.leaf_visits += c[RT_CNT_LEAVES];
    sum.shades += c[RT_CNT_SHADES]; sum.backgrounds += c[RT_CNT_BG]; sum.textured += c[RT_CNT_TEXTURED];
  }
  T.gather_ms = (float)(now_ms() - t_g);
  {
    std::lock_guard<std::mutex> lk(g_multi_mutex);
    g_multi_counters = sum;
    g_multi_counters_valid = true;
  }
  T.total_ms = (float)(now_ms() - t0);
  D0.timing = T;
  return 0;
}
