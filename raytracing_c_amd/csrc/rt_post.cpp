// rt_post.cpp -- what runs on a frame and its first-hit feature planes (include/rt_hip.h): the guided denoiser (the edge-stopping
// a-trous filter, rt_guided.hip) and temporal accumulation (the frame blended with the reprojected history of the frames before it,
// rt_temporal.hip), and what SVGF adds to the two (rt_variance.hip): the luminance moments carried through the accumulation, the variance
// estimated from them, and the filter steered by that variance.  Each on the device level (device pointers, launches on the caller's stream), on the host level (host arrays
// through library-owned staging) and behind a frame (rt_render_denoised, rt_render_temporal, rt_render_svgf: one pipeline -- frame,
// feature pass, optionally the accumulation, optionally the filter -- in ONE scene-checked call).  Nothing here computes a pixel on the CPU.

#include "rt_host.h"

static_assert(sizeof(RT_Guided_Params) == 20, "iterations, three sigmas, demodulate");
static_assert(sizeof(RT_Temporal_Params) == 20, "alpha, max_history, two tolerances, demodulate");
static_assert(sizeof(RT_Variance_Params) == 8, "two sigmas");

#define RT_GUIDED_WORK_PER_PIXEL 64        // two colour buffers (r, g, b, L) and the guides (N, coverage), (P, 0): four float4
#define RT_TEMPORAL_HISTORY_PER_PIXEL 48   // (c, len), (N, coverage), (W, 0): three float4
#define RT_TEMPORAL_MOMENTS_PER_PIXEL 16   // (m1, m2, 0, 0): one float4
#define RT_TEMPORAL_MAX_HISTORY (1 << 20)
#define RT_HOST_FRAME_F32 (3 + RT_FEATURE_CHANNELS)   // a staged host frame, f32 per pixel: the colour, then the planes as FeatureState keeps them

// ---------------------------------------------------------------------------------
// what can be checked without the device.  `who` prefixes the messages.

static int check_guided(const char *who, i32 width, i32 height, RT_Guided_Params const *g) {
  if (check_image_size(who, width, height) != 0) return -1;
  if (!g) return rt_fail("%s: guided params are NULL", who);
  if (g->iterations < 1 || g->iterations > 8) return rt_fail("%s: iterations must be 1 .. 8 (got %d)", who, g->iterations);
  // (written so that NaN fails: it is not > 0)
  if (!(g->sigma_color > 0.0f)) return rt_fail("%s: sigma_color must be > 0 (got %g)", who, (double)g->sigma_color);
  if (!(g->sigma_normal > 0.0f)) return rt_fail("%s: sigma_normal must be > 0 (got %g)", who, (double)g->sigma_normal);
  if (!(g->sigma_position > 0.0f)) return rt_fail("%s: sigma_position must be > 0 (got %g)", who, (double)g->sigma_position);
  if (g->demodulate != 0 && g->demodulate != 1) return rt_fail("%s: demodulate must be 0 or 1 (got %d)", who, g->demodulate);
  return 0;
}

static int check_temporal(const char *who, i32 width, i32 height, RT_Temporal_Params const *t) {
  if (check_image_size(who, width, height) != 0) return -1;
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

static int check_variance(const char *who, RT_Variance_Params const *v) {
  if (!v) return rt_fail("%s: variance params are NULL", who);
  // (written so that NaN fails)
  if (!(v->sigma_normal > 0.0f)) return rt_fail("%s: variance sigma_normal must be > 0 (got %g)", who, (double)v->sigma_normal);
  if (!(v->sigma_position > 0.0f)) return rt_fail("%s: variance sigma_position must be > 0 (got %g)", who, (double)v->sigma_position);
  return 0;
}

// A frame on the device: the colour and the four planes (the albedo only where `demodulate` reads it).
static int check_device_frame(const char *who, void const *d_color, void const *d_coverage, void const *d_albedo, void const *d_normal,
                              void const *d_position, int demodulate) {
  if (!d_color) return rt_fail("%s: d_color is NULL", who);
  if (!d_coverage) return rt_fail("%s: d_coverage is NULL", who);
  if (!d_albedo && demodulate) return rt_fail("%s: d_albedo is NULL and demodulate is set", who);
  if (!d_normal) return rt_fail("%s: d_normal is NULL", who);
  if (!d_position) return rt_fail("%s: d_position is NULL", who);
  return 0;
}

// ... and in host arrays.
static int check_host_frame(const char *who, f32 const *color, RT_Features const *planes, int demodulate) {
  if (!color) return rt_fail("%s: color is NULL", who);
  if (!planes) return rt_fail("%s: planes is NULL", who);
  if (!planes->coverage) return rt_fail("%s: planes->coverage is NULL", who);
  if (!planes->albedo && demodulate) return rt_fail("%s: planes->albedo is NULL and demodulate is set", who);
  if (!planes->normal) return rt_fail("%s: planes->normal is NULL", who);
  if (!planes->position) return rt_fail("%s: planes->position is NULL", who);
  return 0;
}

// The calls that answer with a size or an object have ONE message for a size check_image_size() refuses.
static bool size_refused(const char *who, i32 width, i32 height) {
  if (width > 0 && height > 0 && (int64_t)width * height <= RT_MAX_PIXELS) return false;
  rt_fail("%s: image size %dx%d is invalid", who, width, height);
  return true;
}

extern "C" i64 rt_guided_work_bytes(i32 width, i32 height) {
  return size_refused("rt_guided_work_bytes", width, height) ? -1 : (i64)width * height * RT_GUIDED_WORK_PER_PIXEL;
}

extern "C" i64 rt_temporal_history_bytes(i32 width, i32 height) {
  return size_refused("rt_temporal_history_bytes", width, height) ? -1 : (i64)width * height * RT_TEMPORAL_HISTORY_PER_PIXEL;
}

extern "C" i64 rt_guided_variance_work_bytes(i32 width, i32 height) {
  return size_refused("rt_guided_variance_work_bytes", width, height) ? -1 : (i64)width * height * RT_GUIDED_WORK_PER_PIXEL;
}

extern "C" i64 rt_temporal_moments_bytes(i32 width, i32 height) {
  return size_refused("rt_temporal_moments_bytes", width, height) ? -1 : (i64)width * height * RT_TEMPORAL_MOMENTS_PER_PIXEL;
}

// ---------------------------------------------------------------------------------
// the stages

// Enqueues the pack launch and g->iterations filter launches on `stream`.  Every pointer is on the current device; every input
// is in d_work before d_out / d_image are written (the last launch reads a pixel's colour and albedo only to write that pixel).
// d_variance given: THE VARIANCE-GUIDED FILTER -- the colour records carry the variance, k_c is not scaled per iteration, and
// d_variance_out (optional) receives the last v.
static int enqueue_guided(i32 width, i32 height, RT_Guided_Params const *g, void const *d_color, void const *d_coverage,
                          void const *d_albedo, void const *d_normal, void const *d_position, void *d_out, void *d_image, void *d_work,
                          hipStream_t stream, void const *d_variance = nullptr, void *d_variance_out = nullptr) {
  const size_t pixels = (size_t)width * height;
  uint8_t *w = (uint8_t *)d_work;
  void *buf[2] = {w, w + pixels * 16}, *g0 = w + pixels * 32, *g1 = w + pixels * 48;
  int rc = d_variance ? rt_launch_variance_pack((int)pixels, g->demodulate, (const float *)d_color, (const float *)d_coverage,
                                                (const float *)d_albedo, (const float *)d_normal, (const float *)d_position,
                                                (const float *)d_variance, buf[0], g0, g1, stream)
                      : rt_launch_guided_pack((int)pixels, g->demodulate, (const float *)d_color, (const float *)d_coverage,
                                              (const float *)d_albedo, (const float *)d_normal, (const float *)d_position, buf[0], g0, g1,
                                              stream);
  if (rc != 0) return rt_fail("guided pack kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  const float k_c = 1.0f / (g->sigma_color * g->sigma_color), k_n = 1.0f / (g->sigma_normal * g->sigma_normal),
              k_p = 1.0f / (g->sigma_position * g->sigma_position);
  for (int i = 0; i < g->iterations; i++) {
    const int last = i == g->iterations - 1;
    if (d_variance) {
      rc = rt_launch_variance_filter(width, height, 1 << i, k_n, k_p, k_c, last, g->demodulate, buf[i & 1], buf[(i & 1) ^ 1], g0, g1,
                                     (const float *)d_color, (const float *)d_albedo, last ? (float *)d_out : nullptr,
                                     last ? (uint8_t *)d_image : nullptr, last ? (float *)d_variance_out : nullptr, stream);
      if (rc != 0) return rt_fail("variance-guided filter kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
      continue;
    }
    const float kc_i = k_c * (float)(1u << (2 * i));            // the colour sigma halves every iteration
    rc = rt_launch_guided_filter(width, height, 1 << i, k_n, k_p, kc_i, last, g->demodulate, buf[i & 1], buf[(i & 1) ^ 1], g0, g1,
                                 (const float *)d_color, (const float *)d_albedo, last ? (float *)d_out : nullptr,
                                 last ? (uint8_t *)d_image : nullptr, stream);
    if (rc != 0) return rt_fail("guided filter kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  return 0;
}

static void temporal_camera(RT_TCamera *c, Camera const *cam) {
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 3; k++) c->r[i][k] = cam->view_matrix.rows[i][k];
    c->t[i] = cam->view_matrix.rows[i][3];
  }
  c->focal_length = cam->focal_length;
}

// Enqueues the launch on `stream`.  Every pointer is on the current device; prev is read only when d_history_in is given.
// d_moments_out given: THE MOMENTS in the same launch (d_moments_in exactly when d_history_in), and when d_variance is wanted THE
// VARIANCE behind it, which reads d_history_out and d_moments_out.
static int enqueue_temporal(i32 width, i32 height, RT_Temporal_Params const *t, Camera const *cam, Camera const *prev,
                            void const *d_color, void const *d_coverage, void const *d_albedo, void const *d_normal,
                            void const *d_position, void const *d_history_in, void *d_history_out, void *d_out, void *d_length,
                            void *d_image, hipStream_t stream, RT_Variance_Params const *vp = nullptr,
                            void const *d_moments_in = nullptr, void *d_moments_out = nullptr, void *d_variance = nullptr) {
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
  if (!d_moments_out) {
    int rc = rt_launch_temporal(&P, (const float *)d_color, (const float *)d_coverage, (const float *)d_albedo, (const float *)d_normal,
                                (const float *)d_position, d_history_in, d_history_out, (float *)d_out, (float *)d_length,
                                (uint8_t *)d_image, stream);
    if (rc != 0) return rt_fail("temporal kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
  }
  int rc = rt_launch_temporal_moments(&P, (const float *)d_color, (const float *)d_coverage, (const float *)d_albedo,
                                      (const float *)d_normal, (const float *)d_position, d_history_in, d_history_out, (float *)d_out,
                                      (float *)d_length, (uint8_t *)d_image, d_moments_in, d_moments_out, stream);
  if (rc != 0) return rt_fail("temporal moments kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  if (!d_variance) return 0;
  const float k_n = 1.0f / (vp->sigma_normal * vp->sigma_normal), k_p = 1.0f / (vp->sigma_position * vp->sigma_position);
  rc = rt_launch_variance(width, height, k_n, k_p, d_history_out, d_moments_out, (float *)d_variance, stream);
  if (rc != 0) return rt_fail("variance kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- device level -------------------------------------------------------------------------------------------------------------
// (everything that can be checked without the device is checked before it is touched)

// rt_guided_denoise and rt_guided_denoise_variance (with_variance: d_variance is required, d_variance_out optional)
static int guided_device(const char *who, bool with_variance, i32 width, i32 height, RT_Guided_Params const *params, void const *d_color,
                         void const *d_coverage, void const *d_albedo, void const *d_normal, void const *d_position, void *d_out,
                         void *d_image, void *d_work, void *stream, void const *d_variance, void *d_variance_out) {
  if (check_guided(who, width, height, params) != 0) return -1;
  if (check_device_frame(who, d_color, d_coverage, d_albedo, d_normal, d_position, params->demodulate) != 0) return -1;
  if (with_variance) {
    if (!d_variance) return rt_fail("%s: d_variance is NULL", who);
    if (!d_out && !d_image && !d_variance_out)
      return rt_fail("%s: no output is wanted (d_out, d_image and d_variance_out are NULL)", who);
  } else if (!d_out && !d_image) return rt_fail("%s: no output is wanted (d_out and d_image are NULL)", who);
  if (!d_work) return rt_fail("%s: d_work is NULL", who);
  if ((uintptr_t)d_work & 15) return rt_fail("%s: d_work must be 16-byte aligned", who);
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_guided(width, height, params, d_color, d_coverage, d_albedo, d_normal, d_position, d_out, d_image, d_work,
                        (hipStream_t)stream, d_variance, d_variance_out);
}

extern "C" int rt_guided_denoise(i32 width, i32 height, RT_Guided_Params const *params, void const *d_color, void const *d_coverage,
                                 void const *d_albedo, void const *d_normal, void const *d_position, void *d_out, void *d_image,
                                 void *d_work, void *stream) {
  return guided_device("rt_guided_denoise", false, width, height, params, d_color, d_coverage, d_albedo, d_normal, d_position, d_out,
                       d_image, d_work, stream, nullptr, nullptr);
}

extern "C" int rt_guided_denoise_variance(i32 width, i32 height, RT_Guided_Params const *params, void const *d_color,
                                          void const *d_coverage, void const *d_albedo, void const *d_normal, void const *d_position,
                                          void *d_out, void *d_image, void *d_work, void *stream, void const *d_variance,
                                          void *d_variance_out) {
  return guided_device("rt_guided_denoise_variance", true, width, height, params, d_color, d_coverage, d_albedo, d_normal, d_position,
                       d_out, d_image, d_work, stream, d_variance, d_variance_out);
}

// rt_temporal_accumulate and rt_temporal_accumulate_moments (with_moments: d_moments_out is required, d_moments_in goes with
// d_history_in, vp is required when d_variance is wanted)
static int temporal_device(const char *who, bool with_moments, i32 width, i32 height, RT_Temporal_Params const *params,
                           Camera const *camera, Camera const *previous_camera, void const *d_color, void const *d_coverage,
                           void const *d_albedo, void const *d_normal, void const *d_position, void const *d_history_in,
                           void *d_history_out, void *d_out, void *d_length, void *d_image, RT_Variance_Params const *vp,
                           void const *d_moments_in, void *d_moments_out, void *d_variance, void *stream) {
  if (check_temporal(who, width, height, params) != 0) return -1;
  if (with_moments && (vp || d_variance) && check_variance(who, vp) != 0) return -1;
  if (!camera) return rt_fail("%s: camera is NULL", who);
  if (d_history_in && !previous_camera) return rt_fail("%s: previous_camera is NULL and a history is given", who);
  if (check_device_frame(who, d_color, d_coverage, d_albedo, d_normal, d_position, params->demodulate) != 0) return -1;
  if (!d_history_out) return rt_fail("%s: d_history_out is NULL", who);
  if (((uintptr_t)d_history_out | (uintptr_t)d_history_in) & 15) return rt_fail("%s: the histories must be 16-byte aligned", who);
  if (d_history_in) {
    const uintptr_t a = (uintptr_t)d_history_in, b = (uintptr_t)d_history_out;
    const uintptr_t bytes = (uintptr_t)width * height * RT_TEMPORAL_HISTORY_PER_PIXEL;
    if ((a <= b ? b - a : a - b) < bytes) return rt_fail("%s: d_history_in and d_history_out overlap (the reads are gathers)", who);
  }
  if (with_moments) {
    if (!d_moments_out) return rt_fail("%s: d_moments_out is NULL", who);
    if (d_history_in && !d_moments_in) return rt_fail("%s: a history is given without its moments (d_moments_in is NULL)", who);
    if (!d_history_in && d_moments_in) return rt_fail("%s: moments are given without their history (d_history_in is NULL)", who);
    if (((uintptr_t)d_moments_out | (uintptr_t)d_moments_in) & 15) return rt_fail("%s: the moments must be 16-byte aligned", who);
    if (d_moments_in) {
      const uintptr_t a = (uintptr_t)d_moments_in, b = (uintptr_t)d_moments_out;
      const uintptr_t bytes = (uintptr_t)width * height * RT_TEMPORAL_MOMENTS_PER_PIXEL;
      if ((a <= b ? b - a : a - b) < bytes) return rt_fail("%s: d_moments_in and d_moments_out overlap (the reads are gathers)", who);
    }
  }
  Device &D = dev0();
  {
    std::lock_guard<std::mutex> lock(D.mutex);
    if (ensure_device(D) != 0) return -1;
  }
  return enqueue_temporal(width, height, params, camera, previous_camera, d_color, d_coverage, d_albedo, d_normal, d_position,
                          d_history_in, d_history_out, d_out, d_length, d_image, (hipStream_t)stream, vp, d_moments_in, d_moments_out,
                          d_variance);
}

extern "C" int rt_temporal_accumulate(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                      Camera const *previous_camera, void const *d_color, void const *d_coverage, void const *d_albedo,
                                      void const *d_normal, void const *d_position, void const *d_history_in, void *d_history_out,
                                      void *d_out, void *d_length, void *d_image, void *stream) {
  return temporal_device("rt_temporal_accumulate", false, width, height, params, camera, previous_camera, d_color, d_coverage, d_albedo,
                         d_normal, d_position, d_history_in, d_history_out, d_out, d_length, d_image, nullptr, nullptr, nullptr, nullptr,
                         stream);
}

extern "C" int rt_temporal_accumulate_moments(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                              Camera const *previous_camera, void const *d_color, void const *d_coverage,
                                              void const *d_albedo, void const *d_normal, void const *d_position,
                                              void const *d_history_in, void *d_history_out, void *d_out, void *d_length, void *d_image,
                                              RT_Variance_Params const *vp, void const *d_moments_in, void *d_moments_out,
                                              void *d_variance, void *stream) {
  return temporal_device("rt_temporal_accumulate_moments", true, width, height, params, camera, previous_camera, d_color, d_coverage,
                         d_albedo, d_normal, d_position, d_history_in, d_history_out, d_out, d_length, d_image, vp, d_moments_in,
                         d_moments_out, d_variance, stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
// The host-level calls run on the NULL stream: it does not wait for the lane streams of frames in flight.

// Copies a host frame into `in` (RT_HOST_FRAME_F32 f32 per pixel): the colour at `in` itself, behind it the planes, *d; d->albedo
// is NULL when the host gave none.
static int upload_host_frame(float *in, size_t pixels, f32 const *color, RT_Features const *planes, FeaturePlanes *d) {
  const size_t f3 = pixels * 3 * sizeof(float), f1 = pixels * sizeof(float);
  *d = split_feature_planes(in + pixels * 3, pixels);
  HIP_TRY(hipMemcpy(in, color, f3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d->coverage, planes->coverage, f1, hipMemcpyHostToDevice));
  if (planes->albedo) HIP_TRY(hipMemcpy(d->albedo, planes->albedo, f3, hipMemcpyHostToDevice));
  else d->albedo = nullptr;
  HIP_TRY(hipMemcpy(d->normal, planes->normal, f3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d->position, planes->position, f3, hipMemcpyHostToDevice));
  return 0;
}

// rt_guided_denoise_host and rt_guided_denoise_variance_host (with_variance: variance is required, variance_out optional)
static int guided_host(const char *who, bool with_variance, i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                       RT_Features const *planes, f32 *out, u8 *image, f32 const *variance, f32 *variance_out) {
  if (check_guided(who, width, height, params) != 0) return -1;
  if (check_host_frame(who, color, planes, params->demodulate) != 0) return -1;
  if (with_variance) {
    if (!variance) return rt_fail("%s: variance is NULL", who);
    if (!out && !image && !variance_out) return rt_fail("%s: no output is wanted (out, image and variance_out are NULL)", who);
  } else if (!out && !image) return rt_fail("%s: no output is wanted (out and image are NULL)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  GuidedState &S = D.guided;
  const size_t pixels = (size_t)width * height;
  HIP_TRY(S.in.grow(pixels * RT_HOST_FRAME_F32));
  HIP_TRY(S.work.grow(pixels * RT_GUIDED_WORK_PER_PIXEL));
  if (out) HIP_TRY(S.out.grow(pixels * 3));
  if (image) HIP_TRY(S.image.grow(pixels * 3));
  if (variance) HIP_TRY(S.variance.grow(pixels));
  if (variance_out) HIP_TRY(S.variance_out.grow(pixels));
  hipStream_t stream = nullptr;
  FeaturePlanes d;
  if (upload_host_frame(S.in, pixels, color, planes, &d) != 0) return -1;
  if (variance) HIP_TRY(hipMemcpy(S.variance, variance, pixels * sizeof(float), hipMemcpyHostToDevice));
  if (enqueue_guided(width, height, params, S.in, d.coverage, d.albedo, d.normal, d.position, out ? S.out.get() : nullptr,
                     image ? S.image.get() : nullptr, S.work, stream, variance ? S.variance.get() : nullptr,
                     variance_out ? S.variance_out.get() : nullptr) != 0)
    return -1;
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  if (out) HIP_TRY(hipMemcpy(out, S.out, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (image) HIP_TRY(hipMemcpy(image, S.image, pixels * 3, hipMemcpyDeviceToHost));
  if (variance_out) HIP_TRY(hipMemcpy(variance_out, S.variance_out, pixels * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rt_guided_denoise_host(i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                                      RT_Features const *planes, f32 *out, u8 *image) {
  return guided_host("rt_guided_denoise_host", false, width, height, params, color, planes, out, image, nullptr, nullptr);
}

extern "C" int rt_guided_denoise_variance_host(i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                                               RT_Features const *planes, f32 *out, u8 *image, f32 const *variance, f32 *variance_out) {
  return guided_host("rt_guided_denoise_variance_host", true, width, height, params, color, planes, out, image, variance, variance_out);
}

static const char *missing_history_plane(RT_History_Planes const *h) {
  return !h->color ? "color" : !h->length ? "length" : !h->coverage ? "coverage" : !h->normal ? "normal" : !h->position ? "position" : nullptr;
}

// rt_temporal_accumulate_host and rt_temporal_accumulate_moments_host (with_moments: moments_in goes with history_in, moments_out
// and variance are optional outputs, vp is required when variance is wanted)
static int temporal_host(const char *who, bool with_moments, i32 width, i32 height, RT_Temporal_Params const *params,
                         Camera const *camera, Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                         RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out, f32 *length, u8 *image,
                         RT_Variance_Params const *vp, f32 const *moments_in, f32 *moments_out, f32 *variance) {
  if (check_temporal(who, width, height, params) != 0) return -1;
  if (with_moments && (vp || variance) && check_variance(who, vp) != 0) return -1;
  if (!camera) return rt_fail("%s: camera is NULL", who);
  if (history_in && !previous_camera) return rt_fail("%s: previous_camera is NULL and a history is given", who);
  if (check_host_frame(who, color, planes, params->demodulate) != 0) return -1;
  if (history_in && missing_history_plane(history_in)) return rt_fail("%s: history_in->%s is NULL", who, missing_history_plane(history_in));
  if (history_out && missing_history_plane(history_out)) return rt_fail("%s: history_out->%s is NULL", who, missing_history_plane(history_out));
  if (with_moments) {
    if (history_in && !moments_in) return rt_fail("%s: a history is given without its moments (moments_in is NULL)", who);
    if (!history_in && moments_in) return rt_fail("%s: moments are given without their history (history_in is NULL)", who);
    if (!history_out && !out && !length && !image && !moments_out && !variance)
      return rt_fail("%s: no output is wanted (history_out, out, length, image, moments_out and variance are NULL)", who);
  } else if (!history_out && !out && !length && !image)
    return rt_fail("%s: no output is wanted (history_out, out, length and image are NULL)", who);

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  TemporalState &S = D.temporal;
  const size_t pixels = (size_t)width * height, f3 = pixels * 3 * sizeof(float), f1 = pixels * sizeof(float);
  HIP_TRY(S.in.grow(pixels * RT_HOST_FRAME_F32));
  HIP_TRY(S.planar.grow(pixels * 11));
  HIP_TRY(S.hist[0].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  HIP_TRY(S.hist[1].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  if (out) HIP_TRY(S.out.grow(pixels * 3));
  if (length) HIP_TRY(S.length.grow(pixels));
  if (image) HIP_TRY(S.image.grow(pixels * 3));
  if (with_moments) {
    HIP_TRY(S.mom[0].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
    HIP_TRY(S.mom[1].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
    HIP_TRY(S.mom_planar.grow(pixels * 2));
    if (variance) HIP_TRY(S.variance.grow(pixels));
  }
  float *h_col = S.planar, *h_len = S.planar + pixels * 3, *h_cov = S.planar + pixels * 4, *h_nrm = S.planar + pixels * 5,
        *h_pos = S.planar + pixels * 8;
  hipStream_t stream = nullptr;
  FeaturePlanes d;
  if (upload_host_frame(S.in, pixels, color, planes, &d) != 0) return -1;
  if (history_in) {
    HIP_TRY(hipMemcpy(h_col, history_in->color, f3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_len, history_in->length, f1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_cov, history_in->coverage, f1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_nrm, history_in->normal, f3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h_pos, history_in->position, f3, hipMemcpyHostToDevice));
    int rc = rt_launch_temporal_pack((int)pixels, h_col, h_len, h_cov, h_nrm, h_pos, S.hist[0], stream);
    if (rc != 0) return rt_fail("temporal pack kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (with_moments) {
      HIP_TRY(hipMemcpy(S.mom_planar, moments_in, 2 * f1, hipMemcpyHostToDevice));
      rc = rt_launch_moments_pack((int)pixels, S.mom_planar, S.mom[0], stream);
      if (rc != 0) return rt_fail("moments pack kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
  }
  if (enqueue_temporal(width, height, params, camera, previous_camera, S.in, d.coverage, d.albedo, d.normal, d.position,
                       history_in ? S.hist[0].get() : nullptr, S.hist[1], out ? S.out.get() : nullptr,
                       length ? S.length.get() : nullptr, image ? S.image.get() : nullptr, stream, vp,
                       with_moments && history_in ? S.mom[0].get() : nullptr, with_moments ? S.mom[1].get() : nullptr,
                       variance ? S.variance.get() : nullptr) != 0)
    return -1;
  if (moments_out) {
    int rc = rt_launch_moments_unpack((int)pixels, S.mom[1], S.mom_planar, stream);
    if (rc != 0) return rt_fail("moments unpack kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
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
  if (moments_out) HIP_TRY(hipMemcpy(moments_out, S.mom_planar, 2 * f1, hipMemcpyDeviceToHost));
  if (variance) HIP_TRY(hipMemcpy(variance, S.variance, f1, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rt_temporal_accumulate_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                           Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                           RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                           f32 *length, u8 *image) {
  return temporal_host("rt_temporal_accumulate_host", false, width, height, params, camera, previous_camera, color, planes, history_in,
                       history_out, out, length, image, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int rt_temporal_accumulate_moments_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                                   Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                                   RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                                   f32 *length, u8 *image, RT_Variance_Params const *vp, f32 const *moments_in,
                                                   f32 *moments_out, f32 *variance) {
  return temporal_host("rt_temporal_accumulate_moments_host", true, width, height, params, camera, previous_camera, color, planes,
                       history_in, history_out, out, length, image, vp, moments_in, moments_out, variance);
}

// ---- the history a host keeps ---------------------------------------------------------------------------------------------------
// Gives back the staging of the temporal calls and the memory of every RT_History, which start again from nothing (the objects
// stay their hosts', and the list of them stays).  What release_staging() does for this state: D.mutex held, D's GPU current,
// device idle.
void release_temporal_state(Device &D) {
  std::vector<RT_History *> keep = std::move(D.temporal.histories);
  for (RT_History *h : keep) {
    h->buf[0].reset();
    h->buf[1].reset();
    h->mom[0].reset();
    h->mom[1].reset();
    h->valid = false;
    h->moments_valid = false;
  }
  D.temporal = TemporalState();
  D.temporal.histories = std::move(keep);
}

extern "C" RT_History *rt_history_create(i32 width, i32 height) {
  if (size_refused("rt_history_create", width, height)) return nullptr;
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
  history->moments_valid = false;
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
    history->mom[0].reset();
    history->mom[1].reset();
  }
  delete history;
}

// ---- behind a frame -----------------------------------------------------------------------------------------------------------

// What both entry points check of `image` before its size goes into 32 bits, and after their stages' parameters.
static int check_frame_image(const char *who, Image const *image) {
  if (image->width <= 0 || image->height <= 0 || image->width > 0x7fffffff || image->height > 0x7fffffff)
    return rt_fail("%s: image size %ldx%ld is invalid", who, (long)image->width, (long)image->height);
  return 0;
}

static int check_frame_rest(const char *who, Image const *image, isize samples, isize max_bounces) {
  if (check_image_layout(image, who) != 0) return -1;
  if (samples <= 0 || samples > 0x7fffffff) return rt_fail("%s: samples must be positive and fit 32 bits (got %ld)", who, (long)samples);
  if (max_bounces < 0 || max_bounces > 0x7fffffff) return rt_fail("%s: max_bounces must be >= 0 and fit 32 bits (got %ld)", who, (long)max_bounces);
  return 0;
}

// The frame, the four planes of its feature pass, then the stages that are given -- the accumulation against `history` (t), the
// filter (g) -- in one scene-checked call.  W.linear is the noisy frame, D.temporal.out / length serve the accumulation,
// D.guided.work / out the filter, and W.image receives the encoding of the LAST stage.  The arguments are checked by the callers;
// `what` is their word for the frame in the one-device refusal.  vp (with history and g): rt_render_svgf -- the accumulation carries
// the history's moments, the variance launch follows it into D.temporal.variance, and the filter is the variance-guided one.
static int render_post(const char *who, const char *what, Scene const *scene, Image const *image, isize samples, isize max_bounces,
                       RT_History *history, RT_Temporal_Params const *t, RT_Guided_Params const *g, f32 *linear_noisy, f32 *linear_out,
                       f32 *length, RT_Variance_Params const *vp = nullptr, f32 *variance = nullptr) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (history && (image->width != history->width || image->height != history->height))
    return rt_fail("%s: the image is %ldx%ld and the history %dx%d", who, (long)image->width, (long)image->height, history->width,
                   history->height);
  if (vp && history->valid && history->buf[0] && history->buf[1] && !(history->moments_valid && history->mom[0] && history->mom[1]))
    return rt_fail("%s: the history's last frame was written by rt_render_temporal and has no moments: call rt_history_reset first", who);
  const double t_start = now_ms();
  if (ensure_device(D) != 0) return -1;
  if (rt_device_count() > 1)
    return rt_fail("%s: %s renders on one device, and %d are set (rt_set_devices)", who, what, rt_device_count());
  RT_Render_Params p;
  if (fill_frame_params(&p, image, samples, max_bounces, g_seed.load()) != 0) return -1;
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
  const bool want_accumulated = history && (g || linear_out);   // the accumulation's f32 output: the filter's input, or the caller's
  const uint8_t *h_in = nullptr;
  uint8_t *h_out = nullptr, *m_out = nullptr;
  const uint8_t *m_in = nullptr;
  if (history) {
    if (!history->buf[0] || !history->buf[1]) history->valid = false;          // (given back with the staging: from nothing)
    HIP_TRY(history->buf[0].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
    HIP_TRY(history->buf[1].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
    if (want_accumulated) HIP_TRY(S.out.grow(pixels * 3));
    if (length) HIP_TRY(S.length.grow(pixels));
    h_in = history->valid ? history->buf[history->cur].get() : nullptr;
    h_out = history->buf[history->cur ^ 1];
    if (vp) {
      HIP_TRY(history->mom[0].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
      HIP_TRY(history->mom[1].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
      HIP_TRY(S.variance.grow(pixels));
      m_in = h_in ? history->mom[history->cur].get() : nullptr;
      m_out = history->mom[history->cur ^ 1];
    }
  }
  if (g) {
    HIP_TRY(G.work.grow(pixels * RT_GUIDED_WORK_PER_PIXEL));
    if (linear_out) HIP_TRY(G.out.grow(pixels * 3));
  }
  const FeaturePlanes f = split_feature_planes(F.planes, pixels);
  hipStream_t stream = nullptr;
  // (a pass that is run again after a scene edit reads the same old history and writes the same new one)
  auto pass = [&](RT_Device_Scene *d) -> int {
    if (enqueue_frame(D, d, &scene->camera, &p, W, stream, 0, nullptr, nullptr, W.linear) != 0) return -1;
    HIP_TRY(hipMemsetAsync(F.sums, 0, pixels * RT_FEATURE_CHANNELS * sizeof(unsigned long long), stream));
    if (enqueue_features(D, d, &scene->camera, &p, F.sums, stream) != 0) return -1;
    if (enqueue_resolve(&p, F.sums, f.coverage, f.albedo, f.normal, f.position, stream) != 0) return -1;
    if (history && enqueue_temporal(p.width, p.height, t, &scene->camera, &history->camera, W.linear, f.coverage, f.albedo, f.normal,
                                    f.position, h_in, h_out, want_accumulated ? S.out.get() : nullptr,
                                    length ? S.length.get() : nullptr, g ? nullptr : W.image.get(), stream, vp, m_in, m_out,
                                    vp ? S.variance.get() : nullptr) != 0)
      return -1;
    if (!g) return 0;
    return enqueue_guided(p.width, p.height, g, history ? S.out.get() : W.linear.get(), f.coverage, f.albedo, f.normal, f.position,
                          linear_out ? G.out.get() : nullptr, W.image, G.work, stream, vp ? S.variance.get() : nullptr);
  };
  if (!scene_checked(D, scene, stream, &T, pass)) {                // (a scene edited since the copy: uploaded and rendered again)
    if (history) history->valid = history->moments_valid = false;   // (the new history may be half written, the old one is not current)
    return -1;
  }
  if (history) {
    history->cur ^= 1;
    history->valid = true;
    history->moments_valid = vp != nullptr;                       // (rt_render_temporal leaves the moments behind)
    history->camera = scene->camera;
  }

  if (copy_image_out(image, W.image, p.width, p.height, stream) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[4], stream));
  if (linear_noisy) HIP_TRY(hipMemcpy(linear_noisy, W.linear, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (linear_out) HIP_TRY(hipMemcpy(linear_out, g ? G.out.get() : S.out.get(), pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (length) HIP_TRY(hipMemcpy(length, S.length, pixels * sizeof(float), hipMemcpyDeviceToHost));
  if (variance) HIP_TRY(hipMemcpy(variance, S.variance, pixels * sizeof(float), hipMemcpyDeviceToHost));
  return finish_frame(D, W, stream, T, t_start);
}

extern "C" int rt_render_denoised(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                                  RT_Guided_Params const *params, f32 *linear_noisy, f32 *linear_denoised) {
  const char *who = "rt_render_denoised";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!image) return rt_fail("%s: image is NULL", who);
  if (check_frame_image(who, image) != 0) return -1;
  if (check_guided(who, (i32)image->width, (i32)image->height, params) != 0) return -1;
  if (check_frame_rest(who, image, samples, max_bounces) != 0) return -1;
  if (!image->pixels.data && !linear_denoised) return rt_fail("%s: no output is wanted (no pixels and no linear_denoised)", who);
  return render_post(who, "a denoised frame", scene, image, samples, max_bounces, nullptr, nullptr, params, linear_noisy,
                     linear_denoised, nullptr);
}

extern "C" int rt_render_temporal(Scene const *scene, Image const *image, isize samples, isize max_bounces, RT_History *history,
                                  RT_Temporal_Params const *temporal_params, RT_Guided_Params const *guided_params, f32 *linear_noisy,
                                  f32 *linear_out, f32 *length) {
  const char *who = "rt_render_temporal";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!image) return rt_fail("%s: image is NULL", who);
  if (!history) return rt_fail("%s: history is NULL", who);
  if (check_frame_image(who, image) != 0) return -1;
  if (check_temporal(who, (i32)image->width, (i32)image->height, temporal_params) != 0) return -1;
  if (guided_params && check_guided(who, (i32)image->width, (i32)image->height, guided_params) != 0) return -1;
  if (check_frame_rest(who, image, samples, max_bounces) != 0) return -1;
  if (!image->pixels.data && !linear_out && !length) return rt_fail("%s: no output is wanted (no pixels, no linear_out, no length)", who);
  return render_post(who, "an accumulated frame", scene, image, samples, max_bounces, history, temporal_params, guided_params,
                     linear_noisy, linear_out, length);
}

extern "C" int rt_render_svgf(Scene const *scene, Image const *image, isize samples, isize max_bounces, RT_History *history,
                              RT_Temporal_Params const *temporal_params, RT_Variance_Params const *variance_params,
                              RT_Guided_Params const *guided_params, f32 *linear_noisy, f32 *linear_out, f32 *length, f32 *variance) {
  const char *who = "rt_render_svgf";
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!image) return rt_fail("%s: image is NULL", who);
  if (!history) return rt_fail("%s: history is NULL", who);
  if (check_frame_image(who, image) != 0) return -1;
  if (check_temporal(who, (i32)image->width, (i32)image->height, temporal_params) != 0) return -1;
  if (check_variance(who, variance_params) != 0) return -1;
  if (check_guided(who, (i32)image->width, (i32)image->height, guided_params) != 0) return -1;
  if (check_frame_rest(who, image, samples, max_bounces) != 0) return -1;
  if (!image->pixels.data && !linear_out && !length && !variance)
    return rt_fail("%s: no output is wanted (no pixels, no linear_out, no length, no variance)", who);
  return render_post(who, "a variance-guided frame", scene, image, samples, max_bounces, history, temporal_params, guided_params,
                     linear_noisy, linear_out, length, variance_params, variance);
}
