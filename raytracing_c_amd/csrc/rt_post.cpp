// rt_post.cpp -- what runs on a frame and its first-hit feature planes (include/rt_hip.h): the guided denoiser (the edge-stopping
// a-trous filter, rt_guided.hip) and temporal accumulation (the frame blended with the reprojected history of the frames before it,
// rt_temporal.hip), and what SVGF adds to the two (rt_variance.hip): the luminance moments carried through the accumulation, the variance
// estimated from them, and the filter steered by that variance; and feature-guided upsampling of a frame rendered at half the size
// (rt_upsample.hip).  Each on the device level (device pointers, launches on the caller's stream), on the host level (host arrays
// through library-owned staging) and behind a frame (rt_render_denoised, rt_render_temporal, rt_render_svgf, rt_render_upsampled:
// one pipeline, render_post -- frame, feature pass, optionally the accumulation or the upsampling, optionally the filter -- in ONE
// scene-checked call).  Nothing here computes a pixel on the CPU.
// For a mesh that scene_refit_gpu deforms between the frames the accumulation takes one more plane, the motion of the first hits
// (rt_temporal_accumulate_motion; behind a frame rt_history_set_motion switches the motion feature pass and that accumulation on).
//
// The frame a stage reads is ONE value (RT_Frame, rt_device.h), built by whoever has the pointers: the extern "C" entry points
// (frame_of), upload_host_frame and render_post from the staging; the upsampling reads two, the low frame and the planes at full
// size.  That a frame's planes are there is ONE check (check_frame), whatever the entry point calls its pointers; that two arrays
// lie apart is ONE predicate (overlap).  What a stage may write, and what its variance / moments form adds, is one struct per
// stage (FilterIO, AccumulateIO; absent = NULL).  Every stage is launched in ONE place (launch_pack, launch_filter,
// launch_accumulate, enqueue_upsample), which chooses the plain kernel or its variance / moments form by whether the optional
// pointer is given.

#include "rt_host.h"

static_assert(sizeof(RT_Guided_Params) == 20, "iterations, three sigmas, demodulate");
static_assert(sizeof(RT_Temporal_Params) == 20, "alpha, max_history, two tolerances, demodulate");
static_assert(sizeof(RT_Variance_Params) == 8, "two sigmas");
static_assert(sizeof(RT_Upsample_Params) == 16, "two sigmas, demodulate, guide_samples");

#define RT_GUIDED_WORK_PER_PIXEL 64        // two colour buffers (r, g, b, L) and the guides (N, coverage), (P, 0): four float4
#define RT_TEMPORAL_HISTORY_PER_PIXEL 48   // (c, len), (N, coverage), (W, 0): three float4
#define RT_TEMPORAL_MOMENTS_PER_PIXEL 16   // (m1, m2, 0, 0): one float4
#define RT_UPSAMPLE_WORK_PER_LOW_PIXEL 48   // the packed low frame: (c, L), (N, coverage), (P, 0), three float4
#define RT_TEMPORAL_MAX_HISTORY (1 << 20)
#define RT_HOST_FRAME_F32 (3 + RT_FEATURE_CHANNELS)   // a staged host frame, f32 per pixel: the colour, then the planes as FeatureState keeps them

// What the filter may write, and what its variance-guided form adds (device pointers; the host's in the host-level calls).
// variance_in given: THE VARIANCE-GUIDED FILTER -- the colour records carry the variance, k_c is not scaled per iteration, and
// variance_out (optional) receives the last v.
struct FilterIO { float *out; uint8_t *image; const float *variance_in; float *variance_out; };   // [h][w][3], [h][w][3], [h][w], [h][w]

// What the accumulation may write besides the new history, and what its moments form adds.  moments_out given: THE MOMENTS in the
// same launch (moments_in exactly when there is a history to read; records on the device, f32[h][w][2] in the host-level calls), and
// when `variance` is wanted THE VARIANCE behind it, with vp.  motion given: THE ACCUMULATION WITH MOTION, plain or with the moments
// (f32[h][w][3] as rt_resolve_motion writes it).
struct AccumulateIO {
  float *out, *length; uint8_t *image;                                             // [h][w][3], [h][w], [h][w][3]
  const void *moments_in; void *moments_out; float *variance; RT_Variance_Params const *vp;
  const float *motion;
};

// A history as a host has it (RT_History_Planes) and as TemporalState::planar stages it: the planes in the order
// rt_temporal_pack_history / rt_temporal_unpack_history take them -- name, f32 per pixel, where it begins in `planar` (in pixels).
struct HistoryPlane { const char *name; int floats, offset; f32 *RT_History_Planes::*member; };
static constexpr HistoryPlane HISTORY_PLANES[5] = {
    {"color", 3, 0, &RT_History_Planes::color},       {"length", 1, 3, &RT_History_Planes::length},
    {"coverage", 1, 4, &RT_History_Planes::coverage}, {"normal", 3, 5, &RT_History_Planes::normal},
    {"position", 3, 8, &RT_History_Planes::position}};
#define RT_HISTORY_PLANAR_F32 (HISTORY_PLANES[4].offset + HISTORY_PLANES[4].floats)   // 11: TemporalState::planar, f32 per pixel

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

// What can be checked of an upsampled frame: the full size -- even, >= 2, at most RT_MAX_PIXELS -- and the parameters but
// guide_samples.
static int check_upsample_size(const char *who, i64 width, i64 height) {
  if (width < 2 || height < 2 || width > 0x7fffffff || height > 0x7fffffff)
    return rt_fail("%s: image size %ldx%ld is invalid (an upsampled frame is at least 2x2)", who, (long)width, (long)height);
  if ((width | height) & 1)
    return rt_fail("%s: image size %ldx%ld is odd (the low frame is width / 2 x height / 2)", who, (long)width, (long)height);
  return check_image_size(who, (i32)width, (i32)height);
}

static int check_upsample(const char *who, i64 width, i64 height, RT_Upsample_Params const *u) {
  if (check_upsample_size(who, width, height) != 0) return -1;
  if (!u) return rt_fail("%s: upsample params are NULL", who);
  // (written so that NaN fails)
  if (!(u->sigma_normal > 0.0f)) return rt_fail("%s: sigma_normal must be > 0 (got %g)", who, (double)u->sigma_normal);
  if (!(u->sigma_position > 0.0f)) return rt_fail("%s: sigma_position must be > 0 (got %g)", who, (double)u->sigma_position);
  if (u->demodulate != 0 && u->demodulate != 1) return rt_fail("%s: demodulate must be 0 or 1 (got %d)", who, u->demodulate);
  return 0;
}

// The planes of a frame are there -- its colour when `with_color`, the albedo only where `demodulate` reads it -- wherever the
// pointers are.  A message names a pointer as the entry point's arguments do: in a struct `owner` of host arrays "owner->plane",
// among device pointers (owner NULL) "d_plane" with `suffix` behind it ("", "_low").
static int check_frame(const char *who, RT_Frame const &f, bool with_color, int demodulate, const char *owner, const char *suffix = "") {
  char n[48];
  auto name = [&](const char *plane) {
    if (owner) snprintf(n, sizeof n, "%s->%s", owner, plane);
    else snprintf(n, sizeof n, "d_%s%s", plane, suffix);
    return n;
  };
  if (with_color && !f.color) return rt_fail("%s: %s is NULL", who, name("color"));
  if (!f.coverage) return rt_fail("%s: %s is NULL", who, name("coverage"));
  if (!f.albedo && demodulate) return rt_fail("%s: %s is NULL and demodulate is set", who, name("albedo"));
  if (!f.normal) return rt_fail("%s: %s is NULL", who, name("normal"));
  if (!f.position) return rt_fail("%s: %s is NULL", who, name("position"));
  return 0;
}

// A frame in host arrays: the colour, then the struct of its planes.
static int check_host_frame(const char *who, f32 const *color, RT_Features const *planes, int demodulate) {
  if (!color) return rt_fail("%s: color is NULL", who);
  if (!planes) return rt_fail("%s: planes is NULL", who);
  return check_frame(who, device_frame(nullptr, *planes), false, demodulate, "planes");
}

// An output an entry point offers, by the name its message has for it; name NULL: this form of the entry point does not offer it.
struct Output { const char *name; const void *p; };
// Refuses a call that wants none of them: "a, b and c are NULL".
template <int N> static int check_wanted(const char *who, const Output (&outs)[N]) {
  int offered = 0, k = 0;
  for (const Output &o : outs) {
    if (o.name && o.p) return 0;
    offered += o.name != nullptr;
  }
  char names[128] = "";
  for (const Output &o : outs)
    if (o.name) snprintf(names + strlen(names), sizeof names - strlen(names), "%s%s", ++k == 1 ? "" : k == offered ? " and " : ", ", o.name);
  return rt_fail("%s: no output is wanted (%s are NULL)", who, names);
}

// An array an entry point reads or writes, by the name its message has for it; p NULL: not given.
struct Range { const char *name; const void *p; uintptr_t bytes; };
// Two arrays that are given share a byte.
static bool overlap(Range const &x, Range const &y) {
  const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
  return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
}

// d_<what>_in (optional) and d_<what>_out, `bytes` each, must lie apart: a pixel reads records that other pixels write.
static int check_apart(const char *who, const char *what, const void *in, const void *out, uintptr_t bytes) {
  if (overlap({nullptr, in, bytes}, {nullptr, out, bytes}))
    return rt_fail("%s: d_%s_in and d_%s_out overlap (the reads are gathers)", who, what, what);
  return 0;
}

// No output may overlap an input: the upsampling writes a pixel while other pixels still read.
template <int N, int M> static int check_ranges_apart(const char *who, const Range (&outs)[N], const Range (&ins)[M]) {
  for (const Range &o : outs)
    for (const Range &i : ins)
      if (overlap(o, i)) return rt_fail("%s: %s overlaps %s", who, o.name, i.name);
  return 0;
}

// The calls that answer with a size or an object have ONE message for a size check_image_size() refuses.  (check_image_size has
// two, "is invalid" and "is too large", which every other call here reports: the one text cannot come out of it.)
static bool size_refused(const char *who, i32 width, i32 height) {
  if (width > 0 && height > 0 && (int64_t)width * height <= RT_MAX_PIXELS) return false;
  rt_fail("%s: image size %dx%d is invalid", who, width, height);
  return true;
}
static i64 bytes_of(const char *who, i32 width, i32 height, int per_pixel) {
  return size_refused(who, width, height) ? -1 : (i64)width * height * per_pixel;
}

extern "C" i64 rt_guided_work_bytes(i32 w, i32 h) { return bytes_of("rt_guided_work_bytes", w, h, RT_GUIDED_WORK_PER_PIXEL); }
extern "C" i64 rt_temporal_history_bytes(i32 w, i32 h) { return bytes_of("rt_temporal_history_bytes", w, h, RT_TEMPORAL_HISTORY_PER_PIXEL); }
extern "C" i64 rt_guided_variance_work_bytes(i32 w, i32 h) { return bytes_of("rt_guided_variance_work_bytes", w, h, RT_GUIDED_WORK_PER_PIXEL); }
extern "C" i64 rt_temporal_moments_bytes(i32 w, i32 h) { return bytes_of("rt_temporal_moments_bytes", w, h, RT_TEMPORAL_MOMENTS_PER_PIXEL); }
// (its sizes are the upsampling's, with their own messages)
extern "C" i64 rt_guided_upsample_work_bytes(i32 width, i32 height) {
  if (check_upsample_size("rt_guided_upsample_work_bytes", width, height) != 0) return -1;
  return (i64)(width / 2) * (height / 2) * RT_UPSAMPLE_WORK_PER_LOW_PIXEL;
}

// ---------------------------------------------------------------------------------
// the stages.  Every pointer is on the current device; the launches go on `stream`.

// The filter's work area (rt_guided_work_bytes): the two colour buffers the iterations ping-pong between, then the two guide planes.
struct GuidedWork { void *buf[2], *g0, *g1; };

// 0, or the refusal of a launch whose launcher returned the HIP error rc: `message` is "... kernel launch failed: %s".
static int launched(int rc, const char *message) { return rc == 0 ? 0 : rt_fail(message, hipGetErrorString((hipError_t)rc)); }

// THE VARIANT OF A STAGE IS CHOSEN HERE, in its one launch: the plain kernel (rt_guided.hip, rt_temporal.hip) or its variance /
// moments form (rt_variance.hip), by whether the optional input or output is given.
static int launch_pack(size_t pixels, int demodulate, RT_Frame const &f, const float *variance, GuidedWork const &w, hipStream_t stream) {
  return launched(variance ? rt_launch_variance_pack((int)pixels, demodulate, f, variance, w.buf[0], w.g0, w.g1, stream)
                           : rt_launch_guided_pack((int)pixels, demodulate, f, w.buf[0], w.g0, w.g1, stream),
                  "guided pack kernel launch failed: %s");
}

// Iteration i of g->iterations, step 1 << i, from w.buf[i & 1] into the other; the last one writes what `o` wants.
static int launch_filter(i32 width, i32 height, RT_Guided_Params const *g, int i, GuidedWork const &w, RT_Frame const &f,
                         FilterIO const &o, hipStream_t stream) {
  const float k_c = 1.0f / (g->sigma_color * g->sigma_color), k_n = 1.0f / (g->sigma_normal * g->sigma_normal),
              k_p = 1.0f / (g->sigma_position * g->sigma_position);
  const bool variance_guided = o.variance_in != nullptr;
  const float kc_i = variance_guided ? k_c : k_c * (float)(1u << (2 * i));     // the plain filter's colour sigma halves every iteration
  const int last = i == g->iterations - 1;
  void *const src = w.buf[i & 1], *const dst = w.buf[(i & 1) ^ 1];
  const FilterIO lo = last ? o : FilterIO{};
  if (variance_guided)
    return launched(rt_launch_variance_filter(width, height, 1 << i, k_n, k_p, kc_i, last, g->demodulate, src, dst, w.g0, w.g1, f, lo.out,
                                              lo.image, lo.variance_out, stream),
                    "variance-guided filter kernel launch failed: %s");
  return launched(rt_launch_guided_filter(width, height, 1 << i, k_n, k_p, kc_i, last, g->demodulate, src, dst, w.g0, w.g1, f, lo.out,
                                          lo.image, stream),
                  "guided filter kernel launch failed: %s");
}

static int launch_accumulate(RT_TParams const &P, RT_Frame const &f, const void *history_in, void *history_out, AccumulateIO const &a,
                             hipStream_t stream) {
  if (a.moments_out && a.motion)
    return launched(rt_launch_temporal_moments_motion(&P, f, a.motion, history_in, history_out, a.out, a.length, a.image, a.moments_in,
                                                      a.moments_out, stream),
                    "temporal moments kernel launch failed: %s");
  if (a.moments_out)
    return launched(rt_launch_temporal_moments(&P, f, history_in, history_out, a.out, a.length, a.image, a.moments_in, a.moments_out, stream),
                    "temporal moments kernel launch failed: %s");
  if (a.motion)
    return launched(rt_launch_temporal_motion(&P, f, a.motion, history_in, history_out, a.out, a.length, a.image, stream),
                    "temporal kernel launch failed: %s");
  return launched(rt_launch_temporal(&P, f, history_in, history_out, a.out, a.length, a.image, stream), "temporal kernel launch failed: %s");
}

// Enqueues the pack launch and g->iterations filter launches.  Every input is in d_work before o.out / o.image are written (the last
// launch reads a pixel's colour and albedo only to write that pixel).
static int enqueue_guided(i32 width, i32 height, RT_Guided_Params const *g, RT_Frame const &f, FilterIO const &o, void *d_work,
                          hipStream_t stream) {
  const size_t pixels = (size_t)width * height;
  uint8_t *b = (uint8_t *)d_work;
  const GuidedWork w = {{b, b + pixels * 16}, b + pixels * 32, b + pixels * 48};
  if (launch_pack(pixels, g->demodulate, f, o.variance_in, w, stream) != 0) return -1;
  for (int i = 0; i < g->iterations; i++)
    if (launch_filter(width, height, g, i, w, f, o, stream) != 0) return -1;
  return 0;
}

// Enqueues the pack launch over the low frame and the upsampling launch (d_work: rt_guided_upsample_work_bytes).  `full`: the
// full-resolution planes (its colour is not read).
static int enqueue_upsample(i32 width, i32 height, RT_Upsample_Params const *u, RT_Frame const &low, RT_Frame const &full, float *out,
                            uint8_t *image, void *d_work, hipStream_t stream) {
  const size_t low_pixels = (size_t)(width / 2) * (height / 2);
  uint8_t *b = (uint8_t *)d_work;
  const GuidedWork w = {{b, nullptr}, b + low_pixels * 16, b + low_pixels * 32};
  if (launch_pack(low_pixels, u->demodulate, low, nullptr, w, stream) != 0) return -1;
  const float k_n = 1.0f / (u->sigma_normal * u->sigma_normal), k_p = 1.0f / (u->sigma_position * u->sigma_position);
  return launched(rt_launch_upsample(width, height, k_n, k_p, u->demodulate, w.buf[0], w.g0, w.g1, full, out, image, stream),
                  "upsample kernel launch failed: %s");
}

static void temporal_camera(RT_TCamera *c, Camera const *cam) {
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 3; k++) c->r[i][k] = cam->view_matrix.rows[i][k];
    c->t[i] = cam->view_matrix.rows[i][3];
  }
  c->focal_length = cam->focal_length;
}

// Enqueues the accumulation, and behind its moments form, when a.variance is wanted, the variance launch, which reads d_history_out
// and a.moments_out.  prev is read only when d_history_in is given.
static int enqueue_temporal(i32 width, i32 height, RT_Temporal_Params const *t, Camera const *cam, Camera const *prev, RT_Frame const &f,
                            const void *d_history_in, void *d_history_out, AccumulateIO const &a, hipStream_t stream) {
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
  if (launch_accumulate(P, f, d_history_in, d_history_out, a, stream) != 0) return -1;
  if (!a.moments_out || !a.variance) return 0;
  const float k_n = 1.0f / (a.vp->sigma_normal * a.vp->sigma_normal), k_p = 1.0f / (a.vp->sigma_position * a.vp->sigma_position);
  return launched(rt_launch_variance(width, height, k_n, k_p, d_history_out, a.moments_out, a.variance, stream),
                  "variance kernel launch failed: %s");
}

// ---- device level -------------------------------------------------------------------------------------------------------------
// (everything that can be checked without the device is checked before it is touched)

// The frame of an entry point's five device pointers: the only casts.
static RT_Frame frame_of(void const *d_color, void const *d_coverage, void const *d_albedo, void const *d_normal,
                                void const *d_position) {
  return {(const float *)d_color, (const float *)d_coverage, (const float *)d_albedo, (const float *)d_normal, (const float *)d_position};
}

static int device_ready() {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  return ensure_device(D);
}

// rt_guided_denoise and rt_guided_denoise_variance (with_variance: o.variance_in is required, o.variance_out optional)
static int guided_device(const char *who, bool with_variance, i32 width, i32 height, RT_Guided_Params const *params, RT_Frame const &f,
                         FilterIO const &o, void *d_work, hipStream_t stream) {
  if (check_guided(who, width, height, params) != 0) return -1;
  if (check_frame(who, f, true, params->demodulate, nullptr) != 0) return -1;
  if (with_variance && !o.variance_in) return rt_fail("%s: d_variance is NULL", who);
  const Output outs[] = {{"d_out", o.out}, {"d_image", o.image}, {with_variance ? "d_variance_out" : nullptr, o.variance_out}};
  if (check_wanted(who, outs) != 0) return -1;
  if (!d_work) return rt_fail("%s: d_work is NULL", who);
  if ((uintptr_t)d_work & 15) return rt_fail("%s: d_work must be 16-byte aligned", who);
  if (device_ready() != 0) return -1;
  return enqueue_guided(width, height, params, f, o, d_work, stream);
}

extern "C" int rt_guided_denoise(i32 width, i32 height, RT_Guided_Params const *params, void const *d_color, void const *d_coverage,
                                 void const *d_albedo, void const *d_normal, void const *d_position, void *d_out, void *d_image,
                                 void *d_work, void *stream) {
  return guided_device("rt_guided_denoise", false, width, height, params, frame_of(d_color, d_coverage, d_albedo, d_normal, d_position),
                       {(float *)d_out, (uint8_t *)d_image}, d_work, (hipStream_t)stream);
}

extern "C" int rt_guided_denoise_variance(i32 width, i32 height, RT_Guided_Params const *params, void const *d_color,
                                          void const *d_coverage, void const *d_albedo, void const *d_normal, void const *d_position,
                                          void *d_out, void *d_image, void *d_work, void *stream, void const *d_variance,
                                          void *d_variance_out) {
  return guided_device("rt_guided_denoise_variance", true, width, height, params, frame_of(d_color, d_coverage, d_albedo, d_normal, d_position),
                       {(float *)d_out, (uint8_t *)d_image, (const float *)d_variance, (float *)d_variance_out}, d_work, (hipStream_t)stream);
}

// rt_temporal_accumulate, rt_temporal_accumulate_moments and rt_temporal_accumulate_motion (with_moments: a.moments_out is
// required, a.moments_in goes with d_history_in, a.vp is required when a.variance is wanted; with_motion: a.motion is required)
static int temporal_device(const char *who, bool with_moments, bool with_motion, i32 width, i32 height, RT_Temporal_Params const *params,
                           Camera const *camera, Camera const *previous_camera, RT_Frame const &f, void const *d_history_in,
                           void *d_history_out, AccumulateIO const &a, hipStream_t stream) {
  if (check_temporal(who, width, height, params) != 0) return -1;
  if (with_moments && (a.vp || a.variance) && check_variance(who, a.vp) != 0) return -1;
  if (!camera) return rt_fail("%s: camera is NULL", who);
  if (d_history_in && !previous_camera) return rt_fail("%s: previous_camera is NULL and a history is given", who);
  if (check_frame(who, f, true, params->demodulate, nullptr) != 0) return -1;
  if (with_motion && !a.motion) return rt_fail("%s: d_motion is NULL", who);
  if (!d_history_out) return rt_fail("%s: d_history_out is NULL", who);
  if (((uintptr_t)d_history_out | (uintptr_t)d_history_in) & 15) return rt_fail("%s: the histories must be 16-byte aligned", who);
  const uintptr_t pixels = (uintptr_t)width * height;
  if (check_apart(who, "history", d_history_in, d_history_out, pixels * RT_TEMPORAL_HISTORY_PER_PIXEL) != 0) return -1;
  if (with_moments) {
    if (!a.moments_out) return rt_fail("%s: d_moments_out is NULL", who);
    if (d_history_in && !a.moments_in) return rt_fail("%s: a history is given without its moments (d_moments_in is NULL)", who);
    if (!d_history_in && a.moments_in) return rt_fail("%s: moments are given without their history (d_history_in is NULL)", who);
    if (((uintptr_t)a.moments_out | (uintptr_t)a.moments_in) & 15) return rt_fail("%s: the moments must be 16-byte aligned", who);
    if (check_apart(who, "moments", a.moments_in, a.moments_out, pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL) != 0) return -1;
  }
  if (device_ready() != 0) return -1;
  return enqueue_temporal(width, height, params, camera, previous_camera, f, d_history_in, d_history_out, a, stream);
}

extern "C" int rt_temporal_accumulate(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                      Camera const *previous_camera, void const *d_color, void const *d_coverage, void const *d_albedo,
                                      void const *d_normal, void const *d_position, void const *d_history_in, void *d_history_out,
                                      void *d_out, void *d_length, void *d_image, void *stream) {
  return temporal_device("rt_temporal_accumulate", false, false, width, height, params, camera, previous_camera,
                         frame_of(d_color, d_coverage, d_albedo, d_normal, d_position), d_history_in, d_history_out,
                         {(float *)d_out, (float *)d_length, (uint8_t *)d_image}, (hipStream_t)stream);
}

extern "C" int rt_temporal_accumulate_moments(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                              Camera const *previous_camera, void const *d_color, void const *d_coverage,
                                              void const *d_albedo, void const *d_normal, void const *d_position,
                                              void const *d_history_in, void *d_history_out, void *d_out, void *d_length, void *d_image,
                                              RT_Variance_Params const *vp, void const *d_moments_in, void *d_moments_out,
                                              void *d_variance, void *stream) {
  const AccumulateIO a = {(float *)d_out, (float *)d_length, (uint8_t *)d_image, d_moments_in, d_moments_out, (float *)d_variance, vp};
  return temporal_device("rt_temporal_accumulate_moments", true, false, width, height, params, camera, previous_camera,
                         frame_of(d_color, d_coverage, d_albedo, d_normal, d_position), d_history_in, d_history_out, a, (hipStream_t)stream);
}

// (vp, d_moments_in, d_moments_out and d_variance all NULL: the plain accumulation; otherwise the moments form, by its rules)
extern "C" int rt_temporal_accumulate_motion(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                             Camera const *previous_camera, void const *d_color, void const *d_coverage,
                                             void const *d_albedo, void const *d_normal, void const *d_position,
                                             void const *d_history_in, void *d_history_out, void *d_out, void *d_length, void *d_image,
                                             RT_Variance_Params const *vp, void const *d_moments_in, void *d_moments_out,
                                             void *d_variance, void *stream, void const *d_motion) {
  const bool with_moments = vp || d_moments_in || d_moments_out || d_variance;
  const AccumulateIO a = {(float *)d_out, (float *)d_length, (uint8_t *)d_image, d_moments_in, d_moments_out, (float *)d_variance, vp,
                          (const float *)d_motion};
  return temporal_device("rt_temporal_accumulate_motion", with_moments, true, width, height, params, camera, previous_camera,
                         frame_of(d_color, d_coverage, d_albedo, d_normal, d_position), d_history_in, d_history_out, a, (hipStream_t)stream);
}

// No output may lie over an input or the work area (or the image over the f32 output): the launch writes pixels while others read.
extern "C" int rt_guided_upsample(i32 width, i32 height, RT_Upsample_Params const *params, void const *d_color_low,
                                  void const *d_coverage_low, void const *d_albedo_low, void const *d_normal_low,
                                  void const *d_position_low, void const *d_coverage, void const *d_albedo, void const *d_normal,
                                  void const *d_position, void *d_out, void *d_image, void *d_work, void *stream) {
  const char *who = "rt_guided_upsample";
  if (check_upsample(who, width, height, params) != 0) return -1;
  const RT_Frame low = frame_of(d_color_low, d_coverage_low, d_albedo_low, d_normal_low, d_position_low);
  const RT_Frame full = frame_of(nullptr, d_coverage, d_albedo, d_normal, d_position);
  if (check_frame(who, low, true, params->demodulate, nullptr, "_low") != 0) return -1;
  if (check_frame(who, full, false, params->demodulate, nullptr) != 0) return -1;
  const Output wanted[] = {{"d_out", d_out}, {"d_image", d_image}};
  if (check_wanted(who, wanted) != 0) return -1;
  if (!d_work) return rt_fail("%s: d_work is NULL", who);
  if ((uintptr_t)d_work & 15) return rt_fail("%s: d_work must be 16-byte aligned", who);
  const uintptr_t pixels = (uintptr_t)width * height, f1 = pixels * sizeof(float), l1 = f1 / 4;
  const Range outs[] = {{"d_out", d_out, f1 * 3}, {"d_image", d_image, pixels * 3}};
  const Range ins[] = {{"d_color_low", low.color, l1 * 3}, {"d_coverage_low", low.coverage, l1}, {"d_albedo_low", low.albedo, l1 * 3},
                       {"d_normal_low", low.normal, l1 * 3}, {"d_position_low", low.position, l1 * 3}, {"d_coverage", full.coverage, f1},
                       {"d_albedo", full.albedo, f1 * 3}, {"d_normal", full.normal, f1 * 3}, {"d_position", full.position, f1 * 3},
                       {"d_work", d_work, (uintptr_t)(pixels / 4) * RT_UPSAMPLE_WORK_PER_LOW_PIXEL}};
  if (check_ranges_apart(who, outs, ins) != 0) return -1;
  if (overlap(outs[1], outs[0])) return rt_fail("%s: d_image overlaps d_out", who);
  if (device_ready() != 0) return -1;
  return enqueue_upsample(width, height, params, low, full, (float *)d_out, (uint8_t *)d_image, d_work, (hipStream_t)stream);
}

// ---- host level ---------------------------------------------------------------------------------------------------------------
// The host-level calls run on the NULL stream: it does not wait for the lane streams of frames in flight.

// Copies a host frame into `in`: the colour (optional) at `in` itself, behind it the planes as FeatureState keeps them -- with a
// colour RT_HOST_FRAME_F32 f32 per pixel, without one RT_FEATURE_CHANNELS.  *f is the frame on the device; f->color is NULL
// without a colour, f->albedo when the host gave none.
static int upload_host_frame(float *in, size_t pixels, f32 const *color, RT_Features const *planes, RT_Frame *f) {
  const size_t f3 = pixels * 3 * sizeof(float), f1 = pixels * sizeof(float);
  RT_Features d = split_feature_planes(color ? in + pixels * 3 : in, pixels);
  if (color) HIP_TRY(hipMemcpy(in, color, f3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.coverage, planes->coverage, f1, hipMemcpyHostToDevice));
  if (planes->albedo) HIP_TRY(hipMemcpy(d.albedo, planes->albedo, f3, hipMemcpyHostToDevice));
  else d.albedo = nullptr;
  HIP_TRY(hipMemcpy(d.normal, planes->normal, f3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.position, planes->position, f3, hipMemcpyHostToDevice));
  *f = device_frame(color ? in : nullptr, d);
  return 0;
}

// rt_guided_denoise_host and rt_guided_denoise_variance_host (with_variance: h.variance_in is required, h.variance_out optional);
// h holds the host's pointers
static int guided_host(const char *who, bool with_variance, i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                       RT_Features const *planes, FilterIO const &h) {
  if (check_guided(who, width, height, params) != 0) return -1;
  if (check_host_frame(who, color, planes, params->demodulate) != 0) return -1;
  if (with_variance && !h.variance_in) return rt_fail("%s: variance is NULL", who);
  const Output outs[] = {{"out", h.out}, {"image", h.image}, {with_variance ? "variance_out" : nullptr, h.variance_out}};
  if (check_wanted(who, outs) != 0) return -1;

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  GuidedState &S = D.guided;
  const size_t pixels = (size_t)width * height;
  HIP_TRY(S.in.grow(pixels * RT_HOST_FRAME_F32));
  HIP_TRY(S.work.grow(pixels * RT_GUIDED_WORK_PER_PIXEL));
  if (h.out) HIP_TRY(S.out.grow(pixels * 3));
  if (h.image) HIP_TRY(S.image.grow(pixels * 3));
  if (h.variance_in) HIP_TRY(S.variance.grow(pixels));
  if (h.variance_out) HIP_TRY(S.variance_out.grow(pixels));
  hipStream_t stream = nullptr;
  RT_Frame f;
  if (upload_host_frame(S.in, pixels, color, planes, &f) != 0) return -1;
  if (h.variance_in) HIP_TRY(hipMemcpy(S.variance, h.variance_in, pixels * sizeof(float), hipMemcpyHostToDevice));
  const FilterIO d = {h.out ? S.out.get() : nullptr, h.image ? S.image.get() : nullptr, h.variance_in ? S.variance.get() : nullptr,
                      h.variance_out ? S.variance_out.get() : nullptr};
  if (enqueue_guided(width, height, params, f, d, S.work, stream) != 0) return -1;
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  if (h.out) HIP_TRY(hipMemcpy(h.out, S.out, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (h.image) HIP_TRY(hipMemcpy(h.image, S.image, pixels * 3, hipMemcpyDeviceToHost));
  if (h.variance_out) HIP_TRY(hipMemcpy(h.variance_out, S.variance_out, pixels * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rt_guided_denoise_host(i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                                      RT_Features const *planes, f32 *out, u8 *image) {
  return guided_host("rt_guided_denoise_host", false, width, height, params, color, planes, {out, image});
}

extern "C" int rt_guided_denoise_variance_host(i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                                               RT_Features const *planes, f32 *out, u8 *image, f32 const *variance, f32 *variance_out) {
  return guided_host("rt_guided_denoise_variance_host", true, width, height, params, color, planes, {out, image, variance, variance_out});
}

extern "C" int rt_guided_upsample_host(i32 width, i32 height, RT_Upsample_Params const *params, f32 const *color_low,
                                       RT_Features const *low, RT_Features const *full, f32 *out, u8 *image) {
  const char *who = "rt_guided_upsample_host";
  if (check_upsample(who, width, height, params) != 0) return -1;
  if (!color_low) return rt_fail("%s: color_low is NULL", who);
  if (!low) return rt_fail("%s: low is NULL", who);
  if (!full) return rt_fail("%s: full is NULL", who);
  if (check_frame(who, device_frame(nullptr, *low), false, params->demodulate, "low") != 0) return -1;
  if (check_frame(who, device_frame(nullptr, *full), false, params->demodulate, "full") != 0) return -1;
  const Output wanted[] = {{"out", out}, {"image", image}};
  if (check_wanted(who, wanted) != 0) return -1;

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  UpsampleState &S = D.upsample;
  const size_t pixels = (size_t)width * height, low_pixels = pixels / 4;
  HIP_TRY(S.in_low.grow(low_pixels * RT_HOST_FRAME_F32));
  HIP_TRY(S.in_full.grow(pixels * RT_FEATURE_CHANNELS));
  HIP_TRY(S.work.grow(low_pixels * RT_UPSAMPLE_WORK_PER_LOW_PIXEL));
  if (out) HIP_TRY(S.out.grow(pixels * 3));
  if (image) HIP_TRY(S.image.grow(pixels * 3));
  hipStream_t stream = nullptr;
  RT_Frame fl, ff;
  if (upload_host_frame(S.in_low, low_pixels, color_low, low, &fl) != 0) return -1;
  if (upload_host_frame(S.in_full, pixels, nullptr, full, &ff) != 0) return -1;
  if (enqueue_upsample(width, height, params, fl, ff, out ? S.out.get() : nullptr, image ? S.image.get() : nullptr, S.work, stream) != 0)
    return -1;
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  if (out) HIP_TRY(hipMemcpy(out, S.out, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (image) HIP_TRY(hipMemcpy(image, S.image, pixels * 3, hipMemcpyDeviceToHost));
  return 0;
}

static const char *missing_history_plane(RT_History_Planes const *h) {
  for (const HistoryPlane &pl : HISTORY_PLANES)
    if (!(h->*pl.member)) return pl.name;
  return nullptr;
}

// rt_temporal_accumulate_host and rt_temporal_accumulate_moments_host (with_moments: h.moments_in goes with history_in,
// h.moments_out and h.variance are optional outputs, h.vp is required when h.variance is wanted) and
// rt_temporal_accumulate_motion_host (with_motion: h.motion is required); h holds the host's pointers
static int temporal_host(const char *who, bool with_moments, bool with_motion, i32 width, i32 height, RT_Temporal_Params const *params,
                         Camera const *camera, Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                         RT_History_Planes const *history_in, RT_History_Planes const *history_out, AccumulateIO const &h) {
  if (check_temporal(who, width, height, params) != 0) return -1;
  if (with_moments && (h.vp || h.variance) && check_variance(who, h.vp) != 0) return -1;
  if (!camera) return rt_fail("%s: camera is NULL", who);
  if (history_in && !previous_camera) return rt_fail("%s: previous_camera is NULL and a history is given", who);
  if (check_host_frame(who, color, planes, params->demodulate) != 0) return -1;
  if (with_motion && !h.motion) return rt_fail("%s: motion is NULL", who);
  if (history_in && missing_history_plane(history_in)) return rt_fail("%s: history_in->%s is NULL", who, missing_history_plane(history_in));
  if (history_out && missing_history_plane(history_out)) return rt_fail("%s: history_out->%s is NULL", who, missing_history_plane(history_out));
  if (with_moments && history_in && !h.moments_in) return rt_fail("%s: a history is given without its moments (moments_in is NULL)", who);
  if (with_moments && !history_in && h.moments_in) return rt_fail("%s: moments are given without their history (history_in is NULL)", who);
  const Output outs[] = {{"history_out", history_out}, {"out", h.out}, {"length", h.length}, {"image", h.image},
                         {with_moments ? "moments_out" : nullptr, h.moments_out}, {with_moments ? "variance" : nullptr, h.variance}};
  if (check_wanted(who, outs) != 0) return -1;

  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  TemporalState &S = D.temporal;
  const size_t pixels = (size_t)width * height, f3 = pixels * 3 * sizeof(float), f1 = pixels * sizeof(float);
  HIP_TRY(S.in.grow(pixels * RT_HOST_FRAME_F32));
  HIP_TRY(S.planar.grow(pixels * RT_HISTORY_PLANAR_F32));
  HIP_TRY(S.hist[0].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  HIP_TRY(S.hist[1].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
  if (h.out) HIP_TRY(S.out.grow(pixels * 3));
  if (h.length) HIP_TRY(S.length.grow(pixels));
  if (h.image) HIP_TRY(S.image.grow(pixels * 3));
  if (with_moments) {
    HIP_TRY(S.mom[0].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
    HIP_TRY(S.mom[1].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
    HIP_TRY(S.mom_planar.grow(pixels * 2));
    if (h.variance) HIP_TRY(S.variance.grow(pixels));
  }
  if (with_motion) HIP_TRY(S.motion.grow(pixels * RT_MOTION_CHANNELS));
  float *pl[5];                                                 // the staged planes, in HISTORY_PLANES' order
  for (int k = 0; k < 5; k++) pl[k] = S.planar + pixels * HISTORY_PLANES[k].offset;
  hipStream_t stream = nullptr;
  RT_Frame f;
  if (upload_host_frame(S.in, pixels, color, planes, &f) != 0) return -1;
  if (with_motion) HIP_TRY(hipMemcpy(S.motion, h.motion, f3, hipMemcpyHostToDevice));
  if (history_in) {
    for (int k = 0; k < 5; k++)
      HIP_TRY(hipMemcpy(pl[k], history_in->*HISTORY_PLANES[k].member, f1 * HISTORY_PLANES[k].floats, hipMemcpyHostToDevice));
    int rc = rt_launch_temporal_pack((int)pixels, pl[0], pl[1], pl[2], pl[3], pl[4], S.hist[0], stream);
    if (launched(rc, "temporal pack kernel launch failed: %s") != 0) return -1;
    if (with_moments) {
      HIP_TRY(hipMemcpy(S.mom_planar, h.moments_in, 2 * f1, hipMemcpyHostToDevice));
      rc = rt_launch_moments_pack((int)pixels, S.mom_planar, S.mom[0], stream);
      if (launched(rc, "moments pack kernel launch failed: %s") != 0) return -1;
    }
  }
  const AccumulateIO d = {h.out ? S.out.get() : nullptr, h.length ? S.length.get() : nullptr, h.image ? S.image.get() : nullptr,
                          with_moments && history_in ? S.mom[0].get() : nullptr, with_moments ? S.mom[1].get() : nullptr,
                          h.variance ? S.variance.get() : nullptr, h.vp, with_motion ? S.motion.get() : nullptr};
  if (enqueue_temporal(width, height, params, camera, previous_camera, f, history_in ? S.hist[0].get() : nullptr, S.hist[1], d,
                       stream) != 0)
    return -1;
  const int rc_m = h.moments_out ? rt_launch_moments_unpack((int)pixels, S.mom[1], S.mom_planar, stream) : 0;
  if (launched(rc_m, "moments unpack kernel launch failed: %s") != 0) return -1;
  const int rc_h = history_out ? rt_launch_temporal_unpack((int)pixels, S.hist[1], pl[0], pl[1], pl[2], pl[3], pl[4], stream) : 0;
  if (launched(rc_h, "temporal unpack kernel launch failed: %s") != 0) return -1;
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipGetLastError());
  if (history_out)
    for (int k = 0; k < 5; k++)
      HIP_TRY(hipMemcpy(history_out->*HISTORY_PLANES[k].member, pl[k], f1 * HISTORY_PLANES[k].floats, hipMemcpyDeviceToHost));
  if (h.out) HIP_TRY(hipMemcpy(h.out, S.out, f3, hipMemcpyDeviceToHost));
  if (h.length) HIP_TRY(hipMemcpy(h.length, S.length, f1, hipMemcpyDeviceToHost));
  if (h.image) HIP_TRY(hipMemcpy(h.image, S.image, pixels * 3, hipMemcpyDeviceToHost));
  if (h.moments_out) HIP_TRY(hipMemcpy(h.moments_out, S.mom_planar, 2 * f1, hipMemcpyDeviceToHost));
  if (h.variance) HIP_TRY(hipMemcpy(h.variance, S.variance, f1, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rt_temporal_accumulate_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                           Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                           RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                           f32 *length, u8 *image) {
  return temporal_host("rt_temporal_accumulate_host", false, false, width, height, params, camera, previous_camera, color, planes, history_in,
                       history_out, {out, length, image});
}

extern "C" int rt_temporal_accumulate_moments_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                                   Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                                   RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                                   f32 *length, u8 *image, RT_Variance_Params const *vp, f32 const *moments_in,
                                                   f32 *moments_out, f32 *variance) {
  return temporal_host("rt_temporal_accumulate_moments_host", true, false, width, height, params, camera, previous_camera, color, planes,
                       history_in, history_out, {out, length, image, moments_in, moments_out, variance, vp});
}

// (vp, moments_in, moments_out and variance all NULL: the plain accumulation; otherwise the moments form, by its rules)
extern "C" int rt_temporal_accumulate_motion_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                                  Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                                  RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                                  f32 *length, u8 *image, RT_Variance_Params const *vp, f32 const *moments_in,
                                                  f32 *moments_out, f32 *variance, f32 const *motion) {
  const bool with_moments = vp || moments_in || moments_out || variance;
  return temporal_host("rt_temporal_accumulate_motion_host", with_moments, true, width, height, params, camera, previous_camera, color,
                       planes, history_in, history_out, {out, length, image, moments_in, moments_out, variance, vp, motion});
}

// ---- the history a host keeps ---------------------------------------------------------------------------------------------------
// Gives back the staging of the temporal calls and the memory of every RT_History, which start again from nothing (the objects
// stay their hosts', and the list of them stays).  What release_staging() does for this state: D.mutex held, D's GPU current,
// device idle.
void release_temporal_state(Device &D) {
  std::vector<RT_History *> keep = std::move(D.temporal.histories);
  for (RT_History *h : keep) h->release();
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
  history->valid = history->moments_valid = false;              // (the memory stays for the next frame)
  return 0;
}

extern "C" int rt_history_set_motion(RT_History *history, int on) {
  if (!history) return rt_fail("rt_history_set_motion: history is NULL");
  if (on != 0 && on != 1) return rt_fail("rt_history_set_motion: on must be 0 or 1 (got %d)", on);
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  history->motion = on != 0;                                    // (the history itself stays: W_p is kept either way)
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
    history->release();
  }
  delete history;
}

// ---- behind a frame -----------------------------------------------------------------------------------------------------------

// The four entry points: their word for the frame in the one-device refusal; their stages -- `history`: the accumulation,
// `variance`: it carries the moments and the filter is the variance-guided one, `upsample`: the frame is rendered at half the size
// and upsampled, `must_filter`: the filter's params are required --; their list of the outputs in the refusal of a call that wants
// none.  (No entry point has both a history and the upsampling.)
struct PostFrame { const char *what; bool history, variance, upsample, must_filter; const char *outputs; };
static const PostFrame DENOISED = {"a denoised frame", false, false, false, true, "no pixels and no linear_denoised"};
static const PostFrame ACCUMULATED = {"an accumulated frame", true, false, false, false, "no pixels, no linear_out, no length"};
static const PostFrame SVGF = {"a variance-guided frame", true, true, false, true, "no pixels, no linear_out, no length, no variance"};
static const PostFrame UPSAMPLED = {"an upsampled frame", false, false, true, false, "no pixels, no linear_upsampled, no linear_out"};

// The stages' arguments (NULL: the entry point has no such stage, or g: the caller wants no filter), and what the caller wants back
// besides the Image (f32, each optional): the frame as rendered (at half the size when it is upsampled), the last stage's output,
// the history lengths, the filter's variance, the upsampling's output.
struct PostStages {
  RT_Guided_Params const *g; RT_History *history; RT_Temporal_Params const *t; RT_Variance_Params const *vp; RT_Upsample_Params const *u;
};
struct PostOutputs { f32 *linear_noisy, *linear_out, *length, *variance, *linear_upsampled; };

// The frame, the four planes of its feature pass, then the stages that are given -- the accumulation against s.history (s.t) or
// the upsampling (s.u), the filter (s.g) -- in one scene-checked call.  W.linear is the noisy frame, D.temporal.out / length serve
// the accumulation, D.upsample.work / out the upsampling, D.guided.work / out the filter, and W.image receives the encoding of the
// LAST stage.  s.vp (with history and g): rt_render_svgf -- the accumulation carries the history's moments, the variance launch
// follows it into D.temporal.variance, and the filter is the variance-guided one.  A history with motion on
// (rt_history_set_motion): the feature pass is the motion kernel's -- one launch -- against the scene's kept geometry, its motion
// sums are resolved into F.motion, and the accumulation is THE ACCUMULATION WITH MOTION.  s.u: rt_render_upsampled -- the frame
// and its feature pass (into D.upsample.low_planes) are at half the Image's size, a second feature pass with guide_samples fills
// D.features.planes at full size, and the upsampling and the filter run at full size.
static int render_post(const char *who, PostFrame const &kind, Scene const *scene, Image const *image, isize samples, isize max_bounces,
                       PostStages const &s, PostOutputs const &o) {
  // before the device lock: the image's size before it goes into 32 bits, the stages' parameters, the rest of the frame's
  if (!scene) return rt_fail("%s: scene is NULL", who);
  if (!image) return rt_fail("%s: image is NULL", who);
  if (kind.history && !s.history) return rt_fail("%s: history is NULL", who);
  if (kind.upsample) {
    if (check_upsample(who, image->width, image->height, s.u) != 0) return -1;
  } else if (image->width <= 0 || image->height <= 0 || image->width > 0x7fffffff || image->height > 0x7fffffff)
    return rt_fail("%s: image size %ldx%ld is invalid", who, (long)image->width, (long)image->height);
  const i32 width = (i32)image->width, height = (i32)image->height;
  if (kind.history && check_temporal(who, width, height, s.t) != 0) return -1;
  if (kind.variance && check_variance(who, s.vp) != 0) return -1;
  if ((kind.must_filter || s.g) && check_guided(who, width, height, s.g) != 0) return -1;
  if (check_image_layout(image, who) != 0) return -1;
  if (samples <= 0 || samples > 0x7fffffff) return rt_fail("%s: samples must be positive and fit 32 bits (got %ld)", who, (long)samples);
  if (max_bounces < 0 || max_bounces > 0x7fffffff) return rt_fail("%s: max_bounces must be >= 0 and fit 32 bits (got %ld)", who, (long)max_bounces);
  if (kind.upsample) {
    if (s.u->guide_samples < 0 || s.u->guide_samples > samples)
      return rt_fail("%s: guide_samples must be 0 .. samples (got %d, samples %ld)", who, s.u->guide_samples, (long)samples);
    if (o.linear_out && !s.g) return rt_fail("%s: linear_out is the filter's output and guided params are NULL", who);
  }
  if (!image->pixels.data && !o.linear_out && !o.length && !o.variance && !o.linear_upsampled)
    return rt_fail("%s: no output is wanted (%s)", who, kind.outputs);

  RT_History *const history = s.history;
  RT_Guided_Params const *const g = s.g;
  RT_Upsample_Params const *const u = s.u;
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (history && (image->width != history->width || image->height != history->height))
    return rt_fail("%s: the image is %ldx%ld and the history %dx%d", who, (long)image->width, (long)image->height, history->width,
                   history->height);
  if (s.vp && history->valid && history->buf[0] && history->buf[1] && !(history->moments_valid && history->mom[0] && history->mom[1]))
    return rt_fail("%s: the history's last frame was written by rt_render_temporal and has no moments: call rt_history_reset first", who);
  const double t_start = now_ms();
  if (ensure_device(D) != 0) return -1;
  if (rt_device_count() > 1)
    return rt_fail("%s: %s renders on one device, and %d are set (rt_set_devices)", who, kind.what, rt_device_count());
  // p: the frame and its feature pass -- at half the Image's size when it is upsampled, and then pf: the full-size feature pass
  Image frame_image = *image;                                      // (the frame's size alone is read from it)
  if (u) {
    frame_image.width = width / 2;
    frame_image.height = height / 2;
  }
  RT_Render_Params p, pf;
  if (fill_frame_params(&p, &frame_image, samples, max_bounces, g_seed.load()) != 0) return -1;
  if (u && fill_frame_params(&pf, image, u->guide_samples ? u->guide_samples : samples, max_bounces, g_seed.load()) != 0) return -1;
  forget_multi_counters();

  FrameTiming T;
  Workspace &W = D.ws;
  FeatureState &F = D.features;
  GuidedState &G = D.guided;
  TemporalState &S = D.temporal;
  UpsampleState &U = D.upsample;
  const size_t pixels = (size_t)width * height, frame_pixels = (size_t)p.width * p.height;
  if (ensure_ws_buffers(W, p.width, p.height, 0, 0) != 0) return -1;
  HIP_TRY(F.sums.grow(pixels * RT_FEATURE_CHANNELS));
  HIP_TRY(F.planes.grow(pixels * RT_FEATURE_CHANNELS));
  const bool want_upsampled = u && (g || o.linear_upsampled);       // the upsampling's f32 output: the filter's input, or the caller's
  if (u) {
    HIP_TRY(W.image.grow(pixels * 3));                              // (the workspace is the low frame's)
    HIP_TRY(U.low_planes.grow(frame_pixels * RT_FEATURE_CHANNELS));
    HIP_TRY(U.work.grow(frame_pixels * RT_UPSAMPLE_WORK_PER_LOW_PIXEL));
    if (want_upsampled) HIP_TRY(U.out.grow(pixels * 3));
  }
  const bool motion = history && history->motion;
  if (motion) {
    HIP_TRY(F.motion_sums.grow(pixels * RT_MOTION_CHANNELS));
    HIP_TRY(F.motion.grow(pixels * RT_MOTION_CHANNELS));
  }
  const bool want_accumulated = history && (g || o.linear_out);   // the accumulation's f32 output: the filter's input, or the caller's
  const uint8_t *h_in = nullptr;
  uint8_t *h_out = nullptr;
  AccumulateIO a = {};                                            // (a.variance: the variance launch's output, the filter's input)
  if (history) {
    if (!history->buf[0] || !history->buf[1]) history->valid = false;          // (given back with the staging: from nothing)
    HIP_TRY(history->buf[0].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
    HIP_TRY(history->buf[1].grow(pixels * RT_TEMPORAL_HISTORY_PER_PIXEL));
    if (want_accumulated) HIP_TRY(S.out.grow(pixels * 3));
    if (o.length) HIP_TRY(S.length.grow(pixels));
    h_in = history->valid ? history->buf[history->cur].get() : nullptr;
    h_out = history->buf[history->cur ^ 1];
    a = {want_accumulated ? S.out.get() : nullptr, o.length ? S.length.get() : nullptr, g ? nullptr : W.image.get()};
    if (s.vp) {
      HIP_TRY(history->mom[0].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
      HIP_TRY(history->mom[1].grow(pixels * RT_TEMPORAL_MOMENTS_PER_PIXEL));
      HIP_TRY(S.variance.grow(pixels));
      a.moments_in = h_in ? history->mom[history->cur].get() : nullptr;
      a.moments_out = history->mom[history->cur ^ 1];
      a.variance = S.variance;
      a.vp = s.vp;
    }
    a.motion = motion ? F.motion.get() : nullptr;
  }
  if (g) {
    HIP_TRY(G.work.grow(pixels * RT_GUIDED_WORK_PER_PIXEL));
    if (o.linear_out) HIP_TRY(G.out.grow(pixels * 3));
  }
  // the planes at the Image's size, and those of the frame: the same, but for a frame that is upsampled
  const RT_Features planes = split_feature_planes(F.planes, pixels);
  const RT_Features frame_planes = u ? split_feature_planes(U.low_planes, frame_pixels) : planes;
  const float *const filter_in = history ? S.out.get() : u ? U.out.get() : W.linear.get();   // the stage before the filter wrote it
  hipStream_t stream = nullptr;
  // (a pass that is run again after a scene edit reads the same old history and writes the same new one)
  auto pass = [&](RT_Device_Scene *d) -> int {
    if (enqueue_frame(D, d, &scene->camera, &p, W, stream, 0, nullptr, nullptr, W.linear) != 0) return -1;
    if (enqueue_feature_pass(D, d, &scene->camera, &p, F.sums, frame_planes, stream, motion ? F.motion_sums.get() : nullptr,
                             motion ? F.motion.get() : nullptr) != 0)
      return -1;
    if (history && enqueue_temporal(width, height, s.t, &scene->camera, &history->camera, device_frame(W.linear, planes), h_in, h_out, a,
                                    stream) != 0)
      return -1;
    if (u && (enqueue_feature_pass(D, d, &scene->camera, &pf, F.sums, planes, stream) != 0 ||
              enqueue_upsample(width, height, u, device_frame(W.linear, frame_planes), device_frame(nullptr, planes),
                               want_upsampled ? U.out.get() : nullptr, g ? nullptr : W.image.get(), U.work, stream) != 0))
      return -1;
    if (!g) return 0;
    const FilterIO f = {o.linear_out ? G.out.get() : nullptr, W.image, a.variance};
    return enqueue_guided(width, height, g, device_frame(filter_in, planes), f, G.work, stream);
  };
  if (!scene_checked(D, scene, stream, &T, pass)) {                // (a scene edited since the copy: uploaded and rendered again)
    if (history) history->valid = history->moments_valid = false;   // (the new history may be half written, the old one is not current)
    return -1;
  }
  if (history) {
    history->cur ^= 1;
    history->valid = true;
    history->moments_valid = s.vp != nullptr;                     // (rt_render_temporal leaves the moments behind)
    history->camera = scene->camera;
  }

  if (copy_image_out(image, W.image, width, height, stream) != 0) return -1;
  HIP_TRY(hipEventRecord(W.ev_frame[4], stream));
  if (o.linear_noisy) HIP_TRY(hipMemcpy(o.linear_noisy, W.linear, frame_pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (o.linear_upsampled) HIP_TRY(hipMemcpy(o.linear_upsampled, U.out, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (o.linear_out) HIP_TRY(hipMemcpy(o.linear_out, g ? G.out.get() : S.out.get(), pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (o.length) HIP_TRY(hipMemcpy(o.length, S.length, pixels * sizeof(float), hipMemcpyDeviceToHost));
  if (o.variance) HIP_TRY(hipMemcpy(o.variance, S.variance, pixels * sizeof(float), hipMemcpyDeviceToHost));
  return finish_frame(D, W, stream, T, t_start);
}

extern "C" int rt_render_denoised(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                                  RT_Guided_Params const *params, f32 *linear_noisy, f32 *linear_denoised) {
  return render_post("rt_render_denoised", DENOISED, scene, image, samples, max_bounces, {params}, {linear_noisy, linear_denoised});
}

extern "C" int rt_render_temporal(Scene const *scene, Image const *image, isize samples, isize max_bounces, RT_History *history,
                                  RT_Temporal_Params const *temporal_params, RT_Guided_Params const *guided_params, f32 *linear_noisy,
                                  f32 *linear_out, f32 *length) {
  return render_post("rt_render_temporal", ACCUMULATED, scene, image, samples, max_bounces, {guided_params, history, temporal_params},
                     {linear_noisy, linear_out, length});
}

extern "C" int rt_render_svgf(Scene const *scene, Image const *image, isize samples, isize max_bounces, RT_History *history,
                              RT_Temporal_Params const *temporal_params, RT_Variance_Params const *variance_params,
                              RT_Guided_Params const *guided_params, f32 *linear_noisy, f32 *linear_out, f32 *length, f32 *variance) {
  return render_post("rt_render_svgf", SVGF, scene, image, samples, max_bounces,
                     {guided_params, history, temporal_params, variance_params}, {linear_noisy, linear_out, length, variance});
}

extern "C" int rt_render_upsampled(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                                   RT_Upsample_Params const *upsample_params, RT_Guided_Params const *guided_params, f32 *linear_low,
                                   f32 *linear_upsampled, f32 *linear_out) {
  return render_post("rt_render_upsampled", UPSAMPLED, scene, image, samples, max_bounces,
                     {guided_params, nullptr, nullptr, nullptr, upsample_params}, {linear_low, linear_out, nullptr, nullptr, linear_upsampled});
}
