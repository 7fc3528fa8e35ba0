// rt_temporal.hip -- temporal accumulation (include/rt_hip.h: rt_temporal_accumulate): the frame's linear radiance blended with the
// history of the frames before it, fetched where the pixel's first hits WERE in the previous camera.  The arithmetic is the contract
// of rt_hip.h ("THE ACCUMULATION"), restated here operation by operation: f32 + - * / and floorf only, every operation rounded on
// its own (-ffp-contract=off), `/` the correctly rounded division, sums left to right, the four taps in one fixed order -- so a
// float32 restatement on the CPU (tests/_temporal.py) equals the result bit for bit.
//
// rt_temporal_kernel: one thread per pixel, a 32 x 8 tile per workgroup (a wave is two rows of 32 pixels).  A pixel reads its own
// 13 planar f32, projects the mean world position of its first hits into both cameras and gathers 2 x 2 history pixels, three float4
// records each (the history is three planes of float4: a tap is three 16-byte loads); neighbouring pixels move alike, so the taps
// of a tile fall on a tile-sized window of the old history and share its cache lines.  It writes the new history (48 B) and, when
// wanted, the modulated output, the history length and the u8 encoding.  Nothing is staged in LDS: every history record is used by
// at most four pixels, which the caches serve.
//
// rt_temporal_pack_history / rt_temporal_unpack_history move a history between the three float4 planes and the planar arrays of
// the host-level call (colour, length, coverage, N, W); they copy, they compute nothing.

#include "rt_temporal_pixel.hip.h"

// (the pixel itself -- projection, taps, validity tests, weights, blend, stores -- is rt_temporal_pixel.hip.h's, shared with the
// moments kernel of rt_variance.hip)
__global__ __launch_bounds__(TP_TX * TP_TY) void rt_temporal_kernel(RT_TParams P, const float *color, const float *coverage,
                                                                     const float *albedo, const float *normal, const float *position,
                                                                     const float4 *hist_in, float4 *hist_out, float *out, float *length,
                                                                     uint8_t *image) {
  temporal_pixel<false>(P, color, coverage, albedo, normal, position, hist_in, hist_out, out, length, image, nullptr, nullptr);
}

// ... with one more plane, the motion of the first hits (include/rt_hip.h, "THE ACCUMULATION WITH MOTION")
__global__ __launch_bounds__(TP_TX * TP_TY) void rt_temporal_motion_kernel(RT_TParams P, const float *color, const float *coverage,
                                                                            const float *albedo, const float *normal,
                                                                            const float *position, const float *motion,
                                                                            const float4 *hist_in, float4 *hist_out, float *out,
                                                                            float *length, uint8_t *image) {
  temporal_pixel<false, true>(P, color, coverage, albedo, normal, position, hist_in, hist_out, out, length, image, nullptr, nullptr, motion);
}

// planar (colour [n][3], length [n], coverage [n], N [n][3], W [n][3]) -> the three float4 planes
__global__ __launch_bounds__(256) void rt_temporal_pack_history(int n_pixels, const float *c, const float *len, const float *cov,
                                                                const float *n, const float *w, float4 *hist) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pixels) return;
  const size_t p3 = (size_t)p * 3;
  hist[p] = make_float4(c[p3], c[p3 + 1], c[p3 + 2], len[p]);
  hist[(size_t)n_pixels + p] = make_float4(n[p3], n[p3 + 1], n[p3 + 2], cov[p]);
  hist[2 * (size_t)n_pixels + p] = make_float4(w[p3], w[p3 + 1], w[p3 + 2], 0.0f);
}

__global__ __launch_bounds__(256) void rt_temporal_unpack_history(int n_pixels, const float4 *hist, float *c, float *len, float *cov,
                                                                  float *n, float *w) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pixels) return;
  const size_t p3 = (size_t)p * 3;
  const float4 h0 = hist[p], h1 = hist[(size_t)n_pixels + p], h2 = hist[2 * (size_t)n_pixels + p];
  c[p3] = h0.x; c[p3 + 1] = h0.y; c[p3 + 2] = h0.z;
  len[p] = h0.w;
  n[p3] = h1.x; n[p3 + 1] = h1.y; n[p3 + 2] = h1.z;
  cov[p] = h1.w;
  w[p3] = h2.x; w[p3 + 1] = h2.y; w[p3 + 2] = h2.z;
}

extern "C" int rt_launch_temporal(const RT_TParams *P, RT_Frame frame, const void *hist_in, void *hist_out, float *out, float *length,
                                  uint8_t *image, hipStream_t stream) {
  // tiles_x * tiles_y <= pixels / 256 + width / 32 + height / 8 + 1 < 2^26 for the 2^28 pixels the host admits
  const unsigned blocks = (unsigned)P->tiles_x * (unsigned)((P->height + TP_TY - 1) / TP_TY);
  hipLaunchKernelGGL(rt_temporal_kernel, dim3(blocks), dim3(TP_TX, TP_TY), 0, stream, *P, frame.color, frame.coverage, frame.albedo, frame.normal,
                     frame.position, (const float4 *)hist_in, (float4 *)hist_out, out, length, image);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_temporal_motion(const RT_TParams *P, RT_Frame frame, const float *motion, const void *hist_in, void *hist_out,
                                         float *out, float *length, uint8_t *image, hipStream_t stream) {
  const unsigned blocks = (unsigned)P->tiles_x * (unsigned)((P->height + TP_TY - 1) / TP_TY);
  hipLaunchKernelGGL(rt_temporal_motion_kernel, dim3(blocks), dim3(TP_TX, TP_TY), 0, stream, *P, frame.color, frame.coverage, frame.albedo,
                     frame.normal, frame.position, motion, (const float4 *)hist_in, (float4 *)hist_out, out, length, image);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_temporal_pack(int n_pixels, const float *c, const float *len, const float *cov, const float *n, const float *w,
                                       void *hist, hipStream_t stream) {
  hipLaunchKernelGGL(rt_temporal_pack_history, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, c, len, cov, n, w,
                     (float4 *)hist);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_temporal_unpack(int n_pixels, const void *hist, float *c, float *len, float *cov, float *n, float *w,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(rt_temporal_unpack_history, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, (const float4 *)hist, c,
                     len, cov, n, w);
  return (int)hipGetLastError();
}
