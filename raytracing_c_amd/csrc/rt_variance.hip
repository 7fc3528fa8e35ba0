// rt_variance.hip -- variance-guided denoising (include/rt_hip.h: rt_temporal_accumulate_moments, rt_guided_denoise_variance,
// rt_render_svgf): what SVGF (Schied et al. 2017) adds to the accumulation and the a-trous filter -- per-pixel luminance moments
// carried through the reprojection, a variance estimate from them, and a filter whose luminance term is measured in the pixel's
// own standard deviation.  The arithmetic is the contract of rt_hip.h ("THE MOMENTS", "THE VARIANCE", "THE VARIANCE-GUIDED FILTER"),
// operation by operation: f32 + - * / only, every operation rounded on its own (-ffp-contract=off), sums left to right, taps in a
// fixed order -- a float32 restatement on the CPU (tests/_variance.py) equals the result bit for bit.
//
// rt_temporal_moments_kernel: rt_temporal_kernel with the moments, ONE launch and ONE reprojection (rt_temporal_pixel.hip.h);
// rt_temporal_moments_motion_kernel: the same with the motion plane of a deforming mesh.
//
// rt_variance_kernel: one thread per pixel, a 32 x 8 tile per workgroup, a one-dimensional grid.  A pixel whose new history is at
// least 4 frames long takes the temporal variance from its own moments record.  Only a workgroup that has a shorter pixel stages
// the 3-pixel halo (38 x 14) in LDS -- the moments as float2, (N, coverage) and (W, 0) as float4: 21 280 B -- and those pixels
// estimate the variance from the 7 x 7 window; every other workgroup leaves after the per-pixel branch, which after the first
// frames of a sequence is nearly every one.  A row of the halo tile is 38 consecutive slots: the 16 lanes of a ds_read_b128 group
// lie in one row of the tile and read 16 consecutive 16-byte slots (all 64 banks once), the 32 lanes of a ds_read_b64 half read 32
// consecutive 8-byte slots (all 64 banks once), whatever the row pitch.
//
// rt_variance_filter_kernel: rt_guided_filter_kernel's decomposition (rt_guided_filter.hip.h) over the record (r, g, b, v).
//
// rt_moments_pack / rt_moments_unpack move moments between the float4 plane and the host-level call's f32[h][w][2].

#include "rt_guided_filter.hip.h"
#include "rt_temporal_pixel.hip.h"

#define VR_R  3                   // halo: the 7 x 7 window
#define VR_PX (TP_TX + 2 * VR_R)  // 38
#define VR_PY (TP_TY + 2 * VR_R)  // 14

__global__ __launch_bounds__(TP_TX * TP_TY) void rt_temporal_moments_kernel(RT_TParams P, const float *color, const float *coverage,
                                                                             const float *albedo, const float *normal,
                                                                             const float *position, const float4 *hist_in,
                                                                             float4 *hist_out, float *out, float *length, uint8_t *image,
                                                                             const float4 *mom_in, float4 *mom_out) {
  temporal_pixel<true>(P, color, coverage, albedo, normal, position, hist_in, hist_out, out, length, image, mom_in, mom_out);
}

// ... with the motion plane ("THE ACCUMULATION WITH MOTION"): the moments ride through the taps the motion chose
__global__ __launch_bounds__(TP_TX * TP_TY) void rt_temporal_moments_motion_kernel(RT_TParams P, const float *color, const float *coverage,
                                                                                    const float *albedo, const float *normal,
                                                                                    const float *position, const float *motion,
                                                                                    const float4 *hist_in, float4 *hist_out, float *out,
                                                                                    float *length, uint8_t *image, const float4 *mom_in,
                                                                                    float4 *mom_out) {
  temporal_pixel<true, true>(P, color, coverage, albedo, normal, position, hist_in, hist_out, out, length, image, mom_in, mom_out, motion);
}

// hist: the NEW history's three planes; mom: the NEW moments.  Block b is tile (b % tiles_x, b / tiles_x).
__global__ __launch_bounds__(TP_TX * TP_TY) void rt_variance_kernel(int width, int height, int tiles_x, float k_n, float k_p,
                                                                     const float4 *hist, const float4 *mom, float *variance) {
  __shared__ float2 s_m[VR_PY * VR_PX];       // (m1, m2)
  __shared__ float4 s_n[VR_PY * VR_PX];       // (N, coverage)
  __shared__ float4 s_w[VR_PY * VR_PX];       // (W, 0)
  const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * TP_TX, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * TP_TY;
  const int x = tx0 + (int)threadIdx.x, y = ty0 + (int)threadIdx.y;
  const bool in = x < width && y < height;
  const size_t pixels = (size_t)width * height;
  const size_t p = in ? (size_t)y * width + x : 0;
  float len = 0.0f, cov = 0.0f, var = 0.0f;
  if (in) {
    len = hist[p].w;
    cov = hist[pixels + p].w;
    const float4 m = mom[p];
    const float v = m.y - m.x * m.x;
    var = v > 0.0f ? v : 0.0f;                                                  // var_t
  }
  const bool spatial = in && cov != 0.0f && !(len >= 4.0f);
  if (!__syncthreads_or(spatial ? 1 : 0)) {                                     // no short history in this tile: no halo
    if (in) variance[p] = cov != 0.0f ? var : 0.0f;
    return;
  }
  const int tid = threadIdx.y * TP_TX + threadIdx.x;
  for (int i = tid; i < VR_PY * VR_PX; i += TP_TX * TP_TY) {
    const int xx = tx0 - VR_R + i % VR_PX, yy = ty0 - VR_R + i / VR_PX;
    float2 m = make_float2(0.0f, 0.0f);
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;                      // outside the image: coverage 0, which no tap counts
    if (xx >= 0 && xx < width && yy >= 0 && yy < height) {
      const size_t q = (size_t)yy * width + xx;
      const float4 mq = mom[q];
      m = make_float2(mq.x, mq.y);
      a = hist[pixels + q];
      b = hist[2 * pixels + q];
    }
    s_m[i] = m;
    s_n[i] = a;
    s_w[i] = b;
  }
  __syncthreads();
  if (!in) return;                                                              // (no barrier below)
  if (spatial) {
    const int centre = (threadIdx.y + VR_R) * VR_PX + threadIdx.x + VR_R;
    const float4 np = s_n[centre], wp = s_w[centre];
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    // (dy outer and rolled -- 49 unrolled taps cost 119 VGPRs and spilled SGPRs --, dx inner and unrolled)
#pragma unroll 1
    for (int dy = -VR_R; dy <= VR_R; dy++)
#pragma unroll
    for (int dx = -VR_R; dx <= VR_R; dx++) {
      const int slot = centre + dy * VR_PX + dx;
      const float4 nq = s_n[slot], wq = s_w[slot];
      const float2 mq = s_m[slot];
      const bool counts = nq.w != 0.0f;                                         // inside the image and on a surface
      const float dnx = np.x - nq.x, dny = np.y - nq.y, dnz = np.z - nq.z;
      const float dn2 = dnx * dnx + dny * dny + dnz * dnz;
      const float dcov = cov - nq.w;
      const float ex = wq.x - wp.x, ey = wq.y - wp.y, ez = wq.z - wp.z;
      const float pl = np.x * ex + np.y * ey + np.z * ez;
      const float D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p;
      const float r = 1.0f / (1.0f + D);
      const float wgt = r * r;
      sw = counts ? sw + wgt : sw;
      s1 = counts ? s1 + wgt * mq.x : s1;
      s2 = counts ? s2 + wgt * mq.y : s2;
    }
    const float e1 = s1 / sw, e2 = s2 / sw;                                     // (the centre counts with wgt = 1)
    float v = e2 - e1 * e1;
    v = v > 0.0f ? v : 0.0f;
    var = v * (4.0f / len);
  }
  variance[p] = cov != 0.0f ? var : 0.0f;
}

__global__ __launch_bounds__(256) void rt_variance_pack_kernel(int n_pixels, int demodulate, const float *color, const float *coverage,
                                                               const float *albedo, const float *normal, const float *position,
                                                               const float *variance, float4 *c0, float4 *g0, float4 *g1) {
  guided_pack_pixel<true>(n_pixels, demodulate, color, coverage, albedo, normal, position, variance, c0, g0, g1);
}

__global__ __launch_bounds__(GD_TX * GD_TY) void rt_variance_filter_kernel(int width, int height, int step, int phases_x, int phases_y,
                                                                           int tiles_x, float k_n, float k_p, float k_c, int last,
                                                                           int demodulate, const float4 *src, float4 *dst,
                                                                           const float4 *g0, const float4 *g1, const float *color,
                                                                           const float *albedo, float *out, uint8_t *image,
                                                                           float *var_out) {
  guided_filter_pixel<true>(width, height, step, phases_x, phases_y, tiles_x, k_n, k_p, k_c, last, demodulate, src, dst, g0, g1, color,
                            albedo, out, image, var_out);
}

// f32[n][2] -> the plane of float4 (m1, m2, 0, 0), and back
__global__ __launch_bounds__(256) void rt_moments_pack(int n_pixels, const float *planar, float4 *mom) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pixels) return;
  mom[p] = make_float4(planar[(size_t)p * 2], planar[(size_t)p * 2 + 1], 0.0f, 0.0f);
}

__global__ __launch_bounds__(256) void rt_moments_unpack(int n_pixels, const float4 *mom, float *planar) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pixels) return;
  const float4 m = mom[p];
  planar[(size_t)p * 2] = m.x;
  planar[(size_t)p * 2 + 1] = m.y;
}

extern "C" int rt_launch_temporal_moments(const RT_TParams *P, RT_Frame frame, const void *hist_in, void *hist_out, float *out,
                                          float *length, uint8_t *image, const void *mom_in, void *mom_out, hipStream_t stream) {
  // (as rt_launch_temporal: fewer than 2^26 blocks for the 2^28 pixels the host admits)
  const unsigned blocks = (unsigned)P->tiles_x * (unsigned)((P->height + TP_TY - 1) / TP_TY);
  hipLaunchKernelGGL(rt_temporal_moments_kernel, dim3(blocks), dim3(TP_TX, TP_TY), 0, stream, *P, frame.color, frame.coverage, frame.albedo,
                     frame.normal, frame.position, (const float4 *)hist_in, (float4 *)hist_out, out, length, image,
                     (const float4 *)mom_in, (float4 *)mom_out);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_temporal_moments_motion(const RT_TParams *P, RT_Frame frame, const float *motion, const void *hist_in,
                                                 void *hist_out, float *out, float *length, uint8_t *image, const void *mom_in,
                                                 void *mom_out, hipStream_t stream) {
  const unsigned blocks = (unsigned)P->tiles_x * (unsigned)((P->height + TP_TY - 1) / TP_TY);
  hipLaunchKernelGGL(rt_temporal_moments_motion_kernel, dim3(blocks), dim3(TP_TX, TP_TY), 0, stream, *P, frame.color, frame.coverage,
                     frame.albedo, frame.normal, frame.position, motion, (const float4 *)hist_in, (float4 *)hist_out, out, length, image,
                     (const float4 *)mom_in, (float4 *)mom_out);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_variance(int width, int height, float k_n, float k_p, const void *hist, const void *mom, float *variance,
                                  hipStream_t stream) {
  const int tiles_x = (width + TP_TX - 1) / TP_TX;
  const unsigned blocks = (unsigned)tiles_x * (unsigned)((height + TP_TY - 1) / TP_TY);
  hipLaunchKernelGGL(rt_variance_kernel, dim3(blocks), dim3(TP_TX, TP_TY), 0, stream, width, height, tiles_x, k_n, k_p,
                     (const float4 *)hist, (const float4 *)mom, variance);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_variance_pack(int n_pixels, int demodulate, RT_Frame frame, const float *variance, void *c0, void *g0, void *g1,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(rt_variance_pack_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, demodulate, frame.color,
                     frame.coverage, frame.albedo, frame.normal, frame.position, variance, (float4 *)c0, (float4 *)g0, (float4 *)g1);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_variance_filter(int width, int height, int step, float k_n, float k_p, float k_c, int last, int demodulate,
                                         const void *src, void *dst, const void *g0, const void *g1, RT_Frame frame, float *out,
                                         uint8_t *image, float *var_out, hipStream_t stream) {
  const GuidedGrid G = guided_grid(width, height, step);
  hipLaunchKernelGGL(rt_variance_filter_kernel, dim3(G.blocks), dim3(GD_TX, GD_TY), 0, stream, width, height, step, G.phases_x,
                     G.phases_y, G.tiles_x, k_n, k_p, k_c, last, demodulate, (const float4 *)src, (float4 *)dst, (const float4 *)g0,
                     (const float4 *)g1, frame.color, frame.albedo, out, image, var_out);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_moments_pack(int n_pixels, const float *planar, void *mom, hipStream_t stream) {
  hipLaunchKernelGGL(rt_moments_pack, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, planar, (float4 *)mom);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_moments_unpack(int n_pixels, const void *mom, float *planar, hipStream_t stream) {
  hipLaunchKernelGGL(rt_moments_unpack, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, (const float4 *)mom, planar);
  return (int)hipGetLastError();
}
