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

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_math.h"
#include "rt_device.h"

#define TP_TX 32
#define TP_TY 8

// what the colour is divided by before the accumulation and multiplied with after it (the guided filter's)
__device__ __forceinline__ float temporal_modulation(float albedo, float coverage) { return albedo + ((1.0f - coverage) + 1e-3f); }

// proj(cam, W) of the contract: front, the continuous pixel coordinates (fx, fy) and the depth d
__device__ __forceinline__ bool temporal_project(const RT_TCamera &c, float aspect, float half_w, float half_h, float wx, float wy,
                                                 float wz, float &fx, float &fy, float &d) {
  const float ex = wx - c.t[0], ey = wy - c.t[1], ez = wz - c.t[2];
  const float cx = c.r[0][0] * ex + c.r[1][0] * ey + c.r[2][0] * ez;
  const float cy = c.r[0][1] * ex + c.r[1][1] * ey + c.r[2][1] * ez;
  const float cz = c.r[0][2] * ex + c.r[1][2] * ey + c.r[2][2] * ez;
  d = 0.0f - cz;
  const float ux = ((cx * c.focal_length) / d) / aspect;
  const float uy = 0.0f - ((cy * c.focal_length) / d);
  fx = (ux + 1.0f) * half_w;
  fy = (uy + 1.0f) * half_h;
  return cz < 0.0f;
}

__global__ __launch_bounds__(TP_TX * TP_TY) void rt_temporal_kernel(RT_TParams P, const float *color, const float *coverage,
                                                                     const float *albedo, const float *normal, const float *position,
                                                                     const float4 *hist_in, float4 *hist_out, float *out, float *length,
                                                                     uint8_t *image) {
  // (a one-dimensional grid: an image of one column may be 2^28 rows high)
  const int tile_x = (int)(blockIdx.x % (unsigned)P.tiles_x), tile_y = (int)(blockIdx.x / (unsigned)P.tiles_x);
  const int x = tile_x * TP_TX + (int)threadIdx.x, y = tile_y * TP_TY + (int)threadIdx.y;
  const int width = P.width, height = P.height;
  if (x >= width || y >= height) return;
  const size_t pixels = (size_t)width * height;
  const size_t p = (size_t)y * width + x, p3 = p * 3;
  const float cov = coverage[p];
  const float col[3] = {color[p3], color[p3 + 1], color[p3 + 2]};
  float4 h0, h1, h2;
  float o[3], len;
  if (cov == 0.0f) {                                                            // sky: the input, bit for bit; no guides
    h0 = make_float4(col[0], col[1], col[2], 0.0f);
    h1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    h2 = h1;
    o[0] = col[0]; o[1] = col[1]; o[2] = col[2];
    len = 0.0f;
  } else {
    const float nx = normal[p3] * 2.0f - cov, ny = normal[p3 + 1] * 2.0f - cov, nz = normal[p3 + 2] * 2.0f - cov;
    float m[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      m[k] = P.demodulate ? temporal_modulation(albedo[p3 + k], cov) : 1.0f;
      c[k] = P.demodulate ? col[k] / m[k] : col[k];
    }
    const float wx = position[p3] / cov, wy = position[p3 + 1] / cov, wz = position[p3 + 2] / cov;
    float fxc, fyc, dc, fxv, fyv, dv;
    const bool front_c = temporal_project(P.cur, P.aspect, P.half_w, P.half_h, wx, wy, wz, fxc, fyc, dc);
    const bool front_v = temporal_project(P.prev, P.aspect, P.half_w, P.half_h, wx, wy, wz, fxv, fyv, dv);
    const float hx = (float)x + (fxv - fxc), hy = (float)y + (fyv - fyc);
    // (every comparison is false for NaN)
    const bool usable = hist_in != nullptr && front_c && front_v && hx >= -1.0f && hx < (float)width && hy >= -1.0f && hy < (float)height;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
    if (usable) {
      const int x0 = (int)floorf(hx), y0 = (int)floorf(hy);                      // -1 .. width - 1, -1 .. height - 1
      const float ax = hx - (float)x0, ay = hy - (float)y0;
      const float bx[2] = {1.0f - ax, ax}, by[2] = {1.0f - ay, ay};
      const float plane_bound = (P.tp2 * dv) * dv;
#pragma unroll
      for (int k = 0; k < 4; k++) {                                             // (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
        const int xq = x0 + (k & 1), yq = y0 + (k >> 1);
        if (xq < 0 || xq >= width || yq < 0 || yq >= height) continue;          // a tap outside the image is not valid
        const size_t q = (size_t)yq * width + xq;
        const float4 q1 = hist_in[pixels + q];                                  // (N, coverage)
        if (!(q1.w > 0.0f)) continue;
        const float4 q0 = hist_in[q], q2 = hist_in[2 * pixels + q];             // (c, len), (W, 0)
        const float b = bx[k & 1] * by[k >> 1];
        const float dnx = nx - q1.x, dny = ny - q1.y, dnz = nz - q1.z;
        const float dn2 = dnx * dnx + dny * dny + dnz * dnz;
        const float ex = q2.x - wx, ey = q2.y - wy, ez = q2.z - wz;
        const float pl = nx * ex + ny * ey + nz * ez;                           // distance of the old point from p's tangent plane
        if (dn2 <= P.tn2 && pl * pl <= plane_bound) {
          sw = sw + b;
          sr = sr + b * q0.x;
          sg = sg + b * q0.y;
          sb = sb + b * q0.z;
          sn = sn + b * q0.w;
        }
      }
    }
    len = 1.0f;
    if (usable && sw > 0.0f) {
      const float hn = sn / sw;
      const float n = hn < P.max_history ? hn : P.max_history;
      float a = 1.0f / (n + 1.0f);
      if (a < P.alpha) a = P.alpha;
      const float hc[3] = {sr / sw, sg / sw, sb / sw};
#pragma unroll
      for (int k = 0; k < 3; k++) c[k] = hc[k] + (c[k] - hc[k]) * a;
      len = n + 1.0f;
    }
    h0 = make_float4(c[0], c[1], c[2], len);
    h1 = make_float4(nx, ny, nz, cov);
    h2 = make_float4(wx, wy, wz, 0.0f);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = P.demodulate ? c[k] * m[k] : c[k];
  }
  hist_out[p] = h0;
  hist_out[pixels + p] = h1;
  hist_out[2 * pixels + p] = h2;
  if (out) { out[p3] = o[0]; out[p3 + 1] = o[1]; out[p3 + 2] = o[2]; }
  if (length) length[p] = len;
  if (image) { image[p3] = rt_encode_u8(o[0]); image[p3 + 1] = rt_encode_u8(o[1]); image[p3 + 2] = rt_encode_u8(o[2]); }
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

extern "C" int rt_launch_temporal(const RT_TParams *P, const float *color, const float *coverage, const float *albedo,
                                  const float *normal, const float *position, const void *hist_in, void *hist_out, float *out,
                                  float *length, uint8_t *image, hipStream_t stream) {
  // tiles_x * tiles_y <= pixels / 256 + width / 32 + height / 8 + 1 < 2^26 for the 2^28 pixels the host admits
  const unsigned blocks = (unsigned)P->tiles_x * (unsigned)((P->height + TP_TY - 1) / TP_TY);
  hipLaunchKernelGGL(rt_temporal_kernel, dim3(blocks), dim3(TP_TX, TP_TY), 0, stream, *P, color, coverage, albedo, normal, position,
                     (const float4 *)hist_in, (float4 *)hist_out, out, length, image);
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
