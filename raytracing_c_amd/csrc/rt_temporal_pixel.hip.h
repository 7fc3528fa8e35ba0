// rt_temporal_pixel.hip.h -- ONE pixel of temporal accumulation (include/rt_hip.h, "THE ACCUMULATION"): the projection into both
// cameras, the four taps, their validity tests and bilinear weights, the blend and the stores.  The ONE definition of the
// reprojection, shared by rt_temporal_kernel (rt_temporal.hip: MOMENTS = false) and rt_temporal_moments_kernel (rt_variance.hip:
// MOMENTS = true), which carries the first and second moment of the demodulated luminance through the same taps with the same
// weights ("THE MOMENTS") and writes the 16-byte moments record next to the history.  With MOMENTS = false nothing of the moments
// is compiled: rt_temporal_kernel pays nothing for them.  MOTION = true ("THE ACCUMULATION WITH MOTION": rt_temporal_motion_kernel,
// rt_temporal_moments_motion_kernel) reads one more plane, the mean motion of the pixel's first hits, projects where the surface
// point WAS into the previous camera and measures a tap's plane distance from there; with MOTION = false nothing of that is compiled
// either, and the two instances above are what they were.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_math.h"
#include "rt_device.h"

#define TP_TX 32
#define TP_TY 8

// what the colour is divided by before the accumulation and multiplied with after it (the guided filter's)
__device__ __forceinline__ float temporal_modulation(float albedo, float coverage) { return albedo + ((1.0f - coverage) + 1e-3f); }

// lum(c) of the contracts, left to right
__device__ __forceinline__ float temporal_luminance(float r, float g, float b) { return r * 0.2126f + g * 0.7152f + b * 0.0722f; }

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

// The pixel of thread (threadIdx.x, threadIdx.y) of block blockIdx.x.  mom_in / mom_out: planes of float4 (m1, m2, 0, 0), read and
// written only when MOMENTS; mom_in is given exactly when hist_in is.  motion: f32[h][w][3] as rt_resolve_motion writes it, read only
// when MOTION.
template <bool MOMENTS, bool MOTION = false>
__device__ __forceinline__ void temporal_pixel(const RT_TParams &P, const float *color, const float *coverage, const float *albedo,
                                               const float *normal, const float *position, const float4 *hist_in, float4 *hist_out,
                                               float *out, float *length, uint8_t *image, const float4 *mom_in, float4 *mom_out,
                                               const float *motion = nullptr) {
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
  float m1 = 0.0f, m2 = 0.0f;                                                   // sky: the moments record is (0, 0, 0, 0)
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
    if (MOMENTS) {
      m1 = temporal_luminance(c[0], c[1], c[2]);                                // L_p, S_p: what a pixel without usable history keeps
      m2 = m1 * m1;
    }
    const float wx = position[p3] / cov, wy = position[p3 + 1] / cov, wz = position[p3 + 2] / cov;
    float fxc, fyc, dc, fxv, fyv, dv;
    const bool front_c = temporal_project(P.cur, P.aspect, P.half_w, P.half_h, wx, wy, wz, fxc, fyc, dc);
    // V_p: where the mean surface point was (MOTION: W_p + M_p, M_p = motion_p / cov; otherwise W_p itself)
    float vx = wx, vy = wy, vz = wz;
    if (MOTION) {
      vx = wx + motion[p3] / cov;
      vy = wy + motion[p3 + 1] / cov;
      vz = wz + motion[p3 + 2] / cov;
    }
    const bool front_v = temporal_project(P.prev, P.aspect, P.half_w, P.half_h, vx, vy, vz, fxv, fyv, dv);
    const float hx = (float)x + (fxv - fxc), hy = (float)y + (fyv - fyc);
    // (every comparison is false for NaN)
    const bool usable = hist_in != nullptr && front_c && front_v && hx >= -1.0f && hx < (float)width && hy >= -1.0f && hy < (float)height;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
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
        const float ex = q2.x - vx, ey = q2.y - vy, ez = q2.z - vz;
        const float pl = nx * ex + ny * ey + nz * ez;                           // distance of the old point from p's tangent plane
        if (dn2 <= P.tn2 && pl * pl <= plane_bound) {
          sw = sw + b;
          sr = sr + b * q0.x;
          sg = sg + b * q0.y;
          sb = sb + b * q0.z;
          sn = sn + b * q0.w;
          if (MOMENTS) {
            const float4 qm = mom_in[q];                                        // (m1, m2, 0, 0)
            s1 = s1 + b * qm.x;
            s2 = s2 + b * qm.y;
          }
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
      if (MOMENTS) {
        const float g1 = s1 / sw, g2 = s2 / sw;
        m1 = g1 + (m1 - g1) * a;
        m2 = g2 + (m2 - g2) * a;
      }
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
  if (MOMENTS) mom_out[p] = make_float4(m1, m2, 0.0f, 0.0f);
  if (out) { out[p3] = o[0]; out[p3 + 1] = o[1]; out[p3 + 2] = o[2]; }
  if (length) length[p] = len;
  if (image) { image[p3] = rt_encode_u8(o[0]); image[p3 + 1] = rt_encode_u8(o[1]); image[p3 + 2] = rt_encode_u8(o[2]); }
}
