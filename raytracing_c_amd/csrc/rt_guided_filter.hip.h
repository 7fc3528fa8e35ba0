// rt_guided_filter.hip.h -- ONE iteration of the a-trous filter for ONE pixel of a workgroup's tile (include/rt_hip.h, "THE FILTER"
// and "THE VARIANCE-GUIDED FILTER"): the ONE definition of the decomposition -- a 32 x 8 tile of one phase sub-lattice, the strided
// fill of its (36 x 12) halo tile in LDS, the phase-fastest block numbering over min(s, w) x min(s, h) phases -- and of the 25 taps,
// shared by rt_guided_filter_kernel (rt_guided.hip: VARIANCE = false) and rt_variance_filter_kernel (rt_variance.hip: VARIANCE =
// true).
//
// VARIANCE = false: the colour record is (r, g, b, L) and the luminance term of D is dl * dl * k_c, k_c the iteration's.
// VARIANCE = true: the colour record is (r, g, b, v), v the variance of the demodulated luminance.  L is computed when the halo is
// filled and kept in a fourth LDS plane of f32 (a row is 36 consecutive dwords: a wave's two rows of 32 lanes read 32 consecutive
// banks each); the luminance term is (dl * dl) * kv_p, kv_p = k_c / (g_p + 1e-8f), g_p the 3 x 3 Gaussian of v at UNIT spacing --
// its eight neighbours are read from `src` (the launch's read-only ping-pong buffer): for a step >= 2 they lie in other phases and
// not in the tile; and v is filtered with the squared weights.  Nothing of this is compiled with VARIANCE = false.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_math.h"
#include "rt_device.h"

#define GD_TX 32                  // pixels of a sub-lattice per workgroup tile: 32 x 8, one thread each
#define GD_TY 8
#define GD_R  2                   // halo: the 5 x 5 taps
#define GD_PX (GD_TX + 2 * GD_R)  // 36
#define GD_PY (GD_TY + 2 * GD_R)  // 12

__device__ __forceinline__ float guided_luminance(float r, float g, float b) { return r * 0.2126f + g * 0.7152f + b * 0.0722f; }
// H[|d|] of the B-spline kernel, H = {0.375, 0.25, 0.0625}
__device__ __forceinline__ float guided_tap(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1 ? 0.25f : 0.0625f); }
// what the colour is divided by before the filter and multiplied with after it
__device__ __forceinline__ float guided_modulation(float albedo, float coverage) { return albedo + ((1.0f - coverage) + 1e-3f); }

// The planar inputs of pixel blockIdx.x * 256 + threadIdx.x as float4 records: the demodulated colour with its luminance (r, g, b, L)
// -- with VARIANCE: with the pixel's variance, (r, g, b, v) -- and the guides (N, coverage) and (P, 0).
template <bool VARIANCE>
__device__ __forceinline__ void guided_pack_pixel(int n_pixels, int demodulate, const float *color, const float *coverage,
                                                  const float *albedo, const float *normal, const float *position, const float *variance,
                                                  float4 *c0, float4 *g0, float4 *g1) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pixels) return;
  const size_t p3 = (size_t)p * 3;
  const float cov = coverage[p];
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float m = demodulate ? guided_modulation(albedo[p3 + k], cov) : 1.0f;
    c[k] = color[p3 + k] / m;
  }
  c0[p] = make_float4(c[0], c[1], c[2], VARIANCE ? variance[p] : guided_luminance(c[0], c[1], c[2]));
  g0[p] = make_float4(normal[p3] * 2.0f - cov, normal[p3 + 1] * 2.0f - cov, normal[p3 + 2] * 2.0f - cov, cov);
  g1[p] = make_float4(position[p3], position[p3 + 1], position[p3 + 2], 0.0f);
}

// The launch's grid: phases x tiles x 256 threads cover every pixel once and no phase is empty (fewer than 4 x width x height
// <= 2^30 blocks).
struct GuidedGrid {
  int phases_x, phases_y, tiles_x;
  unsigned blocks;
};
static inline GuidedGrid guided_grid(int width, int height, int step) {
  GuidedGrid g;
  g.phases_x = step < width ? step : width;
  g.phases_y = step < height ? step : height;
  const int sub_x = (width + step - 1) / step, sub_y = (height + step - 1) / step;        // the largest sub-lattice (phase 0, 0)
  g.tiles_x = (sub_x + GD_TX - 1) / GD_TX;
  const int tiles_y = (sub_y + GD_TY - 1) / GD_TY;
  g.blocks = (unsigned)g.phases_x * g.phases_y * g.tiles_x * tiles_y;
  return g;
}

// One iteration with step `step`.  Block b: phase b % (phases_x * phases_y) -- phases_x = min(step, width), so every phase has a
// pixel -- and tile b / (phases_x * phases_y) of that phase's sub-lattice.  last: `dst` is not written; out / image (and, with
// VARIANCE, var_out) are.
template <bool VARIANCE>
__device__ __forceinline__ void guided_filter_pixel(int width, int height, int step, int phases_x, int phases_y, int tiles_x, float k_n,
                                                    float k_p, float k_c, int last, int demodulate, const float4 *src, float4 *dst,
                                                    const float4 *g0, const float4 *g1, const float *color, const float *albedo,
                                                    float *out, uint8_t *image, float *var_out) {
  __shared__ float4 s_c[GD_PY * GD_PX];       // (r, g, b, L) or (r, g, b, v)
  __shared__ float4 s_g0[GD_PY * GD_PX];      // (N, coverage)
  __shared__ float4 s_g1[GD_PY * GD_PX];      // (P, 0)
  __shared__ float s_l[VARIANCE ? GD_PY * GD_PX : 1];   // L, when the record carries v
  const int n_phases = phases_x * phases_y;
  const int phase = (int)(blockIdx.x % (unsigned)n_phases), tile = (int)(blockIdx.x / (unsigned)n_phases);
  const int px = phase % phases_x, py = phase / phases_x;
  const int u0 = (tile % tiles_x) * GD_TX, v0 = (tile / tiles_x) * GD_TY;      // the tile's origin on the sub-lattice
  const int tid = threadIdx.y * GD_TX + threadIdx.x;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int i = tid; i < GD_PY * GD_PX; i += GD_TX * GD_TY) {
    const int xx = px + step * (u0 - GD_R + i % GD_PX), yy = py + step * (v0 - GD_R + i / GD_PX);
    const bool in = xx >= 0 && xx < width && yy >= 0 && yy < height;           // (a slot outside the image is never used: zeros)
    const size_t q = (size_t)yy * width + xx;
    float4 c = zero, a = zero, b = zero;
    if (in) { c = src[q]; a = g0[q]; b = g1[q]; }
    s_c[i] = c;
    s_g0[i] = a;
    s_g1[i] = b;
    if (VARIANCE) s_l[i] = guided_luminance(c.x, c.y, c.z);
  }
  __syncthreads();
  const int x = px + step * (u0 + (int)threadIdx.x), y = py + step * (v0 + (int)threadIdx.y);
  if (x >= width || y >= height) return;                                        // (no barrier below)

  const int centre = (threadIdx.y + GD_R) * GD_PX + threadIdx.x + GD_R;
  const float4 cp = s_c[centre], np = s_g0[centre], pp = s_g1[centre];
  const float cov = np.w;
  const size_t p = (size_t)y * width + x;
  float4 res = cp;                                                              // a sky pixel keeps its colour (and its variance)
  if (cov != 0.0f) {
    float lp = cp.w, kc = k_c;
    if (VARIANCE) {
      lp = s_l[centre];
      float gs = 0.0f, gw = 0.0f;
#pragma unroll
      for (int t = 0; t < 9; t++) {                                             // dy outer, dx inner, at unit spacing
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        const int xq = x + dx, yq = y + dy;
        if (xq < 0 || xq >= width || yq < 0 || yq >= height) continue;          // a tap outside the image is skipped
        const float g = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
        const float vq = (dy == 0 && dx == 0) ? cp.w : src[(size_t)yq * width + xq].w;
        gs = gs + g * vq;
        gw = gw + g;
      }
      kc = k_c / (gs / gw + 1e-8f);                                             // kv_p
    }
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
#pragma unroll
    for (int t = 0; t < 25; t++) {                                              // dy outer, dx inner
      const int dy = t / 5 - 2, dx = t % 5 - 2;
      const int xq = x + step * dx, yq = y + step * dy;
      const bool valid = xq >= 0 && xq < width && yq >= 0 && yq < height;       // a tap outside the image is skipped, not clamped
      const int slot = centre + dy * GD_PX + dx;
      const float4 cq = s_c[slot], nq = s_g0[slot], pq = s_g1[slot];
      const float dnx = np.x - nq.x, dny = np.y - nq.y, dnz = np.z - nq.z;
      const float dn2 = dnx * dnx + dny * dny + dnz * dnz;
      const float dcov = cov - nq.w;
      const float ex = pq.x - pp.x, ey = pq.y - pp.y, ez = pq.z - pp.z;
      const float pl = np.x * ex + np.y * ey + np.z * ez;                       // distance of q from p's tangent plane
      const float dl = lp - (VARIANCE ? s_l[slot] : cq.w);
      const float D = VARIANCE ? dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p + (dl * dl) * kc
                               : dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p + dl * dl * kc;
      const float r = 1.0f / (1.0f + D);
      const float wgt = ((guided_tap(dy) * guided_tap(dx)) * r) * r;
      sr = valid ? sr + wgt * cq.x : sr;
      sg = valid ? sg + wgt * cq.y : sg;
      sb = valid ? sb + wgt * cq.z : sb;
      sw = valid ? sw + wgt : sw;
      if (VARIANCE) sv = valid ? sv + (wgt * wgt) * cq.w : sv;
    }
    res.x = sr / sw;                                                            // (the centre tap alone has wgt = 0.140625)
    res.y = sg / sw;
    res.z = sb / sw;
    res.w = VARIANCE ? sv / (sw * sw) : guided_luminance(res.x, res.y, res.z);
  }
  if (!last) {
    dst[p] = res;
    return;
  }
  auto put = [&](int k, float c) {
    const float m = demodulate ? guided_modulation(albedo[p * 3 + k], cov) : 1.0f;
    const float o = cov != 0.0f ? c * m : color[p * 3 + k];                     // sky: the input, bit for bit
    if (out) out[p * 3 + k] = o;
    if (image) image[p * 3 + k] = rt_encode_u8(o);
  };
  put(0, res.x);
  put(1, res.y);
  put(2, res.z);
  if (VARIANCE && var_out) var_out[p] = res.w;
}
