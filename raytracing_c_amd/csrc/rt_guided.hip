// rt_guided.hip -- the guided denoiser (include/rt_hip.h: rt_guided_denoise): an edge-stopping a-trous filter (Dammertz et al.
// 2010) of the linear frame, steered by the first-hit feature buffers (rt_features.hip): coverage, albedo, shading normal and
// world position.  The arithmetic is the contract of rt_hip.h, restated here operation by operation: f32 + - * / only, every
// operation rounded on its own (-ffp-contract=off), `/` the correctly rounded division, the 25 taps in one fixed order -- so a
// float32 restatement on the CPU (tests/_guided.py) equals the result bit for bit.
//
// Two kernels.  rt_guided_pack_kernel turns the planar inputs into float4 records in the caller's work buffer, once: the
// demodulated colour with its luminance (r, g, b, L), and the guides (N, coverage) and (P, 0), N = normal * 2 - coverage = the mean
// unit normal over the samples that hit.  rt_guided_filter_kernel is ONE iteration, launched once per step s = 1, 2, 4, ...: the
// step-s filter couples only pixels of one phase sub-lattice (x = px + s u, y = py + s v), and on that sub-lattice it is a dense
// 5 x 5 -- so a workgroup filters a 32 x 8 tile of ONE sub-lattice with a 2-pixel halo, whatever the step.  The (36 x 12) halo tile
// is staged in LDS as three float4 planes (20.25 KB); a row is 36 consecutive 16-byte slots, so the lanes of a wave's two rows sit on
// consecutive slots and every ds_read_b128 group of 16 lanes covers 16 distinct slots.  Blocks are numbered with the phase fastest:
// the workgroups that share cache lines at s >= 2 (neighbouring phases of one tile) run next to each other.  The colour ping-pongs
// between two buffers of the work area; the last iteration's launch multiplies the albedo back, keeps sky pixels and stores f32
// and / or u8.  64 B per pixel and iteration are read at least (three records in, one out).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_math.h"

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

__global__ __launch_bounds__(256) void rt_guided_pack_kernel(int n_pixels, int demodulate, const float *color, const float *coverage,
                                                             const float *albedo, const float *normal, const float *position,
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
  c0[p] = make_float4(c[0], c[1], c[2], guided_luminance(c[0], c[1], c[2]));
  g0[p] = make_float4(normal[p3] * 2.0f - cov, normal[p3 + 1] * 2.0f - cov, normal[p3 + 2] * 2.0f - cov, cov);
  g1[p] = make_float4(position[p3], position[p3 + 1], position[p3 + 2], 0.0f);
}

// One iteration with step `step`.  Block b: phase b % (phases_x * phases_y) -- phases_x = min(step, width), so every phase has a
// pixel -- and tile b / (phases_x * phases_y) of that phase's sub-lattice.  last: `dst` is not written; out / image are.
__global__ __launch_bounds__(GD_TX * GD_TY) void rt_guided_filter_kernel(int width, int height, int step, int phases_x, int phases_y,
                                                                         int tiles_x, float k_n, float k_p, float k_c, int last,
                                                                         int demodulate, const float4 *src, float4 *dst,
                                                                         const float4 *g0, const float4 *g1, const float *color,
                                                                         const float *albedo, float *out, uint8_t *image) {
  __shared__ float4 s_c[GD_PY * GD_PX];       // (r, g, b, L)
  __shared__ float4 s_g0[GD_PY * GD_PX];      // (N, coverage)
  __shared__ float4 s_g1[GD_PY * GD_PX];      // (P, 0)
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
  }
  __syncthreads();
  const int x = px + step * (u0 + (int)threadIdx.x), y = py + step * (v0 + (int)threadIdx.y);
  if (x >= width || y >= height) return;                                        // (no barrier below)

  const int centre = (threadIdx.y + GD_R) * GD_PX + threadIdx.x + GD_R;
  const float4 cp = s_c[centre], np = s_g0[centre], pp = s_g1[centre];
  const float cov = np.w;
  float4 res = cp;                                                              // a sky pixel keeps its colour
  if (cov != 0.0f) {
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
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
      const float dl = cp.w - cq.w;
      const float D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p + dl * dl * k_c;
      const float r = 1.0f / (1.0f + D);
      const float wgt = ((guided_tap(dy) * guided_tap(dx)) * r) * r;
      sr = valid ? sr + wgt * cq.x : sr;
      sg = valid ? sg + wgt * cq.y : sg;
      sb = valid ? sb + wgt * cq.z : sb;
      sw = valid ? sw + wgt : sw;
    }
    res.x = sr / sw;                                                            // (the centre tap alone has wgt = 0.140625)
    res.y = sg / sw;
    res.z = sb / sw;
    res.w = guided_luminance(res.x, res.y, res.z);
  }
  const size_t p = (size_t)y * width + x;
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
}

extern "C" int rt_launch_guided_pack(int n_pixels, int demodulate, const float *color, const float *coverage, const float *albedo,
                                     const float *normal, const float *position, void *c0, void *g0, void *g1, hipStream_t stream) {
  hipLaunchKernelGGL(rt_guided_pack_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, demodulate, color, coverage,
                     albedo, normal, position, (float4 *)c0, (float4 *)g0, (float4 *)g1);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_guided_filter(int width, int height, int step, float k_n, float k_p, float k_c, int last, int demodulate,
                                       const void *src, void *dst, const void *g0, const void *g1, const float *color,
                                       const float *albedo, float *out, uint8_t *image, hipStream_t stream) {
  const int phases_x = step < width ? step : width, phases_y = step < height ? step : height;
  const int sub_x = (width + step - 1) / step, sub_y = (height + step - 1) / step;        // the largest sub-lattice (phase 0, 0)
  const int tiles_x = (sub_x + GD_TX - 1) / GD_TX, tiles_y = (sub_y + GD_TY - 1) / GD_TY;
  // (phases x tiles x 256 threads cover every pixel once and no phase is empty: fewer than 4 x width x height <= 2^30 blocks)
  const unsigned blocks = (unsigned)phases_x * phases_y * tiles_x * tiles_y;
  hipLaunchKernelGGL(rt_guided_filter_kernel, dim3(blocks), dim3(GD_TX, GD_TY), 0, stream, width, height, step, phases_x, phases_y,
                     tiles_x, k_n, k_p, k_c, last, demodulate, (const float4 *)src, (float4 *)dst, (const float4 *)g0,
                     (const float4 *)g1, color, albedo, out, image);
  return (int)hipGetLastError();
}
