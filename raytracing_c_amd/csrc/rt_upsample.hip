// rt_upsample.hip -- feature-guided upsampling of a half-resolution frame to full size (include/rt_hip.h: rt_guided_upsample, "THE
// UPSAMPLING"): the demodulated colour of a frame traced at (W / 2) x (H / 2) is interpolated to W x H by a separable quadratic
// B-spline on the low lattice whose taps are weighed by how well the low pixel's first hit agrees with the full pixel's -- normal,
// coverage, distance from the tangent plane, the guided filter's three geometric terms -- and multiplied with the FULL-resolution
// albedo.  The arithmetic is the contract of rt_hip.h, restated here operation by operation: f32 + - * / only, every operation
// rounded on its own (-ffp-contract=off), `/` the correctly rounded division, the taps in one fixed order -- so a float32
// restatement on the CPU (tests/_upsample.py) equals the result bit for bit.
//
// One kernel.  The low frame arrives as the float4 records rt_guided_pack_kernel (rt_guided.hip) writes for a frame of the low
// size -- (c, L), (N, coverage), (P, 0); L is not read --, so the division c = color / m and N = normal * 2 - coverage are done once
// per low pixel and not once per tap.  A workgroup writes a 16 x 8 tile of full pixels, one thread each.  Their taps lie in the
// 8 x 4 low pixels under the tile and a halo of ONE low pixel around them: the (10 x 6) records are staged in LDS as three float4
// planes (2880 B); every low record is read from memory by one thread of a workgroup and from LDS by up to nine.  The
// full-resolution planes are read once per pixel, by the pixel's own thread: 40 B with the albedo, 28 B without; 12 B and / or
// 3 B are written.
//
// The taps along x of full pixel x, X0 = x >> 1: the contract names X0 - 1 + (x & 1) + i, i = 0, 1, 2, with the weights {0.125, 0.75,
// 0.125} for even x and {0.5, 0.5, 0} for odd x.  The kernel reads X0 - 1 + i for both parities with {0.125, 0.75, 0.125} and {0,
// 0.5, 0.5}: the same taps with the same weights in the same order -- a tap with weight 0 is skipped either way -- and no slot
// beyond the halo.  Likewise along y.

#include "rt_guided_filter.hip.h"

#define UP_TX 16                  // full pixels per workgroup tile: 16 x 8, one thread each
#define UP_TY 8
#define UP_LX (UP_TX / 2 + 2)     // 10: the low pixels under the tile and one more on either side
#define UP_LY (UP_TY / 2 + 2)     // 6

// the weight of slot X0 - 1 + i (Y0 - 1 + j) for a full pixel of parity `odd`
__device__ __forceinline__ float upsample_tap(int odd, int i) {
  return odd ? (i == 0 ? 0.0f : 0.5f) : (i == 1 ? 0.75f : 0.125f);
}

// Block b: tile (b % tiles_x, b / tiles_x).  width and height are even; c0, g0, g1 hold (width / 2) x (height / 2) records.
__global__ __launch_bounds__(UP_TX * UP_TY) void rt_upsample_kernel(int width, int height, int tiles_x, float k_n, float k_p,
                                                                    int demodulate, const float4 *c0, const float4 *g0,
                                                                    const float4 *g1, const float *coverage, const float *albedo,
                                                                    const float *normal, const float *position, float *out,
                                                                    uint8_t *image) {
  __shared__ float4 s_c[UP_LY * UP_LX];       // (c, L)
  __shared__ float4 s_g0[UP_LY * UP_LX];      // (N, coverage)
  __shared__ float4 s_g1[UP_LY * UP_LX];      // (P, 0)
  const int wl = width >> 1, hl = height >> 1;
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
  const int lx0 = tx * (UP_TX / 2) - 1, ly0 = ty * (UP_TY / 2) - 1;             // the low pixel of slot (0, 0)
  const int tid = threadIdx.y * UP_TX + threadIdx.x;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int i = tid; i < UP_LY * UP_LX; i += UP_TX * UP_TY) {
    const int X = lx0 + i % UP_LX, Y = ly0 + i / UP_LX;
    const bool in = X >= 0 && X < wl && Y >= 0 && Y < hl;                       // (a slot outside the low image is never used: zeros)
    const size_t q = (size_t)Y * wl + X;
    float4 c = zero, a = zero, b = zero;
    if (in) { c = c0[q]; a = g0[q]; b = g1[q]; }
    s_c[i] = c;
    s_g0[i] = a;
    s_g1[i] = b;
  }
  __syncthreads();
  const int x = tx * UP_TX + (int)threadIdx.x, y = ty * UP_TY + (int)threadIdx.y;
  if (x >= width || y >= height) return;                                        // (no barrier below)

  const size_t p = (size_t)y * width + x, p3 = p * 3;
  const float cov = coverage[p];
  const float npx = normal[p3] * 2.0f - cov, npy = normal[p3 + 1] * 2.0f - cov, npz = normal[p3 + 2] * 2.0f - cov;
  const float ppx = position[p3], ppy = position[p3 + 1], ppz = position[p3 + 2];
  const int ox = x & 1, oy = y & 1;
  const int corner = ((int)threadIdx.y >> 1) * UP_LX + ((int)threadIdx.x >> 1);  // slot of low pixel (X0 - 1, Y0 - 1)
  const int X0 = x >> 1, Y0 = y >> 1;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll
  for (int t = 0; t < 9; t++) {                                                 // j outer, i inner
    const int j = t / 3, i = t % 3;
    const int X = X0 - 1 + i, Y = Y0 - 1 + j;
    const float hy = upsample_tap(oy, j), hx = upsample_tap(ox, i);
    // a tap with a zero spline weight is skipped; a tap outside the low image is skipped, not clamped
    const bool valid = hy != 0.0f && hx != 0.0f && X >= 0 && X < wl && Y >= 0 && Y < hl;
    const int slot = corner + j * UP_LX + i;
    const float4 cq = s_c[slot], nq = s_g0[slot], pq = s_g1[slot];
    const float dnx = npx - nq.x, dny = npy - nq.y, dnz = npz - nq.z;
    const float dn2 = dnx * dnx + dny * dny + dnz * dnz;
    const float dcov = cov - nq.w;
    const float ex = pq.x - ppx, ey = pq.y - ppy, ez = pq.z - ppz;
    const float pl = npx * ex + npy * ey + npz * ez;                            // distance of q from p's tangent plane
    const float D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p;
    const float r = 1.0f / (1.0f + D);
    const float wgt = ((hy * hx) * r) * r;
    sr = valid ? sr + wgt * cq.x : sr;
    sg = valid ? sg + wgt * cq.y : sg;
    sb = valid ? sb + wgt * cq.z : sb;
    sw = valid ? sw + wgt : sw;
  }
  // (sum_w > 0 fails when pl * pl overflows for every tap -- r = 0, or NaN with k_p = 0 --: the pixel takes the low pixel under it)
  const float4 under = s_c[corner + UP_LX + 1];                                 // low pixel (X0, Y0): always inside the low image
  const bool summed = sw > 0.0f;
  const float cr = summed ? sr / sw : under.x, cg = summed ? sg / sw : under.y, cb = summed ? sb / sw : under.z;
  auto put = [&](int k, float c) {
    const float m = demodulate ? guided_modulation(albedo[p3 + k], cov) : 1.0f;
    const float o = c * m;
    if (out) out[p3 + k] = o;
    if (image) image[p3 + k] = rt_encode_u8(o);
  };
  put(0, cr);
  put(1, cg);
  put(2, cb);
}

extern "C" int rt_launch_upsample(int width, int height, float k_n, float k_p, int demodulate, const void *c0, const void *g0,
                                  const void *g1, RT_Frame full, float *out, uint8_t *image, hipStream_t stream) {
  const int tiles_x = (width + UP_TX - 1) / UP_TX, tiles_y = (height + UP_TY - 1) / UP_TY;      // (at most 2^28 / 2 / 8 = 2^24 blocks)
  hipLaunchKernelGGL(rt_upsample_kernel, dim3((unsigned)tiles_x * tiles_y), dim3(UP_TX, UP_TY), 0, stream, width, height, tiles_x, k_n,
                     k_p, demodulate, (const float4 *)c0, (const float4 *)g0, (const float4 *)g1, full.coverage, full.albedo, full.normal,
                     full.position, out, image);
  return (int)hipGetLastError();
}
