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

#include "rt_guided_filter.hip.h"

__global__ __launch_bounds__(256) void rt_guided_pack_kernel(int n_pixels, int demodulate, const float *color, const float *coverage,
                                                             const float *albedo, const float *normal, const float *position,
                                                             float4 *c0, float4 *g0, float4 *g1) {
  guided_pack_pixel<false>(n_pixels, demodulate, color, coverage, albedo, normal, position, nullptr, c0, g0, g1);
}

// One iteration with step `step`: the pixel, the tile and the numbering of the blocks are rt_guided_filter.hip.h's, shared with the
// variance-guided filter of rt_variance.hip.
__global__ __launch_bounds__(GD_TX * GD_TY) void rt_guided_filter_kernel(int width, int height, int step, int phases_x, int phases_y,
                                                                         int tiles_x, float k_n, float k_p, float k_c, int last,
                                                                         int demodulate, const float4 *src, float4 *dst,
                                                                         const float4 *g0, const float4 *g1, const float *color,
                                                                         const float *albedo, float *out, uint8_t *image) {
  guided_filter_pixel<false>(width, height, step, phases_x, phases_y, tiles_x, k_n, k_p, k_c, last, demodulate, src, dst, g0, g1, color,
                             albedo, out, image, nullptr);
}

extern "C" int rt_launch_guided_pack(int n_pixels, int demodulate, RT_Frame frame, void *c0, void *g0, void *g1, hipStream_t stream) {
  hipLaunchKernelGGL(rt_guided_pack_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, demodulate, frame.color,
                     frame.coverage, frame.albedo, frame.normal, frame.position, (float4 *)c0, (float4 *)g0, (float4 *)g1);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_guided_filter(int width, int height, int step, float k_n, float k_p, float k_c, int last, int demodulate,
                                       const void *src, void *dst, const void *g0, const void *g1, RT_Frame frame, float *out,
                                       uint8_t *image, hipStream_t stream) {
  const GuidedGrid G = guided_grid(width, height, step);
  hipLaunchKernelGGL(rt_guided_filter_kernel, dim3(G.blocks), dim3(GD_TX, GD_TY), 0, stream, width, height, step, G.phases_x,
                     G.phases_y, G.tiles_x, k_n, k_p, k_c, last, demodulate, (const float4 *)src, (float4 *)dst, (const float4 *)g0,
                     (const float4 *)g1, frame.color, frame.albedo, out, image);
  return (int)hipGetLastError();
}
