// rt_adaptive.hip -- the two kernels of adaptive sampling (include/rt_hip.h: rt_adaptive_merge, rt_resolve_adaptive, "THE MERGE"):
// a chunk that holds n samples per pixel in `accum` has received samples [n, 2n) into `fresh`; the two buffers are independent
// halves of equal size, their difference estimates the chunk's error, their sum is the chunk's 2n-sample frame.  The arithmetic is
// the contract of rt_hip.h, restated here operation by operation: f32 + - / and sqrt, every operation rounded on its own
// (-ffp-contract=off), the error summed as integers -- so a numpy restatement (tests/_adaptive.py) equals the result bit for bit.
//
// rt_adaptive_merge_kernel: one workgroup of 256 threads per listed chunk, a thread per pixel of eight chunk rows at a time, four
// times.  A pixel is three u64 per buffer, 24 B apart from its neighbour's: a wave's three 8-byte loads of a buffer cover the same
// 1536 contiguous bytes (two rows of 32 pixels), every line of which is used in full.  Per pixel 48 B are read and 48 B written --
// 96 B, 200 MB for a 1920 x 1080 frame whose chunks are all listed, a few tens of microseconds beside launches of milliseconds.
// The chunk's error: every thread adds the q of its (at most four) pixels, a wave sums its 64 lanes by shuffles, the four waves meet
// in LDS and thread 0 STORES the sum -- no atomic, no zeroing before the launch; integer adds are order-free.
//
// rt_resolve_adaptive_kernel: rt_resolve_kernel (rt_kernels.hip) with the divisor read per chunk, a thread per pixel in row-major
// order (the compact tiles of a multi-device frame are not written: adaptive frames render on one device).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_math.h"
#include "rt_device.h"

#define AD_CHUNK 32               // the side of a chunk (RT_CHUNK_SIZE, rt_scene.h)
#define AD_THREADS 256            // 8 rows of a chunk's 32 pixels

__device__ __forceinline__ float adaptive_clamped_mean(unsigned long long sum, uint32_t samples) {
  const float v = rt_accum_resolve(sum, samples);
  return v < 1.0f ? v : 1.0f;     // the output stage clamps at 1: error above that is invisible
}

// Block b: chunk chunks[b].  accum, fresh: u64[height][width][3]; err: u64[chunks of the image].
__global__ __launch_bounds__(AD_THREADS) void rt_adaptive_merge_kernel(int width, int height, int samples, int chunks_x,
                                                                       const int32_t *chunks, unsigned long long *accum,
                                                                       unsigned long long *fresh, unsigned long long *err) {
  __shared__ unsigned long long s_wave[AD_THREADS / 64];
  const int chunk = chunks[blockIdx.x];
  const int x = (chunk % chunks_x) * AD_CHUNK + ((int)threadIdx.x & 31);
  const int y0 = (chunk / chunks_x) * AD_CHUNK + ((int)threadIdx.x >> 5);
  const uint32_t n = (uint32_t)samples;
  unsigned long long q_sum = 0ull;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int y = y0 + k * 8;
    if (x < width && y < height) {
      const size_t p3 = ((size_t)y * width + x) * 3;
      const unsigned long long a0 = accum[p3], a1 = accum[p3 + 1], a2 = accum[p3 + 2];
      const unsigned long long f0 = fresh[p3], f1 = fresh[p3 + 1], f2 = fresh[p3 + 2];
      const float ar = adaptive_clamped_mean(a0, n), ag = adaptive_clamped_mean(a1, n), ab = adaptive_clamped_mean(a2, n);
      const float br = adaptive_clamped_mean(f0, n), bg = adaptive_clamped_mean(f1, n), bb = adaptive_clamped_mean(f2, n);
      const float d = (__builtin_fabsf(ar - br) + __builtin_fabsf(ag - bg)) + __builtin_fabsf(ab - bb);
      const float m = ((ar + br) + (ag + bg)) + (ab + bb);
      const float e = d / rt_sqrtf(m + 1e-4f);
      q_sum += (unsigned long long)(e * 4294967296.0f);      // e <= 300: the product is exact, the conversion truncates
      accum[p3] = a0 + f0;
      accum[p3 + 1] = a1 + f1;
      accum[p3 + 2] = a2 + f2;
      fresh[p3] = 0ull;
      fresh[p3 + 1] = 0ull;
      fresh[p3 + 2] = 0ull;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) q_sum += __shfl_down(q_sum, off, 64);
  if (((int)threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = q_sum;
  __syncthreads();
  if (threadIdx.x == 0) err[chunk] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// One thread per pixel; chunk_samples: i32[chunks of the image], every entry >= 1.
__global__ __launch_bounds__(AD_THREADS) void rt_resolve_adaptive_kernel(int width, int height, int chunks_x,
                                                                         const int32_t *chunk_samples,
                                                                         const unsigned long long *accum, uint8_t *image,
                                                                         float *linear, int32_t *sample_map) {
  const size_t pix = (size_t)blockIdx.x * AD_THREADS + threadIdx.x;
  if (pix >= (size_t)width * height) return;
  const int x = (int)(pix % (size_t)width), y = (int)(pix / (size_t)width);
  const int32_t samples = chunk_samples[(y / AD_CHUNK) * chunks_x + x / AD_CHUNK];
  if (sample_map) sample_map[pix] = samples;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float lin = rt_accum_resolve(accum[pix * 3 + c], (uint32_t)samples);
    if (linear) linear[pix * 3 + c] = lin;
    if (image) image[pix * 3 + c] = rt_encode_u8(lin);
  }
}

extern "C" int rt_launch_adaptive_merge(int width, int height, int samples, int n_list, const int32_t *chunks,
                                        unsigned long long *accum, unsigned long long *fresh, unsigned long long *err,
                                        hipStream_t stream) {
  if (n_list <= 0) return 0;
  const int chunks_x = (width + AD_CHUNK - 1) / AD_CHUNK;
  hipLaunchKernelGGL(rt_adaptive_merge_kernel, dim3((unsigned)n_list), dim3(AD_THREADS), 0, stream, width, height, samples, chunks_x,
                     chunks, accum, fresh, err);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_resolve_adaptive(int width, int height, const int32_t *chunk_samples, const unsigned long long *accum,
                                          uint8_t *image, float *linear, int32_t *sample_map, hipStream_t stream) {
  const size_t pixels = (size_t)width * height;                    // (at most 2^28: 2^20 blocks)
  const int chunks_x = (width + AD_CHUNK - 1) / AD_CHUNK;
  hipLaunchKernelGGL(rt_resolve_adaptive_kernel, dim3((unsigned)((pixels + AD_THREADS - 1) / AD_THREADS)), dim3(AD_THREADS), 0, stream,
                     width, height, chunks_x, chunk_samples, accum, image, linear, sample_map);
  return (int)hipGetLastError();
}
