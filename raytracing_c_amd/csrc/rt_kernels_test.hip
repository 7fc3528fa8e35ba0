// rt_kernels_test.hip -- unit-level kernels for parity tests and their launchers (called from rt_diag.cpp): compiled into the
// DIAGNOSTIC library only (librt_hip_diag.so, include/rt_hip_diag.h).  They instantiate the same device functions as the
// product's kernels (rt_dev.hip.h; traversal_blocks() is the path kernel's own traversal); the product library carries no
// test entry point.

#include "rt_dev.hip.h"

// feature_hit() is defined beside its kernel in rt_features.hip.  This unit reads that file as it is, so that
// rt_test_feature_hit_kernel below instantiates the same feature_hit() text; the diagnostic library links rt_features_dev.o too,
// which has the real kernels and launchers, so here the kernels go into an unnamed namespace and the four launchers -- declared
// static first, which their definitions inherit -- stay local to this object.
namespace {
static int rt_launch_features(const RT_KParams *P, const RT_FParams *F, int n_blocks, int smem_bytes, hipStream_t stream);
static int rt_launch_features_resolve(int n_pixels, int samples, const unsigned long long *sums, float *coverage, float *albedo,
                                      float *normal, float *position, hipStream_t stream);
static int rt_launch_features_motion(const RT_KParams *P, const RT_FParams *F, const float *kept, unsigned long long *motion_sums,
                                     int n_blocks, int smem_bytes, hipStream_t stream);
static int rt_launch_motion_resolve(int n_pixels, int samples, const unsigned long long *sums, float *motion, hipStream_t stream);
#include "rt_features.hip"
}

__global__ void rt_test_math_kernel(int op, int n, const float *x, const float *y, float *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a = x[i], b = y ? y[i] : 0.0f, s, c;
  float r = 0.0f;
  switch (op) {
  case 0: r = rt_logf(a); break;
  case 1: r = rt_expf(a); break;
  case 2: r = rt_powf(a, b); break;
  case 3: rt_sincosf(a, &s, &c); r = s; break;
  case 4: rt_sincosf(a, &s, &c); r = c; break;
  case 5: r = rt_atan2f(a, b); break;
  case 6: r = rt_asinf(a); break;
  case 7: r = rt_srgb_to_linear1(a); break;
  case 8: r = rt_linear_to_srgb(a); break;
  case 9: r = rt_sqrtf(a); break;
  case 10: r = 1.0f / a; break;
  case 11: r = rcp_exact(a); break;
  case 12: r = rcp_exact_outside(a) ? 1.0f : 0.0f; break;
  case 13: r = srgb_to_linear_tex1(a); break;
  case 14: r = atan2_dev(a, b); break;
  case 15: r = atan_pos_dev(a); break;
  case 16: r = asin_dev(a); break;
  case 17: r = inv_sqrt_exact(a); break;
  case 18: r = sqrt_dev(a); break;
  default: break;
  }
  out[i] = r;
}

// All 2^32 bit patterns x: rcp_exact(x) against the IEEE quotient 1.0f / x.  counts[0] = patterns inside the claimed
// domain (|x| < 2^102, infinity, NaN) that differ (NaN equals NaN), counts[1] = patterns outside it, counts[2] = of those,
// how many differ (why the domain ends there), counts[3] = first differing pattern inside the domain + 1.
// rcp_leaf(x), the leaf blocks' form without the fix-up: counts[4] = finite non-zero patterns with |x| < 2^102 that differ from
// 1.0f / x, counts[5] = patterns x = +-0, +-infinity, NaN for which it is NOT NaN (what the leaf blocks' argument rests on).
__global__ void rt_test_rcp_sweep_kernel(unsigned long long *counts) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t bad_in = 0, n_out = 0, bad_out = 0, first = 0, leaf_bad = 0, leaf_special = 0;
  for (uint32_t k = 0; k < 256u; k++) {
    const uint32_t b = tid * 256u + k;
    const float x = __uint_as_float(b);
    const uint32_t w = __float_as_uint(1.0f / x), g = __float_as_uint(rcp_exact(x));
    const bool w_nan = (w & 0x7FFFFFFFu) > 0x7F800000u, g_nan = (g & 0x7FFFFFFFu) > 0x7F800000u;
    const bool same = w_nan ? g_nan : (g == w);
    if (rcp_exact_outside(x)) { n_out += 1; bad_out += same ? 0u : 1u; }
    else if (!same) { bad_in += 1; if (!first) first = b + 1u; }
    const uint32_t l = __float_as_uint(rcp_leaf(x)), mag = b & 0x7FFFFFFFu;
    const bool l_nan = (l & 0x7FFFFFFFu) > 0x7F800000u;
    if (mag == 0u || mag >= 0x7F800000u) leaf_special += l_nan ? 0u : 1u;
    else if (!rcp_exact_outside(x)) leaf_bad += (l == w) ? 0u : 1u;
  }
  if (leaf_bad) atomicAdd(&counts[4], (unsigned long long)leaf_bad);
  if (leaf_special) atomicAdd(&counts[5], (unsigned long long)leaf_special);
  if (bad_in) atomicAdd(&counts[0], (unsigned long long)bad_in);
  if (n_out) atomicAdd(&counts[1], (unsigned long long)n_out);
  if (bad_out) atomicAdd(&counts[2], (unsigned long long)bad_out);
  if (first) atomicMax(&counts[3], (unsigned long long)first);
}

// accum_quantize_dev(x) against rt_accum_quantize(x) for all 2^32 bit patterns: counts[0] = patterns that differ,
// counts[1] = first differing pattern + 1.
__global__ void rt_test_quantize_sweep_kernel(unsigned long long *counts) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t bad = 0, first = 0;
  for (uint32_t k = 0; k < 256u; k++) {
    const uint32_t b = tid * 256u + k;
    const float x = __uint_as_float(b);
    if (accum_quantize_dev(x) != (unsigned long long)rt_accum_quantize(x)) { bad += 1; if (!first) first = b + 1u; }
  }
  if (bad) atomicAdd(&counts[0], (unsigned long long)bad);
  if (first) atomicMax(&counts[1], (unsigned long long)first);
}

// rt_encode_u8(x) -- the last step of every image: rt_resolve, the post passes -- on all 2^32 bit patterns, 256 consecutive ones
// per thread.  counts[k], k < 256: 2^32 - the LOWEST pattern in [0, 0x3F800000] (the floats of [0, 1]) that encodes to k, 0 when
// there is none (a maximum over the threads; rt_test_encode_sweep turns it into the pattern); counts[256] = patterns of that range
// whose byte is below that of the pattern before, counts[257] = patterns in (1.0, +inf] that do not give 255, counts[258] =
// negative patterns, -0 and -inf included, that do not give 0, counts[259] = NaN patterns that do not give 0.  A byte's lowest
// pattern is one whose predecessor has another byte (or pattern 0), so only those reach the atomics.
__global__ void rt_test_encode_sweep_kernel(unsigned long long *counts) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t b0 = tid * 256u;
  uint32_t descents = 0, above = 0, negative = 0, nan = 0;
  int prev = (b0 != 0u && b0 <= 0x3F800000u) ? (int)rt_encode_u8(__uint_as_float(b0 - 1u)) : -1;
  for (uint32_t k = 0; k < 256u; k++) {
    const uint32_t b = b0 + k;
    const int v = (int)rt_encode_u8(__uint_as_float(b));
    if (b <= 0x3F800000u) {
      if (v != prev) {
        atomicMax(&counts[v], 0x100000000ull - (unsigned long long)b);
        descents += v < prev ? 1u : 0u;
        prev = v;
      }
    } else if (b <= 0x7F800000u) above += v != 255 ? 1u : 0u;
    else if ((b & 0x7FFFFFFFu) > 0x7F800000u) nan += v != 0 ? 1u : 0u;
    else negative += v != 0 ? 1u : 0u;
  }
  if (descents) atomicAdd(&counts[256], (unsigned long long)descents);
  if (above) atomicAdd(&counts[257], (unsigned long long)above);
  if (negative) atomicAdd(&counts[258], (unsigned long long)negative);
  if (nan) atomicAdd(&counts[259], (unsigned long long)nan);
}

// group_sum3_u64<G> (the sky loop's sample reduction, three values at once) on values a test chooses: one wave per block, lane
// i & 63 of wave i >> 6, channel c at [c * n + i]; a lane that is not valid contributes 0, as in the loop.  Every lane writes
// what it holds afterwards.
template <int G>
__global__ __launch_bounds__(64) void rt_test_group_sum_kernel(const unsigned long long *in, const unsigned char *valid, unsigned long long *out) {
  const size_t n = (size_t)gridDim.x * 64, i = (size_t)blockIdx.x * 64 + threadIdx.x;
  unsigned long long r = 0ull, g = 0ull, b = 0ull;
  if (valid[i]) { r = in[i]; g = in[n + i]; b = in[2 * n + i]; }
  group_sum3_u64<G>(r, g, b);
  out[i] = r; out[n + i] = g; out[2 * n + i] = b;
}

// The two orderings of a node block's children (rt_dev.hip.h) on distances a test chooses, one lane per case: t_min[8 i + k] = the
// bit pattern of child k's entry distance (at least that of RT_EPS, as every FAST slab form gives it), cand[8 i + k] != 0 = the
// child is a candidate.  out[3 i] = the word of node_order_keys(), [3 i + 1] = the word of node_order_rank(), [3 i + 2] = 1 when
// the keys of the case are not exact (node_keys_exact) and a node block takes the rank sort.
__global__ void rt_test_node_order_kernel(int n, const uint32_t *t_min, const unsigned char *cand, uint32_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  NodeKeys K;
  K.max_raw = 0u;
  K.n_cand = 0u;
  int d[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float t = __uint_as_float(t_min[(size_t)i * 8 + k]);
    const bool c = cand[(size_t)i * 8 + k] != 0;
    node_child_put<true>(K, d, k, t, c);
    node_child_put<false>(K, d, k, t, c);
  }
  const bool exact = node_keys_exact(K);
  out[(size_t)i * 3 + 0] = node_order_keys(K);
  out[(size_t)i * 3 + 1] = node_order_rank(d);
  out[(size_t)i * 3 + 2] = exact ? 0u : 1u;
}

extern "C" int rt_launch_test_node_order(int n, const uint32_t *t_min, const unsigned char *cand, uint32_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_node_order_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, t_min, cand, out);
  return (int)hipGetLastError();
}

// srgb_to_linear_tex1(x) against rt_srgb_to_linear1(x) for every float in [0, 2] and in [-0.046875, -0.03125]: counts[0] =
// patterns compared (2^30 + 2^22), counts[1] = patterns that differ, counts[2] = first differing pattern + 1.
__global__ void rt_test_srgb_sweep_kernel(unsigned long long *counts) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;       // 2^22 threads x 256 patterns = [0, 0x40000000)
  uint32_t n = 0, bad = 0, first = 0;
  for (uint32_t k = 0; k < 257u; k++) {
    uint32_t b = tid * 256u + k;
    if (k == 256u) b = tid == 0 ? 0x40000000u : 0xBD000000u + tid - 1u;        // 2.0, and 2^22 - 1 negative values from -0.03125 down
    const float x = __uint_as_float(b);
    const uint32_t w = __float_as_uint(rt_srgb_to_linear1(x)), g = __float_as_uint(srgb_to_linear_tex1(x));
    n += 1;
    if (w != g) { bad += 1; if (!first) first = b + 1u; }
  }
  atomicAdd(&counts[0], (unsigned long long)n);
  if (bad) atomicAdd(&counts[1], (unsigned long long)bad);
  if (first) atomicMax(&counts[2], (unsigned long long)first);
}

// The short forms of the environment lookup and of the normalisations (rt_dev.hip.h) against the UNMODIFIED rt_math.h functions,
// compiled here for the device.  WHICH 0 .. 5 walk all 2^32 bit patterns x:
//   0  atan_pos_dev(x)    against rt_atanf_pos(x)
//   1  asin_dev(x)        against rt_asinf(x)
//   2  inv_sqrt_exact(x)  against rcp_exact(rt_sqrtf(x)), and against the division 1.0f / rt_sqrtf(x) that rcp_exact() stands for
//   3  the background's u for the angle x, tex_wrap_fract<false>(bg_coord_u(x)) against tex_taps' wrap and fract
//      tex_wrap_fract<true>(...), over every x atan2_dev() can return: |x| <= RT_PI, or NaN
//   4  the same for v = bg_coord_v(x) over every x asin_dev() can return: |x| <= pi/2 (as a float), or NaN
//   5  sqrt_dev(x)        against rt_sqrtf(x)
// WHICH 6: atan2_dev(y, x) against rt_atan2f(y, x) on 2^26 pairs drawn from `seed`: even pairs two random bit patterns (every
// exponent, so quotients that overflow, underflow and are NaN), odd pairs two random values of either sign between 2^-7 and 1
// (quotients in all three ranges of the arctangent).
// counts[0] = patterns (pairs) compared, [1] = differing ones, NaN equal to NaN, [2] = 2^32 - the LOWEST differing pattern (pair
// index), 0 when there is none (a maximum over the threads; rt_test_env_sweep turns it into the pattern + 1), [3] = differing ones
// when a NaN must have the same bits too.
template <int WHICH>
__device__ __forceinline__ bool env_form_pair(uint32_t b, uint32_t seed, float &want, float &got) {
  const float x = __uint_as_float(b);
  switch (WHICH) {
  case 0: want = rt_atanf_pos(x); got = atan_pos_dev(x); return true;
  case 1: want = rt_asinf(x); got = asin_dev(x); return true;
  case 2: want = rcp_exact(rt_sqrtf(x)); got = inv_sqrt_exact(x); return true;
  case 3: want = tex_wrap_fract<true>(bg_coord_u(x)); got = tex_wrap_fract<false>(bg_coord_u(x)); return !(__builtin_fabsf(x) > RT_PI);
  case 4: want = tex_wrap_fract<true>(bg_coord_v(x)); got = tex_wrap_fract<false>(bg_coord_v(x)); return !(__builtin_fabsf(x) > 1.5707963267948966192f);
  case 5: want = rt_sqrtf(x); got = sqrt_dev(x); return true;
  default: {
    uint32_t by = rt_pcg(seed ^ (2u * b)), bx = rt_pcg(seed ^ (2u * b + 1u));
    if (b & 1u) {
      by = (by & 0x807FFFFFu) | ((120u + ((by >> 23) & 7u)) << 23);
      bx = (bx & 0x807FFFFFu) | ((120u + ((bx >> 23) & 7u)) << 23);
    }
    want = rt_atan2f(__uint_as_float(by), __uint_as_float(bx));
    got = atan2_dev(__uint_as_float(by), __uint_as_float(bx));
    return true;
  }
  }
}

template <int WHICH>
__global__ void rt_test_env_sweep_kernel(uint32_t per_thread, uint32_t seed, unsigned long long *counts) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t n = 0, bad = 0, strict = 0;
  unsigned long long first = 0;
  for (uint32_t k = 0; k < per_thread; k++) {
    const uint32_t b = tid * per_thread + k;
    float want, got;
    if (!env_form_pair<WHICH>(b, seed, want, got)) continue;
    if (WHICH == 2) {                                   // ... and the division itself
      const float q = 1.0f / rt_sqrtf(__uint_as_float(b));
      const bool q_nan = q != q;
      if (q_nan ? got == got : __float_as_uint(q) != __float_as_uint(got)) { bad += 1; if (!first) first = (unsigned long long)b + 1ull; }
    }
    const uint32_t w = __float_as_uint(want), g = __float_as_uint(got);
    const bool w_nan = (w & 0x7FFFFFFFu) > 0x7F800000u, g_nan = (g & 0x7FFFFFFFu) > 0x7F800000u;
    n += 1;
    if (w_nan ? !g_nan : g != w) { bad += 1; if (!first) first = (unsigned long long)b + 1ull; }
    strict += (g != w) ? 1u : 0u;
  }
  atomicAdd(&counts[0], (unsigned long long)n);
  if (bad) atomicAdd(&counts[1], (unsigned long long)bad);
  if (first) atomicMax(&counts[2], 0x100000000ull - (first - 1ull));
  if (strict) atomicAdd(&counts[3], (unsigned long long)strict);
}

extern "C" int rt_launch_test_env_sweep(int which, uint32_t seed, unsigned long long *counts, hipStream_t stream) {
  const dim3 grid(65536), block(256);                  // 2^24 threads: 256 patterns each, or 4 pairs each
  switch (which) {
  case 0: hipLaunchKernelGGL(rt_test_env_sweep_kernel<0>, grid, block, 0, stream, 256u, seed, counts); break;
  case 1: hipLaunchKernelGGL(rt_test_env_sweep_kernel<1>, grid, block, 0, stream, 256u, seed, counts); break;
  case 2: hipLaunchKernelGGL(rt_test_env_sweep_kernel<2>, grid, block, 0, stream, 256u, seed, counts); break;
  case 3: hipLaunchKernelGGL(rt_test_env_sweep_kernel<3>, grid, block, 0, stream, 256u, seed, counts); break;
  case 4: hipLaunchKernelGGL(rt_test_env_sweep_kernel<4>, grid, block, 0, stream, 256u, seed, counts); break;
  case 5: hipLaunchKernelGGL(rt_test_env_sweep_kernel<5>, grid, block, 0, stream, 256u, seed, counts); break;
  default: hipLaunchKernelGGL(rt_test_env_sweep_kernel<6>, grid, block, 0, stream, 4u, seed, counts); break;
  }
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(RT_BLOCK_THREADS) void rt_test_trace_kernel(RT_KParams P, int n, const float *rays,
                                                                         float *out_t, int *out_tri, float *out_uv) {
  __shared__ uint32_t s_perm[RT_BLOCK_WAVES][RT_MAX_DEPTH * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  LaneCounters cn;
  cn.rays = cn.nodes = cn.leaves = cn.shades = cn.bgs = cn.textured = cn.paths = 0;
  if (i >= n) return;
  Ray3 r;
  ray_setup(r, rt_v3_make(rays[i * 6 + 0], rays[i * 6 + 1], rays[i * 6 + 2]),
            rt_v3_make(rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]));
  HitRec hit;
  if (r.fast) trace_ray<true>(P, r, hit, s_perm[wave], lane, cn);
  else trace_ray<false>(P, r, hit, s_perm[wave], lane, cn);
  out_t[i] = hit.t;
  out_tri[i] = hit.tri;
  out_uv[i * 2 + 0] = hit.u;
  out_uv[i * 2 + 1] = hit.v;
}

__global__ void rt_test_texture_kernel(RT_KParams P, int tex, int n, const float *uv, float *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rt_v3 c = tex_bilinear(P, tex, uv[i * 2], uv[i * 2 + 1]);
  out[i * 3 + 0] = c.x;
  out[i * 3 + 1] = c.y;
  out[i * 3 + 2] = c.z;
}

// The shade block on inputs a test chooses: shade() (disney_shader_proc / debug_shader_proc) on the material of triangle
// tri[i] -- float 3 of its 28-float record, as shade_hit() reads it -- with the 14 floats of in[] as direction, normal,
// tangent, bitangent, uv.  Item i is lane i & 63 of wave i >> 6 (the block is four whole waves), so the caller decides which
// waves are material-uniform and read the record through the scalar cache; the lanes past n of the last wave have left
// before shade(), as the lanes of a partial block of the path kernel have.  SP = ShadeParamsLds: the sRGB scale table in LDS,
// filled before the barrier as the path kernel does.
template <class SP>
__global__ __launch_bounds__(RT_BLOCK_THREADS) void rt_test_shade_kernel(RT_KParams P, int n, const int *tri, const float *in,
                                                                         const uint32_t *state_in, float *out, uint32_t *state_out,
                                                                         int *terminate, int *textured) {
  if (Pow24InLds<SP>::value) {
    pow24_lds_init((int)threadIdx.x);
    __syncthreads();
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SP S;
  shade_params(S, &P, true);
  const float4 q0 = ld4(S.tris + (size_t)tri[i] * 28, 0);
  const float *f = in + (size_t)i * 14;
  ShadeIn si;
  si.direction = rt_v3_make(f[0], f[1], f[2]);
  si.normal = rt_v3_make(f[3], f[4], f[5]);
  si.tangent = rt_v3_make(f[6], f[7], f[8]);
  si.bitangent = rt_v3_make(f[9], f[10], f[11]);
  si.uvx = f[12];
  si.uvy = f[13];
  LaneCounters cn;
  cn.rays = cn.nodes = cn.leaves = cn.shades = cn.bgs = cn.textured = cn.paths = 0;
  uint32_t rng = state_in[i];
  rt_v3 out_dir, tint, emission;
  bool term;
  shade(S, as_i(q0.w), si, rng, out_dir, tint, emission, term, cn);
  float *o = out + (size_t)i * 9;
  o[0] = out_dir.x; o[1] = out_dir.y; o[2] = out_dir.z;
  o[3] = tint.x; o[4] = tint.y; o[5] = tint.z;
  o[6] = emission.x; o[7] = emission.y; o[8] = emission.z;
  state_out[i] = rng;
  terminate[i] = term ? 1 : 0;
  textured[i] = (int)cn.textured;
}

// One path step on a hit a test chooses: shade_hit<PT>() -- face test, surface_at(), shade(), carried tint and emission, the next
// origin, the bounce count -- for PT = ShadeParams (the wavefront shade kernel's), ShadeParamsLds (the path kernel's: the sRGB
// scale table in LDS, filled before the barrier) and RT_KParams (cast_ray_lane's, the lightmap).  Item i is lane i & 63 of wave
// i >> 6 as in rt_test_shade_kernel; the lanes past n have left before shade_hit(), so which lanes are active inside its `else`
// -- the lanes shade()'s ballot sees -- is decided by the order of the items alone.
//   hit  t, u, v           ray  origin, direction        carry  tint, emission
//   out  15 floats: origin, direction, tint, emission, radiance (as they stand afterwards; radiance starts as -1, -2, -3)
//   iout 5 words: rng, bounce, done, shades increment, textured increment
template <class PT>
__device__ __forceinline__ void test_shade_hit_item(const PT &S, int i, const int *tri, const float *hit_in, const float *ray_in,
                                                    const float *carry, const uint32_t *state_in, const int *bounce_in, float *out,
                                                    uint32_t *iout) {
  HitRec hit;
  hit.t = hit_in[(size_t)i * 3 + 0]; hit.u = hit_in[(size_t)i * 3 + 1]; hit.v = hit_in[(size_t)i * 3 + 2];
  hit.tri = tri[i];
  const float *r = ray_in + (size_t)i * 6, *c = carry + (size_t)i * 6;
  rt_v3 org = rt_v3_make(r[0], r[1], r[2]), dir = rt_v3_make(r[3], r[4], r[5]);
  rt_v3 tint = rt_v3_make(c[0], c[1], c[2]), emis = rt_v3_make(c[3], c[4], c[5]);
  rt_v3 radiance = rt_v3_make(-1.0f, -2.0f, -3.0f);
  uint32_t rng = state_in[i];
  int bounce = bounce_in[i];
  LaneCounters cn;
  cn.rays = cn.nodes = cn.leaves = cn.shades = cn.bgs = cn.textured = cn.paths = 0;
  const bool done = shade_hit(S, hit, org, dir, tint, emis, rng, bounce, cn, radiance);
  float *o = out + (size_t)i * 15;
  o[0] = org.x; o[1] = org.y; o[2] = org.z; o[3] = dir.x; o[4] = dir.y; o[5] = dir.z;
  o[6] = tint.x; o[7] = tint.y; o[8] = tint.z; o[9] = emis.x; o[10] = emis.y; o[11] = emis.z;
  o[12] = radiance.x; o[13] = radiance.y; o[14] = radiance.z;
  uint32_t *w = iout + (size_t)i * 5;
  w[0] = rng; w[1] = (uint32_t)bounce; w[2] = done ? 1u : 0u; w[3] = (uint32_t)cn.shades; w[4] = (uint32_t)cn.textured;
}

template <class SP>
__global__ __launch_bounds__(RT_BLOCK_THREADS) void rt_test_shade_hit_kernel(RT_KParams P, int n, const int *tri, const float *hit_in,
                                                                             const float *ray_in, const float *carry,
                                                                             const uint32_t *state_in, const int *bounce_in, float *out,
                                                                             uint32_t *iout) {
  if (Pow24InLds<SP>::value) {
    pow24_lds_init((int)threadIdx.x);
    __syncthreads();
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SP S;
  shade_params(S, &P, true);
  test_shade_hit_item(S, i, tri, hit_in, ray_in, carry, state_in, bounce_in, out, iout);
}

// ... and with the kernel arguments themselves as PT, as cast_ray_lane() has them
__global__ __launch_bounds__(RT_BLOCK_THREADS) void rt_test_shade_hit_kparams_kernel(RT_KParams P, int n, const int *tri, const float *hit_in,
                                                                                     const float *ray_in, const float *carry,
                                                                                     const uint32_t *state_in, const int *bounce_in,
                                                                                     float *out, uint32_t *iout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  test_shade_hit_item(P, i, tri, hit_in, ray_in, carry, state_in, bounce_in, out, iout);
}

// feature_hit<ShadeParamsLds>() (rt_features.hip), the feature kernel's instance, on the same kind of item.
//   out 12 floats: origin afterwards, albedo, normal, position (the last three start as 0 and stay so on a back face); flag[n] 0 / 1
__global__ __launch_bounds__(RT_BLOCK_THREADS) void rt_test_feature_hit_kernel(RT_KParams P, int n, const int *tri, const float *hit_in,
                                                                               const float *ray_in, float *out, int *flag) {
  pow24_lds_init((int)threadIdx.x);
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ShadeParamsLds S;
  shade_params(S, &P, true);
  HitRec hit;
  hit.t = hit_in[(size_t)i * 3 + 0]; hit.u = hit_in[(size_t)i * 3 + 1]; hit.v = hit_in[(size_t)i * 3 + 2];
  hit.tri = tri[i];
  const float *r = ray_in + (size_t)i * 6;
  rt_v3 org = rt_v3_make(r[0], r[1], r[2]);
  const rt_v3 dir = rt_v3_make(r[3], r[4], r[5]);
  rt_v3 albedo = rt_v3_make(0, 0, 0), normal = rt_v3_make(0, 0, 0), position = rt_v3_make(0, 0, 0);
  const bool f = feature_hit(S, hit, org, dir, albedo, normal, position);
  float *o = out + (size_t)i * 12;
  o[0] = org.x; o[1] = org.y; o[2] = org.z; o[3] = albedo.x; o[4] = albedo.y; o[5] = albedo.z;
  o[6] = normal.x; o[7] = normal.y; o[8] = normal.z; o[9] = position.x; o[10] = position.y; o[11] = position.z;
  flag[i] = f ? 1 : 0;
}

// sample_disney() on a raw BrdfIn: params = roughness, metalness, sheen, sheen_tint, aniso2, base colour
__global__ void rt_test_brdf_kernel(int n, const float *params, const float *in_dir, const uint32_t *state_in, float *out_dir,
                                    float *brdf, uint32_t *state_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = params + (size_t)i * 8;
  BrdfIn m;
  m.roughness = p[0]; m.metalness = p[1]; m.sheen = p[2]; m.sheen_tint = p[3]; m.aniso2 = p[4];
  m.base_color = rt_v3_make(p[5], p[6], p[7]);
  uint32_t rng = state_in[i];
  rt_v3 o, rgb;
  float a;
  sample_disney(m, rt_v3_make(in_dir[i * 3 + 0], in_dir[i * 3 + 1], in_dir[i * 3 + 2]), rng, o, rgb, a);
  out_dir[i * 3 + 0] = o.x; out_dir[i * 3 + 1] = o.y; out_dir[i * 3 + 2] = o.z;
  brdf[i * 4 + 0] = rgb.x; brdf[i * 4 + 1] = rgb.y; brdf[i * 4 + 2] = rgb.z; brdf[i * 4 + 3] = a;
  state_out[i] = rng;
}

// SP = BgImageParams / BgImageParamsLds: background_lookup_image() on the float image; any other: background_lookup() on the texel pool
template <class SP>
__global__ __launch_bounds__(RT_BLOCK_THREADS) void rt_test_background_kernel(RT_KParams P, int n, const float *dir, float *rgb) {
  if (Pow24InLds<SP>::value) {
    pow24_lds_init((int)threadIdx.x);
    __syncthreads();
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SP S;
  const rt_v3 d = rt_v3_make(dir[i * 3 + 0], dir[i * 3 + 1], dir[i * 3 + 2]);
  rt_v3 c;
  if constexpr (std::is_base_of<BgImageParams, SP>::value) {
    bg_image_params(S, &P);
    c = background_lookup_image(S, d);
  } else {
    shade_params(S, &P, false);
    c = background_lookup(S, d);
  }
  rgb[i * 3 + 0] = c.x; rgb[i * 3 + 1] = c.y; rgb[i * 3 + 2] = c.z;
}

// primary_ray() of (x, y, sample) with the frame constants the host computed (camera_frame_kparams)
__global__ void rt_test_primary_ray_kernel(RT_KParams P, int n, const int *xys, float *rays) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PrimaryParams PP;
  primary_params(PP, &P, &P);
  rt_v3 o, d;
  primary_ray(PP, xys[i * 3 + 0], xys[i * 3 + 1], xys[i * 3 + 2], o, d);
  float *r = rays + (size_t)i * 6;
  r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

// Arbitrary rays through the PRODUCTION traversal: traversal_blocks() -- the NODE / LEAF / pop code of the path kernels --
// in the path kernel's workgroup geometry (16 waves, tree in LDS, per-wave perm stacks), lanes refilled from the ray list
// as they finish, blocks mixed exactly as a frame mixes them.  With a pyramid (`pyr`: 4 outward plane normals at
// [4 q .. 4 q + 2], the common ray origin at [16 .. 18]) every ray counts as a camera ray of one tile: node blocks take
// the culled form (pyramid_cull_mask, node_enter_few) whenever the path kernel would.  visits[0 / 1] += node / leaf
// visits (raytracer.c:452 / :476 calls).  Compared with oracle_trace_rays_counted() by tests/test_gpu_trace_stream.py.
template <bool SHORT_DIV, bool PYRAMID>
__global__ __launch_bounds__(16 * 64, 1) void rt_test_trace_stream_kernel(RT_KParams P, int n, const float *rays, const float *pyr_in,
                                                                         int exit_lanes, float *out_t, int *out_tri, float *out_uv,
                                                                         unsigned long long *visits) {
  extern __shared__ float4 smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n_lds = P.n_lds_nodes;
  const float4 *lds_nodes = smem;
  const WaveLds L = wave_lds(smem, n_lds, P.depth, wave);      // the path kernel's slice
  const int pyr_off = L.pyr_off;
  lds_load_nodes<16 * 64>(smem, P.nodes, n_lds);
  __syncthreads();
  if (PYRAMID) {
    float *pyr = lds_at(smem, pyr_off);
    if (lane < RT_PYR_ORIGIN + 3) pyr[lane] = pyr_in[lane];      // planes and origin, as the caller built them
    if (lane < RT_PYR_CACHE_WORDS) reinterpret_cast<uint32_t *>(pyr)[RT_PYR_LEAF_CACHE + lane] = 0u;
  }
  const int leaf_level = P.depth - 1;
  const TravWave W = {smem, lds_nodes, L.perm, n_lds, PYRAMID ? P.pyr_nodes : 0, pyr_off, leaf_level, lane};
  const int n_waves = (int)gridDim.x * 16, wave_id = (int)blockIdx.x * 16 + wave;
  const int per_wave = (n + n_waves - 1) / n_waves;
  int next = wave_id * per_wave;                                   // this wave's slice of the ray list
  const int end = next + per_wave < n ? next + per_wave : n;

  int   idx = 0;
  Ray3  ray;
  ray_setup(ray, rt_v3_make(0, 0, 0), rt_v3_make(0, 0, 1));
  uint32_t w_nodes = 0, w_leaves = 0;
  TravState T = RT_TRAV_IDLE;
  for (;;) {
    if (T.phase == PH_HIT || T.phase == PH_MISS) {
      out_t[idx] = T.hit.t;
      out_tri[idx] = T.hit.tri;
      out_uv[idx * 2 + 0] = T.hit.u;
      out_uv[idx * 2 + 1] = T.hit.v;
      T.phase = PH_NEED;
    }
    if (next < end) {
      const unsigned long long need = __ballot(T.phase == PH_NEED);
      const int rank = lane_rank(need);
      if (T.phase == PH_NEED && next + rank < end) {
        idx = next + rank;
        const float *r = rays + (size_t)idx * 6;
        ray_setup<SHORT_DIV>(ray, rt_v3_make(r[0], r[1], r[2]), rt_v3_make(r[3], r[4], r[5]));
        trav_start(T, leaf_level, P.last_row_offset);
      }
      next += (int)__popcll(need);
    }
    const int n_trav0 = (int)__popcll(__ballot(T.phase == PH_NODE || T.phase == PH_LEAF));
    if (n_trav0 == 0) {
      if (next >= end) break;
      continue;
    }
    traversal_blocks<true, SHORT_DIV, PYRAMID>(P, W, ray, true, T, next < end ? exit_lanes : 1, n_trav0, w_nodes, w_leaves);
  }
  if (lane == 0) {
    atomicAdd(visits + 0, (unsigned long long)w_nodes);
    atomicAdd(visits + 1, (unsigned long long)w_leaves);
  }
}

extern "C" int rt_launch_test_trace_stream(const RT_KParams *P, int n, const float *rays, const float *pyr, int exit_lanes, int n_blocks,
                                           int smem_bytes, float *out_t, int *out_tri, float *out_uv, unsigned long long *visits,
                                           hipStream_t stream) {
#define RT_TTS(SD, PY)                                                                                                          \
  do {                                                                                                                          \
    static uint32_t attr_devices = 0;                                                                                           \
    if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&rt_test_trace_stream_kernel<SD, PY>), &attr_devices, smem_bytes, \
                                 RT_LDS_BYTES))                                                                                 \
      return rc;                                                                                                                \
    hipLaunchKernelGGL((rt_test_trace_stream_kernel<SD, PY>), dim3(n_blocks), dim3(16 * 64), smem_bytes, stream, *P, n, rays,  \
                       pyr, exit_lanes, out_t, out_tri, out_uv, visits);                                                        \
  } while (0)
  if (P->short_div) { if (pyr) RT_TTS(true, true); else RT_TTS(true, false); }
  else { if (pyr) RT_TTS(false, true); else RT_TTS(false, false); }
#undef RT_TTS
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_math(int op, int n, const float *x, const float *y, float *out, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_math_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, op, n, x, y, out);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_rcp_sweep(unsigned long long *counts, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_rcp_sweep_kernel, dim3(65536), dim3(256), 0, stream, counts);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_group_sum(int group, int n_waves, const unsigned long long *in, const unsigned char *valid,
                                        unsigned long long *out, hipStream_t stream) {
  if (group == 4) hipLaunchKernelGGL(rt_test_group_sum_kernel<4>, dim3(n_waves), dim3(64), 0, stream, in, valid, out);
  else if (group == 16) hipLaunchKernelGGL(rt_test_group_sum_kernel<16>, dim3(n_waves), dim3(64), 0, stream, in, valid, out);
  else hipLaunchKernelGGL(rt_test_group_sum_kernel<64>, dim3(n_waves), dim3(64), 0, stream, in, valid, out);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_sky_add_group(void) { return RT_SKY_ADD_GROUP; }

extern "C" int rt_launch_test_quantize_sweep(unsigned long long *counts, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_quantize_sweep_kernel, dim3(65536), dim3(256), 0, stream, counts);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_encode_sweep(unsigned long long *counts, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_encode_sweep_kernel, dim3(65536), dim3(256), 0, stream, counts);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_srgb_sweep(unsigned long long *counts, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_srgb_sweep_kernel, dim3(16384), dim3(256), 0, stream, counts);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_trace(const RT_KParams *P, int n, const float *rays, float *out_t, int *out_tri,
                                    float *out_uv, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_trace_kernel, dim3((n + RT_BLOCK_THREADS - 1) / RT_BLOCK_THREADS),
                     dim3(RT_BLOCK_THREADS), 0, stream, *P, n, rays, out_t, out_tri, out_uv);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_texture(const RT_KParams *P, int tex, int n, const float *uv, float *out,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_texture_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *P, tex, n, uv, out);
  return (int)hipGetLastError();
}

// mode: 0 = ShadeParams, 1 = ShadeParamsLds (the instance of the path kernel); + RT_TEST_SHARED_TAPS (4): the same two with one set
// of bilinear taps per item (ShadeParamsShared, ShadeParamsLdsShared) -- the caller has checked that the scene's materials qualify
extern "C" int rt_launch_test_shade(const RT_KParams *P, int mode, int n, const int *tri, const float *in, const uint32_t *state_in,
                                    float *out, uint32_t *state_out, int *terminate, int *textured, hipStream_t stream) {
  const dim3 grid((n + RT_BLOCK_THREADS - 1) / RT_BLOCK_THREADS), block(RT_BLOCK_THREADS);
  const int lds = mode & 1;
  if (mode & 4) {
    if (lds) hipLaunchKernelGGL(rt_test_shade_kernel<ShadeParamsLdsShared>, grid, block, 0, stream, *P, n, tri, in, state_in, out, state_out, terminate, textured);
    else hipLaunchKernelGGL(rt_test_shade_kernel<ShadeParamsShared>, grid, block, 0, stream, *P, n, tri, in, state_in, out, state_out, terminate, textured);
  } else if (lds) hipLaunchKernelGGL(rt_test_shade_kernel<ShadeParamsLds>, grid, block, 0, stream, *P, n, tri, in, state_in, out, state_out, terminate, textured);
  else hipLaunchKernelGGL(rt_test_shade_kernel<ShadeParams>, grid, block, 0, stream, *P, n, tri, in, state_in, out, state_out, terminate, textured);
  return (int)hipGetLastError();
}

// mode: 0 = ShadeParams, 1 = ShadeParamsLds, 2 = RT_KParams; 4, 5 = the first two with shared taps (see rt_launch_test_shade)
extern "C" int rt_launch_test_shade_hit(const RT_KParams *P, int mode, int n, const int *tri, const float *hit, const float *ray,
                                        const float *carry, const uint32_t *state_in, const int *bounce_in, float *out, uint32_t *iout,
                                        hipStream_t stream) {
  const dim3 grid((n + RT_BLOCK_THREADS - 1) / RT_BLOCK_THREADS), block(RT_BLOCK_THREADS);
  if (mode == 4) hipLaunchKernelGGL(rt_test_shade_hit_kernel<ShadeParamsShared>, grid, block, 0, stream, *P, n, tri, hit, ray, carry, state_in, bounce_in, out, iout);
  else if (mode == 5) hipLaunchKernelGGL(rt_test_shade_hit_kernel<ShadeParamsLdsShared>, grid, block, 0, stream, *P, n, tri, hit, ray, carry, state_in, bounce_in, out, iout);
  else if (mode == 0) hipLaunchKernelGGL(rt_test_shade_hit_kernel<ShadeParams>, grid, block, 0, stream, *P, n, tri, hit, ray, carry, state_in, bounce_in, out, iout);
  else if (mode == 1) hipLaunchKernelGGL(rt_test_shade_hit_kernel<ShadeParamsLds>, grid, block, 0, stream, *P, n, tri, hit, ray, carry, state_in, bounce_in, out, iout);
  else hipLaunchKernelGGL(rt_test_shade_hit_kparams_kernel, grid, block, 0, stream, *P, n, tri, hit, ray, carry, state_in, bounce_in, out, iout);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_feature_hit(const RT_KParams *P, int n, const int *tri, const float *hit, const float *ray, float *out,
                                          int *flag, hipStream_t stream) {
  const dim3 grid((n + RT_BLOCK_THREADS - 1) / RT_BLOCK_THREADS), block(RT_BLOCK_THREADS);
  hipLaunchKernelGGL(rt_test_feature_hit_kernel, grid, block, 0, stream, *P, n, tri, hit, ray, out, flag);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_brdf(int n, const float *params, const float *in_dir, const uint32_t *state_in, float *out_dir,
                                   float *brdf, uint32_t *state_out, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_brdf_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, params, in_dir, state_in, out_dir, brdf, state_out);
  return (int)hipGetLastError();
}

// mode: 0 = ShadeParams, 1 = ShadeParamsLds; + RT_TEST_BG_IMAGE (8): the lookup on the float image, BgImageParams / BgImageParamsLds
extern "C" int rt_launch_test_background(const RT_KParams *P, int mode, int n, const float *dir, float *rgb, hipStream_t stream) {
  const dim3 grid((n + RT_BLOCK_THREADS - 1) / RT_BLOCK_THREADS), block(RT_BLOCK_THREADS);
  const int lds = mode & 1;
  if (mode & 8) {
    if (lds) hipLaunchKernelGGL(rt_test_background_kernel<BgImageParamsLds>, grid, block, 0, stream, *P, n, dir, rgb);
    else hipLaunchKernelGGL(rt_test_background_kernel<BgImageParams>, grid, block, 0, stream, *P, n, dir, rgb);
  } else if (lds) hipLaunchKernelGGL(rt_test_background_kernel<ShadeParamsLds>, grid, block, 0, stream, *P, n, dir, rgb);
  else hipLaunchKernelGGL(rt_test_background_kernel<ShadeParams>, grid, block, 0, stream, *P, n, dir, rgb);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_test_primary_ray(const RT_KParams *P, int n, const int *xys, float *rays, hipStream_t stream) {
  hipLaunchKernelGGL(rt_test_primary_ray_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *P, n, xys, rays);
  return (int)hipGetLastError();
}
