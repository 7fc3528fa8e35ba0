// rt_features.hip -- first-hit feature buffers (include/rt_hip.h: rt_render_accumulate_features, rt_resolve_features): coverage,
// albedo, shading normal and world position of what the camera sees at the first surface, per pixel the mean over the frame's own
// samples.
//
// For pixel (x, y) and sample s the path is the frame's: primary_ray() and cast_ray's loop (raytracer.c:505-558) for at most
// max_bounces iterations -- a hit whose geometric or shading normal faces along the ray is passed through (origin = point +
// EPSILON * direction) and uses up an iteration.  The first hit the reference would hand to a shader is the FEATURE HIT:
//   coverage 1; albedo = base_color (x the decoded albedo texture, driver.c:364-368); normal = debug_shader_proc's emission
//   (driver.c:411-418: the normal-mapped normal * 0.5 + 0.5); position = Shader_Input.position.
// A miss or an exhausted loop adds nothing.  Sums are 32.32 fixed point (rt_math.h; position signed), order-free.
//
// A persistent kernel in the query kernel's launch geometry (rt_kernels.hip, rt_query_kernel): one workgroup per CU, the leading
// BVH nodes in LDS, a perm stack per wave, traversal_blocks() itself for the NODE / LEAF / pop blocks.  The work item is a UNIT
// (RT_FParams, rt_device.h): 64 camera paths of one 8x8 tile, pixel-major, from ONE counter; a wave takes F.grab consecutive units
// per atomic and traces one at a time until every lane has its feature hit, has left the scene or has used up its iterations --
// lanes whose segment ended on a back face go into traversal again from the advanced origin.  The samples of a pixel are
// (1 << shift) neighbouring lanes: their ten sums are reduced in the wave (xor shuffles) and the group's first lane issues one
// 64-bit atomic per non-zero channel.  No pyramid culling; IEEE division in ray_setup and in the leaf blocks.
//
// rt_features_motion_kernel (rt_render_accumulate_features_motion) is the same loop -- one text, rt_features_loop.hip.h -- with
// THE MOTION of a deforming mesh: at a feature hit, where the point (triangle, u, v) WAS in the kept leaf tiles minus where it is
// in the current ones, three more sums per pixel in a buffer of their own; rt_motion_resolve_kernel turns them into means.

#include "rt_dev.hip.h"

#define RT_FEATURE_CHANNELS 10      // coverage, albedo rgb, normal xyz, position xyz (include/rt_hip.h)
#define RT_MOTION_CHANNELS  3       // THE MOTION xyz, in a buffer of its own (include/rt_hip.h)

// rt_accum_quantize_signed() (rt_math.h) on the magnitude path of accum_quantize_dev(): truncation towards zero is symmetric, so
// the signed value is the negated quantised magnitude; NaN -> 0 in both.
__device__ __forceinline__ unsigned long long accum_quantize_signed_dev(float c) {
  const unsigned long long m = accum_quantize_dev(__builtin_fabsf(c));
  return c < 0.0f ? 0ull - m : m;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask) {
  const int lo = __shfl_xor((int)(uint32_t)v, mask, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
  return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

// One accepted closest hit (raytracer.c:515-552): a back face -> `org` advanced, returns false; else the feature values of the
// hit, from surface_at() as shade_hit() reads it and the normal / albedo fetches of shade() (rt_dev.hip.h).
template <class PT>
__device__ __forceinline__ bool feature_hit(const PT &P, const HitRec &hit, rt_v3 &org, const rt_v3 dir, rt_v3 &albedo, rt_v3 &normal,
                                            rt_v3 &position) {
  const Surface s = surface_at(P.tris + (size_t)hit.tri * 28, hit, org, dir);
  const rt_v3 point = s.point;
  if (rt_v3_dot(s.n_geo, dir) > 0.0f || rt_v3_dot(s.n_int, dir) > 0.0f) {
    org = rt_v3_madd(dir, RT_EPS, point);            // back face: pass through, costs an iteration (raytracer.c:516-522)
    return false;
  }
  ShadeIn in;
  in.direction = dir;
  in.normal = normalize_dev(s.n_int);
  in.tangent = s.tangent();
  in.bitangent = s.bitangent();
  in.uvx = s.uvx();
  in.uvy = s.uvy();
  // the material record: base colour, normal-map strength, the albedo and normal textures with their descriptors -- through the
  // scalar cache when every lane has the same material (see shade())
  const int mat = s.material();
  float4 m0;
  float strength;
  int tex_albedo, tex_normal;
  RT_DTexture D[2];
  const int mat0 = __builtin_amdgcn_readfirstlane(mat);
  if (__ballot(mat != mat0) == 0ull) {
    cfloat *sb = as_scalar_ptr(P.mats) + (size_t)mat0 * RT_MAT_FLOATS;
    m0 = make_float4(sb[0], sb[1], sb[2], sb[3]);
    strength = sb[8];
    tex_albedo = as_i(sb[12]); tex_normal = as_i(sb[13]);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      D[k].offset = (uint32_t)as_i(sb[20 + 4 * k]); D[k].width = as_i(sb[21 + 4 * k]); D[k].height = as_i(sb[22 + 4 * k]); D[k].stride = as_i(sb[23 + 4 * k]);
    }
  } else {
    const float *mb = P.mats + (size_t)mat * RT_MAT_FLOATS;
    m0 = ld4(mb, 0);
    const float4 m2 = ld4(mb, 2), m3 = ld4(mb, 3);
    strength = m2.x;
    tex_albedo = as_i(m3.x); tex_normal = as_i(m3.y);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const float4 dk = ld4(mb, 5 + k);
      D[k].offset = (uint32_t)as_i(dk.x); D[k].width = as_i(dk.y); D[k].height = as_i(dk.z); D[k].stride = as_i(dk.w);
    }
  }
  const bool ha = tex_albedo >= 0, hn = tex_normal >= 0;      // (debug materials too: the albedo is the record's, whatever shades it)
  TexTaps tn, ta;
  TexQuad qn, qa;
  if (hn) { tn = tex_taps(D[1], in.uvx, in.uvy); qn = tex_fetch(P.texels + D[1].offset, tn); }
  if (ha) { ta = tex_taps(D[0], in.uvx, in.uvy); qa = tex_fetch(P.texels + D[0].offset, ta); }
  const rt_v3 n = normal_map(hn, hn ? tex_combine(qn, tn) : rt_v3_make(0, 0, 0), strength, in);
  normal = rt_v3_madd(n, 0.5f, rt_v3_make(0.5f, 0.5f, 0.5f));
  albedo = rt_v3_make(m0.x, m0.y, m0.z);
  if (ha) albedo = rt_v3_mul(albedo, srgb_to_linear_tex<Pow24InLds<PT>::value>(tex_combine(qa, ta)));
  position = point;
  return true;
}

// THE MOTION of one feature hit (include/rt_hip.h): where the surface point (tri, u, v) WAS in the kept leaf tiles minus where it is
// in the current ones -- two barycentric evaluations of the tiles' (a, b - a, c - a) columns, plain f32, left to right, nothing
// fused (-ffp-contract=off).  A column that equals its kept column gives +0 bit for bit.
__device__ __forceinline__ rt_v3 feature_motion(const float *leaves, const float *kept, const HitRec &hit) {
  const size_t col = (size_t)(hit.tri >> 3) * 72 + (size_t)(hit.tri & 7);
  const float *l = leaves + col, *lk = kept + col;
  float m[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float cur = (l[(3 * r) * 8] + hit.u * l[(3 * r + 1) * 8]) + hit.v * l[(3 * r + 2) * 8];
    const float was = (lk[(3 * r) * 8] + hit.u * lk[(3 * r + 1) * 8]) + hit.v * lk[(3 * r + 2) * 8];
    m[r] = was - cur;
  }
  return rt_v3_make(m[0], m[1], m[2]);
}

// Both kernels are one text, rt_features_loop.hip.h (see there why it is not a function).
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void rt_features_kernel(RT_KParams P, RT_FParams F) {
  constexpr bool MOTION = false;
  const float *const kept = nullptr;
  unsigned long long *const motion_sums = nullptr;
#include "rt_features_loop.hip.h"
}

// ... with THE MOTION: kept = the leaf tiles as rt_device_scene_keep_geometry saved them (or P.leaves itself: every sum is 0)
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void rt_features_motion_kernel(RT_KParams P, RT_FParams F, const float *kept,
                                                                           unsigned long long *motion_sums) {
  constexpr bool MOTION = true;
#include "rt_features_loop.hip.h"
}

// sums -> means, planar f32: coverage [h][w], albedo / normal / position [h][w][3]; one thread per pixel, NULL = not wanted
__global__ void rt_features_resolve_kernel(int n_pixels, int samples, const unsigned long long *sums, float *coverage, float *albedo,
                                           float *normal, float *position) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pixels) return;
  const unsigned long long *s = sums + (size_t)i * RT_FEATURE_CHANNELS;
  if (coverage) coverage[i] = rt_accum_resolve(s[0], (uint32_t)samples);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (albedo) albedo[(size_t)i * 3 + c] = rt_accum_resolve(s[1 + c], (uint32_t)samples);
    if (normal) normal[(size_t)i * 3 + c] = rt_accum_resolve(s[4 + c], (uint32_t)samples);
    if (position) position[(size_t)i * 3 + c] = rt_accum_resolve_signed(s[7 + c], (uint32_t)samples);
  }
}

// motion sums -> means, f32[h][w][3] (what the motion accumulation divides by the coverage); one thread per pixel
__global__ void rt_motion_resolve_kernel(int n_pixels, int samples, const unsigned long long *sums, float *motion) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pixels) return;
#pragma unroll
  for (int c = 0; c < RT_MOTION_CHANNELS; c++)
    motion[(size_t)i * RT_MOTION_CHANNELS + c] = rt_accum_resolve_signed(sums[(size_t)i * RT_MOTION_CHANNELS + c], (uint32_t)samples);
}

// `n_blocks` workgroups of 16 waves; smem_bytes = the LDS nodes + 16 perm stacks (lds_split as rt_features.cpp, enqueue_features, calls it)
extern "C" int rt_launch_features(const RT_KParams *P, const RT_FParams *F, int n_blocks, int smem_bytes, hipStream_t stream) {
  static uint32_t attr_devices = 0;
  if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&rt_features_kernel<16>), &attr_devices, smem_bytes,
                               RT_LDS_BYTES - RT_LDS_TABLE_BYTES))      // (the kernel has the sRGB scale table)
    return rc;
  hipLaunchKernelGGL((rt_features_kernel<16>), dim3(n_blocks), dim3(16 * 64), smem_bytes, stream, *P, *F);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_features_resolve(int n_pixels, int samples, const unsigned long long *sums, float *coverage, float *albedo,
                                          float *normal, float *position, hipStream_t stream) {
  hipLaunchKernelGGL(rt_features_resolve_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, samples, sums, coverage,
                     albedo, normal, position);
  return (int)hipGetLastError();
}

// rt_launch_features with THE MOTION (the same launch geometry; one launch, not two)
extern "C" int rt_launch_features_motion(const RT_KParams *P, const RT_FParams *F, const float *kept, unsigned long long *motion_sums,
                                         int n_blocks, int smem_bytes, hipStream_t stream) {
  static uint32_t attr_devices = 0;
  if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&rt_features_motion_kernel<16>), &attr_devices, smem_bytes,
                               RT_LDS_BYTES - RT_LDS_TABLE_BYTES))
    return rc;
  hipLaunchKernelGGL((rt_features_motion_kernel<16>), dim3(n_blocks), dim3(16 * 64), smem_bytes, stream, *P, *F, kept, motion_sums);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_motion_resolve(int n_pixels, int samples, const unsigned long long *sums, float *motion, hipStream_t stream) {
  hipLaunchKernelGGL(rt_motion_resolve_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, stream, n_pixels, samples, sums, motion);
  return (int)hipGetLastError();
}
