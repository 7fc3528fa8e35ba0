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

#include "rt_dev.hip.h"

#define RT_FEATURE_CHANNELS 10      // coverage, albedo rgb, normal xyz, position xyz (include/rt_hip.h)

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

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void rt_features_kernel(RT_KParams P, RT_FParams F) {
  extern __shared__ float4 smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n_lds = P.n_lds_nodes;
  pow24_lds_init((int)threadIdx.x);
  lds_load_nodes<WAVES * 64>(smem, P.nodes, n_lds);
  __syncthreads();
  const int leaf_level = P.depth - 1;
  // (the wave's slice is the perm stack alone; no pyramid)
  const TravWave W = {smem, smem, wave_perm(smem, n_lds, perm_stack_f4(P.depth), wave), n_lds, 0, 0, leaf_level, lane};
  const int shift = F.shift;
  uint32_t next = 0, end = 0;                                     // the wave's current grab: units [next, end)
  uint32_t w_nodes = 0, w_leaves = 0;                             // (traversal_blocks counts them; not reported)
  ShadeParamsLds SP;
  shade_params(SP, &P, true);

  for (;;) {
    if (next >= end) {
      uint32_t s = 0;
      if (lane == 0) s = atomicAdd(F.head, (uint32_t)F.grab);
      s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
      if (s >= (uint32_t)F.n_units) break;
      next = s;
      end = ((uint32_t)F.n_units - s < (uint32_t)F.grab) ? (uint32_t)F.n_units : s + (uint32_t)F.grab;
    }
    const uint32_t unit = next++;
    // unit -> (tile, pixel group, sample block); lane -> (pixel of the group, sample of the block), pixel-major
    const uint32_t tile = unit / (uint32_t)F.units_per_tile, r = unit - tile * (uint32_t)F.units_per_tile;
    const uint32_t grp = r / (uint32_t)F.n_sample_blocks, sb = r - grp * (uint32_t)F.n_sample_blocks;
    const int tile_y = (int)(tile / (uint32_t)F.tiles_x), tile_x = (int)tile - tile_y * F.tiles_x;
    const int p = (int)grp * (64 >> shift) + (lane >> shift);     // pixel of the tile, 0 .. 63
    const int x = tile_x * 8 + (p & 7), y = tile_y * 8 + (p >> 3);
    const int sm = P.sample_first + (int)(sb << shift) + (lane & ((1 << shift) - 1));
    const bool valid = x < P.width && y < P.height && sm < P.sample_end && P.max_bounces > 0;

    int   bounce = 0;
    Ray3  ray;
    rt_v3 org = rt_v3_make(0, 0, 0), dir = rt_v3_make(0, 0, 1);
    if (valid) primary_ray(P, x, y, sm, org, dir);
    TravState T = RT_TRAV_IDLE;
    float cov = 0.0f;
    rt_v3 albedo = rt_v3_make(0, 0, 0), normal = rt_v3_make(0, 0, 0), position = rt_v3_make(0, 0, 0);
    bool start = valid;
    for (;;) {
      // a new segment: traversal starts at the root (or at leaf group 0)
      ray_setup<false>(ray, org, dir);
      if (start) trav_start(T, leaf_level, P.last_row_offset);
      const int n_trav0 = (int)__popcll(__ballot(T.phase == PH_NODE || T.phase == PH_LEAF));
      if (n_trav0 == 0) break;
      traversal_blocks<true, false, false>(P, W, ray, false, T, 64, n_trav0, w_nodes, w_leaves);
      // every lane that traversed has ended its segment: a feature hit, a back face (again, while iterations are left), or nothing
      start = false;
      if (T.phase == PH_HIT) {
        if (feature_hit(SP, T.hit, org, dir, albedo, normal, position)) cov = 1.0f;
        else start = ++bounce < P.max_bounces;
      }
      T.phase = PH_NEED;
    }

    // ---- the unit's sums: the samples of a pixel are (1 << shift) neighbouring lanes ----
    if (__ballot(cov != 0.0f) == 0ull) continue;                 // (nothing was hit: nothing to add)
    unsigned long long q[RT_FEATURE_CHANNELS];
    q[0] = cov != 0.0f ? 1ull << 32 : 0ull;                       // rt_accum_quantize(1.0f)
    q[1] = accum_quantize_dev(albedo.x); q[2] = accum_quantize_dev(albedo.y); q[3] = accum_quantize_dev(albedo.z);
    q[4] = accum_quantize_dev(normal.x); q[5] = accum_quantize_dev(normal.y); q[6] = accum_quantize_dev(normal.z);
    q[7] = accum_quantize_signed_dev(position.x); q[8] = accum_quantize_signed_dev(position.y); q[9] = accum_quantize_signed_dev(position.z);
    for (int k = 0; k < shift; k++) {
#pragma unroll
      for (int c = 0; c < RT_FEATURE_CHANNELS; c++) q[c] += shfl_xor_u64(q[c], 1 << k);
    }
    if ((lane & ((1 << shift) - 1)) == 0 && q[0] != 0ull) {       // (q[0] == 0: no sample of this pixel has a feature hit; implies valid pixels only)
      unsigned long long *dst = F.sums + ((size_t)y * P.width + x) * RT_FEATURE_CHANNELS;
#pragma unroll
      for (int c = 0; c < RT_FEATURE_CHANNELS; c++)
        if (q[c] != 0ull) atomicAdd(dst + c, q[c]);
    }
  }
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
