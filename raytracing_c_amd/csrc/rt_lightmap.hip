// rt_lightmap.hip -- HDR lightmaps (include/rt_hip.h: rt_lightmap_texels, rt_lightmap_trace, rt_lightmap_resolve,
// rt_lightmap_dilate): the light arriving at the texels of a UV layout, as order-free 32.32 sums that can be filled by sample and
// texel ranges, a float image, and seam padding around the charts.  lightmap_bake (rt_kernels.hip) stays the reference's entry point.
//
// THE TEXEL LIST.  rt_lightmap_texel_owner_kernel: one workgroup per triangle slot, atomicMax -- the LAST slot whose UV triangle
// accepts the integer point (x, y) owns it (rt_lightmap_weights.hip.h: the one text of the acceptance test).  rt_lightmap_row_count_
// kernel + rt_lightmap_row_scan_kernel: owned texels per row, then their exclusive prefix sums in ONE workgroup.
// rt_lightmap_texel_write_kernel: one wave per row walks it in 64-texel steps, ballot + lane rank, so that the list is row-major
// without a sort; entry j = {position + normal * EPSILON, texel index, normal, triangle}, the plain f32 expressions of
// rt_lightmap_bake_kernel, every operation rounded on its own.
//
// rt_lightmap_kernel: a sibling of rt_probe_kernel (rt_probes.hip) -- one workgroup of 16 waves per CU, the leading BVH nodes in
// LDS, a perm stack per wave, traversal_blocks() itself, ONE work counter and the query kernel's grab rule, the S block of the path
// kernel without its parking, IEEE division (a caller's scene gives no bound for these origins), no pyramid.  Path idx of a launch
// is sample s0 + idx / m of list entry j0 + idx % m (sample-major: the lanes a refill fills read one contiguous run of 32-byte
// entries and end on distinct addresses).  A path draws directions from rt_path_seed(seed, texel, s) until one has a positive cosine c
// with the entry's normal, at most RT_LIGHTMAP_TRIES times; cast_ray goes on from that state; the lane that ends the path adds
// rt_accum_quantize(L[ch] * c) to sums[j][ch] with three 64-bit atomics.  Beyond the probe kernel's lane state: c and j.
//
// rt_lightmap_resolve_kernel: one thread per list entry, {rt_accum_resolve(sum, samples) * scale, 1}.  rt_lightmap_dilate_kernel:
// one pass of the seam padding over a 32 x 8 tile with a one-texel halo staged in LDS (rt_denoise.hip's tile).

#include "rt_dev.hip.h"
#include "rt_lightmap_weights.hip.h"

// ---- the texel list ------------------------------------------------------------------------------------------------------------
__global__ void rt_lightmap_texel_owner_kernel(const float *tris, int n_tris, int lw, int lh, int *owner) {
  int i = blockIdx.x;
  if (i >= n_tris) return;
  const float *tb = tris + (size_t)i * 28;
  float uax = tb[7], uay = tb[11], ubx = tb[15], uby = tb[19], ucx = tb[23], ucy = tb[24];
  float flw = (float)lw, flh = (float)lh;
  int min_x = (int)(min3f(uax, ubx, ucx) * flw), max_x = (int)(max3f(uax, ubx, ucx) * flw);
  int min_y = (int)(min3f(uay, uby, ucy) * flh), max_y = (int)(max3f(uay, uby, ucy) * flh);
  float p0x = uax * flw, p0y = uay * flh, p1x = ubx * flw, p1y = uby * flh, p2x = ucx * flw, p2y = ucy * flh;
  // clip the loop to the image (texels outside are skipped, see oracle.h)
  int x0 = min_x < 0 ? 0 : min_x, x1 = max_x >= lw ? lw - 1 : max_x;
  int y0 = min_y < 0 ? 0 : min_y, y1 = max_y >= lh ? lh - 1 : max_y;
  int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
  if (bw <= 0 || bh <= 0) return;
  for (long long t = threadIdx.x; t < (long long)bw * bh; t += blockDim.x) {
    int x = x0 + (int)(t % bw), y = y0 + (int)(t / bw);
    float w0, w1, w2;
    if (lightmap_weights(p0x, p0y, p1x, p1y, p2x, p2y, x, y, w0, w1, w2)) atomicMax(&owner[(size_t)y * lw + x], i);
  }
}

// one wave per row: rows[y] = the number of owned texels of row y
__global__ __launch_bounds__(64) void rt_lightmap_row_count_kernel(int lw, const int *owner, int *rows) {
  const int y = blockIdx.x, lane = threadIdx.x;
  const int *row = owner + (size_t)y * lw;
  int n = 0;
  for (int x0 = 0; x0 < lw; x0 += 64) {
    const bool own = x0 + lane < lw && row[x0 + lane] >= 0;
    n += (int)__popcll(__ballot(own));
  }
  if (lane == 0) rows[y] = n;
}

// ONE workgroup: rows[] becomes its exclusive prefix sums, *count the total
#define RT_SCAN_THREADS 256
__global__ __launch_bounds__(RT_SCAN_THREADS) void rt_lightmap_row_scan_kernel(int lh, int *rows, long long *count) {
  __shared__ int part[RT_SCAN_THREADS];
  __shared__ int carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < lh; base += RT_SCAN_THREADS) {
    const int i = base + t;
    const int v = i < lh ? rows[i] : 0;
    part[t] = v;
    __syncthreads();
    for (int d = 1; d < RT_SCAN_THREADS; d <<= 1) {      // Hillis-Steele, inclusive
      const int a = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += a;
      __syncthreads();
    }
    const int before = carry;
    if (i < lh) rows[i] = before + part[t] - v;
    __syncthreads();
    if (t == RT_SCAN_THREADS - 1) carry = before + part[t];
    __syncthreads();
  }
  if (t == 0) *count = (long long)carry;
}

// one wave per row: the row's owned texels, in x order, from list index rows[y] on
__global__ __launch_bounds__(64) void rt_lightmap_texel_write_kernel(const float *tris, const float *verts, int lw, int lh,
                                                                     const int *owner, const int *rows, float4 *texels) {
  const int y = blockIdx.x, lane = threadIdx.x;
  const int *row = owner + (size_t)y * lw;
  const float flw = (float)lw, flh = (float)lh;
  int at = rows[y];
  for (int x0 = 0; x0 < lw; x0 += 64) {
    const int x = x0 + lane;
    const int i = x < lw ? row[x] : -1;
    const unsigned long long own = __ballot(i >= 0);
    if (i >= 0) {
      const float *tb = tris + (size_t)i * 28;
      float w0, w1, w2;
      lightmap_weights(tb[7] * flw, tb[11] * flh, tb[15] * flw, tb[19] * flh, tb[23] * flw, tb[24] * flh, x, y, w0, w1, w2);
      const float *v = verts + (size_t)i * 9;       // x0 x1 x2 y0 y1 y2 z0 z1 z2 (original vertices, scene.h:53-60)
      rt_v3 position = rt_v3_make(v[0] * w0 + v[1] * w1 + v[2] * w2, v[3] * w0 + v[4] * w1 + v[5] * w2,
                                  v[6] * w0 + v[7] * w1 + v[8] * w2);
      rt_v3 normal = rt_v3_make(tb[4] * w0 + tb[8] * w1 + tb[12] * w2, tb[5] * w0 + tb[9] * w1 + tb[13] * w2,
                                tb[6] * w0 + tb[10] * w1 + tb[14] * w2);
      rt_v3 org = rt_v3_add(position, rt_v3_scale(normal, RT_EPS));
      float4 *e = texels + (size_t)(at + lane_rank(own)) * RT_LIGHTMAP_TEXEL_F4;
      e[0] = make_float4(org.x, org.y, org.z, __uint_as_float((uint32_t)x + (uint32_t)y * (uint32_t)lw));
      e[1] = make_float4(normal.x, normal.y, normal.z, __int_as_float(i));
    }
    at += (int)__popcll(own);
  }
}

// ---- the paths -----------------------------------------------------------------------------------------------------------------
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void rt_lightmap_kernel(RT_KParams P, RT_LParams R) {
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
  int  next = 0, end = 0;                                         // the wave's current grab: paths [next, end) are not handed out yet
  bool drained = false;                                           // the launch's counter has run past the list (wave-uniform)
  uint32_t w_paths = 0, w_rays = 0, w_nodes = 0, w_leaves = 0, w_shades = 0, w_bgs = 0, w_tex = 0;

  // ---------------- per-lane state ----------------
  int   j = 0, bounce = 0;                                        // j: the list entry the lane's path adds to
  uint32_t rng = 0;
  float cosv = 0.0f;                                              // c = dot(direction, normal) of the lane's path
  Ray3  ray;
  ray_setup(ray, rt_v3_make(0, 0, 0), rt_v3_make(0, 0, 1));
  rt_v3 tint = rt_v3_make(1, 1, 1), emis = rt_v3_make(0, 0, 0);
  TravState T = RT_TRAV_IDLE;
  const float4 *const texels = reinterpret_cast<const float4 *>(R.texels);

  for (;;) {
    // ================= S: shade the hits, environment for the misses, the adds of the paths that ended =================
    bool start = false;
    rt_v3 org = ray.o, dir = ray.d;
    {
      LaneCounters cn;
      cn.rays = cn.nodes = cn.leaves = cn.shades = cn.bgs = cn.textured = cn.paths = 0;
      bool  done = false;
      rt_v3 radiance = rt_v3_make(0, 0, 0);
      ShadeParamsLds SP;
      shade_params(SP, &P, true);
      if (T.phase == PH_MISS) {
        cn.bgs = 1;
        radiance = rt_v3_mul_add(background_lookup(SP, dir), tint, emis);
        done = true;
      }
      if (T.phase == PH_HIT) {
        done = shade_hit(SP, T.hit, org, dir, tint, emis, rng, bounce, cn, radiance);
        start = !done;
      }
      if (done) {
#ifndef RT_LIGHTMAP_NO_ADDS                                       // (a timing-only build: the kernel without its adds, profiles/lightmap_hdr.md)
        unsigned long long *q = R.sums + (size_t)j * 3;
        atomicAdd(q + 0, (unsigned long long)rt_accum_quantize(radiance.x * cosv));
        atomicAdd(q + 1, (unsigned long long)rt_accum_quantize(radiance.y * cosv));
        atomicAdd(q + 2, (unsigned long long)rt_accum_quantize(radiance.z * cosv));
#endif
        T.phase = PH_NEED;
      }
      w_shades += (uint32_t)__popcll(__ballot(cn.shades != 0));
      w_tex += (uint32_t)__popcll(__ballot(cn.textured != 0));
      w_bgs += (uint32_t)__popcll(__ballot(cn.bgs != 0));
    }

    // ---- regeneration: every lane without a path takes the next one of the wave's grab; a grab that runs out is followed by the next ----
    for (;;) {
      const unsigned long long need = __ballot(T.phase == PH_NEED && !start);      // (start: took a path in this block already)
      if (need == 0ull || drained) break;
      if (next >= end) {
        uint32_t s = 0;
        if (lane == 0) s = atomicAdd(R.head, (uint32_t)R.grab);
        s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
        if (s >= (uint32_t)R.n_paths) { drained = true; break; }
        next = (int)s;
        end = (R.n_paths - next < R.grab) ? R.n_paths : next + R.grab;
      }
      const int rank = lane_rank(need);
      const bool got = T.phase == PH_NEED && !start && next + rank < end;
      if (got) {
        const uint32_t idx = (uint32_t)(next + rank);
        const uint32_t ds = idx / (uint32_t)R.m;
        j = R.texel_first + (int)(idx - ds * (uint32_t)R.m);
        const float4 ta = texels[(size_t)j * RT_LIGHTMAP_TEXEL_F4], tb = texels[(size_t)j * RT_LIGHTMAP_TEXEL_F4 + 1];
        const rt_v3 normal = rt_v3_make(tb.x, tb.y, tb.z);
        rng = rt_path_seed(P.seed, __float_as_uint(ta.w), (uint32_t)R.sample_first + ds);
        // a direction in the normal's hemisphere, by rejection; a zero or NaN normal accepts none and the path is given up:
        // nothing is cast, nothing is added, the lane asks again.  max_bounces == 0: no ray is cast either (raytracer.c:512 runs
        // zero times), L = 0, nothing to add.
        bool accepted = false;
        if (P.max_bounces > 0) {
          for (int tries = 0; tries < RT_LIGHTMAP_TRIES && !accepted; tries++) {
            dir = rt_rand_unit_vec3(&rng);
            cosv = rt_v3_dot(dir, normal);
            accepted = cosv > 0.0f;
          }
        }
        if (accepted) {
          org = rt_v3_make(ta.x, ta.y, ta.z);
          bounce = 0;
          tint = rt_v3_make(1, 1, 1);
          emis = rt_v3_make(0, 0, 0);
          start = true;
        }
      }
      w_paths += (uint32_t)__popcll(__ballot(got));
      next += (int)__popcll(need);
    }
    if (start) {                          // a new ray: traversal starts at the root (or at leaf group 0)
      ray_setup<false>(ray, org, dir);
      trav_start(T, leaf_level, P.last_row_offset);
    }
    w_rays += (uint32_t)__popcll(__ballot(start));

    const int n_trav0 = (int)__popcll(__ballot(T.phase == PH_NODE || T.phase == PH_LEAF));
    if (n_trav0 == 0) break;                                      // (only a drained wave gets here without a ray in flight)
    traversal_blocks<true, false, false>(P, W, ray, false, T, drained ? 64 : R.exit_lanes, n_trav0, w_nodes, w_leaves);
  }
  if (lane == 0) {
    atomicAdd(R.counters + RT_CNT_PATHS, (unsigned long long)w_paths);
    atomicAdd(R.counters + RT_CNT_RAYS, (unsigned long long)w_rays);
    atomicAdd(R.counters + RT_CNT_NODES, (unsigned long long)w_nodes);
    atomicAdd(R.counters + RT_CNT_LEAVES, (unsigned long long)w_leaves);
    atomicAdd(R.counters + RT_CNT_SHADES, (unsigned long long)w_shades);
    atomicAdd(R.counters + RT_CNT_BG, (unsigned long long)w_bgs);
    atomicAdd(R.counters + RT_CNT_TEXTURED, (unsigned long long)w_tex);
  }
}

// ---- the resolve ---------------------------------------------------------------------------------------------------------------
// sums -> the image, one thread per list entry: the mean over ALL `samples`, rounded once, times scale (one f32 multiply); .w = 1
__global__ void rt_lightmap_resolve_kernel(long long n, long long n_pixels, int samples, float scale, const float4 *texels,
                                           const unsigned long long *sums, float4 *image) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint32_t p = __float_as_uint(texels[(size_t)e * RT_LIGHTMAP_TEXEL_F4].w);
  if ((long long)p >= n_pixels) return;                           // (a list of another map: no store outside this one)
  const unsigned long long *q = sums + (size_t)e * 3;
  image[p] = make_float4(rt_accum_resolve(q[0], (uint32_t)samples) * scale, rt_accum_resolve(q[1], (uint32_t)samples) * scale,
                         rt_accum_resolve(q[2], (uint32_t)samples) * scale, 1.0f);
}

// ---- the dilation --------------------------------------------------------------------------------------------------------------
#define LM_TX 32      // texels per workgroup tile: 32 x 8, one thread per texel
#define LM_TY 8

// One pass: a texel with .w == 0 in `src` becomes the mean of its neighbours with .w > 0 -- visited dy = -1, 0, 1 and inside that
// dx = -1, 0, 1, f32 adds in that order from the first usable neighbour's value, one IEEE division by their number -- and
// .w = w_filled; every other texel, and one without such a neighbour, is copied.  Halo slots off the image hold .w = 0: skipped.
__global__ __launch_bounds__(LM_TX * LM_TY) void rt_lightmap_dilate_kernel(int width, int height, int tiles_x, float w_filled,
                                                                            const float4 *src, float4 *dst) {
  __shared__ float4 tile[(LM_TY + 2) * (LM_TX + 2)];
  const int tid = threadIdx.y * LM_TX + threadIdx.x;
  const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);      // (a flat grid: a map may be 2^28 rows high)
  const int x0 = bx * LM_TX - 1, y0 = by * LM_TY - 1;
  for (int i = tid; i < (LM_TY + 2) * (LM_TX + 2); i += LM_TX * LM_TY) {
    const int xx = x0 + i % (LM_TX + 2), yy = y0 + i / (LM_TX + 2);
    const bool on = xx >= 0 && xx < width && yy >= 0 && yy < height;
    tile[i] = on ? src[(size_t)yy * width + xx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  __syncthreads();
  const int x = bx * LM_TX + threadIdx.x, y = by * LM_TY + threadIdx.y;
  if (x >= width || y >= height) return;
  const int centre = (threadIdx.y + 1) * (LM_TX + 2) + threadIdx.x + 1;
  float4 out = tile[centre];
  if (out.w == 0.0f) {
    float r = 0.0f, g = 0.0f, b = 0.0f;
    int n = 0;
#pragma unroll
    for (int t = 0; t < 9; t++) {
      if (t == 4) continue;
      const float4 v = tile[(threadIdx.y + t / 3) * (LM_TX + 2) + threadIdx.x + t % 3];
      if (v.w > 0.0f) {
        r = n ? r + v.x : v.x;
        g = n ? g + v.y : v.y;
        b = n ? b + v.z : v.z;
        n++;
      }
    }
    if (n) out = make_float4(r / (float)n, g / (float)n, b / (float)n, w_filled);
  }
  dst[(size_t)y * width + x] = out;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
// owner: i32[width x height] set to -1 by the caller on the same stream; rows: i32[height]
extern "C" int rt_launch_lightmap_texels(const float *tris, const float *verts, int n_tris, int lw, int lh, int *owner, int *rows,
                                         float *texels, long long *count, hipStream_t stream) {
  if (n_tris > 0) hipLaunchKernelGGL(rt_lightmap_texel_owner_kernel, dim3(n_tris), dim3(64), 0, stream, tris, n_tris, lw, lh, owner);
  hipLaunchKernelGGL(rt_lightmap_row_count_kernel, dim3(lh), dim3(64), 0, stream, lw, (const int *)owner, rows);
  hipLaunchKernelGGL(rt_lightmap_row_scan_kernel, dim3(1), dim3(RT_SCAN_THREADS), 0, stream, lh, rows, count);
  hipLaunchKernelGGL(rt_lightmap_texel_write_kernel, dim3(lh), dim3(64), 0, stream, tris, verts, lw, lh, (const int *)owner,
                     (const int *)rows, reinterpret_cast<float4 *>(texels));
  return (int)hipGetLastError();
}

// `n_blocks` workgroups of 16 waves; smem_bytes = the LDS nodes + 16 perm stacks (lds_split as rt_extras.cpp, enqueue_lightmap_trace, calls it)
extern "C" int rt_launch_lightmap_trace(const RT_KParams *P, const RT_LParams *R, int n_blocks, int smem_bytes, hipStream_t stream) {
  static uint32_t attr_devices = 0;
  if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&rt_lightmap_kernel<16>), &attr_devices, smem_bytes,
                               RT_LDS_BYTES - RT_LDS_TABLE_BYTES))      // (the kernel has the sRGB scale table)
    return rc;
  hipLaunchKernelGGL((rt_lightmap_kernel<16>), dim3(n_blocks), dim3(16 * 64), smem_bytes, stream, *P, *R);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_lightmap_resolve(long long n, long long n_pixels, int samples, float scale, const float *texels,
                                          const unsigned long long *sums, float *image, hipStream_t stream) {
  hipLaunchKernelGGL(rt_lightmap_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, n_pixels, samples, scale,
                     reinterpret_cast<const float4 *>(texels), sums, reinterpret_cast<float4 *>(image));
  return (int)hipGetLastError();
}

extern "C" int rt_launch_lightmap_dilate(int width, int height, int pass, const float *src, float *dst, hipStream_t stream) {
  const int tiles_x = (width + LM_TX - 1) / LM_TX, tiles_y = (height + LM_TY - 1) / LM_TY;
  dim3 block(LM_TX, LM_TY), grid((unsigned)tiles_x * (unsigned)tiles_y);
  hipLaunchKernelGGL(rt_lightmap_dilate_kernel, grid, block, 0, stream, width, height, tiles_x, (float)(1 + pass),
                     reinterpret_cast<const float4 *>(src), reinterpret_cast<float4 *>(dst));
  return (int)hipGetLastError();
}
