// rt_probes.hip -- light probes (include/rt_hip.h: rt_probe_trace, rt_probe_project, rt_probe_resolve): the incoming radiance at
// points a host supplies, as path-traced samples over the whole sphere and as their projection onto the nine real spherical
// harmonics of bands 0-2.
//
// For probe i (global index g = probe_first + i, position o) and sample s the path is
//   state = rt_path_seed(seed, g, s);  d = rt_rand_unit_vec3(&state);  L = cast_ray({o, d}, max_bounces, &state)
// (raytracer.c:505-558; the RNG stream goes on where the direction left it), t = the distance of the first segment's closest hit,
// +inf on a miss and when no ray is cast.  Record j = i * sample_count + (s - sample_first) is {L, t, d, 0}: two 16-byte stores.
//
// rt_probe_kernel: a persistent kernel in the query kernel's launch geometry (rt_kernels.hip, rt_query_kernel): one workgroup of 16
// waves per CU, the leading BVH nodes in LDS, a perm stack per wave, traversal_blocks() itself for the NODE / LEAF / pop blocks, ONE
// work counter for the launch and that kernel's grab rule; lanes are refilled as their paths end, so the lanes of a wave may hold
// samples of different probes.  Per round: traversal until R.exit_lanes lanes wait (64 once the counter has run dry), then the S
// block of the path kernel without its parking -- environment for the misses, shade_hit() for the hits, records of the paths that
// ended, new paths for the idle lanes.  IEEE division in ray_setup and in the leaf blocks (a caller's position carries no bound,
// see rt_query_kernel), no pyramid.
//
// rt_probe_project_kernel: records -> 27 sums per probe (9 coefficients x rgb, k-major), rt_accum_quantize_signed(L[c] * Y_k),
// 32.32, order-free, added with atomics so that a buffer can be filled by sample ranges.  rt_probe_resolve_kernel: sums -> the
// coefficients, rt_accum_resolve_signed(sum, samples) * 4 pi.

#include "rt_dev.hip.h"

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void rt_probe_kernel(RT_KParams P, RT_PParams R) {
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
  int   idx = 0, bounce = 0;
  uint32_t rng = 0;
  float t_first = RT_INF;                                         // the first segment's closest hit, for the record
  Ray3  ray;
  ray_setup(ray, rt_v3_make(0, 0, 0), rt_v3_make(0, 0, 1));
  rt_v3 tint = rt_v3_make(1, 1, 1), emis = rt_v3_make(0, 0, 0);
  TravState T = RT_TRAV_IDLE;
  float4 *const records = reinterpret_cast<float4 *>(R.records);

  for (;;) {
    // ================= S: shade the hits, environment for the misses, records of the paths that ended =================
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
        if (bounce == 0) t_first = T.hit.t;                       // (back faces and shaded hits both use up an iteration: 0 = the first segment)
        done = shade_hit(SP, T.hit, org, dir, tint, emis, rng, bounce, cn, radiance);
        start = !done;
      }
      if (done) {
        records[(size_t)idx * RT_PROBE_RECORD_F4] = make_float4(radiance.x, radiance.y, radiance.z, t_first);
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
        idx = next + rank;
        const uint32_t probe = (uint32_t)idx / (uint32_t)R.sample_count;
        const uint32_t sample = (uint32_t)R.sample_first + ((uint32_t)idx - probe * (uint32_t)R.sample_count);
        rng = rt_path_seed(P.seed, R.probe_first + probe, sample);
        dir = rt_rand_unit_vec3(&rng);
        const float *o = R.positions + (size_t)probe * 3;
        org = rt_v3_make(o[0], o[1], o[2]);
        // (the record's second half now, while the direction is at hand: a path keeps no copy of it across its bounces)
        records[(size_t)idx * RT_PROBE_RECORD_F4 + 1] = make_float4(dir.x, dir.y, dir.z, 0.0f);
        if (P.max_bounces > 0) {
          bounce = 0;
          t_first = RT_INF;
          tint = rt_v3_make(1, 1, 1);
          emis = rt_v3_make(0, 0, 0);
          start = true;
        } else {
          // no ray is cast (raytracer.c:512 runs zero times): the emission, 0, and no first hit; the lane asks again
          records[(size_t)idx * RT_PROBE_RECORD_F4] = make_float4(0.0f, 0.0f, 0.0f, RT_INF);
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

__device__ __forceinline__ unsigned long long probe_shfl_xor_u64(unsigned long long v, int mask) {
  const int lo = __shfl_xor((int)(uint32_t)v, mask, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
  return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

// One workgroup of 256 threads per probe: every thread strides over the probe's records with 27 sums in registers; the sums are
// reduced in the wave (xor shuffles), across the four waves through LDS, and 27 threads add them to the probe's row of d_sums.
#define RT_PROJECT_THREADS 256
__global__ __launch_bounds__(RT_PROJECT_THREADS) void rt_probe_project_kernel(int sample_count, const float *records_f,
                                                                              unsigned long long *sums) {
  __shared__ unsigned long long part[RT_PROJECT_THREADS / 64][RT_PROBE_SUMS];
  const float4 *rec = reinterpret_cast<const float4 *>(records_f) + (size_t)blockIdx.x * (size_t)sample_count * RT_PROBE_RECORD_F4;
  unsigned long long q[RT_PROBE_SUMS];
#pragma unroll
  for (int k = 0; k < RT_PROBE_SUMS; k++) q[k] = 0ull;
  for (int s = (int)threadIdx.x; s < sample_count; s += RT_PROJECT_THREADS) {
    const float4 a = rec[(size_t)s * RT_PROBE_RECORD_F4], b = rec[(size_t)s * RT_PROBE_RECORD_F4 + 1];
    float y[RT_SH9];
    rt_sh9_basis(rt_v3_make(b.x, b.y, b.z), y);                  // (the record's direction, not a recomputed one)
    const float L[3] = {a.x, a.y, a.z};
#pragma unroll
    for (int k = 0; k < RT_SH9; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) q[k * 3 + c] += rt_accum_quantize_signed(L[c] * y[k]);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1)
#pragma unroll
    for (int k = 0; k < RT_PROBE_SUMS; k++) q[k] += probe_shfl_xor_u64(q[k], m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RT_PROBE_SUMS; k++) part[wave][k] = q[k];
  }
  __syncthreads();
  if (threadIdx.x < RT_PROBE_SUMS) {
    unsigned long long v = 0ull;
#pragma unroll
    for (int w = 0; w < RT_PROJECT_THREADS / 64; w++) v += part[w][threadIdx.x];
    atomicAdd(sums + (size_t)blockIdx.x * RT_PROBE_SUMS + threadIdx.x, v);
  }
}

// sums -> coefficients: the mean over ALL `samples` of the probe, rounded once, times 4 pi (one f32 multiply); one thread each
__global__ void rt_probe_resolve_kernel(long long n_coeffs, int samples, const unsigned long long *sums, float *coeffs) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_coeffs) return;
  coeffs[i] = rt_accum_resolve_signed(sums[i], (uint32_t)samples) * RT_FOUR_PI;
}

// `n_blocks` workgroups of 16 waves; smem_bytes = the LDS nodes + 16 perm stacks (lds_split as rt_query.cpp, enqueue_trace, calls it)
extern "C" int rt_launch_probes(const RT_KParams *P, const RT_PParams *R, int n_blocks, int smem_bytes, hipStream_t stream) {
  static uint32_t attr_devices = 0;
  if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&rt_probe_kernel<16>), &attr_devices, smem_bytes,
                               RT_LDS_BYTES - RT_LDS_TABLE_BYTES))      // (the kernel has the sRGB scale table)
    return rc;
  hipLaunchKernelGGL((rt_probe_kernel<16>), dim3(n_blocks), dim3(16 * 64), smem_bytes, stream, *P, *R);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_probe_project(int n_probes, int sample_count, const float *records, unsigned long long *sums,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(rt_probe_project_kernel, dim3(n_probes), dim3(RT_PROJECT_THREADS), 0, stream, sample_count, records, sums);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_probe_resolve(long long n_coeffs, int samples, const unsigned long long *sums, float *coeffs,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(rt_probe_resolve_kernel, dim3((unsigned)((n_coeffs + 255) / 256)), dim3(256), 0, stream, n_coeffs, samples, sums,
                     coeffs);
  return (int)hipGetLastError();
}
