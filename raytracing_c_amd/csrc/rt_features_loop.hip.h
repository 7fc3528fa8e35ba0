// rt_features_loop.hip.h -- the body of rt_features_kernel and rt_features_motion_kernel (rt_features.hip), which include it
// between their braces: NOT a header of declarations.  It reads the kernel's P and F and, as names of the including scope,
//   constexpr bool MOTION;  const float *kept;  unsigned long long *motion_sums;
// MOTION: three more sums per pixel, THE MOTION of the feature hits against the leaf tiles `kept`, into motion_sums
// u64[h][w][RT_MOTION_CHANNELS]; they are reduced and added after the ten, in the same registers.  Without MOTION nothing of it is
// compiled.  The text is shared as text, not as a function: behind a device function, even a forced-inline one, the compiler
// schedules rt_features_kernel<16> differently (4483 instead of 4490 instructions), and that instance is to stay what it was,
// instruction for instruction (profiles/motion.md).

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
    rt_v3 motion = rt_v3_make(0, 0, 0);
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
        if (feature_hit(SP, T.hit, org, dir, albedo, normal, position)) {
          cov = 1.0f;
          if (MOTION) motion = feature_motion(P.leaves, kept, T.hit);
        } else start = ++bounce < P.max_bounces;
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
    if (MOTION) {                                                  // (a lane without a feature hit has motion 0)
      const bool hit_any = q[0] != 0ull;
      q[0] = accum_quantize_signed_dev(motion.x); q[1] = accum_quantize_signed_dev(motion.y); q[2] = accum_quantize_signed_dev(motion.z);
      for (int k = 0; k < shift; k++) {
#pragma unroll
        for (int c = 0; c < RT_MOTION_CHANNELS; c++) q[c] += shfl_xor_u64(q[c], 1 << k);
      }
      if ((lane & ((1 << shift) - 1)) == 0 && hit_any) {
        unsigned long long *dst = motion_sums + ((size_t)y * P.width + x) * RT_MOTION_CHANNELS;
#pragma unroll
        for (int c = 0; c < RT_MOTION_CHANNELS; c++)
          if (q[c] != 0ull) atomicAdd(dst + c, q[c]);
      }
    }
  }
