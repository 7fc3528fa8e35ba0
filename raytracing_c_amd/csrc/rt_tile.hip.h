// rt_tile.hip.h -- the stages of the tile loop of the kernels in which a wave owns an 8x8-pixel tile: the path kernel
// (rt_path_kernel_stream, rt_kernels.hip) and the camera kernel of the wavefront pipeline (rt_wf_camera_kernel, rt_wavefront.hip;
// its trace kernel shares the wave's LDS slice and flush_tile).  Included at the end of rt_dev.hip.h.  One pass of the loop:
//
//   take_queue_tile / join_open_tile   a tile of its own from the queue, or one that still has units
//   tile_origin                        where the tile lies in the image (and in which view)
//   tile_pyramid                       the tile's camera-ray pyramid into the wave's LDS slice; can a camera ray touch the root's children?
//   leafless_walk                      (path kernel) does the pyramid, pruned through the tree, reach a triangle at all?
//   grab_units / unit_decode           the tile's units, one or more per atomic, and the pixels and samples of a unit
//   regen_paths                        the wave's idle lanes take the next paths of the tile's units
//   flush_tile                         the wave's accumulator tile to the frame
//
// Every stage is wave-uniform in what it decides.  Kernel arguments are read through cold_args() where they are used (rt_dev.hip.h),
// `lane` is the kernel's own lane index, `lg` the wave's ledger row (LG_ARG; ledger builds only).
#ifndef RT_TILE_HIP_H
#define RT_TILE_HIP_H

// Multi-view launches (VIEWS, rt_render_views): the tile list is n_views x n_local_chunks x 16 tiles long, tile t renders view
// t / tiles_per_view.  A wave keeps only the pointer to its tile's view record (scalar, constant address space) and reads the
// camera and seed from it where the one-view kernel reads them from the kernel arguments.
typedef const RT_KView __attribute__((address_space(4))) *RT_KViewP;
template <bool VIEWS> struct CamSrc { typedef RT_KArgs type; };       // where camera and seed come from
template <> struct CamSrc<true> { typedef RT_KViewP type; };

// The next tile of the queue (expensive tiles first), or -1 when the queue has run dry: `queue_open` goes false.
__device__ __forceinline__ int take_queue_tile(const int lane, bool &queue_open) {
  RT_KArgs A = cold_args();
  uint32_t pos = 0;
  if (lane == 0) pos = atomicAdd(A->work_head, 1u);
  pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);
  const uint32_t *order = A->order;
  if (pos < (uint32_t)A->n_tiles) return order ? (int)order[pos] : (int)pos;
  queue_open = false;
  return -1;
}

// A tile that still has units, or -1.  Two-level scan with agent-scope loads: groups of 64 tiles that still have an open tile
// (open_groups[g] > 0), then the tiles of one such group.  Start positions differ per wave and per try so that joiners spread
// over the open tiles.
__device__ __forceinline__ int join_open_tile(const int lane, const int wave_id, const int steal_tries, const uint32_t n_chunks_tile,
                                              uint32_t *lg = nullptr) {
  LGT0();
  int tile_idx = -1;
  RT_KArgs A = cold_args();
  const int n_tiles = A->n_tiles;
  const uint32_t *open_groups = A->open_groups, *tile_next = A->tile_next;
  const int n_groups = (n_tiles + 63) >> 6;
  const int g_rounds = (n_groups + 63) >> 6;
  const uint32_t hsh = ((uint32_t)wave_id * 2654435761u + (uint32_t)steal_tries * 40503u) >> 8;
  const int g_start = (int)(hsh % (uint32_t)g_rounds);
  for (int i = 0; i < g_rounds && tile_idx < 0; i++) {
    int r = g_start + i;
    if (r >= g_rounds) r -= g_rounds;
    int g = r * 64 + lane;
    uint32_t n_open = 0;
    if (g < n_groups) n_open = __hip_atomic_load(&open_groups[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long gm = __ballot(n_open != 0u);
    while (gm && tile_idx < 0) {
      int nth = (int)((hsh >> 6) % (uint32_t)__popcll(gm));
      unsigned long long m = gm;
      for (int k = 0; k < nth; k++) m &= m - 1ull;
      int gl = (int)__builtin_ctzll(m);
      gm &= ~(1ull << gl);
      int cand = (r * 64 + gl) * 64 + lane;
      uint32_t taken = 0xFFFFFFFFu;
      if (cand < n_tiles) taken = __hip_atomic_load(&tile_next[cand], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned long long open = __ballot(taken < n_chunks_tile);
      if (open) {
        // two random open tiles of the group, the one with more units left: fewer, longer joins (every join ends with
        // a drain of the paths in flight)
        const int n_open_tiles = (int)__popcll(open);
        int best = 0;
        uint32_t best_taken = 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < RT_JOIN_CHOICES; c++) {
          int nt = (int)(((hsh >> 12) * (uint32_t)(2 * c + 1) + (uint32_t)c * 7u) % (uint32_t)n_open_tiles);
          unsigned long long mm = open;
          for (int k = 0; k < nt; k++) mm &= mm - 1ull;
          const int pk_lane = (int)__builtin_ctzll(mm);
          const uint32_t tk = (uint32_t)__builtin_amdgcn_readlane((int)taken, pk_lane);
          if (tk < best_taken) { best_taken = tk; best = pk_lane; }
        }
        tile_idx = cand - lane + best;
      }
    }
  }
  LGT1(LG_CYC_JOIN);
  return tile_idx;
}

// tile_idx -> the tile's first pixel, and with VIEWS the record of its view.  False for a tile that lies entirely outside the
// image (the last chunks of a frame whose size is no multiple of 32): it is marked exhausted, once, so that no wave tries to join it.
template <bool VIEWS>
__device__ __forceinline__ bool tile_origin(const int lane, const int tile_idx, const uint32_t n_chunks_tile, int &tile_x0, int &tile_y0,
                                            RT_KViewP &vrec) {
  RT_KArgs A = cold_args();
  int vt = tile_idx;                  // the tile within its view
  if constexpr (VIEWS) {
    const int tu = __builtin_amdgcn_readfirstlane(tile_idx);
    const uint32_t view = (uint32_t)tu / (uint32_t)A->tiles_per_view;
    vt = tu - (int)view * A->tiles_per_view;
    vrec = (RT_KViewP)A->views + view;
  }
  const int lchunk = vt >> 4, sub = vt & 15;
  const int chunk = A->local_chunks[lchunk];
  const int chunks_x = A->chunks_x;
  tile_x0 = (chunk % chunks_x) * 32 + (sub & 3) * 8;
  tile_y0 = (chunk / chunks_x) * 32 + (sub >> 2) * 8;
  if (tile_x0 < A->width && tile_y0 < A->height) return true;
  if (lane == 0) {
    uint32_t old = atomicMax(&A->tile_next[tile_idx], n_chunks_tile);
    if (old < n_chunks_tile) atomicSub(&A->open_groups[tile_idx >> 6], 1u);
  }
  return false;
}
__device__ __forceinline__ bool tile_origin(const int lane, const int tile_idx, const uint32_t n_chunks_tile, int &tile_x0, int &tile_y0) {
  RT_KViewP no_view = nullptr;        // a one-view launch: the camera of the kernel arguments
  return tile_origin<false>(lane, tile_idx, n_chunks_tile, tile_x0, tile_y0, no_view);
}

// ---- can a camera ray of this tile touch the scene at all? ----
// The primary rays of the tile share the origin and lie inside the pyramid through the corners of the tile's pixel
// footprint.  If every populated child box of the ROOT lies outside one of the pyramid's four side planes -- by a
// relative margin of 1e-3, a thousand times the rounding error of the slab test -- then ray_aabbs_hit_8 returns
// "no candidate" for every one of them (raytracer.c:190-230, :459-472): the ray costs one node visit and goes to the
// environment.  Such rays skip the root block and are counted as that one visit.  (Lanes 0..7 test one child
// box each; only rays with finite reciprocal direction take the shortcut, see ray_setup.)
// Writes the pyramid (RT_PYR_PLANE, RT_PYR_ORIGIN) into the wave's slice for the node and leaf blocks, clears the slice's cull-mask
// caches and returns true when no camera ray of the tile can touch a child of the root.  S: the camera, kernel arguments or view record.
template <class CAM>
__device__ __forceinline__ bool tile_pyramid(const CAM S, const float *nodes, float4 *smem, const int pyr_off, const int lane,
                                             const int tile_x0, const int tile_y0) {
  RT_KArgs A = cold_args();
  const float m = 0.05f;                                   // footprint margin in pixels
  const float ux0 = ((float)tile_x0 - 0.5f - m) * 2.0f * A->inv_width - 1.0f;
  const float ux1 = ((float)tile_x0 + 7.5f + m) * 2.0f * A->inv_width - 1.0f;
  const float uy0 = ((float)tile_y0 - 0.5f - m) * 2.0f * A->inv_height - 1.0f;
  const float uy1 = ((float)tile_y0 + 7.5f + m) * 2.0f * A->inv_height - 1.0f;
  const float asp = A->aspect, fl = S->focal_length;
  rt_v3 c[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    float cx = ((q == 1 || q == 2) ? ux1 : ux0) * asp, cy = -((q >= 2) ? uy1 : uy0), cz = -fl;
    c[q] = rt_v3_make(S->cam[0][0] * cx + S->cam[0][1] * cy + S->cam[0][2] * cz,
                      S->cam[1][0] * cx + S->cam[1][1] * cy + S->cam[1][2] * cz,
                      S->cam[2][0] * cx + S->cam[2][1] * cy + S->cam[2][2] * cz);
  }
  const rt_v3 o = rt_v3_make(S->cam[0][3], S->cam[1][3], S->cam[2][3]);
  rt_v3 pn[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    rt_v3 n = rt_v3_cross(c[q], c[(q + 1) & 3]);
    if (rt_v3_dot(n, c[(q + 2) & 3]) > 0.0f) n = rt_v3_scale(n, -1.0f);      // outward: the opposite corner is inside
    pn[q] = n;
  }
  float *pyr = lds_at(smem, pyr_off);
  if (lane == 0) {                                         // the pyramid of this tile, for the node blocks
#pragma unroll
    for (int q = 0; q < 4; q++) { pyr[RT_PYR_PLANE + q * 4 + 0] = pn[q].x; pyr[RT_PYR_PLANE + q * 4 + 1] = pn[q].y; pyr[RT_PYR_PLANE + q * 4 + 2] = pn[q].z; }
    pyr[RT_PYR_ORIGIN] = o.x; pyr[RT_PYR_ORIGIN + 1] = o.y; pyr[RT_PYR_ORIGIN + 2] = o.z;
  }
  if (lane < RT_PYR_CACHE_WORDS) reinterpret_cast<uint32_t *>(pyr)[RT_PYR_LEAF_CACHE + lane] = 0u;      // the cull masks found for this tile so far
  bool may_hit = false;
  if (lane < 8) {
    const float *nb = nodes + lane;                        // child `lane` of node 0: rows are 8 floats apart
    rt_v3 lo = rt_v3_make(nb[0] - o.x, nb[8] - o.y, nb[16] - o.z);
    rt_v3 hi = rt_v3_make(nb[24] - o.x, nb[32] - o.y, nb[40] - o.z);
    bool outside = child_box_empty(nb);                    // the all-zero box of an unpopulated child never hits
#pragma unroll
    for (int q = 0; q < 4; q++) {
      rt_v3 n = pn[q];
      float lox = n.x * lo.x, hix = n.x * hi.x, loy = n.y * lo.y, hiy = n.y * hi.y, loz = n.z * lo.z, hiz = n.z * hi.z;
      float nearest = fminf(lox, hix) + fminf(loy, hiy) + fminf(loz, hiz);     // smallest n . (p - o) over the box
      float extent = fmaxf(fabsf(lox), fabsf(hix)) + fmaxf(fabsf(loy), fabsf(hiy)) + fmaxf(fabsf(loz), fabsf(hiz));
      // (+ the placement error of a fused slab distance, see pyramid_cull_mask)
      float coarse = fabsf(n.x) * (fabsf(o.x) + fmaxf(fabsf(nb[0]), fabsf(nb[24]))) + fabsf(n.y) * (fabsf(o.y) + fmaxf(fabsf(nb[8]), fabsf(nb[32]))) +
                     fabsf(n.z) * (fabsf(o.z) + fmaxf(fabsf(nb[16]), fabsf(nb[40])));
      if (nearest > 1e-3f * extent + 1e-6f * coarse) outside = true;        // (NaN compares false: not outside)
    }
    may_hit = !outside;
  }
  return __ballot(may_hit) == 0ull;
}

// ---- does the pyramid, pruned through the tree, reach a triangle at all? ----
// Breadth-first from the root with the node blocks' own plane test (pyramid_cull_mask on the LDS nodes): the surviving
// children of a listed node join the list.  A surviving child that is a leaf group gets the leaf blocks' triangle test
// (pyramid_cull_tris): a triangle that survives ends the walk, a group without one joins the list as a group.  A tile whose walk
// ends without a triangle is LEAFLESS (no group listed) or TRIANGLE-LESS: every child box that a NaN-free camera ray of the tile
// can enter is a listed node or group, no listed group holds a triangle the ray can be accepted by, so the ray's outcome is known
// -- no hit -- and only its node and leaf visits remain to be counted (the leafless form of the path kernel's batch loop).
// An all-zero triangle, the padding of a partly filled group of the reference's builder, counts as culled whatever the planes say
// (the camera may stand on the origin's side of all four): its edges are zero, so det = 0, the reciprocal is infinite or NaN,
// s . (d x e2) = 0 and u = inv_det * 0 is NaN, as is t.  No comparison with a NaN holds: tri_test_uniform and
// leaf_test_short_div find `miss` false and then `t < best` false, leaf_test turns the NaN distance into +infinity (dist > 0 is
// false) and `dist < best` is false.  None of the three accepts it.
// Caps: RT_LL_MAX listed nodes and groups together, 4 survivors per node (node_enter_few's limit), every listed node -- and the
// parent of every listed group -- LDS resident; a tile over a cap is an ordinary tile.
// The list lives in row 0 of the wave's perm stack, which is free while no lane of the wave traverses (leafless_list) and has 64
// words: entry i >= 1 at [RT_LL_ENTRY + i] = byte offset of (parent node, child slot) in the LDS node image | index of the parent
// in the list << 20 (5 bits) | RT_LL_GROUP for a leaf group | 1 << 31 (marks an entry), the node or group itself, in the tree's
// implicit numbering, at [RT_LL_NODE + i].
// Returns the number of listed nodes and groups (the root counts), 0 for a tile that is neither.  levels = depth - 1 >= 1,
// n_nodes = pyr_nodes > 0, leaf0 = last_row_offset, leaves = the launch's leaf groups.  Writes every visited node's mask into the
// (tile, node) cache of the node blocks -- the root visit in front of the traversal finds the root's there -- and every tested
// group's into the leaf blocks' (by group & 7, the later of two groups that share a slot).
#define RT_LL_MAX   32
#define RT_LL_ENTRY 0
#define RT_LL_NODE  RT_LL_MAX
#define RT_LL_GROUP 0x40000000u
static_assert(2 * RT_LL_MAX * 4 <= RT_LDS_PERM_LEVEL_BYTES && RT_LL_MAX <= 32, "the list is one row of the perm stack, `entered` one word");
__device__ __forceinline__ uint32_t *leafless_list(float4 *smem, const int pyr_off, const int levels) {
  return reinterpret_cast<uint32_t *>(lds_at(smem, pyr_off) - levels * (RT_LDS_PERM_LEVEL_BYTES / 4));      // the pyramid area is row `levels`
}
__device__ __forceinline__ int leafless_walk(float4 *smem, const float4 *lds_nodes, const int pyr_off, const int levels, const int n_nodes,
                                             const int leaf0, const float *leaves) {
  const float *pyr = lds_at(smem, pyr_off);
  uint32_t *list = leafless_list(smem, pyr_off, levels);
  int n_list = 1;
  for (int head = 0; head < n_list; head++) {
    const int nd = head ? __builtin_amdgcn_readfirstlane((int)list[RT_LL_NODE + head]) : 0;
    if (nd >= leaf0) continue;              // a listed group: nothing below it
    const uint32_t surv = 0xFFu & ~pyramid_cull_mask(lds_nodes, pyr, nd);
    if (lane_now() == 0) reinterpret_cast<uint32_t *>(lds_at(smem, pyr_off))[RT_PYR_NODE_CACHE + (nd & 31)] = ((uint32_t)(nd + 1) << 8) | (0xFFu & ~surv);
    if (surv) {
      const int ns = (int)__popc(surv);
      const bool groups = 8 * nd + 1 >= leaf0;      // the children are leaf groups
      // children that are nodes outside the LDS image (its last node's children at the most), or a cap
      if ((!groups && 8 * nd + 8 >= n_nodes) || ns > 4 || n_list + ns > RT_LL_MAX) return 0;
      if (groups) {
        for (uint32_t m = surv; m; m &= m - 1u) {
          const int g = 8 * nd + 1 + (int)__builtin_ctz(m) - leaf0;
          if ((uint32_t)g >= 0x800000u) return 0;   // (the leaf cache's key has 23 bits)
          uint32_t padding = 0u;            // the group's all-zero triangles
          const uint32_t cull = pyramid_cull_tris<true>(leaves, pyr, g, &padding);
          if (lane_now() == 0) reinterpret_cast<uint32_t *>(lds_at(smem, pyr_off))[RT_PYR_LEAF_CACHE + (g & 7)] = ((0x800000u | (uint32_t)g) << 8) | cull;
          if ((0xFFu & ~(cull | padding)) != 0u) return 0;      // a triangle the pyramid can touch: an ordinary tile
        }
      }
      const int k = lane_now();             // lane k < 8: child k
      if (k < 8 && ((surv >> k) & 1u)) {
        const int at = n_list + (int)__popc(surv & ((1u << k) - 1u));
        list[RT_LL_ENTRY + at] = (uint32_t)(nd * RT_LDS_NODE_BYTES + k * 4) | ((uint32_t)head << 20) | (groups ? RT_LL_GROUP : 0u) | 0x80000000u;
        list[RT_LL_NODE + at] = (uint32_t)(8 * nd + 1 + k);
      }
      n_list += ns;
    }
  }
  return n_list;
}

// ---- units ----
// The tile hands out UNITS (2 pixels x one block of samples = 128 paths at 64 samples, lanes on one or two pixels).  A wave
// grabs `grab` consecutive units per atomic, `grab_max` while the tile has plenty left, fewer towards its end: what a wave still
// holds when the launch runs dry is its tail.  (The path kernel's batch loop grabs by the same rule with `grab_batch` for
// `grab_max`: its tiles hold no bounce chains.)  All wave-uniform.
struct TileUnits {
  uint32_t u_cur, u_end, grab;       // the grabbed units [u_cur, u_end) (u_cur: the current one), units to ask for next
  int  c_next, c_end;                // the current unit: its paths [c_next, c_end) are not handed out yet
  int  c_x0, c_y, c_pix0, c_s0;      // ... at pixels (c_x0 .. c_x0 + 1, c_y) = pixels c_pix0, c_pix0 + 1 of the tile, samples from c_s0
  bool took_any;                     // the wave was handed a unit of this tile: it has something to flush
};
__device__ __forceinline__ void tile_units_init(TileUnits &U, const bool queue_open) {
  U.c_next = U.c_end = U.c_x0 = U.c_y = U.c_pix0 = U.c_s0 = 0;
  U.u_cur = U.u_end = 0;
  U.grab = queue_open ? (uint32_t)cold_args()->grab_max : 1u;
  U.took_any = false;
}

// The next units of the tile from its counter; false when it has none left.  Every unit is handed out exactly once, and exactly
// one wave receives the tile's last unit: it closes the tile in the group summary.
// Next grab: `grab_max` units while the tile has plenty left, fewer towards its end.  (A launch-wide count of the remaining units
// would be the better guide, but a counter that every grab updates -- one address or 64 shards of one line -- made the frame
// 2x slower: measured, removed.)
// tile_next, open_groups, gmax (grab_max): the kernel arguments of these names, read by the caller at the call.  t_wave_start != 0
// (RT_WAVE_TIMES, diagnostic library): the time of a successful grab goes to t_last_grab.
__device__ __forceinline__ bool grab_units(const int lane, const int tile_idx, const uint32_t n_chunks_tile, uint32_t *tile_next,
                                           uint32_t *open_groups, const uint32_t gmax, TileUnits &U, const unsigned long long t_wave_start,
                                           unsigned long long &t_last_grab, uint32_t *lg = nullptr) {
  uint32_t u0 = 0;
  if (lane == 0) u0 = atomicAdd(&tile_next[tile_idx], U.grab);
  u0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);
  if (u0 >= n_chunks_tile) return false;
  U.u_cur = u0;
  U.u_end = u0 + U.grab < n_chunks_tile ? u0 + U.grab : n_chunks_tile;
  if (U.u_end == n_chunks_tile && lane == 0) atomicSub(&open_groups[tile_idx >> 6], 1u);
  if (t_wave_start) t_last_grab = __builtin_amdgcn_s_memrealtime();
  LG(LG_GRAB_X, 1);
  const uint32_t left = n_chunks_tile - U.u_end;
  U.grab = left >= 8u * gmax ? gmax : (left >= 8u && gmax >= 2u ? 2u : 1u);
  U.took_any = true;
  return true;
}

// unit u_cur -> (row, sample block, pixel pair): all sample blocks of a row before the next row, so a pixel's texture / geometry
// footprint is touched in one burst.  Units outside the image have no paths.  shift = chunk_shift, unit_paths = 2 << shift; n_sb =
// n_sample_blocks, sample_first, width, height: the kernel arguments of these names, as the caller holds them -- across its loop
// or read at the call.
__device__ __forceinline__ void unit_decode(TileUnits &U, const int tile_x0, const int tile_y0, const int shift, const int unit_paths,
                                            const uint32_t n_sb, const int sample_first, const int width, const int height) {
  const uint32_t grp = U.u_cur >> 2, pair = U.u_cur & 3u;
  const uint32_t row = grp / n_sb, sb = grp - row * n_sb;
  U.c_x0 = tile_x0 + (int)pair * 2;
  U.c_y = tile_y0 + (int)row;
  U.c_pix0 = (int)row * 8 + (int)pair * 2;
  U.c_s0 = sample_first + (int)(sb << shift);
  U.c_next = 0;
  U.c_end = (U.c_y < height && U.c_x0 < width) ? unit_paths : 0;
}

// ---- regeneration: the wave's idle lanes take the next paths of the tile, across unit boundaries ----
// A lane that is idle (`phase` == PH_NEED: the lane's own, by reference -- an idle flag computed by the caller compiles to another loop,
// profiles/r10_summary.md) gets at most one path: true for it, `np` = its pixel, sample and pixel of the tile.  k -> (pixel of the row,
// sample of the unit), pixel-major: the lanes of a wave stay on a few pixels.  w_paths += the paths handed out; with !start_paths
// (max_bounces == 0) a path exists and is black -- the loop of raytracer.c:512 runs zero times -- so it is counted and no lane gets it.
// Units come from grab_units() as the wave's run out -- not with `no_grab` (a camera kernel told to stop) -- and tile_open goes false
// when the tile has none left.
struct NewPath { int x, y, sample, pix; };
__device__ __forceinline__ bool regen_paths(const int &phase, NewPath &np, const bool start_paths, TileUnits &U, bool &tile_open, const bool no_grab,
                                            const int lane, const int tile_idx, const uint32_t n_chunks_tile, const int tile_x0, const int tile_y0,
                                            const int shift, const int unit_paths, const unsigned long long t_wave_start,
                                            unsigned long long &t_last_grab, uint32_t &w_paths, uint32_t *lg = nullptr) {
  RT_KArgs A = cold_args();
  unsigned long long need = __ballot(phase == PH_NEED);
  bool got = false;
  const int width = A->width, sample_end = A->sample_end;
  LGM("regen_begin");
  while (need) {
    LG(LG_REGEN_X, 1);
    if (U.c_next >= U.c_end) {
      if (U.u_cur + 1u < U.u_end) {
        U.u_cur += 1u;
      } else if (no_grab || !grab_units(lane, tile_idx, n_chunks_tile, A->tile_next, A->open_groups, (uint32_t)A->grab_max, U, t_wave_start, t_last_grab LG_ARG)) {
        tile_open = false;
        break;
      }
      unit_decode(U, tile_x0, tile_y0, shift, unit_paths, (uint32_t)A->n_sample_blocks, A->sample_first, width, A->height);
      continue;
    }
    const int n_need = (int)__popcll(need);
    const int avail = U.c_end - U.c_next;
    const int take = n_need < avail ? n_need : avail;
    const int rank = lane_rank(need);
    bool valid = false;
    if (phase == PH_NEED && !got && rank < take) {
      const int k = U.c_next + rank;
      const int px = k >> shift;
      const int sm = U.c_s0 + (k & ((1 << shift) - 1));
      const int x = U.c_x0 + px;
      if (x < width && sm < sample_end) {
        valid = true;
        if (start_paths) { got = true; np.x = x; np.y = U.c_y; np.sample = sm; np.pix = U.c_pix0 + px; }
      }
    }
    w_paths += (uint32_t)__popcll(__ballot(valid));
    U.c_next += take;
    need = __ballot(phase == PH_NEED && !got);
  }
  LGM("regen_end");
  return got;
}

// ---- flush: lane p owns pixel p of the tile at (tile_x0, tile_y0) ----
// Adds the wave's accumulator tile `acc` (LDS) to `frame` with 64-bit atomics and clears it; the rays the wave spent on the tile
// go to the tile's cost (tile_idx < 0: none).
__device__ __forceinline__ void flush_tile(unsigned long long *acc, const int lane, const int tile_x0, const int tile_y0,
                                           unsigned long long *frame, const int tile_idx, const uint32_t n_rays) {
  const int x = tile_x0 + (lane & 7), y = tile_y0 + (lane >> 3);
  const unsigned long long r = acc[lane * 3 + 0], g = acc[lane * 3 + 1], b = acc[lane * 3 + 2];
  acc[lane * 3 + 0] = 0ull;
  acc[lane * 3 + 1] = 0ull;
  acc[lane * 3 + 2] = 0ull;
  RT_KArgs A = cold_args();
  const int width = A->width;
  if (x < width && y < A->height && (r | g | b) != 0ull) {
    unsigned long long *dst = frame + ((size_t)y * width + x) * 3;
    atomicAdd(dst + 0, r);
    atomicAdd(dst + 1, g);
    atomicAdd(dst + 2, b);
  }
  if (tile_idx >= 0) {
    uint32_t *tile_cost = A->tile_cost;
    if (tile_cost && lane == 0) atomicAdd(&tile_cost[tile_idx], n_rays);
  }
}

#endif  // RT_TILE_HIP_H
