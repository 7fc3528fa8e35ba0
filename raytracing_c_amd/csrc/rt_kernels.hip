// rt_kernels.hip -- gfx950 device code of the render hot path.
//
// What runs here replaces, on the GPU, the reference's
//   render_thread_proc   raytracer.c:596-720   (pixel / sample loop)
//   cast_ray             raytracer.c:505-558   (bounce loop)
//   ray_bvh_node_hit     raytracer.c:443-483   (near-first 8-ary traversal)
//   ray_aabbs_hit_8      raytracer.c:190-230   (8-box slab test)
//   ray_triangles_hit_8  raytracer.c:84-188    (8-triangle Moeller-Trumbore)
//   disney_shader_proc & friends  driver.c:49-418 (textures, BSDF, background)
//
// Design (DESIGN.md has the long form):
//  * One path kernel, rt_path_kernel_stream (below): a persistent grid of wave64s, one ray per lane, lanes refilled by
//    path regeneration.  A wave owns an 8x8-pixel tile and pulls units of it (2 pixels x a block of samples) from the
//    tile's own counter; when the tiles run out it joins a tile that still has units.
//  * Traversal keeps, per lane and per tree level, one 32-bit word in LDS holding the not-yet-visited children of the
//    node on that level in near-first order (3 bits each + count).  The entry distance of a popped child is recomputed
//    from the node (6 floats) only when the closest hit changed since that node was entered; this reproduces the
//    reference's visiting order and its `dist < hit.distance` test exactly.  The leading BVH nodes sit in LDS.
//  * Radiance is accumulated in 32.32 fixed point (rt_math.h), first in LDS per tile, then with 64-bit integer atomics
//    in HBM: exact and independent of scheduling, so images are bit-identical to the CPU oracle.
//  * All arithmetic goes through include/rt_math.h and is compiled with -ffp-contract=off: no fused multiply-add that
//    the CPU would not do.
//  * Around it: the per-launch preparation kernel (counters, tile order), resolve / untile, the lightmap baker, texture
//    packing, and the launchers the host units call (rt_host.h).  The device functions are in rt_dev.hip.h.

#include "rt_dev.hip.h"

// ---------------------------------------------------------------------------------
// The tile-stream path kernel: where the work comes from and how the loop is cut.
//
//  * A wave OWNS an 8x8-pixel tile (taken from the head counter, expensive tiles first) and pulls UNITS of it --
//    2 neighbouring pixels x 2^chunk_shift samples (128 paths at 64 samples, pixel-major, so the 64 lanes
//    sit on one or two pixels: coherent nodes, leaves and texels), one or two per atomic, up to eight in the batch loop -- from the tile's own counter
//    `tile_next[tile]` until the tile is exhausted.  Lanes whose path ended are refilled across unit boundaries, so
//    there is no drain at the end of a unit (40 us to 0.4 ms each, measured on the kernel generation that had one); the wave
//    drains once per TILE.
//  * When the head counter runs dry a wave JOINS a tile that still has units (two-level scan with agent-scope loads:
//    `open_groups[g]` counts the open tiles of every group of 64) and pulls from the same counter: the tail of a
//    launch is balanced at unit granularity even when a rank of the 8-GPU partition has fewer tiles than the chip has
//    waves.  Every unit is handed out exactly once by an atomic; radiance sums are order-free integers, so results do
//    not depend on who traced what.  Owners always finish their tile, so a joiner may give up at any time: every wave
//    reaches an exit (bounded scans), there is no inter-wave dependency and no grid barrier.
//  * Camera rays of a tile whose pixel pyramid misses every child box of the root skip the root block (below); node blocks
//    whose lanes are (mostly) camera rays about to enter ONE node test only the child boxes that pyramid can touch
//    (pyramid_cull_mask, node_enter_few; the mask of a (tile, node) is cached in LDS).  Tiles whose pyramid, pruned through the
//    tree from the root, reaches no leaf group, or only groups none of whose triangles it can touch, never enter the traversal: a
//    batch loop counts their rays' node and leaf visits.
//  * Hits are parked -- path state to memory, lane to a new path -- while a shade block would run sparse, and shaded
//    together when 48 lanes can be filled (`park`, S block).
//  * The traversal blocks run in an inner loop of their own; shading / environment / regeneration run in the outer
//    loop.  Path state (tint, emission, RNG, pixel) is untouched inside the inner loop, the block choice there is
//    two ballots, and the counters are wave-level scalars.

#ifdef RT_LEDGER
#define RT_LEDGER_WAVES 8192
__device__ uint32_t g_ledger[RT_LEDGER_WAVES * RT_LEDGER_ROW];      // block ledger: one row of LG_* slots per wave (rt_dev.hip.h)
__global__ void rt_ledger_reduce_kernel(unsigned long long *counters) {
  const int slot = threadIdx.x;
  if (slot >= LG_N || slot >= RT_LEDGER_ROW) return;
  unsigned long long sum = 0ull;
  for (int w = 0; w < RT_LEDGER_WAVES; w++) sum += g_ledger[w * RT_LEDGER_ROW + slot];
  counters[RT_CNT_LEDGER + slot] = sum;
}
#endif

template <int WAVES, bool LDSN, int MIN_WAVES_PER_SIMD, bool SHORT_DIV, bool VIEWS, bool SHARED_TAPS>
__global__ __launch_bounds__(WAVES * 64, MIN_WAVES_PER_SIMD) void rt_path_kernel_stream(RT_KParams P) {
  extern __shared__ float4 smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n_lds = LDSN ? P.n_lds_nodes : 0;
  const float4 *lds_nodes = smem;
  const WaveLds L = wave_lds(smem, n_lds, P.depth, wave);      // the wave's LDS slice: perm stack, pyramid area, accumulator tile
  unsigned long long *acc = L.acc;
  const int acc_off = L.acc_off, pyr_off = L.pyr_off;

#ifdef RT_LEDGER
  uint32_t *lg = g_ledger + (size_t)__builtin_amdgcn_readfirstlane((int)blockIdx.x * WAVES + wave) * RT_LEDGER_ROW;
  const unsigned long long lg_wave_t0 = __builtin_amdgcn_s_memtime();
#if RT_LEDGER >= 2
  unsigned long long lg_drain_t0 = 0ull;
#endif
#endif
  pow24_lds_init((int)threadIdx.x);
  if (LDSN) {
    LGT0();
    lds_load_nodes<WAVES * 64>(smem, P.nodes, n_lds);
    __syncthreads();          // the only workgroup barrier of the kernel; waves are independent afterwards
    LGT1(LG_CYC_COPY);
  } else {
    __syncthreads();          // (the sRGB scale table)
  }

  acc_tile_clear(acc, lane);

  // ---- the root's populated children: the only ones a ray's root visit has to test (in front of the traversal call, below) ----
  // The reference builder fills a tree of fixed capacity, so the root of a small scene has children without a triangle below them:
  // all-zero boxes, never a candidate for a NaN-free ray (child_box_empty).  Read from the LDS node image of THIS launch, not kept
  // on the host: a refit rewrites the boxes on the device.  0 = the root visit is left to the node blocks: more than four populated children (node_enter_few's
  // limit), no root in LDS, a tree of depth 0.  A word of the wave's LDS slice, read where it is used, not a scalar register.
  if (LDSN) {
    uint32_t *pw = reinterpret_cast<uint32_t *>(lds_at(smem, pyr_off));
    bool populated = false;
    if (lane_now() < 8 && cold_args()->n_lds_nodes > 0 && cold_args()->depth > 0) {
      populated = !child_box_empty(lds_at(smem, 0) + lane_now());      // child `lane` of node 0
    }
    const uint32_t pm = (uint32_t)__ballot(populated) & 0xFFu;
#ifdef RT_ROOT_AT_NODE_BLOCKS      /* (ledger builds that count the root rounds of the node blocks: profiles/r07_root_visits.md) */
    if (lane_now() == 0) { pw[RT_PYR_ROOT_POP] = 0u; pw[RT_PYR_ROOT_FUSED] = 0u; }
#else
    if (lane_now() == 0) { pw[RT_PYR_ROOT_POP] = __popc(pm) <= 4 ? pm : 0u; pw[RT_PYR_ROOT_FUSED] = 0u; }
#endif
  }

  // wave-level counters (scalar registers)
  uint32_t w_paths = 0, w_rays = 0, w_nodes = 0, w_leaves = 0, w_shades = 0, w_bgs = 0, w_tex = 0;
  const unsigned long long t_wave_start = cold_args()->wave_times ? __builtin_amdgcn_s_memrealtime() : 0ull;   // RT_WAVE_TIMES only
  uint32_t n_tiles_done = 0;
  unsigned long long t_last_grab = 0ull;

  const int shift = P.chunk_shift;                 // samples per unit = 1 << shift
  const int unit_paths = 2 << shift;               // a unit = 2 neighbouring pixels x (1 << shift) samples
  const uint32_t n_chunks_tile = (uint32_t)P.n_chunks_tile;      // units per tile: 8 rows x sample blocks x 4 pixel pairs
  const int leaf_level = P.depth - 1;
  const int thresh = P.sched_thresh;
  const int drain_thresh = P.drain_thresh;
  const int pyr_nodes = LDSN ? P.pyr_nodes : 0;
  const int wave_id = (int)blockIdx.x * WAVES + wave;

  bool queue_open = true;
  int  steal_tries = 0;

  for (;;) {
    // ---------------- take a tile: own one from the queue, or join one that still has units ----------------
    LGT0();
    LGM("tile_begin");
    int tile_idx = queue_open ? take_queue_tile(lane, queue_open) : -1;
    if (tile_idx < 0) {
      if (steal_tries >= RT_STEAL_TRIES) break;
      steal_tries += 1;
      LG(LG_JOIN_X, 1);
      tile_idx = join_open_tile(lane, wave_id, steal_tries, n_chunks_tile LG_ARG);
      if (tile_idx < 0) break;                      // nothing left to join
    }

    int tile_x0, tile_y0;
    RT_KViewP vrec = nullptr;             // VIEWS: the record of this tile's view
    if (!tile_origin<VIEWS>(lane, tile_idx, n_chunks_tile, tile_x0, tile_y0, vrec)) continue;      // a tile outside the image
    // can a camera ray of the tile touch a child of the root at all?  (and the tile's pyramid, for the node and leaf blocks)
    bool tile_root_miss = false;
    if (leaf_level >= 0) {
      typename CamSrc<VIEWS>::type S;
      if constexpr (VIEWS) S = vrec; else S = cold_args();
      tile_root_miss = tile_pyramid(S, P.nodes, smem, pyr_off, lane, tile_x0, tile_y0);
    }
    // does the pyramid, pruned through the tree, reach a triangle at all?  n_list: listed nodes and groups of a LEAFLESS or
    // TRIANGLE-LESS tile, 0: neither
    // (the launch constants through empty asm: tests and offsets formed from them here are not hoisted out of the tile loop into
    //  scalar registers that live, and spill, for the whole kernel)
    int n_list = 0;
    int ll_levels = leaf_level, ll_nodes = pyr_nodes, ll_leaf0 = P.last_row_offset;
    asm volatile("" : "+s"(ll_levels), "+s"(ll_nodes), "+s"(ll_leaf0));
    if (ll_levels >= 1 && ll_nodes > 0 && !tile_root_miss) n_list = leafless_walk(smem, lds_nodes, pyr_off, ll_levels, ll_nodes, ll_leaf0, cold_args()->leaves);
    const uint32_t rays_before = w_rays;
    LG(LG_TILE_X, 1);
    LGM("tile_end");
    LGT1(LG_CYC_TILE);

    // ---------------- per-lane state ----------------
    int   pix = 0, bounce = 0;
    uint32_t rng = 0;
    Ray3  ray;
    ray_setup(ray, rt_v3_make(0, 0, 0), rt_v3_make(0, 0, 1));
    rt_v3 tint = rt_v3_make(1, 1, 1), emis = rt_v3_make(0, 0, 0);
    TravState T = RT_TRAV_IDLE;

    // the tile's units as this wave holds them (grab_units, unit_decode)
    bool tile_open = true;
    TileUnits U;
    tile_units_init(U, queue_open);
    int  n_parked = 0;                   // hits of this tile waiting in the wave's slice of `park`
    uint32_t *park = cold_args()->park;

    // ================= tiles whose pyramid misses every child of the root: a loop of their own =================
    // Every camera ray of such a tile (56 % of the camera paths of config #3: 299 M of 531 M) costs one node visit that finds no candidate and
    // goes to the environment -- no traversal state, no phases, no parking, no RNG draw.  The loop below does exactly that for
    // batches of up to 64 paths: primary ray, environment lookup, sample into the LDS tile; same arithmetic, same counters as
    // the general loop, which takes over at once -- from the same unit, nothing consumed -- should a ray turn up that is not
    // NaN-free (such a ray does not take the shortcut: its root visit must be computed, see tile_root_miss).
    //
    // LEAFLESS tiles (n_list > 0, see the tile set-up: 19 % of the camera paths of config #3, 100 M) take the same loop.  Their rays
    // do enter nodes, but no leaf group: per batch, a wave-uniform pass over the listed nodes gives every lane the set of listed
    // nodes its ray enters -- node i when the ray entered i's parent and the slab test of i's box, the arithmetic of node_enter_few
    // with t_max = infinity (no hit is ever recorded, so every candidate child is visited whatever the near-first order), finds a
    // candidate -- and the number of those nodes is the ray's node visits.  These visits are executed, not skipped.
    //
    // TRIANGLE-LESS tiles (4.6 % of the camera paths of config #3, 24 M) list, beside nodes, the leaf groups their pyramid reaches:
    // none holds a triangle that a ray of the tile can be accepted by (leafless_walk).  A ray that entered a group's parent and finds
    // the group's box a candidate visits the group -- the reference runs its eight tests there and accepts nothing -- so the same
    // pass counts that entry as a leaf visit.
    if ((tile_root_miss || n_list > 0) && cold_args()->max_bounces > 0) {
      RT_KArgs A = cold_args();
      typename CamSrc<VIEWS>::type S;
      if constexpr (VIEWS) S = vrec; else S = A;
      const int width = A->width, height = A->height, sample_first = A->sample_first, sample_end = A->sample_end;
      const uint32_t n_sb = (uint32_t)A->n_sample_blocks, gmax = (uint32_t)A->grab_batch;      // (units per atomic: a batch tile's own)
      if (queue_open) U.grab = gmax;      // (the host has put the tile's size through the taper: the owner's first grab obeys it too)
      PrimaryParams PP;
      primary_params(PP, S, A);
      BgImageParamsLds BP;                // (the environment from its float image: background_lookup_image, rt_dev.hip.h)
      bg_image_params(BP, A);
      uint32_t *tile_next = A->tile_next, *open_groups = A->open_groups;
      uint32_t n_sky = 0;                 // paths served here: their root visit is COUNTED (like the oracle's) but not executed
      // lane i: entry i of the tile's node list, 0 past its end (the pass below stops there: no count in a scalar register)
      const uint32_t *list = leafless_list(smem, pyr_off, ll_levels);
      const uint32_t list_entry = (n_list > 1 && lane_now() < n_list) ? list[RT_LL_ENTRY + (lane_now() & 31)] : 0u;
      for (;;) {
        if (U.c_next >= U.c_end) {
          if (U.u_cur + 1u < U.u_end) {
            U.u_cur += 1u;
          } else {
            // (grab_units() written out: as a call, with the arguments this loop holds, it shifts the SGPR spills of the VIEWS instances)
            uint32_t u0 = 0;
            if (lane == 0) u0 = atomicAdd(&tile_next[tile_idx], U.grab);
            u0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);
            if (u0 >= n_chunks_tile) { tile_open = false; break; }
            U.u_cur = u0;
            U.u_end = u0 + U.grab < n_chunks_tile ? u0 + U.grab : n_chunks_tile;
            if (U.u_end == n_chunks_tile && lane == 0) atomicSub(&open_groups[tile_idx >> 6], 1u);
            if (t_wave_start) t_last_grab = __builtin_amdgcn_s_memrealtime();
            LG(LG_GRAB_X, 1);
            const uint32_t left = n_chunks_tile - U.u_end;
            U.grab = left >= 8u * gmax ? gmax : (left >= 8u && gmax >= 2u ? 2u : 1u);
            U.took_any = true;
          }
          unit_decode(U, tile_x0, tile_y0, shift, unit_paths, n_sb, sample_first, width, height);
          continue;
        }
        // RT_SKY_PATHS paths per lane and iteration.  Two or three -- independent chains of primary ray -> environment lookup for
        // the scheduler to interleave, in a loop that carries no other state -- measure the same as one (32.50 / 32.65 vs 32.55 ms:
        // profiles/r04o_sky_ab.log): what the loop saves is the phase machine's instructions, scalar and vector, not latency.
        // (The switch stays although nothing sets it: the same batch written with scalars instead of one-element arrays compiles to
        // different code -- the lookup's atan2 is no longer if-converted and the whole kernel's register allocation shifts.)
#ifndef RT_SKY_PATHS
#define RT_SKY_PATHS 1
#endif
        LGM("sky_begin");
        LGT0();
        const int avail = U.c_end - U.c_next;
        const int take = avail < 64 * RT_SKY_PATHS ? avail : 64 * RT_SKY_PATHS;
        const int l = lane_now();
        bool valid[RT_SKY_PATHS];
        int  pxs[RT_SKY_PATHS];
        rt_v3 dirs[RT_SKY_PATHS];
        Ray3 rs[RT_SKY_PATHS];
        bool slow = false;
#pragma unroll
        for (int q = 0; q < RT_SKY_PATHS; q++) {
          const int kq = l + 64 * q;
          const int k = U.c_next + kq;
          pxs[q] = k >> shift;
          const int sm = U.c_s0 + (k & ((1 << shift) - 1));
          const int x = U.c_x0 + pxs[q];
          valid[q] = kq < take && x < width && sm < sample_end;
          rt_v3 o = rt_v3_make(0, 0, 0);
          dirs[q] = rt_v3_make(0, 0, 1);
          if (valid[q]) primary_ray(PP, x, U.c_y, sm, o, dirs[q]);
          ray_setup<SHORT_DIV>(rs[q], o, dirs[q]);
          slow = slow || (valid[q] && !rs[q].fast);
        }
        // The general loop redoes this batch, and the rest of the tile.  U.grab stays what this loop left: the general loop's FIRST
        // grab on the tile may take up to grab_batch units, every later one obeys grab_max (grab_units' taper).  Correct either way
        // -- u_end is clamped, the tile closed once -- and only frames that hand every tile over see it; clamping U.grab here costs
        // the VIEWS instances a spilled SGPR (profiles/r17_batch_lanes.md).
        if (__ballot(slow) != 0ull) break;
        uint32_t nv = 0;
        // (leafless tiles; every lane runs every test -- nothing to save under a lane mask, and no mask to keep in scalar registers;
        //  a sky tile pays one readlane and a branch per batch)
        uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)list_entry, 1);
        if ((int)e < 0) {
#pragma unroll
          for (int q = 0; q < RT_SKY_PATHS; q++) {
            const Ray3 &r = rs[q];
            const int nx = (as_i(r.inv_x) >> 31) & 96, ny = (as_i(r.inv_y) >> 31) & 96, nz = (as_i(r.inv_z) >> 31) & 96;
            const rt_v3 bs = slab_bias3(r);
            uint32_t entered = valid[q] ? 1u : 0u;                // bit i: the ray enters listed node i
            int i = 1;
            if (q > 0) e = (uint32_t)__builtin_amdgcn_readlane((int)list_entry, 1);
            do {
              const char *cb = reinterpret_cast<const char *>(lds_nodes) + (e & 0xFFFFFu);
              const float t = slab_entry_ordered(r, bs, cb, 0, nx, ny, nz, RT_INF);
              const uint32_t in = ((entered >> ((e >> 20) & 31u)) & 1u) & (t < RT_INF ? 1u : 0u);
              entered |= in << i;
              const uint32_t n_in = (uint32_t)__popcll(__ballot(in != 0u));
              if (e & RT_LL_GROUP) w_leaves += n_in;                // a visit of a listed group: eight tests, nothing accepted
              else w_nodes += n_in;                                 // a visit of a listed node below the root
              i += 1;
              e = (uint32_t)__builtin_amdgcn_readlane((int)list_entry, i);
            } while ((int)e < 0);
          }
        }
#pragma unroll
        for (int q = 0; q < RT_SKY_PATHS; q++) {
          // The samples of a batch start at sample 0 or a multiple of 64 of their unit (c_next), `shift` bits of k per pixel: the
          // lanes of an aligned group of G share a pixel exactly when G <= 2^shift.  Then the group's samples are summed in
          // registers and one lane adds (tile_add_samples_grouped); with fewer samples per pixel every lane adds its own, as before.
          unsigned long long qr = 0ull, qg = 0ull, qb = 0ull;
          if (valid[q]) {
            const rt_v3 bg = background_lookup_image(BP, dirs[q]);
            const rt_v3 radiance = rt_v3_mul_add(bg, rt_v3_make(1, 1, 1), rt_v3_make(0, 0, 0));      // tint 1, emission 0 (raytracer.c:554)
            qr = accum_quantize_dev(radiance.x); qg = accum_quantize_dev(radiance.y); qb = accum_quantize_dev(radiance.z);
          }
          // (2^shift as half the unit's paths, which the loop holds anyway: the same test on `shift` costs every instance two more spilled SGPRs)
          tile_add_samples_grouped(smem, acc_off, U.c_pix0 + pxs[q], U.c_end >= 2 * RT_SKY_ADD_GROUP, valid[q], qr, qg, qb);
          nv += (uint32_t)__popcll(__ballot(valid[q]));
        }
        w_paths += nv; w_rays += nv; w_nodes += nv; w_bgs += nv;      // (the skipped root visit counts, as in the general loop)
        n_sky += nv;
        LG(LG_SKY_X, 1); LG(LG_SKY_L, nv);
        U.c_next += take;
        LGT1(LG_CYC_SKY);
        LGM("sky_end");
      }
      // counters[RT_CNT_SKIPPED_ROOT]: node visits that are counted but not executed (bench.py's roofline footnote)
      // counters[RT_CNT_LEAFLESS]: paths of leafless and triangle-less tiles served here; their root visits are executed, not skipped
      // counters[RT_CNT_TRIANGLELESS]: those of them whose tile lists a leaf group (from the list's lanes: no flag kept across the loop;
      // lane 0 holds the root's word of the list, which nothing writes)
      if (n_sky != 0u && lane == 0) atomicAdd(cold_args()->counters + (tile_root_miss ? RT_CNT_SKIPPED_ROOT : RT_CNT_LEAFLESS), (unsigned long long)n_sky);
      if (n_sky != 0u && (__ballot((list_entry & RT_LL_GROUP) != 0u) & ~1ull) != 0ull && lane == 0)
        atomicAdd(cold_args()->counters + RT_CNT_TRIANGLELESS, (unsigned long long)n_sky);
    }

    for (;;) {
      // ================= S: shade the hits, environment for the misses, start new paths =================
      {
        LGT0();
        LGM("s_begin");
        LG(LG_S_ITER, 1);
        LaneCounters cn;
        cn.rays = cn.nodes = cn.leaves = cn.shades = cn.bgs = cn.textured = cn.paths = 0;
        bool  done = false, start = false, fresh = false;
        rt_v3 radiance = rt_v3_make(0, 0, 0);
        rt_v3 org = ray.o, dir = ray.d;
        RT_KArgs A = cold_args();
        typename PathShadeParams<SHARED_TAPS>::type SP;      // (SHARED_TAPS: one set of bilinear taps per hit, rt_dev.hip.h)
        shade_params(SP, A, true);
        // ---- environment for the paths that left the scene ----
#ifdef RT_LEDGER
        { const int n_env = (int)__popcll(__ballot(T.phase == PH_MISS)); LG(LG_ENV_X, n_env != 0); LG(LG_ENV_L, n_env); }
#endif
        LGM("env_begin");
        if (T.phase == PH_MISS) {
          cn.bgs = 1;
          rt_v3 bg = background_lookup(SP, dir);
          radiance = rt_v3_mul_add(bg, tint, emis);
          done = true;
        }
        LGM("env_end");
        // ---- hits: shade them now, or park them until a dense shade block can be made of them ----
        // A shade block costs ~2 200 instructions whatever the number of lanes in it, and hits arrive ~34 at a time.  While
        // the tile still hands out paths, the hits of a sparse S block are PARKED (18 dwords of path state per hit into the
        // wave's slice of `park`, struct-of-arrays: every store is one 256-byte line) and their lanes start new camera
        // paths; once the hits at hand plus the parked ones that fit into idle lanes make RT_PARK_DENSE lanes, the parked
        // ones come back into idle lanes and all are shaded in one block.  A draining tile shades what it has.  Which
        // wave-iteration shades a path does not matter: its state (rng included) travels with it, sums are order-free.
        bool shade_now = true;
        if (park) {
          const unsigned long long mHit = __ballot(T.phase == PH_HIT);
          const unsigned long long mIdle = __ballot(T.phase == PH_NEED) | __ballot(T.phase == PH_MISS);
          const int h = (int)__popcll(mHit), f = (int)__popcll(mIdle);
          const int back = n_parked < f ? n_parked : f;                 // parked hits that fit into idle lanes
          uint32_t *pk = park + (size_t)__builtin_amdgcn_readfirstlane(wave_id) * (RT_PARK_FIELDS * RT_PARK_CAP);    // (scalar base)
          if (!tile_open || h + back >= RT_PARK_DENSE || n_parked + h > RT_PARK_CAP) {
            if (back > 0) {
              LG(LG_PLOAD_X, 1); LG(LG_PLOAD_L, back);
              LGM("pload_begin");
              if (done) {                                               // (an environment lane is idle once its sample is added)
                tile_add_sample(smem, acc_off, pix, radiance);
                T.phase = PH_NEED;
                done = false;
              }
              const int rank = lane_rank(mIdle);
              if (T.phase == PH_NEED && rank < back) {
                const uint32_t *q = pk + (n_parked - 1 - rank);         // most recently parked first
                uint32_t v[RT_PARK_FIELDS];
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int i = 0; i < RT_PARK_FIELDS; i++)
                  v[i] = __hip_atomic_load(q + i * RT_PARK_CAP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                T.hit.t = as_f((int)v[0]); T.hit.tri = (int)v[1]; T.hit.u = as_f((int)v[2]); T.hit.v = as_f((int)v[3]);
                org = rt_v3_make(as_f((int)v[4]), as_f((int)v[5]), as_f((int)v[6]));
                dir = rt_v3_make(as_f((int)v[7]), as_f((int)v[8]), as_f((int)v[9]));
                tint = rt_v3_make(as_f((int)v[10]), as_f((int)v[11]), as_f((int)v[12]));
                emis = rt_v3_make(as_f((int)v[13]), as_f((int)v[14]), as_f((int)v[15]));
                rng = v[16]; pix = (int)(v[17] & 63u); bounce = (int)(v[17] >> 6);
                T.phase = PH_HIT;
              }
              n_parked -= back;
              LGM("pload_end");
            }
          } else if (h > 0) {
            LG(LG_PSTORE_X, 1); LG(LG_PSTORE_L, h);
            LGM("pstore_begin");
            shade_now = false;
            const int rank = lane_rank(mHit);
            if (T.phase == PH_HIT) {
              uint32_t *q = pk + (n_parked + rank);
              const uint32_t v[RT_PARK_FIELDS] = {(uint32_t)as_i(T.hit.t), (uint32_t)T.hit.tri, (uint32_t)as_i(T.hit.u), (uint32_t)as_i(T.hit.v),
                                                  (uint32_t)as_i(org.x), (uint32_t)as_i(org.y), (uint32_t)as_i(org.z),
                                                  (uint32_t)as_i(dir.x), (uint32_t)as_i(dir.y), (uint32_t)as_i(dir.z),
                                                  (uint32_t)as_i(tint.x), (uint32_t)as_i(tint.y), (uint32_t)as_i(tint.z),
                                                  (uint32_t)as_i(emis.x), (uint32_t)as_i(emis.y), (uint32_t)as_i(emis.z),
                                                  rng, (uint32_t)pix | ((uint32_t)bounce << 6)};
#pragma unroll
              for (int i = 0; i < RT_PARK_FIELDS; i++) q[i * RT_PARK_CAP] = v[i];
              // the record is read back by ANOTHER lane of this wave (agent-scope loads below): the release / acquire pair at
              // wavefront scope states that order to the compiler; the hardware returns one wave's vector memory operations in order
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              T.phase = PH_NEED;
            }
            n_parked += h;
            LGM("pstore_end");
          }
        }
#ifdef RT_LEDGER
        { const int n_sh = (int)__popcll(__ballot(T.phase == PH_HIT && shade_now)); LG(LG_SHADE_X, n_sh != 0); LG(LG_SHADE_L, n_sh); }
#endif
        LGM("shade_begin");
        if (T.phase == PH_HIT && shade_now) {
          done = shade_hit(SP, T.hit, org, dir, tint, emis, rng, bounce, cn, radiance);
          start = !done;
        }
        LGM("shade_end");
#ifdef RT_LEDGER
        { const int n_acc = (int)__popcll(__ballot(done)); LG(LG_ACCUM_X, n_acc != 0); LG(LG_ACCUM_L, n_acc); }
#endif
        LGM("accum_begin");
        if (done) {
          tile_add_sample(smem, acc_off, pix, radiance);
          T.phase = PH_NEED;
        }
        LGM("accum_end");
        w_shades += (uint32_t)__popcll(__ballot(cn.shades != 0));
        w_tex += (uint32_t)__popcll(__ballot(cn.textured != 0));
        w_bgs += (uint32_t)__popcll(__ballot(cn.bgs != 0));

        // ---- regeneration: idle lanes take the next paths of the tile, across chunk boundaries ----
        if (tile_open) {
          NewPath np = {0, 0, 0, 0};
          const bool got = regen_paths(T.phase, np, SP.max_bounces > 0, U, tile_open, false, lane, tile_idx, n_chunks_tile, tile_x0, tile_y0,
                                       shift, unit_paths, t_wave_start, t_last_grab, w_paths LG_ARG);
          if (!tile_open) LGD0((int)__popcll(__ballot(T.phase != PH_NEED || got)) + n_parked);      // (ledger builds: the tile's drain starts here)
          const int gx = np.x, gy = np.y, gs = np.sample, width = A->width;
#ifdef RT_LEDGER
          { const int n_pr = (int)__popcll(__ballot(got)); LG(LG_PRIM_X, n_pr != 0); LG(LG_PRIM_L, n_pr); LG(LG_REGEN_L, n_pr); }
#endif
          LGM("prim_begin");
          if (got) {
            typename CamSrc<VIEWS>::type S;
            if constexpr (VIEWS) S = vrec; else S = A;
            pix = np.pix;
            bounce = 0;
            rng = rt_path_seed(S->seed, (uint32_t)(gx + gy * width), (uint32_t)gs);
            PrimaryParams PP;
            primary_params(PP, S, A);
            primary_ray(PP, gx, gy, gs, org, dir);
            tint = rt_v3_make(1, 1, 1);
            emis = rt_v3_make(0, 0, 0);
            start = true;
            fresh = true;
          }
          LGM("prim_end");
        }
        bool skip_root = false;
#ifdef RT_LEDGER
        { const int n_st = (int)__popcll(__ballot(start)); LG(LG_START_X, n_st != 0); LG(LG_START_L, n_st); }
#endif
        LGM("start_begin");
        if (start) {                      // a new ray: traversal starts at the root (or at leaf group 0)
          ray_setup<SHORT_DIV>(ray, org, dir);
          trav_start(T, leaf_level, P.last_row_offset);
          // (at level -1 the word holds no children yet: 1 tells the root visit below that it serves this ray -- the ray is NaN-free and
          //  the root has one to four populated children (RT_PYR_ROOT_POP); the LDS read hides behind the ray set-up here, and a scene whose
          //  root the visit does not serve pays one ballot per traversal call for it, no LDS round trip)
          T.cur = (LDSN && ray.fast && reinterpret_cast<const uint32_t *>(lds_at(smem, pyr_off))[RT_PYR_ROOT_POP] != 0u) ? 1u : 0u;
          // camera ray of a tile that cannot touch the scene: its one node visit finds no candidate (see tile_root_miss)
          skip_root = fresh && tile_root_miss && ray.fast;
          if (skip_root) T.phase = PH_MISS;
        }
        LGM("start_end");
        w_rays += (uint32_t)__popcll(__ballot(start));
        {
          const uint32_t n_skip = (uint32_t)__popcll(__ballot(skip_root));
          w_nodes += n_skip;
          if (n_skip != 0u && lane == 0) atomicAdd(cold_args()->counters + RT_CNT_SKIPPED_ROOT, (unsigned long long)n_skip);   // (rare: a sky tile outside the sky loop)
        }
        LGM("s_end");
        LGT1(LG_CYC_S);
      }

      const int n_trav0 = (int)__popcll(__ballot(T.phase == PH_NODE || T.phase == PH_LEAF));
      if (n_trav0 == 0) {
        if (__any(T.phase == PH_MISS)) continue;   // camera rays that skipped the root: straight to the environment
        if (n_parked > 0 || __any(T.phase == PH_HIT)) continue;      // parked hits come back in the next S block
        if (!tile_open) break;            // every path of the tile that this wave took has ended
        continue;                         // (nothing started, e.g. pixels outside the image: pull more)
      }

      // ================= the root visit of the rays that the S block started =================
      // Every such ray sits at the root (level -1, PH_NODE) and would take the first traversal round for it, camera rays in a culled
      // block of their own and bounce rays in a full one: 8 slab tests and the rank order of 8, where only the root's POPULATED
      // children can be candidates.  With at most four of those (the word RT_PYR_ROOT_POP of the pyramid area) the visit runs here, for camera and bounce
      // rays together, as node_enter_few() over a wave-uniform set: the populated children, less those the tile's pyramid cannot
      // touch when every ray at the root is a camera ray of the tile (the root's entry of the (tile, node) mask cache, written by
      // the tile set-up; a child the pyramid culls is a miss for a camera ray anyway).  Same word as the node block's, same state
      // after it: the first child and PH_NODE / PH_LEAF, or PH_MISS at level -1 where the pop would end -- a lane that traversed
      // and has finished, for the exit rule below.  Rays that are not NaN-free, and roots left to the node blocks (RT_PYR_ROOT_POP == 0),
      // keep child = 0, PH_NODE.
      if (LDSN) {
        const bool at_root = T.phase == PH_NODE && T.level < 0 && T.cur != 0u;      // (`cur`: set where the ray starts; ray.fast itself is in scratch here)
        const int n_root = (int)__popcll(__ballot(at_root));
        if (n_root != 0) {
          LGM("root_begin");
          LG(LG_ROOTF_X, 1); LG(LG_ROOTF_L, n_root);
          // (both words in one LDS round trip; this glue runs once per traversal call and waits for whatever it reads)
          uint32_t *pw = reinterpret_cast<uint32_t *>(lds_at(smem, pyr_off));
          const uint32_t w_pop = pw[RT_PYR_ROOT_POP], w_cull = pw[RT_PYR_NODE_CACHE];      // (node 0's cache entry)
          uint32_t rsurv = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_pop);      // (not 0: `cur`)
          w_nodes += (uint32_t)n_root;
          // The count: one LDS add that returns nothing, by lane 0.  Written as the instruction itself: the atomic built-in compiles
          // to the same ds_add_u32 behind a wave-aggregation prologue (a lane count, a multiply) that this one-lane add has no use
          // for -- measured 0.03 ms per step of config #3 (profiles/r07_root_visits.md); same registers either way.  The address is
          // the pointer cast to the LDS address space, i.e. its 32-bit offset.
          if (lane_now() == 0) {
            const uint32_t at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)(pw + RT_PYR_ROOT_FUSED);
            asm volatile("ds_add_u32 %0, %1" : : "v"(at), "v"((uint32_t)n_root) : "memory");
          }
          if (__ballot(at_root && bounce != 0) == 0ull) {
            const uint32_t ce = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_cull);
            if ((ce >> 8) == 1u) rsurv &= ~ce;
          }
          if (at_root) {
            T.level = 0;
            T.cur = rsurv ? node_enter_few<true>(ray, lds_nodes, 0, rsurv, RT_INF) : 0u;
            if (T.cur >> 24) {
              T.child = 1 + (int)(T.cur & 7u);
              T.cur = ((T.cur >> 3) & 0x1FFFFFu) | (((T.cur >> 24) - 1u) << 24);
              T.phase = (leaf_level == 0) ? PH_LEAF : PH_NODE;
            } else {
              T.level = -1;
              T.phase = PH_MISS;
            }
          }
          LGM("root_end");
        }
      }

      // ================= traversal: NODE / LEAF blocks until `thresh` lanes wait for S =================
      // while the tile still hands out paths, wait until `thresh` lanes want the S block (dense shading); once it is
      // exhausted nothing refills the lanes, and what matters is the latency of the remaining paths' bounce chains:
      // shade as soon as `drain_thresh` lanes wait
      const TravWave W = {smem, lds_nodes, L.perm, n_lds, pyr_nodes, pyr_off, leaf_level, lane};
      traversal_blocks<LDSN, SHORT_DIV, true>(P, W, ray, bounce == 0, T, tile_open ? thresh : drain_thresh, n_trav0, w_nodes, w_leaves LG_ARG);
    }

    // ---------------- flush the wave's share of the tile: lane p owns pixel p ----------------
    LGD1();
    LGM("flush_begin");
    if (U.took_any) {
      LGT0();
      LG(LG_FLUSH_X, 1);
      RT_KArgs A = cold_args();
      unsigned long long *frame = A->accum;
      if constexpr (VIEWS) frame += (size_t)(vrec - (RT_KViewP)A->views) * (size_t)A->pixels_per_view * 3;   // this tile's view
      flush_tile(acc, lane, tile_x0, tile_y0, frame, tile_idx, w_rays - rays_before);
      if (LDSN && lane == 0) {            // counters[RT_CNT_FUSED_ROOT]: the root visits this wave ran in front of its traversal calls
        uint32_t *pw = reinterpret_cast<uint32_t *>(lds_at(smem, pyr_off));
        const uint32_t n_fused = pw[RT_PYR_ROOT_FUSED];
        pw[RT_PYR_ROOT_FUSED] = 0u;
        if (n_fused != 0u) atomicAdd(A->counters + RT_CNT_FUSED_ROOT, (unsigned long long)n_fused);
      }
      steal_tries = 0;                    // joined (or owned) a tile that had work: keep looking for more
      n_tiles_done += 1;
      LGT1(LG_CYC_FLUSH);
    }
  }
  RT_KArgs A = cold_args();
  unsigned long long *wave_times = A->wave_times, *counters = A->counters;
  if (wave_times && lane == 0 && wave_id < 65536) {
    wave_times[wave_id * 3 + 0] = t_wave_start;
    wave_times[wave_id * 3 + 1] = __builtin_amdgcn_s_memrealtime();
    wave_times[wave_id * 3 + 2] = ((t_last_grab - t_wave_start) << 16) | (n_tiles_done & 0xFFFFu);
  }

  if (lane == 0) {
    atomicAdd(counters + RT_CNT_PATHS, (unsigned long long)w_paths);
    atomicAdd(counters + RT_CNT_RAYS, (unsigned long long)w_rays);
    atomicAdd(counters + RT_CNT_NODES, (unsigned long long)w_nodes);
    atomicAdd(counters + RT_CNT_LEAVES, (unsigned long long)w_leaves);
    atomicAdd(counters + RT_CNT_SHADES, (unsigned long long)w_shades);
    atomicAdd(counters + RT_CNT_BG, (unsigned long long)w_bgs);
    atomicAdd(counters + RT_CNT_TEXTURED, (unsigned long long)w_tex);
#ifdef RT_LEDGER
    LG(LG_CYC_WAVE, (uint32_t)((__builtin_amdgcn_s_memtime() - lg_wave_t0) >> 4));
#endif
  }
}

// ---------------------------------------------------------------------------------
// accum -> mean -> clamp -> sRGB -> u8 (raytracer.c:700-716), one thread per pixel
// of this rank's chunks.
__global__ void rt_resolve_kernel(int width, int height, int samples, int chunks_x, const int32_t *local_chunks,
                                  int n_local_chunks, const unsigned long long *accum,
                                  uint8_t *tiles, uint8_t *image, float *linear) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_local_chunks * 1024) return;
  int lchunk = idx >> 10, p = idx & 1023;
  int chunk = local_chunks[lchunk];
  int x = (chunk % chunks_x) * 32 + (p & 31);
  int y = (chunk / chunks_x) * 32 + (p >> 5);
  uint8_t rgb[3] = {0, 0, 0};
  if (x < width && y < height) {
    size_t pix = (size_t)y * width + x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float lin = rt_accum_resolve(accum[pix * 3 + c], (uint32_t)samples);
      if (linear) linear[pix * 3 + c] = lin;
      rgb[c] = rt_encode_u8(lin);
      if (image) image[pix * 3 + c] = rgb[c];
    }
  }
  if (tiles) {
    tiles[(size_t)idx * 3 + 0] = rgb[0];
    tiles[(size_t)idx * 3 + 1] = rgb[1];
    tiles[(size_t)idx * 3 + 2] = rgb[2];
  }
}

// gathered compact tiles [world][max_local][1024*3] -> row-major image; owner_slot[chunk] = rank * max_local + slot
__global__ void rt_untile_kernel(int width, int height, int chunks_x, int n_chunks, const int32_t *owner_slot,
                                 const uint8_t *all_tiles, uint8_t *image) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_chunks * 1024) return;
  int chunk = idx >> 10, p = idx & 1023;
  int x = (chunk % chunks_x) * 32 + (p & 31);
  int y = (chunk / chunks_x) * 32 + (p >> 5);
  if (x >= width || y >= height) return;
  const uint8_t *src = all_tiles + ((size_t)owner_slot[chunk] * 1024 + p) * 3;
  uint8_t *dst = image + ((size_t)y * width + x) * 3;
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
}

// ---------------------------------------------------------------------------------
// lightmap_bake (raytracer.c:722-784): the second caller of the path loop.
// Pass 1 rasterises every triangle in UV space and records, per texel, the LAST triangle that covers it
// (the reference's sequential loop overwrites in triangle order); pass 2 bakes each owned texel:
// `samples` cosine-weighted paths of 8 bounces from the interpolated surface point.

// (the acceptance test, raytracer.c:733-747, and min3f / max3f: one text, shared with rt_lightmap.hip)
#include "rt_lightmap_weights.hip.h"

__global__ void rt_lightmap_owner_kernel(RT_KParams P, int n_tris, int lw, int lh, int *owner) {
  int i = blockIdx.x;
  if (i >= n_tris) return;
  const float *tb = P.tris + (size_t)i * 28;
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
  for (int t = threadIdx.x; t < bw * bh; t += blockDim.x) {
    int x = x0 + t % bw, y = y0 + t / bw;
    float w0, w1, w2;
    if (lightmap_weights(p0x, p0y, p1x, p1y, p2x, p2y, x, y, w0, w1, w2)) atomicMax(&owner[y * lw + x], i);
  }
}

// raytracer.c:505-558 for one ray, sequential per lane (used by the lightmap; the frame kernels schedule
// the same steps per phase instead)
__device__ __forceinline__ rt_v3 cast_ray_lane(const RT_KParams &P, rt_v3 org, rt_v3 dir, uint32_t &rng,
                                               uint32_t *perm, int lane, LaneCounters &cn) {
  rt_v3 tint = rt_v3_make(1, 1, 1), emis = rt_v3_make(0, 0, 0), radiance = rt_v3_make(0, 0, 0);
  int bounce = 0;
  bool done = P.max_bounces <= 0;
  while (!done) {
    Ray3 ray;
    ray_setup(ray, org, dir);
    HitRec hit;
    if (ray.fast) trace_ray<true>(P, ray, hit, perm, lane, cn);
    else trace_ray<false>(P, ray, hit, perm, lane, cn);
    if (hit.tri >= 0) {
      done = shade_hit(P, hit, org, dir, tint, emis, rng, bounce, cn, radiance);
    } else {
      cn.bgs += 1;
      radiance = rt_v3_mul_add(background_lookup(P, dir), tint, emis);
      done = true;
    }
  }
  return radiance;
}

// common.h:30-42
__device__ __forceinline__ rt_v3 rand_vec3_dev(uint32_t &rng) {
  for (;;) {
    rt_v3 p;
    p.x = rt_rand_f32(&rng) * (1.0f - -1.0f) + -1.0f;
    p.y = rt_rand_f32(&rng) * (1.0f - -1.0f) + -1.0f;
    p.z = rt_rand_f32(&rng) * (1.0f - -1.0f) + -1.0f;
    float lensq = rt_v3_dot(p, p);
    if (RT_EPS < lensq && lensq <= 1.0f) return rt_v3_scale(p, 1.0f / rt_sqrtf(lensq));
  }
}

__global__ __launch_bounds__(RT_BLOCK_THREADS) void rt_lightmap_bake_kernel(RT_KParams P, const float *verts, int lw, int lh,
                                                                            int stride, int comp, int samples,
                                                                            const int *owner, uint8_t *pixels) {
  __shared__ uint32_t s_perm[RT_BLOCK_WAVES][RT_MAX_DEPTH * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= lw * lh) return;
  int i = owner[idx];
  if (i < 0) return;
  int x = idx % lw, y = idx / lw;
  const float *tb = P.tris + (size_t)i * 28;
  float flw = (float)lw, flh = (float)lh;
  float w0, w1, w2;
  lightmap_weights(tb[7] * flw, tb[11] * flh, tb[15] * flw, tb[19] * flh, tb[23] * flw, tb[24] * flh, x, y, w0, w1, w2);
  const float *v = verts + (size_t)i * 9;       // x0 x1 x2 y0 y1 y2 z0 z1 z2 (original vertices, scene.h:53-60)
  rt_v3 position = rt_v3_make(v[0] * w0 + v[1] * w1 + v[2] * w2, v[3] * w0 + v[4] * w1 + v[5] * w2,
                              v[6] * w0 + v[7] * w1 + v[8] * w2);
  rt_v3 normal = rt_v3_make(tb[4] * w0 + tb[8] * w1 + tb[12] * w2, tb[5] * w0 + tb[9] * w1 + tb[13] * w2,
                            tb[6] * w0 + tb[10] * w1 + tb[14] * w2);
  rt_v3 org = rt_v3_add(position, rt_v3_scale(normal, RT_EPS));
  uint32_t rng = rt_path_seed(P.seed, (uint32_t)(x + y * lw), (uint32_t)i);
  LaneCounters cn;
  cn.rays = cn.nodes = cn.leaves = cn.shades = cn.bgs = cn.textured = cn.paths = 0;
  rt_v3 acc = rt_v3_make(0, 0, 0);
  for (int s = 0; s < samples; s++) {
    float cosv;
    rt_v3 d;
    int guard = 0;
    for (;;) {
      d = rand_vec3_dev(rng);
      cosv = rt_v3_dot(d, normal);
      if (cosv > 0.0f) break;
      if (++guard >= 64) { cosv = 0.0f; break; }
    }
    acc = rt_v3_add(acc, rt_v3_scale(cast_ray_lane(P, org, d, rng, s_perm[wave], lane, cn), cosv));
  }
  float out[3] = {acc.x / (float)samples, acc.y / (float)samples, acc.z / (float)samples};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float q = out[c] > 0.0f ? out[c] : 0.0f;
    q = q > 255.0f ? 255.0f : q;
    pixels[((size_t)x + (size_t)y * stride) * comp + c] = (uint8_t)q;
  }
}

extern "C" int rt_launch_lightmap(const RT_KParams *P, const float *verts, int n_tris, int lw, int lh, int stride, int comp,
                                  int samples, int *owner, uint8_t *pixels, hipStream_t stream) {
  hipLaunchKernelGGL(rt_lightmap_owner_kernel, dim3(n_tris), dim3(64), 0, stream, *P, n_tris, lw, lh, owner);
  int n = lw * lh;
  hipLaunchKernelGGL(rt_lightmap_bake_kernel, dim3((n + RT_BLOCK_THREADS - 1) / RT_BLOCK_THREADS), dim3(RT_BLOCK_THREADS), 0,
                     stream, *P, verts, lw, lh, stride, comp, samples, owner, pixels);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Per-launch preparation in ONE launch of one workgroup: zero the ray counters and the work head, reset every tile's unit
// counter and the open-tile count of every group of 64 tiles, zero the cost buffer this launch will fill, and -- when the
// previous launch of the same view left its costs -- the tile order of this one: counting sort of the tiles by descending
// cost bucket (4 buckets per power of two of that launch's ray count; order inside a bucket is whatever the LDS atomics give:
// only the schedule depends on it, never a pixel).  Round 2 spent three memsets and five small kernels on this, ~25 us
// of launch gaps per frame -- a fifth of a frame at the reference's default size (1024 x 1024, 16 spp).
#define RT_ORDER_BUCKETS 132
__device__ __forceinline__ int cost_bucket(uint32_t c) {
  if (c < 4u) return (int)c;                               // 0..3
  int e = 31 - __clz((int)c);                              // >= 2
  return 4 * (e - 1) + (int)((c >> (e - 2)) & 3u);         // 4..131, monotonic in c
}

__global__ __launch_bounds__(1024) void rt_prepare_kernel(int n_tiles, uint32_t *tile_next, uint32_t *open_groups,
                                                          unsigned long long *counters, uint32_t *work_head, uint32_t *cost_cur,
                                                          const uint32_t *cost_prev, uint32_t *order) {
  // counting sort: every wave counts its own share of the tiles per bucket in its own LDS row, one scan turns the 16 x 132
  // counts into per-(wave, bucket) start positions, and every wave scatters its tiles from its own cursors.  (One shared
  // row of LDS atomics took 100-170 us for the 32 400 tiles of 1080p: most tiles fall into a handful of buckets.)
  __shared__ uint32_t hist[16][RT_ORDER_BUCKETS];
  __shared__ uint32_t bucket_start[RT_ORDER_BUCKETS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < RT_N_COUNTERS) counters[tid] = 0ull;
  if (tid < 16) work_head[tid] = 0u;
  for (int i = tid; i < n_tiles; i += 1024) {
    if (tile_next) tile_next[i] = 0u;
    if (cost_cur) cost_cur[i] = 0u;
  }
  if (open_groups) {
    const int n_groups = (n_tiles + 63) >> 6;
    for (int g = tid; g < n_groups; g += 1024) {
      int left = n_tiles - g * 64;
      open_groups[g] = (uint32_t)(left < 64 ? left : 64);
    }
  }
  if (!cost_prev || !order) return;
  // a wave owns the tiles [wave * per_wave, (wave + 1) * per_wave) and its own row of counters in LDS.  Per batch of 64
  // tiles the (up to) three most common buckets are counted by ballot -- neighbouring tiles cost about the same, most of a
  // batch falls into one or two buckets, and 64 LDS atomics on one word serialise -- the stragglers by LDS atomics.
  for (int b = lane; b < RT_ORDER_BUCKETS; b += 64) hist[wave][b] = 0u;
  const int per_wave = ((n_tiles + 15) / 16 + 63) & ~63;
  const int first = wave * per_wave, last = first + per_wave < n_tiles ? first + per_wave : n_tiles;
  // (16 batches' costs are loaded together: one dependent load per batch would cost its full latency -- the cost buffer was
  // written by the previous launch's atomics and sits at the memory side -- 32 times per wave and phase)
  for (int group = first; group < last; group += 64 * 16) {
    int bk[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int i = group + 64 * k + lane;
      // (an unsigned cost of 2^31 or more must not read as "no tile" -- the tile would drop out of the count AND of the scatter and
      //  leave a stale entry in the order: it saturates; the bucket function is monotonic)
      bk[k] = i < last ? (int)(cost_prev[i] > 0x7FFFFFFFu ? 0x7FFFFFFFu : cost_prev[i]) : -1;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int bkt = bk[k] >= 0 ? cost_bucket((uint32_t)bk[k]) : -1;
      unsigned long long todo = __ballot(bkt >= 0);
#pragma unroll
      for (int round = 0; round < 3; round++) {
        if (!todo) break;
        const int b0 = __builtin_amdgcn_readlane(bkt, (int)__builtin_ctzll(todo));
        const unsigned long long m = __ballot(bkt == b0);
        if (lane == 0) atomicAdd(&hist[wave][b0], (uint32_t)__popcll(m));
        todo &= ~m;
      }
      if ((todo >> lane) & 1ull) atomicAdd(&hist[wave][bkt], 1u);
    }
  }
  __syncthreads();
  if (tid < RT_ORDER_BUCKETS) {                            // per bucket: total, and the waves' shares as running offsets
    uint32_t run = 0;
    for (int w = 0; w < 16; w++) { uint32_t c = hist[w][tid]; hist[w][tid] = run; run += c; }
    bucket_start[tid] = run;                               // (count for now)
  }
  __syncthreads();
  if (tid == 0) {                                          // start offset of every bucket, expensive first
    uint32_t run = 0;
    for (int b = RT_ORDER_BUCKETS - 1; b >= 0; b--) { uint32_t c = bucket_start[b]; bucket_start[b] = run; run += c; }
  }
  __syncthreads();
  for (int b = lane; b < RT_ORDER_BUCKETS; b += 64) hist[wave][b] += bucket_start[b];     // this wave's cursors
  for (int group = first; group < last; group += 64 * 16) {
    int bk[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int i = group + 64 * k + lane;
      // (an unsigned cost of 2^31 or more must not read as "no tile" -- the tile would drop out of the count AND of the scatter and
      //  leave a stale entry in the order: it saturates; the bucket function is monotonic)
      bk[k] = i < last ? (int)(cost_prev[i] > 0x7FFFFFFFu ? 0x7FFFFFFFu : cost_prev[i]) : -1;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int i = group + 64 * k + lane;
      const int bkt = bk[k] >= 0 ? cost_bucket((uint32_t)bk[k]) : -1;
      unsigned long long todo = __ballot(bkt >= 0);
#pragma unroll
      for (int round = 0; round < 3; round++) {
        if (!todo) break;
        const int b0 = __builtin_amdgcn_readlane(bkt, (int)__builtin_ctzll(todo));
        const unsigned long long m = __ballot(bkt == b0);
        uint32_t pos = 0;
        if (lane == 0) pos = atomicAdd(&hist[wave][b0], (uint32_t)__popcll(m));
        pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);
        const int rank = lane_rank(m);
        if (bkt == b0) order[pos + (uint32_t)rank] = (uint32_t)i;
        todo &= ~m;
      }
      if ((todo >> lane) & 1ull) order[atomicAdd(&hist[wave][bkt], 1u)] = (uint32_t)i;
    }
  }
}

extern "C" int rt_launch_prepare(int n_tiles, uint32_t *tile_next, uint32_t *open_groups, unsigned long long *counters,
                                 uint32_t *work_head, uint32_t *cost_cur, const uint32_t *cost_prev, uint32_t *order,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(rt_prepare_kernel, dim3(1), dim3(1024), 0, stream, n_tiles, tile_next, open_groups, counters, work_head, cost_cur,
                     cost_prev, order);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------
// launchers (called from rt_launch.cpp, rt_residency.cpp, rt_extras.cpp)

template <int WAVES, bool LDSN, int MINW, bool SHORT_DIV, bool VIEWS, bool SHARED_TAPS>
static int launch_stream(const RT_KParams *P, int n_waves, int smem_bytes, hipStream_t stream) {
  static uint32_t attr_devices = 0;
  if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&rt_path_kernel_stream<WAVES, LDSN, MINW, SHORT_DIV, VIEWS, SHARED_TAPS>), &attr_devices,
                               smem_bytes, RT_LDS_BYTES - RT_LDS_TABLE_BYTES))      // (the kernel has the sRGB scale table)
    return rc;
#ifdef RT_LEDGER
  {
    void *sym = nullptr;
    if (n_waves > RT_LEDGER_WAVES) return (int)hipErrorInvalidValue;
    hipError_t e = hipGetSymbolAddress(&sym, HIP_SYMBOL(g_ledger));
    if (e == hipSuccess) e = hipMemsetAsync(sym, 0, sizeof(uint32_t) * RT_LEDGER_WAVES * RT_LEDGER_ROW, stream);
    if (e != hipSuccess) return (int)e;
  }
#endif
  hipLaunchKernelGGL((rt_path_kernel_stream<WAVES, LDSN, MINW, SHORT_DIV, VIEWS, SHARED_TAPS>), dim3((n_waves + WAVES - 1) / WAVES),
                     dim3(WAVES * 64), smem_bytes, stream, *P);
#ifdef RT_LEDGER
  hipLaunchKernelGGL(rt_ledger_reduce_kernel, dim3(1), dim3(RT_LEDGER_ROW), 0, stream, P->counters);
#endif
  return (int)hipGetLastError();
}

extern "C" int rt_math_contract(void) { return RT_MATH_CONTRACT; }      // include/rt_math.h: 2 = explicit FMA, 1 = -DRT_MATH_NO_FMA

template <bool VIEWS, bool SHARED_TAPS>
static int launch_stream_wg(const RT_KParams *P, int n_waves, int smem_bytes, int wg_waves, hipStream_t stream) {
  if (wg_waves == 8)
    return P->short_div ? launch_stream<8, true, 1, true, VIEWS, SHARED_TAPS>(P, n_waves, smem_bytes, stream)
                        : launch_stream<8, true, 1, false, VIEWS, SHARED_TAPS>(P, n_waves, smem_bytes, stream);
  if (wg_waves == 12)
    return P->short_div ? launch_stream<12, true, 1, true, VIEWS, SHARED_TAPS>(P, n_waves, smem_bytes, stream)
                        : launch_stream<12, true, 1, false, VIEWS, SHARED_TAPS>(P, n_waves, smem_bytes, stream);
  return P->short_div ? launch_stream<16, true, 1, true, VIEWS, SHARED_TAPS>(P, n_waves, smem_bytes, stream)
                      : launch_stream<16, true, 1, false, VIEWS, SHARED_TAPS>(P, n_waves, smem_bytes, stream);
}

// `wg_waves` = waves per workgroup, 8 / 12 / 16 (one workgroup per CU: 2 / 3 / 4 waves per SIMD), chosen by rt_launch.cpp from the
// size of the launch; the same kernel source, three instances of its launch geometry.
extern "C" int rt_launch_path_kernel(const RT_KParams *P, int n_waves, int smem_bytes, int wg_waves, hipStream_t stream) {
  // (shared_taps: the host found every material's textures of one size, rt_launch.cpp -- the instance with one set of taps per hit)
  if (P->n_views > 0)                                                                                // one launch, K views
    return P->shared_taps ? launch_stream_wg<true, true>(P, n_waves, smem_bytes, wg_waves, stream)
                          : launch_stream_wg<true, false>(P, n_waves, smem_bytes, wg_waves, stream);
  return P->shared_taps ? launch_stream_wg<false, true>(P, n_waves, smem_bytes, wg_waves, stream)
                        : launch_stream_wg<false, false>(P, n_waves, smem_bytes, wg_waves, stream);
}

extern "C" int rt_launch_resolve(int width, int height, int samples, int chunks_x, const int32_t *local_chunks,
                                 int n_local_chunks, const unsigned long long *accum, uint8_t *tiles,
                                 uint8_t *image, float *linear, hipStream_t stream) {
  int n = n_local_chunks * 1024;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(rt_resolve_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, width, height, samples,
                     chunks_x, local_chunks, n_local_chunks, accum, tiles, image, linear);
  return (int)hipGetLastError();
}

extern "C" int rt_launch_untile(int width, int height, int chunks_x, int n_chunks, const int32_t *owner_slot,
                                const uint8_t *all_tiles, uint8_t *image, hipStream_t stream) {
  int n = n_chunks * 1024;
  hipLaunchKernelGGL(rt_untile_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, width, height, chunks_x,
                     n_chunks, owner_slot, all_tiles, image);
  return (int)hipGetLastError();
}

// raw u8 image rows (stride pixels x comp bytes, comp >= 3) -> RGBA8 words in the pool layout of rt_device.h (4 x 4 tiles).
// `rows` rows starting at row y0 of a texture `width` wide whose first texel is out[0] (rt_scene_touch packs a
// few rows of a resident texture again).
__global__ void rt_pack_texture_kernel(const uint8_t *raw, int width, int rows, int y0, int stride, int comp, uint32_t *out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)width * rows) return;
  int yl = (int)(i / width), x = (int)(i % width);
  const uint8_t *p = raw + ((size_t)yl * stride + x) * comp;
  const int y = y0 + yl;
  const size_t o = (size_t)RT_TEX_TILE_INDEX(x, y, (width + 3) >> 2);
  out[o] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | 0xFF000000u;
}

extern "C" int rt_launch_pack_texture(const uint8_t *raw, int width, int rows, int y0, int stride, int comp, uint32_t *out,
                                      hipStream_t stream) {
  size_t n = (size_t)width * rows;
  hipLaunchKernelGGL(rt_pack_texture_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, raw, width, rows, y0, stride,
                     comp, out);
  return (int)hipGetLastError();
}

// The same raw rows -> the float image of the background (rt_device.h: RT_KParams.bg_image): texel (x, y) of the (width + 1) x
// (height + 1) image is texel (min(x, width - 1), y) of the source, r g b as texel_rgb() converts them and a zero; a thread of the
// source's last row writes the pad row below it as well.  `rows` rows starting at row y0, as above.
__global__ void rt_pack_bg_image_kernel(const uint8_t *raw, int width, int height, int rows, int y0, int stride, int comp, float4 *out) {
  const int pitch = width + 1;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)pitch * rows) return;
  int yl = (int)(i / pitch), x = (int)(i % pitch);
  const int xs = x < width ? x : width - 1;
  const uint8_t *p = raw + ((size_t)yl * stride + xs) * comp;
  const int y = y0 + yl;
  const rt_v3 c = texel_rgb((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
  const float4 t = make_float4(c.x, c.y, c.z, 0.0f);
  out[(size_t)y * pitch + x] = t;
  if (y == height - 1) out[(size_t)height * pitch + x] = t;
}

extern "C" int rt_launch_pack_bg_image(const uint8_t *raw, int width, int height, int rows, int y0, int stride, int comp, float *out,
                                       hipStream_t stream) {
  size_t n = (size_t)(width + 1) * rows;
  hipLaunchKernelGGL(rt_pack_bg_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, raw, width, height, rows, y0,
                     stride, comp, reinterpret_cast<float4 *>(out));
  return (int)hipGetLastError();
}

// ---- batch ray queries (include/rt_hip.h: rt_query_closest, rt_query_occluded) ------------------------------------------------------
// ray_scene_hit (raytracer.c:443-503) for a list of rays the HOST supplies: which triangle, where (t, u, v) -- or, ANY, only whether
// there is one (the argument that the two agree: traversal_blocks, rt_dev.hip.h).  A persistent kernel in the path kernel's launch
// geometry: one workgroup per CU, the leading BVH nodes in LDS, a perm stack per wave, lanes refilled from the list as they finish.
//
// Work distribution: ONE counter for the whole launch (Q.head); a wave takes Q.grab consecutive rays per atomic and hands them to
// its lanes in order, so the 24-byte ray records of a refill are one contiguous read.  The grab size comes from the launch size
// (rt_query.cpp): what is left over when the counter runs out is at most one grab per wave, so a grab is an eighth of a wave's mean
// share -- a batch whose rays differ in cost ends with every wave within that eighth -- but never below 64 (one refill of an
// empty wave, and the atomic stays one in 64 rays) and never above 512.
//
// Reciprocals: IEEE division, in ray_setup and in the leaf blocks.  The short forms rcp_exact() / rcp_leaf() equal the division
// for |x| < 2^102 only (rt_test_rcp_sweep); the path kernel may use them because the HOST bounds every direction it can produce
// (unit vectors through a bounded camera matrix, shade()'s outputs) and with them every determinant.  A caller's rays carry no
// bound -- a direction of 2^110 is as legal as one of 2^-30 -- and a bound per batch would cost a pass over the rays before every
// launch, so this kernel has no short-division instance.
//
// No pyramid culling (the rays are no tile's camera rays).  Outputs by plain vector stores: 16 bytes or one byte per ray.
template <int WAVES, bool ANY>
__global__ __launch_bounds__(WAVES * 64, 1) void rt_query_kernel(RT_KParams P, RT_QParams Q) {
  extern __shared__ float4 smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n_lds = P.n_lds_nodes;
  lds_load_nodes<WAVES * 64>(smem, P.nodes, n_lds);
  __syncthreads();
  const int leaf_level = P.depth - 1;
  // (the wave's slice is the perm stack alone; no pyramid)
  const TravWave W = {smem, smem, wave_perm(smem, n_lds, perm_stack_f4(P.depth), wave), n_lds, 0, 0, leaf_level, lane};
  int  next = 0, end = 0;                                         // the wave's current grab: rays [next, end) are not handed out yet
  bool drained = false;                                           // the launch's counter has run past the list (wave-uniform)

  int   idx = 0;
  Ray3  ray;
  ray_setup(ray, rt_v3_make(0, 0, 0), rt_v3_make(0, 0, 1));
  uint32_t w_nodes = 0, w_leaves = 0, w_rays = 0, w_hits = 0;
  TravState T = RT_TRAV_IDLE;
  for (;;) {
    w_rays += (uint32_t)__popcll(__ballot(T.phase == PH_HIT || T.phase == PH_MISS));
    w_hits += (uint32_t)__popcll(__ballot(T.phase == PH_HIT));
    if (T.phase == PH_HIT || T.phase == PH_MISS) {
      // (a miss: t is still the entry bound, triangle -1, u = v = 0 -- nothing was accepted since the refill)
      if (ANY) Q.flags[idx] = T.phase == PH_HIT ? 1 : 0;
      else reinterpret_cast<float4 *>(Q.hits)[idx] = make_float4(T.hit.t, as_f(T.hit.tri), T.hit.u, T.hit.v);
      T.phase = PH_NEED;
    }
    // refill: every lane without a ray takes the next one of the wave's grab; a grab that runs out is followed by the next
    for (;;) {
      const unsigned long long need = __ballot(T.phase == PH_NEED);
      if (need == 0ull || drained) break;
      if (next >= end) {
        uint32_t s = 0;
        if (lane == 0) s = atomicAdd(Q.head, (uint32_t)Q.grab);
        s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
        if (s >= (uint32_t)Q.n) { drained = true; break; }
        next = (int)s;
        end = (Q.n - next < Q.grab) ? Q.n : next + Q.grab;
      }
      const int rank = lane_rank(need);
      if (T.phase == PH_NEED && next + rank < end) {
        idx = next + rank;
        const float *r = Q.rays + (size_t)idx * 6;
        ray_setup<false>(ray, rt_v3_make(r[0], r[1], r[2]), rt_v3_make(r[3], r[4], r[5]));
        trav_start(T, leaf_level, P.last_row_offset);
        if (Q.t_max) T.hit.t = Q.t_max[idx];                        // raytracer.c:452: hit.distance on entry is the upper bound
      }
      next += (int)__popcll(need);
    }
    const int n_trav0 = (int)__popcll(__ballot(T.phase == PH_NODE || T.phase == PH_LEAF));
    if (n_trav0 == 0) break;                                      // (only a drained wave gets here without a ray in flight)
    traversal_blocks<true, false, false, ANY>(P, W, ray, false, T, drained ? 64 : Q.exit_lanes, n_trav0, w_nodes, w_leaves);
  }
  if (lane == 0) {
    atomicAdd(Q.counters + RT_QCNT_RAYS, (unsigned long long)w_rays);
    atomicAdd(Q.counters + RT_QCNT_HITS, (unsigned long long)w_hits);
    atomicAdd(Q.counters + RT_QCNT_NODES, (unsigned long long)w_nodes);
    atomicAdd(Q.counters + RT_QCNT_LEAVES, (unsigned long long)w_leaves);
  }
}

// (ray, t, triangle, u, v) -> the reference's Hit without the Shader pair (RT_Device_Hit, rt_hip.h): the fill of raytracer.c:159-184
// from the 28-float triangle record, by surface_at() as shade_hit() reads it.  One thread per ray; a miss gets distance = t (the
// entry bound), triangle = material = -1 and zeros.  Records are 88 bytes, 8-byte aligned: eleven 8-byte stores.
__global__ void rt_hit_attributes_kernel(const float *tris, int n, const float *rays, const float *hits, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 h = reinterpret_cast<const float4 *>(hits)[i];
  const int tri = as_i(h.y);
  float o[RT_HIT_DWORDS];
#pragma unroll
  for (int k = 0; k < RT_HIT_DWORDS; k++) o[k] = 0.0f;
  o[0] = h.x;
  o[18] = as_f(tri);
  o[19] = as_f(-1);
  if (tri >= 0) {
    const float *r = rays + (size_t)i * 6;
    const rt_v3 org = rt_v3_make(r[0], r[1], r[2]), dir = rt_v3_make(r[3], r[4], r[5]);
    HitRec hit;
    hit.t = h.x; hit.tri = tri; hit.u = h.z; hit.v = h.w;
    const Surface s = surface_at(tris + (size_t)tri * 28, hit, org, dir);
    const rt_v3 tangent = s.tangent(), bitangent = s.bitangent();
    o[1] = s.n_int.x; o[2] = s.n_int.y; o[3] = s.n_int.z;         // normal (interpolated, not normalised: raytracer.c:172-174)
    o[4] = s.n_geo.x; o[5] = s.n_geo.y; o[6] = s.n_geo.z;
    o[7] = s.point.x; o[8] = s.point.y; o[9] = s.point.z;
    o[10] = tangent.x; o[11] = tangent.y; o[12] = tangent.z;
    o[13] = bitangent.x; o[14] = bitangent.y; o[15] = bitangent.z;
    o[16] = s.uvx();                                              // tex_coords
    o[17] = s.uvy();
    o[19] = s.q0.w;                                               // material id (int bits)
  }
  float2 *dst = reinterpret_cast<float2 *>(out + (size_t)i * RT_HIT_DWORDS);
#pragma unroll
  for (int k = 0; k < RT_HIT_DWORDS / 2; k++) dst[k] = make_float2(o[2 * k], o[2 * k + 1]);
}

template <int WAVES, bool ANY>
static int launch_query(const RT_KParams *P, const RT_QParams *Q, int n_blocks, int smem_bytes, hipStream_t stream) {
  static uint32_t attr_devices = 0;
  if (int rc = raise_lds_limit(reinterpret_cast<const void *>(&rt_query_kernel<WAVES, ANY>), &attr_devices, smem_bytes, RT_LDS_BYTES))
    return rc;
  hipLaunchKernelGGL((rt_query_kernel<WAVES, ANY>), dim3(n_blocks), dim3(WAVES * 64), smem_bytes, stream, *P, *Q);
  return (int)hipGetLastError();
}

// `wg_waves` = 8 or 16 waves per workgroup, `any` = the occlusion form (Q->flags) instead of the closest hit (Q->hits)
extern "C" int rt_launch_query(const RT_KParams *P, const RT_QParams *Q, int any, int wg_waves, int n_blocks, int smem_bytes,
                               hipStream_t stream) {
  if (wg_waves == 8)
    return any ? launch_query<8, true>(P, Q, n_blocks, smem_bytes, stream) : launch_query<8, false>(P, Q, n_blocks, smem_bytes, stream);
  return any ? launch_query<16, true>(P, Q, n_blocks, smem_bytes, stream) : launch_query<16, false>(P, Q, n_blocks, smem_bytes, stream);
}

extern "C" int rt_launch_hit_attributes(const RT_KParams *P, int n, const float *rays, const float *hits, float *out,
                                        hipStream_t stream) {
  hipLaunchKernelGGL(rt_hit_attributes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, P->tris, n, rays, hits, out);
  return (int)hipGetLastError();
}
