/* rt_device.h -- layout of the flattened scene in HBM and the kernel argument
 * block.  Shared by the host units (rt_launch.cpp fills it) and the kernels (read it).
 *
 * HBM layout (all read-only during a frame, 16-byte aligned):
 *   nodes   : BVH_Node as is, 12 float4 per node                 192 B / node
 *   leaves  : per leaf group g, 9 rows of 8 f32 (ax e1x e2x ay e1y e2y az e1z e2z,
 *             e1 = b-a, e2 = c-a): the reference's nine SoA arrays (scene.h:53-63)
 *             re-tiled so one group is 288 contiguous bytes, with the two edge
 *             subtractions of raytracer.c:115-122 done at upload  288 B / leaf
 *   tris    : Triangle_AOS without the Shader pair, plus a material id
 *                                                                 112 B / tri
 *   mats    : PBR_Shader_Data with texture pointers replaced by indices
 *                                                                  80 B / mat
 *   textures: descriptor table + one RGBA8 texel pool
 */
#ifndef RT_DEVICE_H
#define RT_DEVICE_H

#include <stdint.h>

#define RT_NODE_F4   12      /* float4 per node           */
#define RT_LEAF_F4   18      /* float4 per leaf group     */
#define RT_TRI_F4     7      /* float4 per triangle record*/
#define RT_MAT_F4     9      /* float4 per material       */
#define RT_MAT_FLOATS 36
#define RT_MAX_DEPTH  8      /* perm-stack levels in LDS  */

/* LDS of a workgroup of the kernels on traversal_blocks(): the leading BVH nodes (level order), then per wave a perm stack of one
 * level per tree level (at least one) and what else the kernel keeps per wave.  Split by lds_split (rt_launch.cpp). */
#define RT_LDS_BYTES            (160 * 1024)   /* LDS of a CU                                                              */
#define RT_LDS_NODE_BYTES       208            /* a node in LDS: 12 float4 of data + 1 of padding                          */
#define RT_LDS_TABLE_BYTES      64             /* static LDS of a kernel with the sRGB scale table (32 bytes, rounded up)   */
#define RT_LDS_PERM_LEVEL_BYTES 256            /* one level of a wave's perm stack                                         */
#define RT_LDS_ACC_TILE_BYTES   1536           /* path kernel, wavefront kernels: a wave's 8x8-pixel accumulator tile      */

#define RT_MAT_DISNEY 0
#define RT_MAT_DEBUG  1

#define RT_TILE      8       /* a tile = 8x8 pixels */
#define RT_TILE_PIX  64

#define RT_PARK_RECORD_DWORDS (18 * 128)   /* a wave's slice of RT_KParams.park: RT_PARK_FIELDS x RT_PARK_CAP (rt_dev.hip.h) */
/* RT_KParams.counters, one array of u64 per launch: index names for the kernels that add and the host units that read */
enum {
  RT_CNT_PATHS = 0, RT_CNT_RAYS, RT_CNT_NODES, RT_CNT_LEAVES, RT_CNT_SHADES, RT_CNT_BG, RT_CNT_TEXTURED,
  RT_CNT_SKIPPED_ROOT,         /* of RT_CNT_NODES: root visits of camera paths whose tile's pyramid misses the root -- counted, not executed */
  RT_CNT_LEDGER,               /* .. + RT_CNT_LEDGER_SLOTS: the block ledger of the path kernel (-DRT_LEDGER builds, LG_* slots in rt_dev.hip.h) */
  RT_CNT_LEAFLESS = 136,       /* camera paths served by the leafless loop (rt_kernels.hip), those of triangle-less tiles included */
  RT_CNT_FUSED_ROOT,           /* rays whose root visit ran in front of the traversal rounds (rt_kernels.hip) */
  RT_CNT_TRIANGLELESS,         /* of RT_CNT_LEAFLESS: paths of tiles whose pyramid reaches leaf groups, but no triangle of them */
  RT_N_COUNTERS
};
#define RT_CNT_LEDGER_SLOTS (RT_CNT_LEAFLESS - RT_CNT_LEDGER)

/* triangle record, 28 floats:
 *  [0..2] face normal      [3]  material id (int bits)
 *  [4..6] normal_a         [7]  uv_a.x
 *  [8..10] normal_b        [11] uv_a.y
 *  [12..14] normal_c       [15] uv_b.x
 *  [16..18] tangent        [19] uv_b.y
 *  [20..22] bitangent      [23] uv_c.x
 *  [24] uv_c.y             [25..27] pad
 */

/* material record, 20 floats:
 *  [0..2] base_color  [3] roughness
 *  [4..6] emission    [7] metalness
 *  [8] normal_map_strength [9] sheen [10] sheen_tint [11] anisotropic_strength
 *  [12] tex_albedo [13] tex_normal [14] tex_metal_roughness [15] tex_emission (int bits, -1 none)
 *  [16] kind (int bits)  [17..19] pad
 *  [20..35] the descriptors of the four textures, (offset, width, height, stride) as int bits each, in the order albedo,
 *           normal, metal_roughness, emission: a copy of textures[tex] so that a shade block needs no third dependent
 *           load between the material record and the texels (zeros for an absent texture)
 */

/* Texel layout in the pool: 4 x 4-texel tiles of 64 bytes (one cache line), tiles row-major, `stride` = tiles per row: the
 * 2 x 2 footprint of a bilinear fetch lies in ONE line 9 times in 16 instead of never (two rows of a row-major image are
 * two lines).  Addressing only: same texels. */
typedef struct {
  uint32_t offset;    /* first texel in the pool */
  int32_t  width, height, stride;
} RT_DTexture;
#define RT_TEX_TILE_INDEX(x, y, tpr) ((((y) >> 2) * (tpr) + ((x) >> 2)) * 16 + (((y) & 3) << 2) + ((x) & 3))

/* The background image a second time, as floats (RT_KParams.bg_image; background_lookup_image(), rt_dev.hip.h): row-major,
 * (width + 1) x (height + 1) texels of 16 bytes -- r, g, b as u8 * (1.0f / 255.999f), the product texel_rgb() forms, and a zero.
 * Column `width` repeats column width - 1 and row `height` repeats row height - 1: the clamp-to-edge rule of tex_taps() as data,
 * so the right and lower neighbours of texel (u, v) sit at +1 and +pitch whatever u and v.  A texel's byte offset is kept in 32
 * bits, which bounds the image (rt_scene_upload refuses a larger background). */
#define RT_BG_TEXEL_FLOATS 4
#define RT_BG_IMAGE_MAX_BYTES 0xFFFFFFFFull

/* One view of a multi-view launch: what RT_KParams.cam / focal_length / seed are to a one-view launch.  64 bytes, so that a
 * view's record is one aligned block of scalar loads. */
typedef struct RT_KView {
  float    cam[3][4];          /* rows 0..2 of view_matrix */
  float    focal_length;
  uint32_t seed;
  uint32_t pad[2];
} RT_KView;

typedef struct {
  /* scene */
  const float    *nodes;
  const float    *leaves;
  const float    *tris;
  const float    *mats;
  const RT_DTexture *textures;
  const uint32_t *texels;      /* RGBA8 */
  int32_t depth;               /* bvh.depth                */
  int32_t last_row_offset;     /* bvh.last_row_offset      */
  int32_t bg_texture;          /* index into textures      */
  int32_t n_nodes;
  /* camera: rows 0..2 of view_matrix (rotation | translation), focal length */
  float cam[3][4];
  float focal_length;
  float inv_width, inv_height, aspect;   /* 1/width, 1/height, width/height in fp32 (raytracer.c:615-617) */
  /* frame */
  int32_t width, height, samples, max_bounces;
  int32_t sample_first, sample_end;   /* this launch traces samples [first, end) of every pixel */
  uint32_t seed;
  int32_t chunks_x, n_chunks;
  int32_t rank, world, n_local_chunks;
  int32_t shared_taps;         /* host only, no kernel reads it: 1 = launch the path-kernel instance that computes one set of bilinear
                                * taps per hit -- every material's textures agree in width, height and stride (rt_residency.cpp) */
  int32_t grab_batch;          /* grab_max (below) of the tiles that take the path kernel's batch loop: units per atomic while such a
                                * tile has plenty left (1 .. 16).  In a slot no kernel read: every other field keeps its offset */
  int32_t unused_pad;          /* no kernel reads this (a work item of retired kernels): it keeps the offsets below; zero */
  int32_t sched_thresh;        /* lanes waiting for shade / environment / regeneration that trigger that block */
  int32_t n_lds_nodes;         /* BVH nodes [0, n) are also in the workgroup's LDS   */
  /* outputs */
  unsigned long long *accum;   /* [height*width*3] 32.32 fixed point      */
  unsigned long long *counters;/* RT_N_COUNTERS                           */
  uint32_t *work_head;         /* dequeue counter                         */
  const int32_t *local_chunks; /* global chunk index of this rank's l-th chunk (partition table) */
  const uint32_t *order;       /* tile visiting order (NULL = identity)   */
  uint32_t *tile_cost;         /* rays per tile of THIS launch (NULL = off)*/
  unsigned long long *wave_times; /* RT_WAVE_TIMES (diagnostic library): per wave start, end (100 MHz), last grab | tiles; NULL = off */
  /* a tile hands out units = 2 pixels x (1 << chunk_shift) samples */
  uint32_t *tile_next;         /* [n_tiles] chunks handed out so far (zero at launch)                       */
  uint32_t *open_groups;       /* [ceil(n_tiles / 64)] tiles of the group that still have chunks            */
  int32_t n_tiles;             /* n_local_chunks * 16                                                       */
  int32_t chunk_shift;         /* log2 samples per chunk                                                    */
  int32_t n_chunks_tile;       /* units per tile: 8 rows x n_sample_blocks x 4 pixel pairs                  */
  int32_t n_sample_blocks;     /* ceil(samples of this launch / samples per unit)                           */
  int32_t drain_thresh;        /* lanes waiting for S that trigger it once the wave's tile is exhausted     */
  int32_t grab_max;            /* units a wave takes per atomic while its tile has plenty left (1, 2 or 4)   */
  uint32_t *park;              /* [waves][18][128] dwords, hits parked until a dense shade block (nullptr = off) */
  int32_t short_div;           /* 1: leaf blocks take 1 / det from rcp_exact() (host-checked determinant bound), 0: IEEE division */
  int32_t pyr_nodes;           /* node blocks of camera rays on nodes [0, n) test only the children the tile's pyramid can touch; 0 = off */
  /* wavefront pipeline (rt_wavefront.hip): camera / trace / shade kernels joined by record queues in HBM.  A queue is
   * an array of chunks of WF_CHUNK records, struct-of-arrays inside a chunk ([field][WF_CHUNK] dwords), plus the number
   * of records in every chunk; chunks are handed to producing waves by an atomic counter (wf_ctl). */
  uint32_t *wf_hit0;           /* camera-ray hits: WF_HIT0_FIELDS dwords per record                                     */
  uint32_t *wf_hit;            /* hits of continuation rays: WF_HIT_FIELDS                                              */
  uint32_t *wf_ray[2];         /* continuation rays, written by the shade kernel of bounce b into [b & 1]: WF_RAY_FIELDS */
  uint32_t *wf_cnt_hit0, *wf_cnt_hit, *wf_cnt_ray[2];   /* records per chunk                                            */
  uint32_t *wf_ctl;            /* WF_CTL_* words, WF_CTL_STRIDE dwords apart                                            */
  int32_t wf_soft_chunks;      /* camera kernel: a wave that is handed chunk >= this of wf_hit0 stops taking units      */
  int32_t wf_bounce;           /* shade / trace kernels: bounce index of the records they read                          */
  int32_t wf_n_waves;          /* waves of this launch (the last one to finish resets the control words it consumed)    */
  /* multi-view launches (rt_render_views): K views of one scene share one tile list -- tile t renders view t / tiles_per_view.
   * Appended, so that every field above keeps its kernarg offset (the one-view instances do not read these). */
  const RT_KView *views;       /* [n_views] camera and seed of every view, on the device (NULL: a one-view launch)          */
  int32_t n_views;             /* views of this launch; 0 = one view, the camera / seed above                                */
  int32_t tiles_per_view;      /* n_local_chunks * 16                                                                         */
  int32_t pixels_per_view;     /* width * height: view v accumulates into accum + v * pixels_per_view * 3                    */
  /* the background once more, as floats (RT_BG_IMAGE_* above): what the path kernel's batch loop reads.  Appended likewise. */
  const float *bg_image;       /* bg_pitch x (height + 1) texels of RT_BG_TEXEL_FLOATS floats                                */
  int32_t bg_pitch;            /* texels per row: the background's width + 1                                                  */
  int32_t bg_pad;
} RT_KParams;

/* Batch ray queries (rt_query_kernel, rt_hit_attributes_kernel; include/rt_hip.h rt_query_closest / rt_query_occluded): what one
 * launch reads and writes besides the scene fields of RT_KParams. */
typedef struct {
  const float *rays;           /* [n][6] origin, direction -- taken as given                                              */
  const float *t_max;          /* [n] upper bound of ray i (hit.distance on entry, raytracer.c:452), NULL = infinity      */
  float       *hits;           /* closest hit: [n][4] t, triangle (int bits), u, v                                        */
  uint8_t     *flags;          /* occlusion: [n], 1 = a triangle in [epsilon, t_max)                                      */
  uint32_t    *head;           /* rays handed out so far (zero at launch)                                                 */
  unsigned long long *counters;/* RT_QUERY_COUNTERS: rays, hits, node visits, leaf visits -- added to                     */
  int32_t      n;
  int32_t      grab;           /* rays a wave takes per atomic on `head`                                                  */
  int32_t      exit_lanes;     /* finished lanes that end a traversal call while rays are left to hand out                */
} RT_QParams;
enum { RT_QCNT_RAYS = 0, RT_QCNT_HITS, RT_QCNT_NODES, RT_QCNT_LEAVES, RT_QUERY_COUNTERS };      /* RT_QParams.counters */
#define RT_HIT_DWORDS     22   /* RT_Device_Hit (rt_hip.h), 88 bytes */

/* First-hit feature buffers (rt_features_kernel, rt_features.hip; include/rt_hip.h rt_render_accumulate_features): what one
 * launch reads and writes besides the scene, camera and frame fields of RT_KParams.  A unit = 64 camera paths of one 8x8 tile:
 * (64 >> shift) neighbouring pixels of the tile x (1 << shift) samples, pixel-major; unit u -> tile u / units_per_tile, then
 * pixel group (u % units_per_tile) / n_sample_blocks, sample block u % n_sample_blocks. */
typedef struct {
  unsigned long long *sums;    /* [height][width][RT_FEATURE_CHANNELS] 32.32 fixed point (position: two's complement), added to */
  uint32_t    *head;           /* units handed out so far (zero at launch)                                                */
  int32_t      n_units;
  int32_t      grab;           /* units a wave takes per atomic on `head`                                                 */
  int32_t      tiles_x;        /* ceil(width / 8)                                                                         */
  int32_t      shift;          /* log2 samples per unit, 0 .. 6                                                           */
  int32_t      n_sample_blocks;/* ceil(samples of this launch >> shift)                                                   */
  int32_t      units_per_tile; /* (1 << shift) pixel groups x n_sample_blocks                                             */
} RT_FParams;

/* Light probes (rt_probe_kernel, rt_probes.hip; include/rt_hip.h rt_probe_trace): what one launch reads and writes besides the
 * scene fields of RT_KParams (max_bounces and seed among them).  The work list is the path index j in [0, n_paths): probe
 * j / sample_count of the caller's array, sample sample_first + j % sample_count; record j is the path's. */
typedef struct {
  const float *positions;      /* [n][3] probe positions -- taken as given                                                */
  float       *records;        /* RT_Probe_Sample[n_paths]: radiance, t, direction, 0 -- two float4 per path              */
  uint32_t    *head;           /* paths handed out so far (zero at launch)                                                */
  unsigned long long *counters;/* RT_Counters layout (RT_CNT_PATHS .. RT_CNT_TEXTURED) -- added to                        */
  int32_t      n_paths;        /* n * sample_count, at most 2^30                                                          */
  int32_t      sample_count, sample_first;
  uint32_t     probe_first;    /* global index of probe 0: the seed rule's pixel index is probe_first + probe             */
  int32_t      grab;           /* paths a wave takes per atomic on `head`                                                 */
  int32_t      exit_lanes;     /* finished lanes that end a traversal call while paths are left to hand out               */
} RT_PParams;
#define RT_PROBE_RECORD_F4 2   /* float4 per RT_Probe_Sample */
#define RT_PROBE_SUMS      27  /* u64 per probe: 9 coefficients x rgb, k-major */

/* HDR lightmaps (rt_lightmap_kernel, rt_lightmap.hip; include/rt_hip.h rt_lightmap_trace): what one launch reads and adds to
 * besides the scene fields of RT_KParams (max_bounces and seed among them).  The work list is SAMPLE-MAJOR: path idx in
 * [0, n_paths) is sample sample_first + idx / m of list entry texel_first + idx % m, so that neighbouring lanes hold
 * neighbouring texels of one sample index. */
typedef struct {
  const float *texels;         /* RT_Lightmap_Texel[]: origin, texel index, normal, triangle -- two float4 per entry      */
  unsigned long long *sums;    /* u64[entries][3], 32.32 -- added to with atomics                                         */
  uint32_t    *head;           /* paths handed out so far (zero at launch)                                                */
  unsigned long long *counters;/* RT_Counters layout (RT_CNT_PATHS .. RT_CNT_TEXTURED) -- added to                        */
  int32_t      n_paths;        /* m * sample_count, at most 2^30                                                          */
  int32_t      m, texel_first; /* the list range of this launch                                                           */
  int32_t      sample_first;
  int32_t      grab;           /* paths a wave takes per atomic on `head`                                                 */
  int32_t      exit_lanes;     /* finished lanes that end a traversal call while paths are left to hand out               */
} RT_LParams;
#define RT_LIGHTMAP_TEXEL_F4 2 /* float4 per RT_Lightmap_Texel */
#define RT_LIGHTMAP_TRIES   64 /* directions tried per sample before the path is given up (raytracer.c:768-772)           */

/* Temporal accumulation (rt_temporal_kernel, rt_temporal.hip; include/rt_hip.h rt_temporal_accumulate): a camera as proj() of the
 * contract reads it, and what the host computes once per launch. */
typedef struct {
  float r[3][3];               /* view_matrix rows[i][0..2]: camera space -> world space, taken as orthonormal             */
  float t[3];                  /* rows[i][3]                                                                               */
  float focal_length;
} RT_TCamera;
typedef struct {
  RT_TCamera cur, prev;        /* the frame's camera, the camera of the history                                            */
  int32_t width, height;
  float   half_w, half_h;      /* (float)w * 0.5f, (float)h * 0.5f                                                         */
  float   aspect;              /* (float)w / (float)h                                                                      */
  float   tn2, tp2;            /* normal_tolerance^2, plane_tolerance^2                                                    */
  float   alpha;
  float   max_history;         /* (float)max_history: at most 2^20, exact                                                  */
  int32_t demodulate;
  int32_t tiles_x;             /* ceil(width / 32): block b is tile (b % tiles_x, b / tiles_x) of 32 x 8 pixels            */
} RT_TParams;

/* A frame on the device, as the post passes read it (rt_guided.hip, rt_temporal.hip, rt_variance.hip and the host side of them,
 * rt_post.cpp): the linear colour f32[h][w][3] and the four first-hit planes of rt_features.hip, coverage f32[h][w], the others
 * f32[h][w][3].  albedo may be NULL where `demodulate` is 0: nothing reads it then. */
typedef struct {
  const float *color, *coverage, *albedo, *normal, *position;
} RT_Frame;

#define WF_CHUNK        256
#define WF_HIT0_FIELDS  9      /* direction (3), t, triangle, u, v, pixel (y << 16 | x), sample                         */
#define WF_HIT_FIELDS   5      /* index of the ray record (chunk * WF_CHUNK + slot), t, triangle, u, v                  */
#define WF_RAY_FIELDS   15     /* origin (3), direction (3), tint (3), emission (3), rng, pixel (y << 16 | x), bounce   */
#define WF_CTL_STRIDE   16     /* one control word per 64-byte line                                                     */
enum {
  WF_HIT0_ALLOC = 0, WF_HIT0_HEAD, WF_HIT_ALLOC, WF_HIT_HEAD, WF_RAY0_ALLOC, WF_RAY0_HEAD, WF_RAY1_ALLOC, WF_RAY1_HEAD,
  WF_STOPPED,      /* set by a camera-kernel wave that ran into wf_soft_chunks: units are left, another pass is needed */
  WF_DONE_WAVES,   /* waves of the running kernel that have finished                                                   */
  WF_N_CTL
};

#endif /* RT_DEVICE_H */
