/* rt_hip.h -- C-ABI of the MI355X render layer beyond the reference's own
 * entry points (rt_raytracer.h).  Plain pointers and sizes only.
 *
 * The reference has no device layer; these calls are what its driver would use
 * to control one (seed, device choice, error text, explicit scene residency)
 * and what a multi-process launcher needs to render a subset of the 32x32
 * chunks of raytracer.c:601-627 on each GPU.  INTEGRATION.md shows the
 * reference-side stubs.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include "rt_raytracer.h"
#include "rt_materials.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the most recent failure in this process ("" when none).  The render
 * entry points are void in the reference (raytracer.h:51-56), so errors are
 * reported here and on stderr. */
extern char const *rt_last_error(void);
extern void        rt_clear_error(void);

/* Selects the HIP device for this process (default 0) and reads the library's configuration -- the environment
 * variables RT_DEVICES / RT_DEVICES_REHEARSE below, nothing else -- once.  0 on success. */
extern int rt_init(int device);

/* A frame behind render_thread_proc() / render() / rt_render_frame() is spread over the first `n_devices` GPUs of the
 * node (primary device, then the following ones): every GPU renders the chunks rt_chunk_owner() gives its rank from its
 * own copy of the scene, the compact u8 tiles go to the primary GPU with one peer copy per device, which untiles and
 * fills the caller's pixels (driver.c:793-818 needs no change: its `-T n` threads enter as before, one of them drives
 * all GPUs).  Default 1, or the environment variable RT_DEVICES read by rt_init().  `rehearse` != 0 (RT_DEVICES_REHEARSE=1)
 * maps all n logical devices onto the primary GPU -- the N-device code path on a one-GPU machine, for tests.
 * rt_device_count() = how many GPUs the next frame will use (min(n_devices, GPUs present)). */
extern int rt_set_devices(i32 n_devices, i32 rehearse);
extern i32 rt_device_count(void);


/* Frame seed of the per-path RNG rule rt_path_seed() (rt_math.h); replaces
 * `random_state = time_now()` of raytracer.c:597.  Default 0x1234ABCD. */
extern void rt_set_seed(u32 seed);
extern u32  rt_get_seed(void);

/* ---- scene residency ------------------------------------------------------- */

typedef struct RT_Device_Scene RT_Device_Scene;

/* Flattens a host Scene into HBM: BVH nodes, per-leaf SoA tiles, trimmed AoS
 * records with material ids, the material table, and every Image referenced by
 * a material or by the background (RGB8/RGBA8 -> RGBA8).  Fails (NULL +
 * rt_last_error) on a shader/background proc that is not one of the exported
 * tokens of rt_materials.h.  render_thread_proc() calls this itself and caches
 * the result per Scene*; rt_scene_invalidate() drops that cache entry after the
 * host Scene was modified. */
extern RT_Device_Scene *rt_scene_upload(Scene const *scene);
extern void             rt_scene_release(RT_Device_Scene *dscene);
extern void             rt_scene_invalidate(Scene const *scene);
/* The reference reads the live Scene every frame (raytracer.c:596-612); a frame here renders from the cached device copy.
 * What keeps the two equal, per frame behind render_thread_proc() / render() / rt_render_frame():
 *  1. BEFORE the frame is enqueued (tens of microseconds): dimensions and base pointers of the host Scene, its material
 *     records and the descriptors of their Images in full, a bounded sample of every block of geometry and texel bytes;
 *  2. WHILE the GPU renders, on the calling thread: every byte of the BVH, the coordinate arrays, the AoS records and the
 *     materials, the texels of images above 64 KB one word in 61.  If that differs from what was uploaded, the frame is
 *     discarded, the scene uploaded again and the frame rendered again: an in-place edit of vertices, boxes or materials is
 *     seen by the next frame like in the reference.  A frame of an unchanged scene waits for max(kernel, check), not for
 *     their sum (RT_Frame_Timing.verify_ms; helmet: ~0.5 ms of host time behind a kernel of 0.6 ms or more).
 *     rt_scene_set_static(scene, 1) switches (2) off for a host that never edits in place (or tells: rt_scene_touch).
 *  3. rt_scene_touch(scene, begin, bytes): "I wrote these bytes" -- nodes, coordinates, AoS records, a material record or
 *     texels of a texture / the background.  The block they belong to is patched on every device (a few texture rows, a few
 *     leaf tiles) instead of the whole scene being uploaded again, and the stamps are refreshed: also the way to get a
 *     single-texel edit seen that the 1-in-61 sampling of (2) can miss.  Returns 0 = patched in place, 1 = not a patchable
 *     range (the copies were dropped, the next frame uploads), -1 = error.
 *     A copy is patched only if the blocks that differ from what it was made from are the one(s) the range lies in; a block that
 *     changed without a word drops the copy instead (1) -- the unreported edit is not absorbed into the new reference.
 * Every device keeps the fingerprint of ITS OWN copy: a frame over N devices is checked device by device, so a copy that one
 * device made before an edit cannot pass because another device has been brought up to date since.
 * rt_scene_invalidate() drops the cached copies on every device (and a rt_scene_set_static() opt-out: a Scene rebuilt at the same
 * address starts checked); rt_scene_verify() is the comparison of (2) on demand, for every device: 1 = every cached copy still
 * matches the host scene, 0 = one did not (the stale ones are dropped; the next frame uploads), -1 = nothing cached on the
 * primary device for this Scene. */
extern int              rt_scene_verify(Scene const *scene);
extern int              rt_scene_touch(Scene const *scene, void const *begin, size_t bytes);
extern void             rt_scene_set_static(Scene const *scene, i32 is_static);
extern i64              rt_scene_device_bytes(RT_Device_Scene const *dscene);

/* Camera used by rt_render_accumulate() for an explicitly uploaded scene;
 * rt_scene_upload() captures scene->camera, this replaces it. */
extern int rt_set_camera(RT_Device_Scene *dscene, Camera const *camera);

/* scene_init() (rt_scene.h, reference scene.c:416-426) with the build done by GPU kernels: fills `scene` with the SAME
 * bytes scene_init() would -- same triangles in the same slots, same child boxes (the cut positions of the reference's
 * split depend on counts only, so the host plans them and the GPU runs the sorts, bounds and inserts level by level;
 * csrc/rt_build.hip).  Host memory comes from `allocator` as in scene_init.  0 on success. */
extern int scene_init_gpu(Scene *scene, Triangle_Slice src_triangles, Allocator allocator);

/* scene_refit() (rt_scene.h) by GPU kernels, on the primary device's cached copy of `scene`, which is updated IN PLACE
 * (csrc/rt_refit.hip): same contract, same validation -- on the host, before anything is launched -- and the same bytes
 * in the host Scene afterwards, which stays the truth for the per-frame check.  One lane per slot writes the slot's
 * record, shading record and leaf-tile column and the wave writes the node above its eight leaf groups; the levels above
 * follow in at most `depth` more launches.  The nodes and the triangle block are copied back into the host Scene (the
 * textures and materials never move), the copy's edge bound is recomputed exactly and its stamps are refreshed: the next
 * frame, query, feature pass or lightmap uploads nothing and renders the moved geometry.  Without a cached copy one is
 * made first by the ordinary upload.  Copies on other device slots are dropped; those devices upload on their next frame.
 * A `src` with a NaN position is refitted by scene_refit itself (the copies are dropped, 0 is returned).  So is a scene whose
 * materials, texels or background were edited in place since the copy was made without rt_scene_touch: the refit takes the host
 * bytes as the copy's new reference, and must not absorb an edit nobody reported -- the next frame uploads the scene as it is.
 * Like rt_scene_touch, not to be called between rt_frame_begin and rt_frame_end of a frame on this scene: the device is
 * synchronised before the kernels write the copy, but a frame begun on the old geometry is checked against the host
 * Scene when it ends.  0 on success, -1 with rt_last_error() otherwise (nothing written after a failed validation). */
extern int scene_refit_gpu(Scene *scene, Triangle_Slice src_triangles, i32 const *slot_of_source);

/* KEPT GEOMETRY: a snapshot of the device copy's leaf tiles -- per leaf group 72 f32, 9 rows x 8: a, b - a, c - a of its eight
 * slots -- what THE MOTION of a later feature pass is measured against ("first-hit feature buffers" below).  The refit keeps every
 * triangle in its slot, so the snapshot and the refitted tiles name the same triangle by the same (group, column).  The snapshot
 * is made by ONE device-to-device copy, replaces an earlier one, and belongs to the device copy: whatever drops the copy --
 * rt_scene_invalidate, a re-upload after an edit, rt_scene_free, a scene_refit_gpu that falls back to scene_refit, a device
 * slot torn down -- drops it too, and rt_scene_has_kept_geometry() says 0 again.  scene_refit_gpu, scene_refit and
 * rt_scene_touch are what they were.  The host loop of an animation:
 *     render frame k - 1  ->  rt_scene_keep_geometry  ->  scene_refit_gpu (any number of times)  ->  render frame k
 * rt_device_scene_keep_geometry(): an explicitly uploaded scene, only enqueues the copy on `stream`.  rt_scene_keep_geometry():
 * the primary device's cached copy of `scene` (made by the ordinary upload when there is none), under the device lock, on the
 * NULL stream.  rt_scene_has_kept_geometry(): 1 / 0 for the primary device's cached copy; touches no device.  0 on success,
 * -1 + rt_last_error(). */
extern int rt_device_scene_keep_geometry(RT_Device_Scene *dscene, void *stream);
extern int rt_scene_keep_geometry(Scene const *scene);
extern int rt_scene_has_kept_geometry(Scene const *scene);

/* ---- rendering -------------------------------------------------------------- */

typedef struct {
  u64 paths;        /* camera paths started                               */
  u64 rays;         /* ray_scene_hit equivalents (raytracer.c:514)        */
  u64 node_visits;  /* 8-box slab tests (raytracer.c:452)                 */
  u64 leaf_visits;  /* 8-triangle tests (raytracer.c:476)                 */
  u64 shades;       /* material evaluations (raytracer.c:535)             */
  u64 backgrounds;  /* environment lookups (raytracer.c:554)              */
  u64 textured;     /* shades on a material with at least one texture     */
} RT_Counters;

typedef struct {
  i32 width, height;     /* image size                                          */
  i32 samples;           /* samples per pixel (Rendering_Context.samples)       */
  i32 max_bounces;       /* Rendering_Context.max_bounces                       */
  u32 seed;              /* frame seed                                          */
  i32 rank, world;       /* this process renders the chunks rt_chunk_owner() gives `rank` */
  i32 slab;              /* samples per work item (0 = library default)         */
  i32 flags;             /* RT_FLAG_*                                           */
  i32 sample_first;      /* this call traces samples [sample_first,             */
  i32 sample_count;      /*   sample_first + sample_count) of every pixel; 0 = all.
                            `samples` stays the pixel's total: the accumulation
                            buffer can be filled by several calls (progressive)
                            and resolved once                                   */
} RT_Render_Params;

enum {
  RT_FLAG_NONE = 0,
};

/* Image partition across the GPUs of a node.  The frame is cut into the reference's 32x32 chunks
 * (raytracer.c:601-610; chunk c = cx + cy * ceil(width / 32)); chunk (cx, cy) belongs to rank
 * (cx + B * cy) mod world, B = the integer coprime to `world` nearest to 0.618 * world, so that every
 * chunk column and row is spread over all ranks.  A rank numbers its chunks in ascending global order.
 * Pure host arithmetic (no GPU needed):
 *   rt_chunk_count           chunks of the image
 *   rt_chunk_owner           rank that owns `chunk`, -1 if out of range
 *   rt_local_chunk_count     chunks `rank` owns
 *   rt_max_local_chunk_count the largest of those over all ranks (= slots per rank in the gathered tile buffer)
 *   rt_local_chunk_list      writes up to `capacity` of rank's chunk indices to out, returns the count */
extern i32 rt_chunk_count(i32 width, i32 height);
extern i32 rt_chunk_owner(i32 width, i32 height, i32 world, i32 chunk);
extern i32 rt_local_chunk_count(i32 width, i32 height, i32 rank, i32 world);
extern i32 rt_max_local_chunk_count(i32 width, i32 height, i32 world);
extern i32 rt_local_chunk_list(i32 width, i32 height, i32 rank, i32 world, i32 *out, i32 capacity);

/* Renders this rank's chunks.  All pointers are DEVICE pointers owned by the
 * caller, `stream` is a hipStream_t (NULL = default stream); the call only
 * enqueues work.
 *   d_accum  : u64[height*width*3] fixed-point radiance sums (rt_math.h), must
 *              be zero on entry for the chunks this rank owns
 * 0 on success. */
extern int rt_render_accumulate(RT_Device_Scene *dscene, RT_Render_Params const *params,
                                void *d_accum, void *stream);

/* accum -> mean radiance -> clamp -> sRGB -> u8 (raytracer.c:700-716) for this
 * rank's chunks.
 *   d_tiles  : u8[n_local_chunks*32*32*3], chunk-major compact tiles, or NULL
 *   d_image  : u8[height*width*3] row-major image, or NULL
 *   d_linear : f32[height*width*3] mean radiance before clamp, or NULL */
extern int rt_resolve(RT_Render_Params const *params, void const *d_accum,
                      void *d_tiles, void *d_image, void *d_linear, void *stream);

/* Scatters gathered compact tiles of ALL ranks (rank-major:
 * [world][rt_max_local_chunk_count()][32*32*3]) into a row-major u8 image on the device. */
extern int rt_untile(i32 width, i32 height, i32 world, void const *d_all_tiles,
                     void *d_image, void *stream);

/* denoise_image() (rt_raytracer.h) on DEVICE buffers: u8[height*width*3] row-major -> same layout. */
extern int rt_denoise(i32 width, i32 height, void const *d_src, void *d_dst, void *stream);

/* Whole frame from host memory to host memory on one GPU: upload/cached scene,
 * accumulate, resolve, copy back.  pixels: u8[height*stride*components] as the
 * reference lays out Image; linear (optional): f32[height*width*3];
 * accum (optional): u64[height*width*3].  0 on success. */
extern int rt_render_frame(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                           f32 *linear, u64 *accum);

/* Frames in flight.  A launch of the path kernel ends with 0.6 - 1.0 ms of thinning bounce chains whatever its size
 * (27 % of the reference driver's default frame, driver.c:733-742); a blocking render_thread_proc() / render() has nothing to
 * fill that with, a host that has a NEXT frame does: rt_frame_begin() enqueues the frame -- scene check, accumulator clear,
 * path kernel, resolve, on one of two internal lanes with a stream, buffers and launch state of its own -- and returns a
 * ticket (>= 0; -1 + rt_last_error() on failure, also when two frames are in flight already); rt_frame_end(ticket) waits
 * for that frame and fills the pixels of the Image given at begin (the header is copied at begin, the pixels must stay valid
 * until end).  begin(A), begin(B), end(A), begin(C), end(B) ... keeps two frames on the GPU: the second one's workgroups take
 * the CUs as the first one's leave them.  Same pixels as render() / rt_render_frame(), bit for bit (per-path seeds, order-free
 * sums); seed and camera are read at begin; rt_get_counters() / rt_get_frame_timing() after an end describe THAT frame.
 * The per-frame scene check is the blocking path's: the sampled stamp at begin, the full content check inside rt_frame_end()
 * while the GPU renders -- a host scene that no longer equals the copy the frame was rendered from is rendered again there,
 * synchronously.  Do not edit (or rt_scene_touch) a scene between the begin and the end of a frame that renders it.
 * rt_frame_end() waits WITHOUT the library's device lock: two host threads can each keep a frame in flight (a ticket is ended
 * by one thread, once).
 * With rt_set_devices(n > 1) the frame is rendered inside rt_frame_begin() over the n devices (that pipeline has its own
 * overlap) and rt_frame_end() returns its status. */
extern int rt_frame_begin(Scene const *scene, Image const *image, isize samples, isize max_bounces);
extern int rt_frame_end(int ticket);

/* Several views of ONE scene in ONE launch of the path kernel.  A launch ends 0.6 - 1.0 ms after its last unit of work was
 * handed out (see rt_frame_begin); K views rendered as K frames pay that K times, a batch pays it once: the tiles of all views
 * go into one work queue.  Use it for the faces of a cube map or light probe, a stereo pair, a turntable, a camera sweep.
 *   views[v]  : the camera of view v (view_matrix, fov, focal_length, exactly as Scene.camera) and its frame seed -- what
 *               rt_set_seed() is to rt_render_frame()
 *   images[v] : receives view v; every image has the same width and height (stride and pixels per image; pixels.data may be
 *               NULL as in rt_render_frame)
 *   linear    : optional f32[n_views][height][width][3];  accum: optional u64[n_views][height][width][3]
 * Every view gets the same pixels, linear values and radiance sums as rt_render_frame() with scene->camera = views[v].camera
 * and rt_set_seed(views[v].seed), bit for bit; the scene check is rt_render_frame()'s.  rt_get_counters(),
 * rt_get_skipped_root_visits(), rt_get_frame_timing() and the kernel timing describe the whole batch afterwards.  One device
 * only: with rt_device_count() > 1 the call fails.  Arguments are checked before the GPU is touched: n_views > 0, equal image
 * sizes, >= 3 components and stride >= width per image, n_views x width x height <= 2^28 pixels and n_views x 16 tiles per
 * 32x32 chunk < 2^31.  0 on success, -1 + rt_last_error(). */
typedef struct {
  Camera camera;
  u32    seed;
} RT_View;
extern int rt_render_views(Scene const *scene, i32 n_views, RT_View const *views, Image const *images, isize samples,
                           isize max_bounces, f32 *linear, u64 *accum);
/* The device-level form, like rt_render_accumulate(): d_accum = u64[n_views][height][width][3] on the device, zero for this
 * rank's chunks on entry; params->seed is ignored (every view has its own); rank / world and sample_first / sample_count are
 * honoured, so a batch can be filled progressively and view v resolved with rt_resolve(params, d_accum + v * height * width * 3,
 * ...).  Only enqueues work on `stream`, on the device the scene was uploaded to. */
extern int rt_render_accumulate_views(RT_Device_Scene *dscene, RT_Render_Params const *params, i32 n_views,
                                      RT_View const *views, void *d_accum, void *stream);

/* ---- batch ray queries ------------------------------------------------------------ */

/* ray_scene_hit (reference raytracer.c:443-503) for a batch of rays against a resident scene: which triangle a ray hits, where,
 * with what normal and texture coordinates -- picking, line of sight, visibility, a host's own ambient-occlusion or probe pass,
 * collision rays, sensor simulation.  Ray i is (origin, direction) = f32[6], taken AS GIVEN: not normalised, zero components, +-0,
 * infinities and NaN give whatever the reference's arithmetic gives.  Its query is ray_scene_hit(&ray[i], scene, &hit) with
 * hit.distance = t_max[i] on entry: the reference's own protocol makes the entry distance the upper bound (raytracer.c:452, :159,
 * :513), the lower bound is its EPSILON; t_max == NULL means F32_INFINITY for every ray.
 *   closest hit : RT_Ray_Hit per ray; on a miss triangle = -1, t = the entry t_max[i], u = v = 0
 *   occlusion   : one byte per ray, 1 exactly when the closest-hit query with the same t_max finds a triangle (the kernel stops a
 *                 ray at the first triangle it accepts: fewer visits, same answer)
 *   full record : RT_Device_Hit = the reference's Hit (raytracer.c:159-184) with the Shader pair replaced by the triangle and
 *                 material indices; on a miss distance = the entry t_max[i], triangle = material = -1, every other field 0
 * One persistent kernel of its own (rt_query_kernel, csrc/rt_kernels.hip) on the traversal of the path kernel; every result equals
 * the reference's bit for bit.  Frames, views, lightmaps and their counters are not affected by queries. */
typedef struct { f32 t; i32 triangle; f32 u, v; } RT_Ray_Hit;                                     /* 16 bytes */
typedef struct {
  f32  distance;
  Vec3 normal, normal_geo, point, tangent, bitangent;
  Vec2 tex_coords;                                                                                /* as in Hit up to here */
  i32  triangle, material;                                                                        /* index into scene->triangles.aos, device material id */
  i32  pad[2];
} RT_Device_Hit;                                                                                  /* 88 bytes = sizeof(Hit) */
typedef struct { u64 rays, hits, node_visits, leaf_visits; } RT_Query_Counters;

/* Device level, like rt_render_accumulate(): every pointer is a DEVICE pointer owned by the caller, on the device the scene was
 * uploaded to; the call only enqueues work on `stream` (NULL = default stream).
 *   d_rays  : f32[n][6]            d_t_max : f32[n] or NULL
 *   d_hits  : RT_Ray_Hit[n]        d_full  : RT_Device_Hit[n] or NULL        d_flags : u8[n]
 * d_rays and d_t_max must be 4-byte aligned, d_hits 16-byte (one 16-byte store per ray), d_full 8-byte (eleven 8-byte stores).
 * Checked before the GPU is touched: dscene, d_rays, d_hits / d_flags not NULL, 0 < n <= 2^30 (RT_QUERY_MAX_RAYS: the kernel holds
 * ray indices in 32-bit integers, and its 32-bit work counter ends at n plus one grab of at most 512 rays per wave; byte offsets
 * are 64-bit).
 * 0 on success, -1 + rt_last_error(). */
#define RT_QUERY_MAX_RAYS ((i64)1 << 30)
extern int rt_query_closest(RT_Device_Scene *dscene, i64 n, void const *d_rays, void const *d_t_max, void *d_hits, void *d_full,
                            void *stream);
extern int rt_query_occluded(RT_Device_Scene *dscene, i64 n, void const *d_rays, void const *d_t_max, void *d_flags, void *stream);

/* Host level: batch ray_scene_hit with the reference's in / out protocol, from host memory to host memory.
 *   rt_scene_hits     : hits[i].distance on entry is ray i's bound.  A hit fills the whole Hit (shader copied on the host from
 *                       scene->triangles.aos[triangle].shader) and sets triangles[i] (optional) to the triangle's index; a miss leaves
 *                       hits[i] untouched and sets triangles[i] = -1.
 *   rt_scene_closest  : hits[i] = (t, triangle, u, v) of ray i under the bound t_max[i] (t_max NULL: infinity), as rt_query_closest
 *                       writes them: 16 bytes per ray, no attribute kernel, no full records -- the cheap form when the
 *                       barycentrics or the triangle are all the host needs (the reference's Hit has no place for u, v).
 *   rt_scene_occluded : flags[i] = 1 when ray i hits anything in [EPSILON, t_max[i]) (t_max NULL: infinity), else 0.
 * All three use the cached device copy of `scene` and the per-call scene check of rt_render_frame() -- the stamp before the launch, the
 * full content check while the GPU works (off after rt_scene_set_static) -- so an in-place edit or an rt_scene_touch() is seen by the
 * next query; they take the library's device lock as frames do and block until the results are in host memory.  n is processed in
 * slices of 2^20 rays (RT_QUERY_SLICE), which bounds the staging memory on the device (133 bytes per ray of a slice at most) and on
 * the host (88); the device staging is kept for the next call.  With rt_device_count() > 1 they run on the PRIMARY device only; spreading a batch over devices is not done.
 * Checked before the GPU is touched: scene, rays, hits / flags not NULL, 0 < n <= 2^30.  0 on success, -1 + rt_last_error(); a
 * call refused for its arguments or for want of a device leaves hits / triangles / flags untouched. */
#define RT_QUERY_SLICE ((i64)1 << 20)
extern int rt_scene_hits(Scene const *scene, i64 n, Ray const *rays, Hit *hits, i32 *triangles);
extern int rt_scene_closest(Scene const *scene, i64 n, Ray const *rays, f32 const *t_max, RT_Ray_Hit *hits);
extern int rt_scene_occluded(Scene const *scene, i64 n, Ray const *rays, f32 const *t_max, u8 *flags);

/* Counters of the last query call of this process (device or host level; a host call's slices summed): rays answered, rays with
 * a hit, 8-box slab tests (raytracer.c:452) and 8-triangle tests (:476).  Synchronises.  rt_get_counters() is not affected. */
extern int rt_get_query_counters(RT_Query_Counters *out);

/* ---- first-hit feature buffers ----------------------------------------------------- */

/* What the camera sees at the first surface, per pixel: coverage, albedo, shading normal and world position -- the inputs of a
 * feature-guided denoiser, a matte, an edge-aware upscaler, outlines, debug views.  For pixel (x, y) and sample s the ray is the
 * frame's own primary ray (raytracer.c:641-694) and the loop is cast_ray's (raytracer.c:505-558) for at most max_bounces
 * iterations: a hit whose geometric or shading normal faces along the ray is passed through and uses up an iteration; the first
 * hit the reference would hand to a shader is the FEATURE HIT.  A miss or an exhausted loop leaves every channel of the sample 0.
 *   coverage : 1
 *   albedo   : PBR_Shader_Data.base_color, times the decoded texture_albedo sample when there is one (driver.c:364-368), for
 *              disney and debug materials alike
 *   normal   : debug_shader_proc's emission (driver.c:411-418): the normal-mapped normal * 0.5 + 0.5
 *   position : Shader_Input.position (world space, signed)
 * A pixel's value is the mean over its `samples` samples, accumulated order-free in 32.32 fixed point like the frame
 * (rt_math.h: rt_accum_quantize / rt_accum_resolve; position rt_accum_quantize_signed / rt_accum_resolve_signed): coverage,
 * albedo and normal are the frame the reference would render if every shader emitted the feature and terminated, under a black
 * background.  The seed is not read (the jitter is a hash of pixel and sample).  One kernel of its own (rt_features_kernel,
 * csrc/rt_features.hip) on the traversal of the path kernel; frames, views, queries and their counters are not affected. */
#define RT_FEATURE_CHANNELS 10   /* coverage, albedo rgb, normal xyz, position xyz -- in this order */
typedef struct { f32 *coverage, *albedo, *normal, *position; } RT_Features;   /* f32[h][w] / f32[h][w][3]; NULL = not wanted */

/* Device level, like rt_render_accumulate(): d_sums = u64[height][width][RT_FEATURE_CHANNELS] on the device the scene was
 * uploaded to, zero on entry; the camera is rt_set_camera()'s (rt_scene_upload() captures scene->camera); only enqueues work on
 * `stream`.  params->sample_first / sample_count are honoured (a buffer can be filled progressively and resolved once), seed is
 * not read, rank / world other than 0 / 1 are refused.  rt_resolve_features(): sums -> means, planar f32 on the device, NULL =
 * not wanted (at least one is).  0 on success, -1 + rt_last_error(). */
extern int rt_render_accumulate_features(RT_Device_Scene *dscene, RT_Render_Params const *params, void *d_sums, void *stream);
extern int rt_resolve_features(RT_Render_Params const *params, void const *d_sums,
                               void *d_coverage, void *d_albedo, void *d_normal, void *d_position, void *stream);
/* Host level: the cached device copy of `scene` with rt_render_frame()'s scene check and device lock, camera = scene->camera;
 * out (optional) names the planes wanted, sums (optional) = u64[height][width][RT_FEATURE_CHANNELS].  One device only: with
 * rt_device_count() > 1 the call fails.  Checked before the GPU is touched: scene not NULL, width, height, samples > 0,
 * max_bounces >= 0, width x height <= 2^28, at least one plane of `out` or `sums` given.  A refused call leaves the outputs
 * untouched.  Runs on the NULL stream like rt_render_frame(): it overlaps a frame in flight (rt_frame_begin). */
extern int rt_render_features(Scene const *scene, i32 width, i32 height, isize samples, isize max_bounces,
                              RT_Features const *out, u64 *sums);

/* THE MOTION: for a deforming mesh, where the surface point of a feature hit WAS minus where it is -- three more sums per pixel,
 * in a buffer of their own, u64[h][w][RT_MOTION_CHANNELS]; RT_FEATURE_CHANNELS and the ten-channel layout stay.  At a FEATURE HIT
 * with triangle slot tri and barycentrics (u, v) -- the (t1, t2) the leaf test accepted --: g = tri >> 3, k = tri & 7, l = the
 * current leaf tile of group g (72 f32: 9 rows x 8, rows a.x, (b - a).x, (c - a).x, a.y, ... as uploaded or refitted), l' = the
 * KEPT tile of group g ("scene residency" above).  For axis r = 0, 1, 2:
 *     cur_r    = (l [(3r) * 8 + k] + u * l [(3r + 1) * 8 + k]) + v * l [(3r + 2) * 8 + k]
 *     was_r    = (l'[(3r) * 8 + k] + u * l'[(3r + 1) * 8 + k]) + v * l'[(3r + 2) * 8 + k]
 *     motion_r = was_r - cur_r
 * Plain f32 + - *, every operation rounded on its own, left to right as written, no fused multiply-add (the units are built with
 * -ffp-contract=off): the same bits under all three numeric contracts.  The motion is a difference of two barycentric evaluations,
 * NOT was - Shader_Input.position: a triangle whose kept column equals its current column has motion +0 bit for bit.  A miss or
 * an exhausted loop adds nothing; a back face that is passed through adds nothing for that hit.  Sums: rt_accum_quantize_signed,
 * 32.32, order-free, one atomic per non-zero channel and pixel group, like position.  Without kept geometry the current tiles
 * serve as the kept ones and every motion sum is 0: the first frame of a sequence.
 * rt_render_accumulate_features_motion(): rt_render_accumulate_features() -- its checks, locking, sample_first / sample_count --
 * by ONE launch of a second kernel on the same loop (rt_features_motion_kernel); d_motion_sums is required and zero on entry; the
 * ten sums it writes into d_sums equal rt_render_accumulate_features()'s bit for bit.  rt_resolve_motion(): sums -> means over
 * params->samples (rt_accum_resolve_signed), d_motion f32[h][w][3]; like position it is the sum over the samples that hit divided
 * by ALL samples: motion / coverage is the mean motion of the first hits.  rt_render_features_motion(): rt_render_features() with
 * two more optional outputs, motion f32[h][w][3] and motion_sums u64[h][w][3], against the kept geometry of the scene's cached
 * copy; at least one of the four outputs. */
#define RT_MOTION_CHANNELS 3
extern int rt_render_accumulate_features_motion(RT_Device_Scene *dscene, RT_Render_Params const *params, void *d_sums,
                                                void *d_motion_sums, void *stream);
extern int rt_resolve_motion(RT_Render_Params const *params, void const *d_motion_sums, void *d_motion, void *stream);
extern int rt_render_features_motion(Scene const *scene, i32 width, i32 height, isize samples, isize max_bounces,
                                     RT_Features const *out, u64 *sums, f32 *motion, u64 *motion_sums);

/* ---- light probes ---------------------------------------------------------------------- */

/* The incoming light at points in space: what lights everything that is not baked into a lightmap -- moving objects, particles,
 * volumetrics, characters sample a probe grid laid through the level.  For probe i of the caller's array, global index
 * g = probe_first + i, position o_i, and sample s of `samples`:
 *     state = rt_path_seed(seed, (u32)g, (u32)s)
 *     d     = rt_rand_unit_vec3(&state)                      rt_math.h; common.h:30-42: uniform on the sphere by rejection,
 *                                                            RT_EPS < |p|^2 <= 1, then p * (1 / rt_sqrtf(|p|^2))
 *     L     = cast_ray(Ray{o_i, d}, max_bounces, &state)     raytracer.c:505-558 unchanged, the RNG stream going on where the
 *                                                            direction left it: back faces pass through at the price of an
 *                                                            iteration, the background is looked up on a miss, exhaustion
 *                                                            returns the emission
 *     t     = the distance of the FIRST segment's closest hit (ray_scene_hit with entry distance F32_INFINITY): +inf on a miss
 *             and when max_bounces <= 0 (no ray is cast; L = 0)
 * The position is taken AS GIVEN: a NaN or infinite coordinate gives whatever the reference's arithmetic gives.
 *
 * THE RECORD of a sample, 32 bytes, written with two 16-byte stores: */
typedef struct { f32 radiance[3]; f32 t; f32 direction[3]; u32 pad; /* 0 */ } RT_Probe_Sample;
/* THE PROJECTION onto the nine real spherical harmonics of bands 0-2, d = (x, y, z) -- rt_sh9_basis() of rt_math.h: plain f32
 * * + -, every operation rounded on its own, left to right as written, no fused multiply-add (the units are built with
 * -ffp-contract=off, like THE MOTION): the same bits under all three numeric contracts.
 *     Y0 = 0.282095f
 *     Y1 = 0.488603f*y        Y2 = 0.488603f*z        Y3 = 0.488603f*x
 *     Y4 = 1.092548f*(x*y)    Y5 = 1.092548f*(y*z)    Y7 = 1.092548f*(x*z)
 *     Y6 = 0.315392f*((3.0f*(z*z)) - 1.0f)
 *     Y8 = 0.546274f*((x*x) - (y*y))
 * THE SUMS: sums[i][k][c] += rt_accum_quantize_signed(radiance[c] * Y_k) -- 27 u64 per probe, k-major, 32.32, two's complement,
 * order-free; NaN counts as 0, as everywhere.  THE COEFFICIENTS: coeff[i][k][c] = rt_accum_resolve_signed(sum, samples) *
 * 12.566371f -- the mean over ALL `samples`, rounded once, then one f32 multiply by 4 pi: the Monte-Carlo estimate of the integral
 * of L Y_k over the sphere.  A buffer of sums can be filled by sample ranges and resolved once; radiance(d) ~ sum_k coeff_k Y_k(d),
 * irradiance by the cosine convolution (band factors pi, 2 pi / 3, pi / 4).
 *
 * Three kernels of their own (csrc/rt_probes.hip): rt_probe_kernel, persistent, in the query kernel's launch geometry on the path
 * kernel's traversal and shade blocks, lanes refilled from ONE list of n x sample_count paths; rt_probe_project_kernel, one
 * workgroup per probe; rt_probe_resolve_kernel.  Every record, sum and coefficient equals the reference's arithmetic bit for bit.
 * Frames, views, queries, features and their counters are not affected by probe calls. */
#define RT_PROBE_COEFFS 9
#define RT_PROBE_MAX_PATHS ((i64)1 << 30)
typedef struct {
  i32 samples;                 /* samples per probe: what the coefficients are the mean over                                  */
  i32 sample_first;            /* this call traces samples [sample_first, sample_first + sample_count) of every probe ...     */
  i32 sample_count;            /* ... 0 = all of them                                                                        */
  i32 max_bounces;
  u32 seed;
  u32 probe_first;             /* global index of positions[0]: a slice of a probe array equals the matching part of the whole */
} RT_Probe_Params;             /* 24 bytes */

/* Device level, like rt_render_accumulate(): every pointer is a DEVICE pointer owned by the caller, on the device the scene was
 * uploaded to (project and resolve: the primary device); the calls only enqueue work on `stream` (NULL = default stream).
 *   d_positions : f32[n][3]                                    d_samples : RT_Probe_Sample[n][sample_count], 16-byte aligned
 *   d_sums      : u64[n][9][3], zero before the first range    d_coeffs  : f32[n][9][3]
 * rt_probe_trace() writes every record of the range; rt_probe_project() ADDS the range's 27 sums per probe to d_sums (atomics: a
 * buffer is filled progressively by sample ranges); rt_probe_resolve() turns sums into coefficients.
 * Refused before a device is touched, each with a text of its own in rt_last_error(): a NULL scene, params, positions or output;
 * n <= 0; samples <= 0; a sample range outside [0, samples]; max_bounces < 0; n x sample_count > 2^30 (RT_PROBE_MAX_PATHS: the
 * kernel holds path indices in 32-bit integers); (u64)probe_first + n > 2^32; d_samples not 16-byte aligned.  A refused call
 * leaves its outputs untouched.  0 on success, -1 + rt_last_error(). */
extern int rt_probe_trace(RT_Device_Scene *dscene, RT_Probe_Params const *params, i64 n, void const *d_positions, void *d_samples,
                          void *stream);
extern int rt_probe_project(RT_Probe_Params const *params, i64 n, void const *d_samples, void *d_sums, void *stream);
extern int rt_probe_resolve(RT_Probe_Params const *params, i64 n, void const *d_sums, void *d_coeffs, void *stream);

/* Host level: the three steps from host memory to host memory, on the cached device copy of `scene` with rt_render_frame()'s scene
 * check and device lock, on the NULL stream, on the PRIMARY device only (as the queries).  coeffs f32[n][9][3], sums u64[n][9][3]
 * (the sums of THIS call's sample range, from zero), samples RT_Probe_Sample[n][sample_count]: each optional, at least one.  The
 * probes are traced in slices of at most 2^21 paths (RT_PROBE_SLICE: 64 MB of records on the device; the staging is kept for the
 * next call); a single probe whose sample_count exceeds the slice is split by sample range; probe_first and sample_first make
 * every slice equal to the matching part of the whole.  The same refusals (n x sample_count is not bounded here). */
#define RT_PROBE_SLICE ((i64)1 << 21)
extern int rt_scene_probes(Scene const *scene, RT_Probe_Params const *params, i64 n, Vec3 const *positions, f32 *coeffs, u64 *sums,
                           RT_Probe_Sample *samples);

/* Counters of the last probe call of this process (device or host level; a host call's slices summed): paths, rays, 8-box slab
 * tests, 8-triangle tests, shader evaluations, background lookups, textured shader evaluations.  Synchronises.  rt_get_counters()
 * and rt_get_query_counters() are not affected. */
extern int rt_get_probe_counters(RT_Counters *out);

/* ---- HDR lightmaps --------------------------------------------------------------------- */

/* The light arriving at the texels of a UV layout: the static-lighting product of this library, beside the probes that light
 * everything not baked.  lightmap_bake() (rt_raytracer.h) stays the reference's entry point -- one u8 image, 8 bounces, no sRGB;
 * this is the baker a user runs: a float image, sums that can be filled progressively, device pointers, seam padding.
 *
 * THE TEXEL LIST of a map of width x height.  Texel (x, y) is owned by the LAST triangle slot i whose UV triangle accepts the
 * integer point (x, y): raytracer.c:733-747, p_k = uv_k * (width, height), the weights w0, w1 and w2 = 1 - w0 - w1 in the
 * reference's association, accepted when all three are >= -EPSILON; texels outside the image are skipped.  The list holds the owned
 * texels in row-major order of x + y * width.  Entry j, 32 bytes, written with two 16-byte stores: */
typedef struct { f32 origin[3]; u32 texel; /* x + y * width */ f32 normal[3]; i32 triangle; /* the owning slot */ } RT_Lightmap_Texel;
/*     normal   = n_a * w0 + n_b * w1 + n_c * w2               NOT normalised, as in the reference
 *     position = v0 * w0 + v1 * w1 + v2 * w2                  over the ORIGINAL vertices triangles.x/y/z[k][i]
 *     origin   = position + normal * EPSILON
 * -- plain f32 * and +, left to right, every operation rounded on its own (every unit is built with -ffp-contract=off).
 *
 * THE PATH of list entry j (texel index p = texel_j) and sample s of `samples`:
 *     state = rt_path_seed(seed, p, (u32)s);  tries = 0
 *     loop:  d = rt_rand_unit_vec3(&state);  c = dot(d, normal);  tries++      accept when c > 0.0f, give up when tries == 64
 *     accepted:  L = cast_ray(Ray{origin, d}, max_bounces, &state)            raytracer.c:505-558, the stream going on where the
 *                sums[j][ch] += rt_accum_quantize(L[ch] * c)                   direction left it; ch = 0..2, u64, 32.32, order-free,
 *                                                                              NaN and negatives count as 0
 *     given up (a zero or NaN normal): nothing is cast, nothing is added; the path still counts as a path
 *     max_bounces == 0: nothing is cast, L = 0, nothing to add
 *
 * THE RESOLVE.  image f32[height][width][4]: an owned texel gets {rt_accum_resolve(sum_ch, samples) * scale ..., 1.0f} -- the mean
 * over ALL `samples`, rounded once, then one f32 multiply; a texel nobody owns gets {0, 0, 0, 0}.  scale = 1.0f gives the number the
 * reference computes before its u8 store, 6.2831855f the irradiance; the baker does not choose.
 *
 * THE DILATION is seam padding, so that a bilinear fetch at a chart's edge reads light and not black: `passes` passes (0-254) over
 * the resolved image, ping-pong.  In pass k = 1..passes every texel whose .w == 0 in the pass's INPUT visits its eight neighbours,
 * dy = -1, 0, 1 and inside that dx = -1, 0, 1, skipping the centre and neighbours off the image; n = the number of neighbours with
 * .w > 0; n == 0 copies the texel; otherwise each colour channel is (((a + b) + c) ...) / (float)n -- f32 adds in visiting order from
 * the first usable neighbour's value, one IEEE division -- and .w = (float)(1 + k).  Texels with .w > 0 are copied.  A consumer reads
 * .w == 1 as measured and .w > 1 as filled in pass .w - 1.
 *
 * Kernels of their own (csrc/rt_lightmap.hip): an owner pass, a row count, a row scan and an ordered row write for the list;
 * rt_lightmap_kernel, persistent, a sibling of the probe kernel, lanes refilled from ONE sample-major list of paths, three 64-bit
 * atomic adds per path that ends; a resolve; a dilation pass over 32 x 8 tiles staged in LDS.  Frames, queries, probes, lightmap_bake
 * and their counters are not affected. */
#define RT_LIGHTMAP_MAX_TEXELS ((i64)1 << 28)
#define RT_LIGHTMAP_MAX_PATHS  ((i64)1 << 30)
#define RT_LIGHTMAP_MAX_PASSES 254
typedef struct {
  i32 width, height;           /* the map                                                                                      */
  i32 samples;                 /* samples per texel: what the image is the mean over                                            */
  i32 sample_first;            /* a trace call runs samples [sample_first, sample_first + sample_count) of its texels ...      */
  i32 sample_count;            /* ... 0 = all of them                                                                          */
  i32 max_bounces;
  u32 seed;
  f32 scale;                   /* the resolve's factor                                                                         */
} RT_Lightmap_Params;          /* 32 bytes */

/* Device level: every pointer is a DEVICE pointer owned by the caller, on the device the scene was uploaded to (resolve and dilate:
 * the primary device); the calls only enqueue work on `stream` (NULL = default stream); nothing synchronises.
 *   d_vertices : f32[slots][9], per slot x0 x1 x2 y0 y1 y2 z0 z1 z2 of the original vertices (triangles.x/y/z[k][i])
 *   d_owner    : i32[width x height + height] scratch: the owners (-1 = none), then the rows' list offsets
 *   d_texels   : RT_Lightmap_Texel[width x height] (room for every texel; the list fills the front), 16-byte aligned
 *   d_count    : i64, the list's length n -- what a caller reads back before it sizes the sums and picks texel ranges
 *   d_sums     : u64[n][3], indexed by LIST entry, zero before the first range; rt_lightmap_trace ADDS (atomics), so a buffer is
 *                filled progressively by sample ranges and by texel ranges [texel_first, texel_first + texel_count)
 *   d_image    : f32[height][width][4], 16-byte aligned;  d_work: rt_lightmap_work_bytes() bytes, 16-byte aligned, not d_image
 * Refused before a device is touched, each with a text of its own in rt_last_error(): a NULL argument; width or height <= 0;
 * width x height > 2^28; samples <= 0; a sample range outside [0, samples]; max_bounces < 0; a texel range that is empty, negative
 * or ends beyond width x height (the list cannot be longer; its true length is the caller's to respect); texel_count x sample_count
 * > 2^30 (the kernel holds path indices in 32-bit integers); n_texels outside [0, width x height]; passes outside [0, 254]; a
 * misaligned pointer.  A refused call leaves its outputs untouched.  0 on success, -1 + rt_last_error(). */
extern int rt_lightmap_texels(RT_Device_Scene *dscene, void const *d_vertices, i32 width, i32 height, void *d_owner, void *d_texels,
                              void *d_count, void *stream);
extern int rt_lightmap_trace(RT_Device_Scene *dscene, RT_Lightmap_Params const *params, void const *d_texels, i64 texel_first,
                             i64 texel_count, void *d_sums, void *stream);
extern int rt_lightmap_resolve(RT_Lightmap_Params const *params, i64 n_texels, void const *d_texels, void const *d_sums, void *d_image,
                               void *stream);
extern i64 rt_lightmap_work_bytes(i32 width, i32 height);      /* -1 + rt_last_error() for a size the calls refuse */
extern int rt_lightmap_dilate(i32 width, i32 height, i32 passes, void *d_image, void *d_work, void *stream);

/* Host level: list, trace, resolve and dilation from a host Scene to host memory, on the cached device copy of `scene` with
 * rt_render_frame()'s scene check and device lock, on the NULL stream, on the PRIMARY device only.  image f32[height][width][4]
 * (required); sums u64[n][3] (the sums of THIS call's sample range, from zero), texels RT_Lightmap_Texel[n] and *n_texels are
 * optional -- a caller who wants sums or texels passes room for width x height entries.  The list is traced in launches of at most
 * 2^21 paths (RT_LIGHTMAP_SLICE): sample ranges of the whole list, or texel ranges of one sample where the list is longer than a
 * slice.  The same refusals (texels x sample_count is not bounded here). */
#define RT_LIGHTMAP_SLICE ((i64)1 << 21)
extern int rt_scene_lightmap(Scene const *scene, RT_Lightmap_Params const *params, i32 dilate_passes, f32 *image, u64 *sums,
                             RT_Lightmap_Texel *texels, i64 *n_texels);

/* Counters of the last lightmap trace of this process (device or host level; a host call's launches summed), as
 * rt_get_probe_counters().  Synchronises.  The other counters are not affected. */
extern int rt_get_lightmap_counters(RT_Counters *out);

/* ---- guided denoiser ------------------------------------------------------------------ */

/* An edge-stopping a-trous filter (Dammertz et al. 2010) of the linear frame, steered by the feature buffers above: what turns the
 * reference driver's default 16 spp frame into a usable picture.  Two kernels of their own (rt_guided_pack_kernel,
 * rt_guided_filter_kernel, csrc/rt_guided.hip); frames, views, queries, feature passes and their counters are not affected.
 *
 * THE FILTER.  Only + - * / , comparisons and selects in f32, every operation rounded on its own (no fused multiply-add, no exp,
 * sqrt or reciprocal), a fixed tap order: a float32 restatement on the CPU is equal bit for bit (tests/_guided.py).
 *   Inputs (all finite): color f32[h][w][3] the linear mean radiance; coverage f32[h][w]; albedo, normal, position f32[h][w][3];
 *     normal is the encoded n * 0.5 + 0.5 mean exactly as rt_resolve_features writes it.
 *   Parameters: iterations 1 .. 8; every sigma > 0 and not NaN, +inf switches that term off; demodulate 0 or 1.  The host
 *     computes k_c = 1.0f / (sigma_color * sigma_color), k_n and k_p likewise, in f32.
 *   Per pixel p, once:
 *     N_p = normal_p * 2.0f - coverage_p per component: the mean of the unit normals over the samples that hit, 0 for sky
 *     m_p = albedo_p + ((1.0f - coverage_p) + 1e-3f) per channel when demodulate is set, otherwise 1
 *     c_p = color_p / m_p
 *   Iteration i = 0 .. iterations - 1, step s = 1 << i, kc_i = k_c * (float)(1u << (2 * i)) (the colour sigma halves every time):
 *     L = c.r * 0.2126f + c.g * 0.7152f + c.b * 0.0722f, evaluated left to right
 *     taps t = 0 .. 24 in this order: dy = t / 5 - 2 (outer), dx = t % 5 - 2 (inner), q = (x + s dx, y + s dy); a tap outside the
 *     image is skipped, not clamped
 *       dn = N_p - N_q;  dn2 = dn.x * dn.x + dn.y * dn.y + dn.z * dn.z
 *       dcov = cov_p - cov_q
 *       e = P_q - P_p;  pl = N_p.x * e.x + N_p.y * e.y + N_p.z * e.z      (the distance of q from p's tangent plane)
 *       dl = L_p - L_q
 *       D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p + dl * dl * kc_i, evaluated left to right
 *       r = 1.0f / (1.0f + D)
 *       wgt = ((H[|dy|] * H[|dx|]) * r) * r,  H = {0.375f, 0.25f, 0.0625f}
 *       sum_c = sum_c + wgt * c_q per channel;  sum_w = sum_w + wgt
 *     c'_p = sum_c / sum_w (the centre tap has wgt = 0.140625, so sum_w > 0)
 *     a pixel with coverage_p == 0 keeps c_p: sky is not noisy, and the features say nothing about it
 *   Output: out_p = c_p * m_p; where coverage_p == 0, out_p = color_p bit for bit.  The u8 image is rt_encode_u8(out) per channel
 *     (rt_math.h), under the library's numeric contract like rt_resolve's; a NaN encodes to 0, here and in every pass below.
 * Not done: several devices, view batches.  (Reuse over time: temporal accumulation below; a luminance term measured in the pixel's
 * own variance: "variance-guided denoising" further below.) */
typedef struct {
  i32 iterations;
  f32 sigma_color, sigma_normal, sigma_position;
  i32 demodulate;
} RT_Guided_Params;                                                                              /* 20 bytes */

/* Device level, like rt_render_accumulate_features(): every pointer is a DEVICE pointer owned by the caller, the call only
 * enqueues work on `stream` (a pack launch, then one filter launch per iteration).
 *   d_out   : f32[h][w][3] or NULL        d_image : u8[h][w][3] or NULL        (at least one of them)
 *   d_work  : rt_guided_work_bytes(width, height) bytes of scratch, 16-byte aligned: 64 B per pixel -- two ping-pong colour
 *             buffers of float4 (r, g, b, L) and the guide planes float4 (N, cov) and (P, 0)
 * d_out == d_color is allowed: every input is packed into d_work before anything is written (the last launch reads a pixel's own
 * colour and albedo once more, to write that pixel).  d_albedo may be NULL only when demodulate == 0.
 * Host level: rt_guided_denoise_host() from host memory to host memory through library-owned staging (kept between calls); it
 * takes the library's device lock and runs on the NULL stream like rt_render_features().  planes: all four (albedo may be NULL
 * when demodulate == 0); out f32[h][w][3] and / or image u8[h][w][3].
 * Checked before the GPU is touched, by all of them: NULL pointers, width, height > 0, width x height <= 2^28, iterations in
 * 1 .. 8, sigmas > 0 and not NaN, demodulate 0 or 1, at least one output.  0 on success, -1 + rt_last_error() (rt_guided_work_bytes:
 * the size, -1 + rt_last_error()); a refused call leaves its outputs untouched. */
extern i64 rt_guided_work_bytes(i32 width, i32 height);
extern int rt_guided_denoise(i32 width, i32 height, RT_Guided_Params const *params, void const *d_color, void const *d_coverage,
                             void const *d_albedo, void const *d_normal, void const *d_position, void *d_out, void *d_image,
                             void *d_work, void *stream);
extern int rt_guided_denoise_host(i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                                  RT_Features const *planes, f32 *out, u8 *image);
/* A denoised frame in one call: rt_render_frame()'s frame sequence, the feature pass of the same frame shape and the filter, in
 * ONE scene-checked call (the scene check and the device lock are rt_render_frame()'s; seed and camera are read as it reads
 * them).  The Image receives the encoded DENOISED frame with rt_render_frame()'s layout rules (stride >= width, >= 3 components;
 * pixels.data may be NULL when linear_denoised is given); linear_noisy (optional) = what rt_render_frame() returns as `linear`,
 * linear_denoised (optional) = the filter's f32 output, f32[h][w][3] each.  rt_get_counters() afterwards describes the frame;
 * rt_get_frame_timing()'s gpu_copy_ms then also covers the feature pass and the filter.  One device only: with
 * rt_device_count() > 1 the call fails. */
extern int rt_render_denoised(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                              RT_Guided_Params const *params, f32 *linear_noisy, f32 *linear_denoised);

/* ---- temporal accumulation -------------------------------------------------------------- */

/* The frame blended with the frames before it: every pixel fetches the accumulated colour from where its surface point WAS in the
 * previous camera and blends the new frame in with weight 1 / (frames accumulated).  For static geometry under a moving camera
 * the correspondence is exact and in closed form: the mean world position of a pixel's first hits (the feature buffers above)
 * is projected into both cameras.  One kernel of its own (rt_temporal_kernel, csrc/rt_temporal.hip); frames, views, queries,
 * feature passes, the guided filter and their counters are not affected.
 *
 * THE ACCUMULATION.  Only + - * / , floorf, int <-> float conversions of exactly representable values, comparisons and selects in
 * f32; every operation rounded on its own (no fused multiply-add, no reciprocal), sums evaluated left to right as written: a
 * float32 restatement on the CPU is equal bit for bit (tests/_temporal.py).
 *   Inputs (all finite): color f32[h][w][3] the linear mean radiance; coverage f32[h][w]; albedo, normal (the encoded n * 0.5 + 0.5
 *     mean), position f32[h][w][3] exactly as rt_resolve_features writes them; the frame's Camera and the history's Camera; a
 *     previous HISTORY or none.
 *   Parameters: alpha in (0, 1]; max_history 1 .. 2^20; both tolerances > 0 and not NaN, +inf switches that test off; demodulate 0
 *     or 1.  The host computes in f32: tn2 = normal_tolerance * normal_tolerance, tp2 = plane_tolerance * plane_tolerance,
 *     half_w = (float)w * 0.5f, half_h = (float)h * 0.5f, aspect = (float)w / (float)h.
 *   A history is 48 B per pixel, three planes of float4 records one after the other ([3][h][w] float4):
 *     (c.r, c.g, c.b, len)  the accumulated, demodulated colour and the history length in frames
 *     (N.x, N.y, N.z, cov)  the signed mean normal and the coverage
 *     (W.x, W.y, W.z, 0)    the mean world position of the first hits
 *     A call reads one history and writes another; the reads are gathers from neighbouring pixels, so the two must not overlap
 *     (refused).
 *   proj(cam, W): R = cam.view_matrix rows[i][0..2], t = rows[i][3].  R IS TAKEN AS ORTHONORMAL: its inverse is its transpose (a
 *     view matrix with scale or shear is projected wrongly; the guides then reject the taps or the reuse is wrong).
 *       e  = W - t per component
 *       cx = R[0][0] * e.x + R[1][0] * e.y + R[2][0] * e.z;  cy, cz likewise with R[.][1], R[.][2]
 *       front = cz < 0.0f;  d = 0.0f - cz
 *       ux = ((cx * cam.focal_length) / d) / aspect;  uy = 0.0f - ((cy * cam.focal_length) / d)
 *       fx = (ux + 1.0f) * half_w;  fy = (uy + 1.0f) * half_h
 *     the inverse of the frame's primary ray (raytracer.c:641-694): fx = x + jitter - 0.5.
 *   Per pixel p = (x, y):
 *     cov = coverage_p;  N_p = normal_p * 2.0f - cov per component (as the guided filter)
 *     m_p = albedo_p + ((1.0f - cov) + 1e-3f) per channel and c_p = color_p / m_p when demodulate is set; otherwise m_p = 1, c_p = color_p
 *     cov == 0 (sky is not noisy, and the features say nothing about it): out_p = color_p bit for bit, the history record is
 *       (color_p, 0), (0, 0, 0, 0), (0, 0, 0, 0), length_p = 0.
 *     Otherwise:
 *       W_p = position_p / cov per component            (the mean world position of the samples that hit)
 *       (front_c, fxc, fyc, .) = proj(camera, W_p);  (front_v, fxv, fyv, dv) = proj(previous camera, W_p)
 *       hx = (float)x + (fxv - fxc);  hy = (float)y + (fyv - fyc)
 *         the motion is the difference of two projections of one point, not fxv itself: the mean jitter of a pixel's samples is not
 *         0.5, and the difference cancels that offset; with equal cameras it is +0 and hx = x exactly
 *       usable = history given && front_c && front_v && hx >= -1.0f && hx < (float)w && hy >= -1.0f && hy < (float)h
 *         (every comparison is false for NaN)
 *       if usable: x0 = (int)floorf(hx), y0 = (int)floorf(hy), ax = hx - (float)x0, ay = hy - (float)y0; taps k = 0 .. 3 in this order
 *           (x0, y0) b = (1.0f - ax) * (1.0f - ay);  (x0 + 1, y0) b = ax * (1.0f - ay);  (x0, y0 + 1) b = (1.0f - ax) * ay;  (x0 + 1, y0 + 1) b = ax * ay
 *         a tap q is VALID when it lies inside the image, cov_q > 0 and
 *           dn = N_p - N_q;  dn.x * dn.x + dn.y * dn.y + dn.z * dn.z <= tn2
 *           e = W_q - W_p;  pl = N_p.x * e.x + N_p.y * e.y + N_p.z * e.z;  pl * pl <= (tp2 * dv) * dv
 *           (the distance of the old surface point from p's tangent plane, relative to its depth in the old camera)
 *         over the valid taps in tap order: sum_w = sum_w + b;  sum_c = sum_c + b * c_q per channel;  sum_n = sum_n + b * len_q
 *       if usable && sum_w > 0:
 *           h_c = sum_c / sum_w;  h_n = sum_n / sum_w;  n = h_n < (float)max_history ? h_n : (float)max_history
 *           a = 1.0f / (n + 1.0f);  if (a < alpha) a = alpha
 *           c' = h_c + (c_p - h_c) * a;  len' = n + 1.0f
 *       otherwise c' = c_p, len' = 1.0f
 *       out_p = c' * m_p (demodulate == 0: c'); the history record is (c', len'), (N_p, cov), (W_p, 0); length_p = len'
 *     The u8 image is rt_encode_u8(out) per channel (rt_math.h), under the library's numeric contract like rt_resolve's.
 *   Two consequences.  Equal cameras over an unchanged scene: hx = x, ax = 0, the centre tap has weight 1 and passes both tests with
 *   0 (the feature pass does not read the seed: old and new guides are the same bits), so the output is the recursion
 *   h + (c - h) * a bit for bit.  No history (first frame, after a reset): out = c_p * m_p and len = 1.
 *
 * THE ACCUMULATION WITH MOTION (moving geometry: a mesh deformed by scene_refit_gpu between two frames).  THE ACCUMULATION -- and
 * THE MOMENTS below -- with one more input, motion f32[h][w][3] as rt_resolve_motion writes it (finite), and these differences and
 * no others.  For a pixel with cov != 0:
 *       M_p = motion_p / cov per component;  V_p = W_p + M_p per component      (where the mean surface point WAS)
 *       (front_c, fxc, fyc, .) = proj(camera, W_p) as before;  (front_v, fxv, fyv, dv) = proj(previous camera, V_p)
 *       in a tap's plane test:  e = W_q - V_p      (N_p, tn2, tp2 and dv -- now V_p's depth in the old camera -- as before)
 *       the history record keeps (W_p, 0), not V_p: the next frame measures from where the surface is now
 *   Consequence: with motion all +0, V_p = W_p and every output equals THE ACCUMULATION's (THE MOMENTS') bit for bit.  THE VARIANCE
 *   and both filters read no previous frame and are what they were.
 *   Known limit: the normal test stays on the CURRENT normal, dn = N_p - N_q.  A surface that turned by more than normal_tolerance
 *   between two frames restarts there (previous normals would need the 28-float shading records kept as well).
 * Still out of scope: TURNING NORMALS (above); TOPOLOGY CHANGES -- the motion pairs a triangle with what its slot held when the
 * geometry was kept, so a mesh whose triangles change slots or count is rebuilt, loses the kept geometry with the device copy, and
 * has motion 0; several devices, view batches, weighting frames by their sample counts.  Without the motion plane, after
 * scene_refit_gpu a surface that moved off its old plane fails the plane test and restarts, and one that slid within its own plane
 * is reused wrongly: a host that deforms the mesh uses the motion calls below or resets the history.  (Moments and variance:
 * "variance-guided denoising" below.) */
typedef struct {
  f32 alpha;
  i32 max_history;
  f32 normal_tolerance, plane_tolerance;
  i32 demodulate;
} RT_Temporal_Params;                                                                            /* 20 bytes */

/* A history as planar host arrays (rt_temporal_accumulate_host): the accumulated colour f32[h][w][3], the length f32[h][w], the
 * coverage f32[h][w], the signed N and W f32[h][w][3] -- the fields of the three records above, one plane each. */
typedef struct { f32 *color, *length, *coverage, *normal, *position; } RT_History_Planes;

/* Device level, like rt_guided_denoise(): every pointer is a DEVICE pointer owned by the caller, the call only enqueues one launch
 * on `stream`.
 *   d_history_in  : rt_temporal_history_bytes(width, height) bytes, 16-byte aligned, or NULL = no history (then previous_camera is
 *                   not read and may be NULL)
 *   d_history_out : as many bytes, 16-byte aligned; receives the new history.  Must not overlap d_history_in.
 *   d_out f32[h][w][3], d_length f32[h][w], d_image u8[h][w][3] : each optional.  d_out == d_color is allowed: a pixel reads only
 *                   its own colour.  d_albedo may be NULL only when demodulate == 0.
 * Host level: rt_temporal_accumulate_host() from host memory to host memory through library-owned staging (kept between calls); it
 * takes the library's device lock and runs on the NULL stream.  planes: all four (albedo may be NULL when demodulate == 0);
 * history_in: NULL = none, otherwise all five planes; history_out: NULL = not wanted, otherwise all five planes (which may be
 * history_in's: the arrays are staged); at least one of history_out, out, length, image.
 * Checked before the GPU is touched, by all of them: NULL pointers, width, height > 0, width x height <= 2^28, alpha in (0, 1],
 * max_history in 1 .. 2^20, tolerances > 0 and not NaN, demodulate 0 or 1, alignment, overlapping histories, no output.  0 on
 * success, -1 + rt_last_error() (rt_temporal_history_bytes: the size, -1 + rt_last_error()); a refused call leaves its outputs
 * untouched. */
extern i64 rt_temporal_history_bytes(i32 width, i32 height);
extern int rt_temporal_accumulate(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                  Camera const *previous_camera, void const *d_color, void const *d_coverage, void const *d_albedo,
                                  void const *d_normal, void const *d_position, void const *d_history_in, void *d_history_out,
                                  void *d_out, void *d_length, void *d_image, void *stream);
extern int rt_temporal_accumulate_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                       Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                       RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                       f32 *length, u8 *image);

/* The history a host keeps for a sequence: two device histories, ping-ponged, and the camera of the last frame accumulated.  The
 * memory is allocated on the primary device by the first frame that uses it (rt_history_create touches no device) and belongs
 * to that device slot's staging: when the slot's staging is given back, the history is empty again and the next frame starts from
 * nothing, as after rt_history_reset().  rt_history_destroy(NULL) is allowed.  A history serves one thread at a time. */
typedef struct RT_History RT_History;
extern RT_History *rt_history_create(i32 width, i32 height);
extern int         rt_history_reset(RT_History *history);
extern void        rt_history_destroy(RT_History *history);
/* on = 1: rt_render_temporal() / rt_render_svgf() on this history run the motion feature pass in place of the plain one (one
 * launch, not two) against the scene's kept geometry, and THE ACCUMULATION WITH MOTION, in the same scene-checked call.  Default 0:
 * what they did before.  The history's contents stay.  0, or -1 + rt_last_error() (NULL, on not 0 / 1). */
extern int         rt_history_set_motion(RT_History *history, int on);

/* An accumulated frame in one call: rt_render_frame()'s frame sequence, the feature pass of the same frame shape, the accumulation
 * against `history` (previous camera = the camera of the last call on this history) and, when guided_params is not NULL, the guided
 * filter over the accumulated output -- in ONE scene-checked call, as rt_render_denoised() is.  The history keeps the UNFILTERED
 * accumulation and the camera of this call.  The Image receives the encoding of the last stage with rt_render_frame()'s layout
 * rules (pixels.data may be NULL when linear_out or length is given); linear_noisy (optional) = what rt_render_frame() returns as
 * `linear`, linear_out (optional) = the last stage's f32 output, f32[h][w][3] each; length (optional) f32[h][w].  The image size
 * must be the history's.  One device only: with rt_device_count() > 1 the call fails. */
extern int rt_render_temporal(Scene const *scene, Image const *image, isize samples, isize max_bounces, RT_History *history,
                              RT_Temporal_Params const *temporal_params, RT_Guided_Params const *guided_params, f32 *linear_noisy,
                              f32 *linear_out, f32 *length);

/* ---- variance-guided denoising ---------------------------------------------------------- */

/* What SVGF (Schied et al. 2017) adds to the two passes above: the filter learns how noisy a pixel still is.  The accumulation
 * carries the first and second moment of the luminance next to the colour; a second launch turns them into a variance per pixel
 * (from the 7 x 7 neighbourhood where the history is shorter than 4 frames); and the filter's luminance term is measured in that
 * variance instead of one fixed sigma_color.  Kernels of their own (csrc/rt_variance.hip), which share the accumulation's pixel and
 * the filter's tile with the kernels above; rt_guided_denoise*, rt_temporal_accumulate*, rt_render_denoised and rt_render_temporal
 * return what they returned, and the 48-byte history record is unchanged.
 *
 * All three contracts: only f32 + - * / , comparisons and selects (floorf only where THE ACCUMULATION has it); every operation
 * rounded on its own (no fused multiply-add, exp, sqrt or reciprocal); sums left to right as written; every comparison with NaN
 * is false; lum(c) = c.r * 0.2126f + c.g * 0.7152f + c.b * 0.0722f left to right.  A float32 restatement on the CPU is equal bit for
 * bit (tests/_variance.py).
 *
 * THE MOMENTS.  A moments buffer is 16 B per pixel: one plane of float4 (m1, m2, 0, 0), the accumulated first and second moment of
 * the luminance of the demodulated colour; rt_temporal_moments_bytes() is its size.  Everything of THE ACCUMULATION holds and
 * gives the same bits for out, the history, length and the image.  In addition, for every pixel with cov != 0:
 *     L_p = lum(c_p);  S_p = L_p * L_p        (c_p the accumulation's own, demodulated when demodulate is set)
 *     over the valid taps in tap order, next to sum_c and sum_n:  sum_1 = sum_1 + b * m1_q;  sum_2 = sum_2 + b * m2_q
 *     if usable && sum_w > 0, with the accumulation's a:
 *         h_1 = sum_1 / sum_w;  h_2 = sum_2 / sum_w;  m1' = h_1 + (L_p - h_1) * a;  m2' = h_2 + (S_p - h_2) * a
 *     otherwise m1' = L_p, m2' = S_p
 *     v = m2' - m1' * m1';  var_t = v > 0.0f ? v : 0.0f;  the moments record is (m1', m2', 0, 0)
 *   A pixel with cov == 0 has the moments record (0, 0, 0, 0) and variance 0.  On the input side a history and its moments are given
 *   both or neither (refused otherwise); the moments output must not overlap the moments input (refused).
 *
 * THE VARIANCE.  A second launch, which reads only what the first wrote -- the new history's planes (c', len'), (N, cov), (W, 0)
 * and the new moments -- and writes the variance plane f32[h][w].
 *   Parameters: sigma_normal, sigma_position > 0 and not NaN, +inf switches the term off; the host computes k_n and k_p as the
 *     guided filter does.
 *   Per pixel p with cov_p != 0:
 *     if len'_p >= 4.0f: var_p = var_t, computed from the moments record by the expression above.
 *     otherwise the 49 taps dy = -3 .. 3 (outer), dx = -3 .. 3 (inner), q = (x + dx, y + dy); a tap outside the image or with
 *     cov_q == 0 is skipped; for each tap that counts
 *         dn = N_p - N_q;  dn2 = dn.x * dn.x + dn.y * dn.y + dn.z * dn.z
 *         dcov = cov_p - cov_q
 *         e = W_q - W_p;  pl = N_p.x * e.x + N_p.y * e.y + N_p.z * e.z
 *         D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p, left to right
 *         r = 1.0f / (1.0f + D);  wgt = r * r                     (the centre has wgt = 1, so s_w >= 1)
 *         s_w = s_w + wgt;  s_1 = s_1 + wgt * m1'_q;  s_2 = s_2 + wgt * m2'_q
 *       e1 = s_1 / s_w;  e2 = s_2 / s_w;  v = e2 - e1 * e1;  v = v > 0.0f ? v : 0.0f;  var_p = v * (4.0f / len'_p)
 *   A pixel with cov_p == 0 has var_p = 0.  The threshold 4 and the boost 4 / len are SVGF's: part of the contract, no parameters.
 *
 * THE VARIANCE-GUIDED FILTER.  THE FILTER, with these differences and no others.
 *   One more input: variance f32[h][w], finite and >= 0, the variance of the demodulated luminance (what THE VARIANCE writes);
 *     v(0) = variance.
 *   In iteration i, for every pixel p:
 *     g_p = a 3 x 3 Gaussian of the current v at UNIT spacing, whatever the step: taps dy = -1 .. 1 (outer), dx = -1 .. 1 (inner),
 *       taps outside the image skipped;  gs = gs + (G[|dy|] * G[|dx|]) * v_q;  gw = gw + G[|dy|] * G[|dx|],  G = {0.5f, 0.25f};
 *       g_p = gs / gw
 *     kv_p = k_c / (g_p + 1e-8f): sigma_color is now a multiple of the pixel's standard deviation (SVGF's value is 4); with
 *       sigma_color = +inf, k_c = 0 and kv_p = 0
 *     the last term of D is (dl * dl) * kv_p in place of dl * dl * kc_i; nothing is halved per iteration; L_q = lum(c_q) as before
 *     next to sum_c and sum_w:  sum_v = sum_v + (wgt * wgt) * v_q
 *     c'_p = sum_c / sum_w;  v'_p = sum_v / (sum_w * sum_w);  a pixel with cov_p == 0 keeps c_p and v_p
 *   Outputs: THE FILTER's, and optionally variance_out f32[h][w], the last v.
 *   Consequence: with sigma_color = +inf the colour output equals rt_guided_denoise's with sigma_color = +inf bit for bit. */
typedef struct { f32 sigma_normal, sigma_position; } RT_Variance_Params;                         /* 8 bytes */

/* rt_temporal_accumulate() / rt_temporal_accumulate_host() with the moments, in the same launch, and the variance launch behind it
 * when a variance is wanted.  Argument checks, aliasing rules, staging and locking are those calls'; in addition:
 *   d_moments_in  : rt_temporal_moments_bytes(width, height) bytes, 16-byte aligned; given exactly when d_history_in is (refused
 *                   otherwise)
 *   d_moments_out : as many bytes, 16-byte aligned, required; must not overlap d_moments_in
 *   d_variance    : f32[h][w], optional; vp is read (and required) only when it is wanted, and checked whenever it is given
 * Host level: moments_in f32[h][w][2] (m1, m2) or NULL, given exactly when history_in is; moments_out f32[h][w][2] and variance
 * f32[h][w] are optional outputs and count as such.  A refused call leaves its outputs untouched. */
extern i64 rt_temporal_moments_bytes(i32 width, i32 height);
extern int rt_temporal_accumulate_moments(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                          Camera const *previous_camera, void const *d_color, void const *d_coverage,
                                          void const *d_albedo, void const *d_normal, void const *d_position, void const *d_history_in,
                                          void *d_history_out, void *d_out, void *d_length, void *d_image, RT_Variance_Params const *vp,
                                          void const *d_moments_in, void *d_moments_out, void *d_variance, void *stream);
extern int rt_temporal_accumulate_moments_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                               Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                               RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                               f32 *length, u8 *image, RT_Variance_Params const *vp, f32 const *moments_in,
                                               f32 *moments_out, f32 *variance);

/* THE ACCUMULATION WITH MOTION ("temporal accumulation" above), kernels of their own (rt_temporal_motion_kernel,
 * rt_temporal_moments_motion_kernel).  d_motion / motion f32[h][w][3] is required.  vp, d_moments_in, d_moments_out and d_variance
 * (host level: vp, moments_in, moments_out, variance) all NULL selects the plain accumulation, with rt_temporal_accumulate()'s
 * rules; any of them given selects the moments form, with rt_temporal_accumulate_moments()'s.  Refusals are those calls' plus a
 * NULL motion; a refused call leaves its outputs untouched. */
extern int rt_temporal_accumulate_motion(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                         Camera const *previous_camera, void const *d_color, void const *d_coverage,
                                         void const *d_albedo, void const *d_normal, void const *d_position, void const *d_history_in,
                                         void *d_history_out, void *d_out, void *d_length, void *d_image, RT_Variance_Params const *vp,
                                         void const *d_moments_in, void *d_moments_out, void *d_variance, void *stream,
                                         void const *d_motion);
extern int rt_temporal_accumulate_motion_host(i32 width, i32 height, RT_Temporal_Params const *params, Camera const *camera,
                                              Camera const *previous_camera, f32 const *color, RT_Features const *planes,
                                              RT_History_Planes const *history_in, RT_History_Planes const *history_out, f32 *out,
                                              f32 *length, u8 *image, RT_Variance_Params const *vp, f32 const *moments_in,
                                              f32 *moments_out, f32 *variance, f32 const *motion);

/* rt_guided_denoise() / rt_guided_denoise_host() as THE VARIANCE-GUIDED FILTER.  d_variance / variance f32[h][w] is required;
 * d_variance_out / variance_out f32[h][w] is optional and counts as an output.  d_work: rt_guided_variance_work_bytes(width,
 * height) bytes, 16-byte aligned: 64 B per pixel -- two ping-pong buffers of float4 (r, g, b, v) and the two guide planes.
 * Everything else as the calls they extend. */
extern i64 rt_guided_variance_work_bytes(i32 width, i32 height);
extern int rt_guided_denoise_variance(i32 width, i32 height, RT_Guided_Params const *params, void const *d_color, void const *d_coverage,
                                      void const *d_albedo, void const *d_normal, void const *d_position, void *d_out, void *d_image,
                                      void *d_work, void *stream, void const *d_variance, void *d_variance_out);
extern int rt_guided_denoise_variance_host(i32 width, i32 height, RT_Guided_Params const *params, f32 const *color,
                                           RT_Features const *planes, f32 *out, u8 *image, f32 const *variance, f32 *variance_out);

/* A variance-guided frame in one call: rt_render_temporal()'s pipeline with the moments pass in place of the plain accumulation,
 * the variance launch behind it and the variance-guided filter -- mandatory here -- over the accumulated output.  The history
 * gains two moments buffers, allocated by the first such frame, ping-ponged with the histories, owned and given back like them
 * and emptied by rt_history_reset().  A non-empty history whose last frame was written by rt_render_temporal() has no valid
 * moments: the call is refused until rt_history_reset().  rt_render_temporal() after rt_render_svgf() is allowed and invalidates
 * the moments.  `variance` (optional, f32[h][w]) returns the INPUT of the filter, THE VARIANCE's estimate; everything else as
 * rt_render_temporal().  One device only. */
extern int rt_render_svgf(Scene const *scene, Image const *image, isize samples, isize max_bounces, RT_History *history,
                          RT_Temporal_Params const *temporal_params, RT_Variance_Params const *variance_params,
                          RT_Guided_Params const *guided_params, f32 *linear_noisy, f32 *linear_out, f32 *length, f32 *variance);

/* ---- half-resolution frames: feature-guided upsampling ------------------------------------ */

/* The one stage behind a frame that takes path-tracing work away: the frame is traced at half the width and half the height -- a
 * quarter of the paths -- and brought to full size over FULL-resolution feature buffers ("first-hit feature buffers" above: their
 * edge-aware upscaler).  The albedo is taken at full resolution, so texture detail does not come from the path frame: only the
 * demodulated colour is interpolated, and a low pixel contributes to a full pixel as far as their first hits agree.  One kernel of
 * its own (rt_upsample_kernel, csrc/rt_upsample.hip) behind the filter's pack kernel; rt_guided_denoise*, rt_render_denoised,
 * rt_render_temporal and rt_render_svgf return what they returned.
 *
 * THE UPSAMPLING.  Only + - * / , comparisons and selects in f32, every operation rounded on its own (no fused multiply-add, no
 * reciprocal, exp or sqrt), a fixed tap order: a float32 restatement on the CPU is equal bit for bit (tests/_upsample.py).
 *   Sizes: the full size W x H, both even and >= 2; the low size wl = W / 2, hl = H / 2.
 *   Geometry: a primary ray goes through uvx = ((x + jitter - 0.5) * 2) / width - 1 (and uvy likewise), so the centre of low pixel
 *     X lies on the centre of full pixel 2 X (both at 2 X / wl - 1), and width / height is the same f32 for both sizes: ONE camera
 *     serves both frames.  With an odd size neither holds, which is why odd sizes are refused.
 *   Inputs (all finite): low -- color f32[hl][wl][3] the linear mean radiance, coverage f32[hl][wl], albedo, normal, position
 *     f32[hl][wl][3]; full -- coverage f32[H][W], albedo, normal, position f32[H][W][3].  normal is the encoded n * 0.5 + 0.5 mean
 *     exactly as rt_resolve_features writes it.
 *   Parameters: sigma_normal, sigma_position > 0 and not NaN, +inf switches that term off; demodulate 0 or 1.  The host computes
 *     k_n = 1.0f / (sigma_normal * sigma_normal) and k_p likewise, in f32.
 *   Per low pixel q and per full pixel p, exactly as THE FILTER has them:
 *     N = normal * 2.0f - coverage per component
 *     m = albedo + ((1.0f - coverage) + 1e-3f) per channel when demodulate is set, otherwise 1
 *     and for low pixels c_q = color_q / m_q
 *   Taps: a separable quadratic B-spline on the low lattice (its weights at whole and half lattice steps are dyadic).  For full
 *     pixel (x, y): X0 = x >> 1, Y0 = y >> 1; along x the taps are X0 - 1 + (x & 1) + i, i = 0, 1, 2, with the weights
 *     Hx = {0.125f, 0.75f, 0.125f} for even x and {0.5f, 0.5f, 0} for odd x; along y likewise with j and Hy; j is the outer loop
 *     and i the inner one.  A tap with a zero spline weight is skipped.  A tap outside the low image is skipped, not clamped.  For
 *     every tap q = (X, Y) that is left:
 *       dn = N_p - N_q;  dn2 = dn.x * dn.x + dn.y * dn.y + dn.z * dn.z
 *       dcov = cov_p - cov_q
 *       e = P_q - P_p;  pl = N_p.x * e.x + N_p.y * e.y + N_p.z * e.z      (the distance of q from p's tangent plane)
 *       D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p, evaluated left to right
 *       r = 1.0f / (1.0f + D)
 *       wgt = ((Hy * Hx) * r) * r
 *       sum_c = sum_c + wgt * c_q per channel;  sum_w = sum_w + wgt
 *   Result: c_p = sum_c / sum_w where sum_w > 0, otherwise c_p = c of low pixel (X0, Y0).  (sum_w > 0 can fail although the low
 *     pixel (X0, Y0) is always a tap: pl * pl overflows to +inf for positions around 3e19 and every r is 0 -- or NaN, with k_p = 0.)
 *   Sky needs no case of its own: with cov_p == 0, N_p is 0 and the plane term vanishes; the normal and the coverage term then
 *     prefer the sky taps.
 *   Output: out_p = c_p * m_p.  The u8 image is rt_encode_u8(out) per channel (rt_math.h), under the library's numeric contract; a
 *     NaN encodes to 0.
 * Not done: factors other than 2, odd sizes, several devices, view batches; an upsampled frame in front of rt_render_temporal /
 * rt_render_svgf (the upsampled frame is an ordinary linear frame: the natural next step); low-resolution guides derived from the
 * full-resolution planes in place of a second feature pass. */
typedef struct {
  f32 sigma_normal, sigma_position;
  i32 demodulate;
  i32 guide_samples;   /* rt_render_upsampled alone reads it: samples of the full-resolution feature pass, 1 .. samples; 0 = samples */
} RT_Upsample_Params;                                                                            /* 16 bytes */

/* Device level, like rt_guided_denoise(): every pointer is a DEVICE pointer owned by the caller, the call only enqueues work on
 * `stream` (the pack launch over the low frame, then the upsampling launch).
 *   d_color_low, d_coverage_low, d_albedo_low, d_normal_low, d_position_low : the low frame, (width / 2) x (height / 2)
 *   d_coverage, d_albedo, d_normal, d_position : the full-resolution planes, width x height
 *   d_out   : f32[height][width][3] or NULL      d_image : u8[height][width][3] or NULL      (at least one of them)
 *   d_work  : rt_guided_upsample_work_bytes(width, height) bytes of scratch, 16-byte aligned: 48 B per LOW pixel = 12 B per full
 *             pixel -- the packed low frame, three planes of float4: (c, L), (N, cov), (P, 0)
 * d_out and d_image must not overlap any input nor d_work (refused).  Both albedo planes may be NULL only when demodulate == 0.
 * Host level: rt_guided_upsample_host() from host memory to host memory through library-owned staging (kept between calls); it takes
 * the library's device lock and runs on the NULL stream like rt_guided_denoise_host().  low / full: all four planes (albedo may be
 * NULL when demodulate == 0); out f32[height][width][3] and / or image u8[height][width][3].
 * Checked before the GPU is touched, by all of them: NULL pointers, width and height even and >= 2, width x height <= 2^28, sigmas
 * > 0 and not NaN, demodulate 0 or 1, at least one output.  0 on success, -1 + rt_last_error() (rt_guided_upsample_work_bytes: the
 * size, -1 + rt_last_error()); a refused call leaves its outputs untouched. */
extern i64 rt_guided_upsample_work_bytes(i32 width, i32 height);
extern int rt_guided_upsample(i32 width, i32 height, RT_Upsample_Params const *params, void const *d_color_low,
                              void const *d_coverage_low, void const *d_albedo_low, void const *d_normal_low,
                              void const *d_position_low, void const *d_coverage, void const *d_albedo, void const *d_normal,
                              void const *d_position, void *d_out, void *d_image, void *d_work, void *stream);
extern int rt_guided_upsample_host(i32 width, i32 height, RT_Upsample_Params const *params, f32 const *color_low,
                                   RT_Features const *low, RT_Features const *full, f32 *out, u8 *image);
/* An upsampled frame in one call: rt_render_frame()'s frame sequence at (W / 2) x (H / 2), the feature pass of that frame (the
 * same samples), the feature pass at W x H with upsample_params->guide_samples samples -- guides are geometric and need few --,
 * the upsampling and, when guided_params is not NULL, the guided filter at W x H over the upsampled frame, in ONE scene-checked call
 * (the scene check and the device lock are rt_render_frame()'s; seed and camera are read as it reads them).  `image` is W x H and
 * receives the encoding of the LAST stage with rt_render_frame()'s layout rules (pixels.data may be NULL when linear_upsampled or
 * linear_out is given); linear_low (optional) f32[H / 2][W / 2][3] = what rt_render_frame() returns as `linear` at the low size,
 * linear_upsampled (optional) f32[H][W][3] = the upsampling's output, linear_out (optional, only with guided_params) f32[H][W][3] =
 * the filter's.  Refused besides what the stages refuse: W or H odd or < 2, guide_samples outside 0 .. samples, linear_out without
 * guided_params.  rt_get_counters() afterwards describes the LOW frame; rt_get_frame_timing()'s gpu_copy_ms then also covers the
 * feature passes, the upsampling and the filter.  One device only: with rt_device_count() > 1 the call fails. */
extern int rt_render_upsampled(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                               RT_Upsample_Params const *upsample_params, RT_Guided_Params const *guided_params, f32 *linear_low,
                               f32 *linear_upsampled, f32 *linear_out);

/* ---- adaptive sampling: chunks double their samples until the error settles ------------------ */

/* The one stage that decides WHERE samples go: sky and flat surfaces stop early, glossy edges go on.  The scheme is Dammertz et
 * al. 2010, "A hierarchical automatic stopping condition for Monte Carlo methods", restricted to the 32x32 chunks of the frame and
 * to doubling: a chunk that holds n samples per pixel in `accum` receives samples [n, 2n) into a second buffer `fresh`; the two
 * buffers are independent halves of equal size, their difference estimates the chunk's error and their sum is the chunk's
 * 2n-sample frame; a chunk whose error is at or under a threshold stops, the others double again, up to a cap.  One launch of the
 * path kernel per round over a shrinking chunk list; the path kernel is what it was (it finds its pixels through a chunk table),
 * and since a path's seed depends on (frame seed, pixel, sample) alone and the sums are order-free, a chunk that ends with n_c
 * samples holds the sums rt_render_frame(samples = n_c) gives its pixels, bit for bit.  Two kernels of their own
 * (rt_adaptive_merge_kernel, rt_resolve_adaptive_kernel, csrc/rt_adaptive.hip); every other entry point returns what it returned.
 *
 * A CHUNK LIST: a HOST array of n_list >= 0 global chunk indices (chunk c = cx + cy * ceil(width / 32)), every one in
 * [0, rt_chunk_count(width, height)), strictly ascending (a duplicate would add a chunk twice).  Checked on the host before the
 * device is touched -- a wrong index would be a write outside the caller's buffers -- and copied to the device before the call
 * returns: the caller may reuse the array at once.  Calls that take a list serve ONE stream at a time.
 *
 * rt_render_accumulate_chunks(): rt_render_accumulate() with the caller's list in place of the partition's: rank 0 of world 1 only.
 * Chunks not listed are neither read nor written; n_list == 0 enqueues the launch's preparation and renders nothing.  These launches
 * have a launch state of their own, run their tiles in list order and keep no schedule feedback: ordinary frames, before and
 * after, are scheduled as if the call had not been made.  rt_get_counters() afterwards describes this launch.
 *
 * THE MERGE.  rt_accum_resolve (rt_math.h), then f32 + - / and sqrt, every operation rounded on its own (no fused multiply-add),
 * evaluated as written; the chunk's sum in integers: a numpy restatement is equal bit for bit (tests/_adaptive.py).  For every pixel
 * of a listed chunk that lies inside the image, n = the samples each buffer holds per pixel:
 *     a_c = min(rt_accum_resolve(accum_c, n), 1.0f),  b_c = min(rt_accum_resolve(fresh_c, n), 1.0f)     per channel c = r, g, b
 *       (the output stage clamps at 1: error above that is invisible)
 *     d = (|a_r - b_r| + |a_g - b_g|) + |a_b - b_b|
 *     m = ((a_r + b_r) + (a_g + b_g)) + (a_b + b_b)
 *     e = d / rt_sqrtf(m + 1e-4f)
 *     q = (u64)(e * 4294967296.0f)      (e <= 300: the product is exact, the conversion truncates)
 *     accum_c = accum_c + fresh_c in u64;  fresh_c = 0
 *   err[chunk] = the sum of the chunk's q, in u64 (stored, not added: no need to clear err).
 * rt_adaptive_merge(): d_accum, d_fresh u64[height][width][3], d_err u64[rt_chunk_count(width, height)] on the primary device;
 * chunks not listed, and their err entries, are neither read nor written.  Only enqueues work on `stream`.
 *
 * rt_resolve_adaptive(): rt_resolve() for rank 0 of 1 with the divisor read per chunk: d_chunk_samples i32[rt_chunk_count(width,
 * height)] on the device, every entry >= 1 (the library cannot check device memory).  Outputs, each optional, at least one:
 * d_image u8[height][width][3], d_linear f32[height][width][3], d_sample_map i32[height][width] -- every pixel's divisor, what a
 * viewer or a later variance-aware stage reads.  Only enqueues work on `stream`.
 * Checked before the GPU is touched, by all three: NULL pointers, the image size, the list, n >= 1, no output. */
extern int rt_render_accumulate_chunks(RT_Device_Scene *dscene, RT_Render_Params const *params, i32 n_list, i32 const *chunks,
                                       void *d_accum, void *stream);
extern int rt_adaptive_merge(i32 width, i32 height, i32 n, i32 n_list, i32 const *chunks, void *d_accum, void *d_fresh, void *d_err,
                             void *stream);
extern int rt_resolve_adaptive(i32 width, i32 height, void const *d_chunk_samples, void const *d_accum, void *d_image, void *d_linear,
                               void *d_sample_map, void *stream);

typedef struct {
  i32 min_samples;   /* first launch: samples [0, min) of every pixel; >= 1                                */
  i32 max_samples;   /* cap; min_samples * 2^k, k >= 1                                                     */
  f32 threshold;     /* a chunk stops when its mean per-pixel error <= threshold; finite, >= 0             */
  i32 reserved;      /* 0 */
} RT_Adaptive_Params;                                                                            /* 16 bytes */

/* An adaptive frame in one call, from host memory to host memory like rt_render_frame() (its scene check, device lock, seed,
 * camera and Image layout rules; pixels.data may be NULL when another output is given):
 *   1. samples [0, min_samples) of every chunk;
 *   2. rounds with n = min_samples, 2 min_samples, ...: samples [n, 2n) of the active chunks into `fresh`, THE MERGE, the errors
 *      copied to the host (one synchronisation per round); in double, err_c = err[c] / 2^32 / (pixels of chunk c inside the
 *      image); chunk c stays active iff err_c > (double)threshold && 2n < max_samples;
 *   3. when no chunk is active: rt_resolve_adaptive and the copies out.
 * Every chunk ends with 2 min_samples .. max_samples samples, a power-of-two multiple of min_samples.  linear (optional)
 * f32[height][width][3], accum (optional) u64[height][width][3] as rt_render_frame() returns them; chunk_samples (optional)
 * i32[rt_chunk_count(width, height)] = n_c.  What is needed by every frame -- step 1 and the first round -- is enqueued before the
 * full content check of the host scene, which runs while the GPU traces them.
 * Afterwards rt_get_counters() is the SUM over the frame's launches (paths = the sum over the chunks of pixels inside the image x
 * n_c); rt_get_skipped_root_visits(), rt_get_leafless_paths(), rt_get_fused_root_visits() and the kernel timing describe single
 * launches, the LAST one where they describe one.  rt_get_frame_timing(): gpu_prep = the clears and the first preparation, gpu_path
 * = from there to the end of the last merge, the host's decisions between the rounds included.  Every launch ends with the tail
 * rt_frame_begin() describes: a frame of up to 1 + log2(max_samples / min_samples) launches pays it that often.
 * Refused before the GPU is touched: NULL scene, image or params, min_samples < 1, max_samples not min_samples * 2^k with k >= 1,
 * a threshold that is negative, infinite or NaN, reserved != 0, the image's size and layout, max_bounces < 0, no output.  One device
 * only: with rt_device_count() > 1 the call fails.  Not done: view batches, the wavefront pipeline, an adaptive frame in front of
 * the post passes, granularity finer than a chunk, the next list built on the device, schedule costs carried across rounds. */
extern int rt_render_adaptive(Scene const *scene, Image const *image, RT_Adaptive_Params const *ap, isize max_bounces, f32 *linear,
                              u64 *accum, i32 *chunk_samples);

/* Counters of the last rt_render_accumulate / rt_render_frame on this process
 * (read back synchronously; summed over the devices of a multi-device frame). */
extern int rt_get_counters(RT_Counters *out);
/* Of node_visits of the last rt_render_accumulate launch (single device): the visits that were counted but not executed -- the
 * ONE root visit of every camera path whose 8x8 tile's pixel pyramid misses every child box of the root (raytracer.c:459-472
 * finds no candidate for any of them; the kernel proves that per tile and skips the block).  The oracle counts them too. */
extern int rt_get_skipped_root_visits(u64 *out);
/* Camera paths of the last rt_render_accumulate launch (single device) that the path kernel's leafless loop served: paths of 8x8
 * tiles whose pixel pyramid, pruned through the tree from the root, reaches no leaf group, or only groups none of whose
 * triangles it can touch (rt_get_triangleless_paths() counts the latter).  Their node visits ARE executed (and
 * are not among the skipped root visits); what they skip is the traversal state machine.  For tests and profile notes. */
extern int rt_get_leafless_paths(u64 *out);
/* Of rt_get_leafless_paths(): the camera paths of TRIANGLE-LESS tiles, whose pyramid does reach leaf groups, but every triangle of
 * every reached group lies outside it (an all-zero padding slot counts as outside).  Their leaf visits are counted like their node
 * visits: one per group whose box the ray enters.  Paths of tiles that reach no leaf group are not among them. */
extern int rt_get_triangleless_paths(u64 *out);
/* Rays of the last rt_render_accumulate launch (single device) whose root visit the path kernel ran at the top of a traversal call,
 * in front of the traversal rounds, over the populated children of the root only (at most four of them; a root with more, a tree of
 * depth 0 and rays that are not NaN-free take the node block as before: 0 for such a frame).  The visits are executed and counted;
 * what they skip is a traversal round.  Equals rays - skipped root visits - leafless paths when every ray is NaN-free.  For tests. */
extern int rt_get_fused_root_visits(u64 *out);
/* Which form of the shade block's texture stage the last path-kernel launch of rt_render_accumulate / rt_render_accumulate_views /
 * rt_render_frame on the primary device ran: 1 = shared, one set of bilinear taps per hit for the material's four textures;
 * 0 = general, one set per texture; -1 = no launch yet.  A launch is shared when rt_materials_share_taps() holds for the resident
 * copy's material table and a material names a texture; decided at upload and again when rt_scene_touch() patches a material.
 * Same frames either way, bit for bit.  For tests and profile notes. */
extern int rt_get_shade_taps_form(void);
/* The predicate behind it, on a table a caller supplies: n_materials packed material rows of 36 words each -- words 12 .. 15 the
 * slot indices of the albedo, normal, metal-roughness and emission textures as int bits (< 0: none), words 20 + 4 k .. 23 + 4 k
 * the descriptor (offset, width, height, stride) of texture k as int bits.  1 when, in every row, all the textures the row names
 * have equal width, height and stride (no texture, one texture, an empty or NULL table: 1), else 0.  Touches no device. */
extern int rt_materials_share_taps(f32 const *mats, i32 n_materials);

/* Where the time of the last frame behind render_thread_proc / render / rt_render_frame went, in milliseconds.
 * Host clock: stamp = the per-frame scene check, upload = the scene upload when one was needed, enqueue = launching the
 * frame, total = the whole call.  HIP events on the frame's stream: gpu_prep = accumulator clear + the preparation kernel,
 * gpu_path = the path kernel, gpu_resolve, gpu_copy = device-to-host copy of the image.  A multi-device frame reports the
 * SLOWEST device's prep / path / resolve times, gpu_copy = that device's tile copy to the primary GPU, the largest stamp /
 * upload / enqueue time of any device, and gather_ms. */
typedef struct {
  f32 stamp_ms, upload_ms, enqueue_ms, gpu_prep_ms, gpu_path_ms, gpu_resolve_ms, gpu_copy_ms, total_ms;
  f32 verify_ms;       /* the full content check of the host scene, on the calling thread WHILE the GPU renders (rt_scene_touch) */
  f32 gather_ms;       /* multi-device frames: waiting for the other devices' tiles + untile + copy to the caller's pixels      */
  i32 n_devices;       /* GPUs the frame was spread over                                                                         */
  i32 slowest_device;  /* multi-device frames: the slot whose prep / path / resolve / copy times are reported above              */
} RT_Frame_Timing;
extern int rt_get_frame_timing(RT_Frame_Timing *out);

/* GPU time of the most recent path-tracing kernel launch in milliseconds
 * (HIP events on the launch stream); negative if none.  Synchronises. */
extern f32 rt_last_kernel_ms(void);

/* Mean GPU time per path-kernel launch over the launches since
 * rt_kernel_timing_reset() (at most the last 256); *n_launches (optional)
 * receives how many were averaged.  Synchronises. */
extern void rt_kernel_timing_reset(void);
extern f32  rt_kernel_timing_mean_ms(i32 *n_launches);

/* Numeric contract the library's kernels were built with (include/rt_math.h): 3 = explicit fused multiply-add + rt_pow24() in
 * the sRGB decode (the product), 2 = -DRT_MATH_V2 (round 4's arithmetic, librt_hip_v2.so), 1 = -DRT_MATH_NO_FMA (round 3's,
 * librt_hip_v1.so) -- the A/B partners.  The CPU checker must be built for the same one. */
extern int rt_math_contract(void);

/* Unit-level device entry points (rt_test_*), the wavefront pipeline switch and the kernel-generation knobs live in the
 * DIAGNOSTIC library only: include/rt_hip_diag.h, librt_hip_diag.so. */

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_H */
