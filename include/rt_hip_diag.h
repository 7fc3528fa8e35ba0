/* rt_hip_diag.h -- entry points of the DIAGNOSTIC library librt_hip_diag.so (make -C raytracing_c_amd/csrc diag,
 * -DRT_DIAG_VARIANTS) that the product library librt_hip.so does NOT export: unit-level device entry points for the parity
 * tests, the wavefront pipeline (built and measured in round 3, slower than the tile-stream kernel on every BASELINE
 * configuration: profiles/r03_experiments.md), the block ledger and the wave timeline of the path kernel.  The diagnostic
 * library links the product's kernel object, reads the RT_* experiment knobs and exports everything rt_hip.h declares as
 * well; tests load it beside the product library (raytracing_c_amd.native.diag).  Nothing here is part of the drop-in boundary.
 */
#ifndef RT_HIP_DIAG_H
#define RT_HIP_DIAG_H

#include "rt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Make this library recognise ANOTHER library's material / background tokens (rt_materials.h) in Shader.proc /
 * Background.proc: a test process that has the product library mapped as well builds its scenes once, with the product's
 * token addresses.  NULL keeps the current one. */
extern void rt_diag_set_tokens(void *disney_proc, void *debug_proc, void *background_proc);

/* Fault injection for the multi-device frame (tests/test_gpu_multi_device.py): no_peer != 0 = treat every device as if peer
 * access to the primary GPU had been refused (its tiles are staged through pinned host memory); failing_slot >= 0 = that
 * device slot fails its part of the next frames (-1 = none). */
extern void rt_diag_multi_fault(i32 no_peer, i32 failing_slot);

/* 0 (default): the tile-stream path kernel.  1: the wavefront pipeline (camera / shade / trace kernels joined by record
 * queues in HBM, csrc/rt_wavefront.hip): the same images and counters bit for bit, measured slower;
 * selectable for measurements.  rt_set_wavefront_capacity(): camera-ray hits its queues hold per pass (default 96 M). */
extern int  rt_set_pipeline(i32 pipeline);
extern i32  rt_get_pipeline(void);
extern void rt_set_wavefront_capacity(i64 records);

/* Block ledger of a -DRT_LEDGER build of the tile-stream kernel (tools/exp_ledger.py): out[0 .. n) = the LG_* slots of
 * csrc/rt_dev.hip.h of the last launch (all zero in other builds). */
extern int rt_get_ledger(u64 *out, i32 n);
/* RT_WAVE_TIMES set in the environment: per wave of the last launch (start tick, end tick, (tick of its last grab - start) << 16
 * | tiles it owned); ticks are 10 ns.  Returns the wave count (-1: no such launch). */
extern int rt_get_wave_times(u64 *out, i32 max_waves);
/* Device bytes the library's host side holds right now, on all devices: scene copies, launch states, workspaces, staging.  Exact
 * (counted at every allocation and release of the library's own), so a test can assert that a sequence leaks nothing. */
extern i64 rt_diag_device_bytes_live(void);
/* Gives back the staging the host-level calls keep on the primary device -- query, feature and guided-denoiser buffers -- the way
 * a device slot's teardown does (rt_set_devices remaps slots >= 1 only): waits for the device, then releases.  The next call
 * that needs staging allocates it again.  Not while a frame is in flight.  0 on success. */
extern int rt_diag_release_staging(void);
/* The primary device's cached copy of `scene`, NULL when there is none: the copy scene_refit_gpu deforms in place and
 * rt_scene_keep_geometry snapshots, for tests that run the device-level calls (rt_render_accumulate_features_motion with a sample
 * range) on a deformed mesh.  The cache keeps owning it: not to be released, and gone with the next re-upload; rt_set_camera()
 * gives it a camera. */
extern RT_Device_Scene *rt_diag_cached_scene(Scene const *scene);

/* ---- unit-level device entry points (parity tests call the same device
 * functions the render kernel uses) ------------------------------------------ */

/* rt_math.h on the GPU; op codes as oracle_math() (oracle/oracle.h).  Host
 * pointers. */
extern int rt_test_math(i32 op, i32 n, f32 const *x, f32 const *y, f32 *out);
/* the leaf blocks' four-instruction reciprocal against IEEE 1.0f / x over all 2^32 bit patterns: out[0] differing patterns
 * inside its domain (0 expected), out[1] patterns outside the domain, out[2] differing ones among those, out[3] first
 * differing pattern inside the domain + 1; the form without the fix-up that the leaf blocks use (rcp_leaf): out[4] finite non-zero
 * patterns below 2^102 that differ (0 expected), out[5] patterns 0 / infinity / NaN whose result is not NaN (0 expected) */
extern int rt_test_rcp_sweep(u64 out[6]);
/* the kernels' sRGB decode of a texture sample against rt_srgb_to_linear1() for every float in [0, 2] (and 4 M negative ones):
 * out[0] patterns compared, out[1] differing (0 expected), out[2] first differing pattern + 1 */
extern int rt_test_srgb_sweep(u64 out[3]);
/* the short forms the environment lookup and the normalisations use on the device (csrc/rt_dev.hip.h) against the rt_math.h
 * functions they stand for, both computed on the device.  which = 0 .. 5 compare all 2^32 bit patterns x:
 *   0 atan_pos_dev(x) / rt_atanf_pos(x)     1 asin_dev(x) / rt_asinf(x)     2 inv_sqrt_exact(x) / the reciprocal of rt_sqrtf(x)
 *   3, 4 the background's u, v of the angle x without tex_taps' negative-coordinate wrap / with it, over the angles the
 *        arctangent (|x| <= RT_PI or NaN) and the arcsine (|x| <= pi/2 or NaN) can return     5 sqrt_dev(x) / rt_sqrtf(x)
 * which = 6 compares atan2_dev(y, x) / rt_atan2f(y, x) on 2^26 pairs drawn from `seed`.
 * out[0] patterns or pairs compared, out[1] differing, a NaN equal to any NaN (0 expected), out[2] first differing pattern or
 * pair index + 1, out[3] differing when a NaN must have the same bits as well.
 * rt_test_math() takes the forms as ops 14 .. 18: atan2_dev(x, y), atan_pos_dev, asin_dev, inv_sqrt_exact, sqrt_dev. */
extern int rt_test_env_sweep(i32 which, u32 seed, u64 out[4]);
/* the tile-stream kernel's fixed-point conversion of a sample against rt_accum_quantize() over all 2^32 bit patterns:
 * out[0] differing patterns (0 expected), out[1] first differing pattern + 1 */
extern int rt_test_quantize_sweep(u64 out[2]);
/* rt_encode_u8() (rt_math.h: the last step of every image, rt_resolve's and the post passes') on the device over all 2^32 bit
 * patterns: out[k], k < 256, the lowest pattern in [0, 0x3F800000] -- the floats of [0, 1] -- that encodes to k (2^32 when none
 * does); out[256] patterns of that range, in ascending order, whose byte is below that of the pattern before (0 expected);
 * out[257] patterns in (1.0, +inf] that do not give 255, out[258] negative patterns, -0 and -inf included, that do not give 0,
 * out[259] NaN patterns that do not give 0 (0 expected each).  The CPU counterpart of the table is oracle_encode_steps(). */
extern int rt_test_encode_sweep(u64 out[260]);
/* the sky loop's sample reduction (group_sum3_u64, rt_dev.hip.h) on lanes a test chooses: three channels of n = n_waves x 64
 * values, channel c of lane i & 63 of wave i >> 6 at in[c * n + i]; a lane with valid[i] == 0 contributes 0.  out[c * n + i] = the
 * sum mod 2^64 of channel c over lane i's aligned group of `group` lanes (4, 16 or 64), which every lane of the group must hold. */
extern int rt_test_group_sum(i32 group, i32 n_waves, u64 const *in, u8 const *valid, u64 *out);
/* the group size the path kernel's sky loop is built with (RT_SKY_ADD_GROUP) */
extern int rt_test_sky_add_group(void);
/* the two orderings of a node block's eight children (node_order_keys, node_order_rank, rt_dev.hip.h) on distances a test chooses,
 * one lane per case: t_min[8 i + k] = the bit pattern of child k's entry distance, at least that of RT_EPSILON; cand[8 i + k] != 0 =
 * the child is a candidate.  out[3 i] = the order word from the 32-bit keys, out[3 i + 1] = the word from the rank sort, out[3 i + 2] =
 * 1 when the keys of the case are not exact, so that a node block takes the rank sort (its first word then means nothing) */
extern int rt_test_node_order(i32 n, u32 const *t_min, u8 const *cand, u32 *out);

/* Closest hit of n rays (host arrays, 6 f32 per ray: origin, direction) against
 * an uploaded scene: out_t[n], out_tri[n] (-1 = miss), out_uv[2n]. */
extern int rt_test_trace(RT_Device_Scene *dscene, i32 n, f32 const *rays,
                         f32 *out_t, i32 *out_tri, f32 *out_uv);

/* The same through the PRODUCTION traversal: traversal_blocks() (csrc/rt_dev.hip.h) -- the NODE / LEAF / pop code the path
 * kernels run -- in the path kernel's launch geometry (16-wave workgroups, tree in LDS), lanes refilled from the ray list as
 * they finish so that blocks mix rays at different depths as a frame does.
 *   pyramid    NULL, or 19 floats: 4 outward plane normals at [4 q .. 4 q + 2], the rays' common origin at [16 .. 18]; every
 *              ray then counts as a camera ray of one tile and node blocks take the pyramid-culled form (node_enter_few)
 *              where the path kernel would.  The caller guarantees origin and planes hold for every ray.
 *   exit_lanes 1 .. 64: finished lanes that end a round of blocks (the path kernel uses 48)
 *   mode       0 = the kernel instance a frame of this scene would use, 1 = IEEE division in the leaf blocks,
 *              2 = nodes through L1 / L2 instead of the LDS copy
 *   visits     [0] += 8-box tests (raytracer.c:452), [1] += 8-triangle tests (raytracer.c:476) */
extern int rt_test_trace_stream(RT_Device_Scene *dscene, i32 n, f32 const *rays, f32 const *pyramid, i32 exit_lanes, i32 mode,
                                f32 *out_t, i32 *out_tri, f32 *out_uv, u64 visits[2]);

/* The visiting order the per-launch preparation kernel derives from per-tile costs (rays a tile needed in the previous
 * launch of the same view): order[0 .. n_tiles) = a permutation of the tiles, most expensive cost bucket first. */
extern int rt_test_tile_order(i32 n_tiles, u32 const *cost, u32 *order);

/* Bilinear fetch (driver.c:49-93) of n (u,v) pairs on texture `tex` of the
 * uploaded scene (index in upload order; -1 = background image). */
extern int rt_test_texture(RT_Device_Scene *dscene, i32 tex, i32 n, f32 const *uv, f32 *out_rgb);

/* ---- the shade block, item by item (tests/test_gpu_shade.py; the CPU counterparts are oracle_disney_shade, oracle_debug_shade,
 * oracle_sample_disney_brdf, oracle_sample_background and oracle_primary_ray of oracle/oracle.h).  Host arrays. */

#define RT_TEST_SHARED_TAPS 4      /* mode bit of rt_test_shade / rt_test_shade_hit */
/* shade() -- disney_shader_proc / debug_shader_proc, driver.c:350-418 -- on n inputs a test chooses.
 *   mode      0 = shade<ShadeParams>, 1 = shade<ShadeParamsLds>: the path kernel's instance, the sRGB scale table in LDS;
 *             either + RT_TEST_SHARED_TAPS: the form with ONE set of bilinear taps per item (what the path kernel runs on a scene
 *             whose materials' textures agree in size, rt_get_shade_taps_form); refused on a scene where
 *             rt_materials_share_taps() does not hold
 *   tri[n]    triangle slot of the uploaded scene whose MATERIAL is evaluated: float 3 of its 28-float record, as shade_hit()
 *             reads it.  Nothing else of the triangle is used.
 *   in        14 floats per item: direction, normal, tangent, bitangent (3 each), texture coordinates (2, finite)
 *   state_in  RNG state per item; state_out[n] the state afterwards
 *   out       9 floats per item: outgoing direction, tint, emission; terminate[n] 0 / 1
 *   textured  per item the increment of the `textured` counter (RT_Counters)
 * LANE LAYOUT, part of the contract: item i is lane i & 63 of wave i >> 6, and n need not be a multiple of 64 (the last wave
 * is partial).  A wave whose items all name one material reads the record through the scalar cache, any other wave through
 * vector loads: the caller decides which by the order of its items. */
extern int rt_test_shade(RT_Device_Scene *dscene, i32 mode, i32 n, i32 const *tri, f32 const *in, u32 const *state_in,
                         f32 *out, u32 *state_out, i32 *terminate, i32 *textured);
/* ONE PATH STEP on hits a test chooses: shade_hit() -- raytracer.c:515-552 and the `for` of :510: face test, the surface at the
 * hit (surface_at), shade(), carried tint and emission, the next origin, the bounce count.  CPU counterpart: oracle_fill_hit +
 * oracle_path_step (tests/test_gpu_shade_hit.py).
 *   mode        0 = shade_hit<ShadeParams> (the wavefront shade kernel's), 1 = <ShadeParamsLds> (the path kernel's), 2 =
 *               <RT_KParams> (cast_ray_lane's, the lightmap); 0 or 1 + RT_TEST_SHARED_TAPS as for rt_test_shade
 *   max_bounces what the step's exhaustion rule compares with
 *   tri[n]      triangle slot of the hit; hit = 3 floats per item: t, u, v; ray = 6: origin, direction; carry = 6: tint, emission;
 *               state_in[n] the RNG state, bounce_in[n] the bounce count before the step
 *   out         15 floats per item: origin, direction, tint, emission as they stand afterwards, radiance (-1, -2, -3 where the
 *               step did not write it)
 *   out_words   5 words per item: RNG state, bounce, done (0 / 1), the increments of the `shades` and `textured` counters
 * Refused with a message: a slot outside the scene or without a triangle, vertex texture coordinates that are not finite, and
 * barycentrics that make the interpolated texture coordinates non-finite.  Everything else -- NaN directions, zero normals,
 * infinite distances -- is the function's business.  LANE LAYOUT as rt_test_shade: item i is lane i & 63 of wave i >> 6, so the
 * order of the items decides which lanes are inside shade_hit()'s `else` when shade() takes its ballot. */
extern int rt_test_shade_hit(RT_Device_Scene *dscene, i32 mode, i32 max_bounces, i32 n, i32 const *tri, f32 const *hit, f32 const *ray,
                             f32 const *carry, u32 const *state_in, i32 const *bounce_in, f32 *out, u32 *out_words);
/* feature_hit<ShadeParamsLds>() (rt_features.hip: the feature kernel's copy of the face test and the pass-through) on the same
 * kind of item.  out = 12 floats per item: origin afterwards, albedo, normal, position (zero on a back face); flag[n] = what it
 * returned (1 = a feature hit, 0 = passed through).  Refuses what rt_test_shade_hit refuses. */
extern int rt_test_feature_hit(RT_Device_Scene *dscene, i32 n, i32 const *tri, f32 const *hit, f32 const *ray, f32 *out, i32 *flag);
/* sample_disney() (driver.c:287-348) on raw parameters: params = 8 floats per item (roughness, metalness, sheen, sheen_tint,
 * aniso2, base colour), in_dir = 3; out_dir = 3, brdf = 4 per item (rgb and the weight-pdf; <= 0 ends the path) */
extern int rt_test_brdf(i32 n, f32 const *params, f32 const *in_dir, u32 const *state_in, f32 *out_dir, f32 *brdf, u32 *state_out);
#define RT_TEST_BG_IMAGE 8         /* mode bit of rt_test_background */
/* background_lookup() (driver.c:95-104) of n directions (3 floats each) on the scene's environment image.
 *   mode      0 = <ShadeParams>, 1 = <ShadeParamsLds>, on the RGBA8 texel pool; either + RT_TEST_BG_IMAGE: background_lookup_image()
 *             on the float copy of the background, what the path kernel's batch loop runs
 * Any float is taken: both forms turn a coordinate that is NaN into texel 0 and a NaN colour, and no direction makes either read
 * outside the image.  The oracle's function is a partner for finite directions only (it converts a NaN coordinate another way). */
extern int rt_test_background(RT_Device_Scene *dscene, i32 mode, i32 n, f32 const *dir, f32 *rgb);
/* primary_ray() (raytracer.c:641-694) of n (x, y, sample) triples of a width x height frame, with the frame constants the host
 * computes for a real frame (1 / width, 1 / height, width / height); rays = 6 floats per item: origin, direction */
extern int rt_test_primary_ray(Camera const *camera, i32 width, i32 height, i32 n, i32 const *xys, f32 *rays);

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_DIAG_H */
