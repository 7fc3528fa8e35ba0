/* oracle.h -- CPU restatement of the reference render path.  TEST INFRASTRUCTURE.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load liboracle.so; nothing under raytracing_c_amd/ links, imports or calls it.
 *
 * PARITY: PINNED TO THE REFERENCE'S OWN TEXT, compiled against a codin stand-in.  The reference includes the absent,
 * unversioned third-party library "codin" everywhere (common.h:3-4, raytracer.c:3-7, scene.c:1-6), but its hot path uses
 * only about forty codin names; oracle/codin_shim/ restates those (each header lists its assumptions about the real codin
 * with the reference lines that use them), and `make -C oracle ref` compiles raytracer.c, scene.c, denoiser.c and the
 * shading stretch of driver.c UNCHANGED into oracle/_ref/libref.so (oracle/ref_harness.c).  tests/test_reference_pin.py
 * compares this oracle with it bit for bit under numeric contract v1 -- box and leaf tests, traversal, builder, sampler,
 * background, BRDF, shader procs, cast_ray, whole frames, denoiser, whole lightmaps -- and tests/golden/ref/ carries the
 * reference's hits and built scenes to the GPU (tests/test_gpu_reference_pin.py).  What STAYS UNPINNED: the semantics of
 * the real codin (the stand-in's assumption lists are the checklist for a maintainer who has it), libm (D5), and the
 * non-literal deviations D1, D2 and D6, which ORACLE_LITERAL switches off for the comparison.
 * The oracle is a restatement, function by function, of common.h:13-92, raytracer.c:15-32,84-230,443-720 and
 * driver.c:49-104,118-418, with these documented deviations:
 *   D1 per-path RNG seeding rt_path_seed() instead of wall clock per thread;
 *   D2 exact 1/sqrt instead of _mm256_rsqrt_ps for primary directions;
 *   D3 depth-0 BVH tests leaf group 0 instead of reading nodes[0];
 *   D4 asin argument clamped to [-1,1] in the background lookup;
 *   D5 libm / codin math replaced by include/rt_math.h: no IMPLICIT contraction anywhere, the explicit fused multiply-adds
 *      of numeric contract v2, and since contract v3 (round 5) rt_pow24() as the power of the sRGB decode (common.h:84);
 *      -DRT_MATH_NO_FMA / -DRT_MATH_V2 build the checker under contracts v1 / v2 (liboracle_v1.so, liboracle_v2.so);
 *   D6 default accumulation is order-free 32.32 fixed point (rt_math.h);
 *      ORACLE_ACCUM_F32 reproduces the reference's fp32 running sum;
 *   D7 (builder, rt_scene_build.c) stable merge sort, early-leaf chain;
 *   D8 expressions that the reference evaluates in DOUBLE because of unsuffixed literals are evaluated
 *      stepwise in fp32: driver.c:220 `(2.0 * NDotV) / (...)` (smith_G), driver.c:238 `2.0 * PI * rand_f32()`,
 *      :242 `(1.0 - s) * sqrt_f32(1.0 - t1 * t1) + s * t2` (one rounding in the reference, three here),
 *      :246 `max(0.0, 1.0 - t1 * t1 - t2 * t2)`, driver.c:119 `rand_f32() * 2 * PI` and :96-97 `1.0f / PI`
 *      (if codin's PI is a double), likewise driver.c:214 `a2 / (PI * pow_f32(..))`, :263 `a * b / PI` and :313 `NoL / PI`,
 *      common.h:37 `1.0 / sqrt_f32(lensq)` (lightmap only).  driver.c:133 `2.0`,
 *      :241 `0.5 * (1.0 + Vh.z)`, :416 `0.5` and common.h:84 `2.4` give the same f32 either way.  The GPU kernels
 *      have no fp64 on the path; the difference is below 1 ulp per expression.
 *   D9 (contract v2 on) the slab distances of a NaN-free ray whose origin components are all below 256 are
 *      fma(plane, inv, -(o * inv)) instead of (plane - o) * inv (raytracer.c:203-208): rt_slab_fast(), rt_math.h, shared
 *      with the kernels; the origin bound (round 5) keeps the fused form's plane placement error below 0.153 EPSILON.
 *   D10 (lightmap) a texel is stored as (u8) of the mean clamped to [0, 255], NaN as 0; the reference converts the raw
 *      float (raytracer.c:777-779), which C leaves undefined outside [0, 256).  Inside that range the two are the same
 *      conversion, and tests/test_reference_pin.py compares whole lightmaps there.
 *   D11 (u8 store) rt_encode_u8()'s clamp is written so that NaN fails it (v > 0 ? v : 0, then the upper bound, as
 *      rt_accum_quantize() clamps): a NaN mean encodes to 0.  The reference clamps with comparisons NaN passes
 *      (raytracer.c:700-716), its power and sRGB formula turn NaN into -0.055, and the conversion of -14.08f to u8 is
 *      undefined in C (242 from gcc here, 0 from a saturating conversion).  A rendered frame's fixed-point sums are
 *      never NaN; the post passes take f32 planes from the host, where it can be.  Every other float keeps its byte:
 *      tests/golden/encode_u8_steps.npz is the step table of the function before the change, per numeric contract.
 *
 * ORACLE_LITERAL (Oracle_Config.literal = 1) switches D1, D2, D6 and D8 back to the reference's literal semantics:
 * ONE thread whose RNG state is seeded once (frame seed in place of time_now(), raytracer.c:597) and runs on across
 * pixels in chunk order, `_mm256_rsqrt_ps` for the primary directions (:663), fp32 running sum in sample order
 * (:695-700), double intermediates at the D8 sites.  In this mode the oracle equals libref.so bit for bit, whole frames
 * included (tests/test_reference_pin.py); tests/test_oracle_literal.py checks that it and the default oracle are the same estimator:
 * per-block means agree within the Monte-Carlo noise, with no bias.
 */
#ifndef ORACLE_H
#define ORACLE_H

#include "../include/rt_raytracer.h"
#include "../include/rt_materials.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  u64 paths;          /* camera paths started                                  */
  u64 rays;           /* ray_scene_hit calls (raytracer.c:514)                 */
  u64 node_visits;    /* ray_aabbs_hit_8 calls (raytracer.c:452)               */
  u64 leaf_visits;    /* ray_triangles_hit_8 calls (raytracer.c:476)           */
  u64 shades;         /* shader.proc calls (raytracer.c:535)                   */
  u64 backgrounds;    /* background.proc calls (raytracer.c:554)               */
  u64 textured;       /* shades whose material has at least one texture        */
} Oracle_Counters;

enum { ORACLE_ACCUM_FIXED = 0, ORACLE_ACCUM_F32 = 1 };

typedef struct {
  /* Addresses that identify the built-in materials inside the Scene (the
   * product's exported tokens, or the oracle's own functions).  A shader.proc
   * that matches none of them is CALLED, as the reference would. */
  Shader_Proc     disney_proc;
  Shader_Proc     debug_proc;
  Background_Proc background_proc;
  u32             seed;
  i32             accum_mode;      /* ORACLE_ACCUM_*                            */
  i32             n_threads;       /* >= 1                                      */
  /* pixel window rendered: [x0,x1) x [y0,y1); zeros = whole image             */
  i32             x0, y0, x1, y1;
  /* only samples [sample0, sample0+sample_count) of each pixel are traced;
   * sample_count == 0 = all.  `samples` still names the pixel's total for
   * the RNG stream and the final mean.                                        */
  i32             sample0, sample_count;
  i32             literal;         /* 1 = ORACLE_LITERAL (see the header comment)  */
} Oracle_Config;

/* Renders ctx-like arguments with the reference's semantics.
 *   image   : u8 output (may be NULL), written as raytracer.c:714-716
 *   linear  : optional W*H*3 f32, mean radiance before clamp/sRGB
 *   accum   : optional W*H*3 u64 fixed-point sums (ORACLE_ACCUM_FIXED only)
 * Returns 0, or -1 on invalid arguments. */
int oracle_render(Scene const *scene, Image const *image, isize samples, isize max_bounces,
                  Oracle_Config const *config, f32 *linear, u64 *accum, Oracle_Counters *counters);

/* Traces one camera path and returns its radiance (raytracer.c:505-558 +
 * primary ray of :641-694) */
void oracle_trace_path(Scene const *scene, Oracle_Config const *config, i32 width, i32 height,
                       i32 x, i32 y, i32 sample, i32 samples, i32 max_bounces, f32 rgb[3]);

/* ---- unit-level entry points for known-answer tests ---------------------- */
void oracle_rand_u32_seq(u32 state, i32 n, u32 *out);                        /* common.h:15-20 */
void oracle_rand_f32_seq(u32 state, i32 n, f32 *out);                        /* common.h:22-24 */
f32  oracle_hash12(f32 px, f32 py);                                          /* raytracer.c:584-594 */
void oracle_ray_aabbs_hit_8(Ray const *ray, f32 t_min, f32 t_max, BVH_Node const *node, f32 *distances); /* raytracer.c:190-230 */
bool oracle_ray_triangles_hit_8(Ray const *ray, Triangles const *tris, isize offset, Hit *hit, i32 *lane); /* raytracer.c:84-188 */
void oracle_ray_scene_hit(Ray const *ray, Scene const *scene, Hit *hit, i32 *triangle);                     /* raytracer.c:443-503 */
/* batch closest hit: out_uv = barycentrics (t1, t2) of the accepted triangle (raytracer.c:164-165) */
void oracle_trace_rays(Scene const *scene, i32 n, f32 const *rays, f32 *out_t, i32 *out_tri, f32 *out_uv);
/* ... and the node / leaf visits they cost in total: visits[0] = ray_aabbs_hit_8 calls, visits[1] = ray_triangles_hit_8 calls */
void oracle_trace_rays_counted(Scene const *scene, i32 n, f32 const *rays, f32 *out_t, i32 *out_tri, f32 *out_uv, u64 visits[2]);
void oracle_sample_texture_bilinear(Image const *texture, f32 u, f32 v, f32 rgb[3]);                        /* driver.c:49-93 */
void oracle_sample_background(Image const *image, f32 const dir[3], f32 rgb[3]);                            /* driver.c:95-104 */
/* driver.c:287-348: returns brdf rgba, writes out_dir; *state is the RNG state */
void oracle_sample_disney_brdf(f32 roughness, f32 metalness, f32 sheen, f32 sheen_tint, f32 aniso2,
                               f32 const base_color[3], f32 const in_dir[3], u32 *state, f32 out_dir[3], f32 brdf[4]);
/* driver.c:350-409 on explicit state */
void oracle_disney_shade(PBR_Shader_Data const *data, Shader_Input const *in, u32 *state, Shader_Output *out);
/* rt_math.h wrappers: op 0 log,1 exp,2 pow(x,y),3 sin,4 cos,5 atan2(x=y,y=x),6 asin,7 srgb_to_linear,8 linear_to_srgb,9 sqrt, 10 1/x */
void oracle_math(i32 op, i32 n, f32 const *x, f32 const *y, f32 *out);
u8   oracle_encode_u8(f32 linear);
void oracle_encode_u8_array(isize n, f32 const *linear, u8 *out);
/* rt_encode_u8() on every float of [0, 1] -- bit patterns 0 .. 0x3F800000 -- in ascending order, on n_threads threads:
 * first[k] = the lowest pattern that encodes to k (0xFFFFFFFF: none), *descents = patterns whose byte is below that of the
 * pattern before.  Returns how many of the 256 bytes occur, -1 on NULL.  With no descent and all 256 present the table IS
 * the function on [0, 1]. */
int  oracle_encode_steps(u32 first[256], u64 *descents, i32 n_threads);
/* test-only: 1 = the calling thread's unit-level entry points evaluate the D8 sites as ORACLE_LITERAL does (they default
 * to 0, and oracle_render sets 0 again); returns the previous mode */
int  oracle_set_literal(int on);
/* raytracer.c:505-558 from a given ray and RNG state, in the mode oracle_set_literal selected */
void oracle_cast_ray(Scene const *scene, Oracle_Config const *config, Ray const *ray, isize max_bounces, u32 *state, f32 rgb[3]);
/* raytracer.c:160-186: the fill of `Hit` for a hit the caller names: triangle index, distance t and barycentrics (u, v) =
 * (t1, t2); the code ray_triangles_hit_8 runs for the hit it accepts */
void oracle_fill_hit(Scene const *scene, Ray const *ray, f32 t, i32 triangle, f32 u, f32 v, Hit *out);
/* raytracer.c:515-551 + the `for` of :510: ONE iteration of cast_ray's loop for a ray whose closest hit is `hit` (the very
 * function cast_ray calls), then the bounce increment and the exhaustion rule.  ray, tint, emission, *state (the RNG) and
 * *bounce are carried in and out; *done = 1 and radiance = emission when the shader terminated or *bounce reached
 * max_bounces, else *done = 0 and radiance is left alone.  counters = { shades, textured } added by this step. */
void oracle_path_step(Scene const *scene, Oracle_Config const *config, Ray *ray, Hit const *hit, f32 tint[3], f32 emission[3],
                      u32 *state, i32 *bounce, isize max_bounces, i32 *done, f32 radiance[3], u64 counters[2]);
/* driver.c:411-418 */
void oracle_debug_shade(PBR_Shader_Data const *data, Shader_Input const *in, Shader_Output *out);
/* raytracer.c:641-694: the primary ray of (x, y, sample) of a width x height frame, out = position, direction; always in the
 * default (non-literal) mode */
void oracle_primary_ray(Camera const *camera, i32 width, i32 height, i32 x, i32 y, i32 sample, f32 out[6]);

/* raytracer.c:722-784: UV-space light baking.  Texels covered by several triangles
 * keep the LAST triangle's value (the reference's loop order); texels outside the image are skipped (the
 * reference would write out of bounds); per-texel RNG seeding rt_path_seed(seed, x + y*width, triangle)
 * replaces the reference's running thread-local stream (D1; config->literal = 1 restores the ONE running stream,
 * seeded with config->seed, and the double intermediates of D8); the f32 -> u8 store is the reference's plain
 * conversion (no *255), clamped to [0, 255] (D10). */
void oracle_lightmap_bake(Image const *lightmap, Scene const *scene, isize samples, Oracle_Config const *config);

/* denoiser.c:51-153: 3x3 luminance-sorted median blended by neighbourhood noisiness; src and dst are
 * u8 images of equal size (components >= 3 are filtered, like min(components, 3) in denoiser.c:24,36) */
void oracle_denoise_image(Image const *src, Image const *dst);

/* The reference's 8-wide AVX2 forms of min_f32x8 / ray_triangles_hit_8 / ray_aabbs_hit_8 (raytracer.c:15-32,84-230) are the
 * default when the checker is compiled for AVX2 (+ FMA under numeric contract v2); the scalar restatement stays selectable
 * and must give the same bits (tests/test_oracle_simd.py).  oracle_set_simd returns the mode now in force; process-wide. */
int oracle_have_avx2(void);
int oracle_set_simd(int on);

#ifdef __cplusplus
}
#endif

#endif /* ORACLE_H */
