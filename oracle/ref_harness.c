/* ref_harness.c -- hosts the reference's OWN hot-path sources, compiled against the codin stand-in
 * (oracle/codin_shim/), and exports thin ref_* wrappers around their `internal` functions.  TEST INFRASTRUCTURE:
 * `make -C oracle ref` builds oracle/_ref/libref.so from $(REFERENCE_DIR); tests/test_reference_pin.py compares it with
 * liboracle_v1.so bit for bit.  Nothing of the reference is copied here: its files are #included from where they lie,
 * and the shading stretch of driver.c is cut into _ref/driver_shading.inc by the Makefile at build time.
 *
 * Compiled with -DRT_MATH_NO_FMA -ffp-contract=off -march=x86-64-v3 -DSIMD_WIDTH=8: the stand-in maps codin's math to
 * include/rt_math.h under numeric contract v1, so every expression of the reference is comparable with liboracle_v1.so.
 */
#include <setjmp.h>
#include <stdio.h>

#include "codin/codin.h"

#define REF_API __attribute__((visibility("default")))

/* assumption A12 (codin.h): a failed assert stops the program.  Here it unwinds to the wrapper that armed the
 * jump buffer, which reports the failure (ref_last_panic) instead of taking the test process down. */
static jmp_buf g_panic_jmp;
static int     g_panic_armed;
static char    g_panic_text[512];

void codin_shim_panic(char const *what, char const *file, int line) {
  snprintf(g_panic_text, sizeof g_panic_text, "%s (%s:%d)", what, file, line);
  if (g_panic_armed) longjmp(g_panic_jmp, 1);
  fprintf(stderr, "reference panic: %s\n", g_panic_text);
  abort();
}

#include "raytracer.c"
#include "scene.c"
#define luminance ref_denoiser_luminance      /* denoiser.c and driver.c each define their own `luminance` */
#include "denoiser.c"
#undef luminance
#define sample_texture(texture, uv) sample_texture_bilinear((texture), (uv))   /* the choice driver.c makes above the stretch */
#include "driver_shading.inc"

_Static_assert(sizeof(BVH_Node) == 192 && sizeof(Triangle) == 112 && sizeof(Triangle_AOS) == 112, "layouts of include/rt_scene.h");
_Static_assert(sizeof(PBR_Shader_Data) == 80 && sizeof(Hit) == 88, "layouts of include/rt_materials.h / rt_raytracer.h");

#define GUARDED(fail_value)                                   \
  codin_shim_n_threads = 0;                                   \
  g_panic_text[0] = 0;                                        \
  if (setjmp(g_panic_jmp)) { g_panic_armed = 0; codin_shim_n_threads = 0; return fail_value; } \
  g_panic_armed = 1;
#define UNGUARD() g_panic_armed = 0

REF_API char const *ref_last_panic(void) { return g_panic_text; }

REF_API f32 ref_min_f32x8(f32 const *vec, f32 epsilon, i32 *index) {
  return min_f32x8(_mm256_loadu_ps(vec), epsilon, index);
}

REF_API void ref_ray_aabbs_hit_8(Ray const *ray, f32 t_min, f32 t_max, BVH_Node const *node, f32 *distances) {
  Ray r = *ray;
  BVH_Node n;
  f32 out[8] __attribute__((aligned(32)));
  memcpy(&n, node, sizeof n);
  ray_aabbs_hit_8(&r, t_min, t_max, n.mins, n.maxs, out);
  memcpy(distances, out, sizeof out);
}

/* the leaf test loads with _mm256_load_ps: a group that does not lie on a 32-byte boundary is tested from an aligned copy */
REF_API i32 ref_ray_triangles_hit_8(Ray const *ray, Triangles const *triangles, isize offset, Hit *hit) {
  bool aligned = true;
  for (int k = 0; k < 3; k++) {
    aligned = aligned && ((uintptr)(triangles->x[k] + offset) % 32 == 0) && ((uintptr)(triangles->y[k] + offset) % 32 == 0) &&
              ((uintptr)(triangles->z[k] + offset) % 32 == 0);
  }
  if (aligned) return ray_triangles_hit_8(ray, triangles, offset, hit) ? 1 : 0;
  f32 buf[9][8] __attribute__((aligned(32)));
  Triangles t = *triangles;
  for (int k = 0; k < 3; k++) {
    memcpy(buf[k],     triangles->x[k] + offset, 32); t.x[k] = buf[k];
    memcpy(buf[3 + k], triangles->y[k] + offset, 32); t.y[k] = buf[3 + k];
    memcpy(buf[6 + k], triangles->z[k] + offset, 32); t.z[k] = buf[6 + k];
  }
  t.aos = triangles->aos + offset;
  return ray_triangles_hit_8(ray, &t, 0, hit) ? 1 : 0;
}

/* 0, or -1 when the scene has no node: ray_bvh_node_hit would read nodes[0] of an empty array (raytracer.c:451; deviation D3) */
REF_API i32 ref_ray_scene_hit(Ray const *ray, Scene const *scene, Hit *hit) {
  if (scene->bvh.nodes.len <= 0 || !scene->bvh.nodes.data) return -1;
  Ray r = *ray;
  ray_scene_hit(&r, scene, hit);
  return 0;
}

/* Batch closest hit in the shape of oracle_trace_rays: (t, triangle slot, u, v).  The reference's Hit names neither the
 * triangle nor its barycentrics, so the rays run over a copy of the scene whose Triangle_AOS payload is replaced:
 * shader.data = the slot number, tex_coords (0,0) (1,0) (0,1), which make raytracer.c:174-177 return (t1, t2) -- exactly
 * but for the sign of a zero.  The payload is not read before a hit is accepted, so traversal is the scene's own. */
REF_API i32 ref_trace_rays(Scene const *scene, i32 n, f32 const *rays, f32 *out_t, i32 *out_tri, f32 *out_uv) {
  if (scene->bvh.nodes.len <= 0 || !scene->bvh.nodes.data) return -1;
  Scene shadow = *scene;
  isize len = scene->triangles.len;
  shadow.triangles.aos = (Triangle_AOS *)calloc((size_t)len, sizeof(Triangle_AOS));
  if (!shadow.triangles.aos) return -2;
  for (isize i = 0; i < len; i++) {
    shadow.triangles.aos[i].shader.data    = (rawptr)(uintptr)(i + 1);
    shadow.triangles.aos[i].tex_coords_b.x = 1.0f;
    shadow.triangles.aos[i].tex_coords_c.y = 1.0f;
  }
  for (i32 i = 0; i < n; i++) {
    Ray r;
    memcpy(&r, rays + 6 * i, sizeof r);
    Hit hit = { .distance = F32_INFINITY };
    ray_scene_hit(&r, &shadow, &hit);
    out_t[i]          = hit.distance;
    out_tri[i]        = (i32)(uintptr)hit.shader.data - 1;
    out_uv[2 * i + 0] = hit.tex_coords.x;
    out_uv[2 * i + 1] = hit.tex_coords.y;
  }
  free(shadow.triangles.aos);
  return 0;
}

REF_API void ref_rand_f32_seq(u32 state, i32 n, f32 *out) {
  random_state = state;
  for (i32 i = 0; i < n; i++) out[i] = rand_f32();
}

/* cast_ray from a given ray and RNG state; 0, or -1 for a scene without nodes (see ref_ray_scene_hit) */
REF_API i32 ref_cast_ray(Scene const *scene, Ray const *ray, isize max_bounces, u32 *state, f32 rgb[3]) {
  if (scene->bvh.nodes.len <= 0 || !scene->bvh.nodes.data) return -1;
  random_state = *state;
  Color3 c = cast_ray(scene, *ray, max_bounces);
  *state = random_state;
  rgb[0] = c.r; rgb[1] = c.g; rgb[2] = c.b;
  return 0;
}

REF_API void ref_hash12x8(f32 const px[8], f32 const py[8], f32 out[8]) {
  Vec2x8 p = { _mm256_loadu_ps(px), _mm256_loadu_ps(py) };
  _mm256_storeu_ps(out, hash12x8(p));
}

/* mean radiance -> u8 in the ORDER of raytracer.c:702-716, composed HERE from the reference's clamp / linear_to_srgb (common.h:90-92):
 * the composition is this harness's restatement, not the reference's text.  The real tail of the pixel loop is pinned by the
 * frame comparison (ref_render); this entry point only pins linear_to_srgb and the conversion at every u8 step. */
REF_API u8 ref_encode_u8(f32 linear) {
  f32 c = clamp(linear, 0, 1);
  c = linear_to_srgb(c);
  c = c * 255.999f;
  return (u8)c;
}

/* render_thread_proc with ONE thread whose RNG state starts at `seed` (time_now(), raytracer.c:597) */
REF_API i32 ref_render(Scene *scene, Image const *image, isize samples, isize max_bounces, u32 seed) {
  if (scene->bvh.nodes.len <= 0 || !scene->bvh.nodes.data) return -1;
  GUARDED(-2)
  Rendering_Context ctx = { .image = *image, .scene = scene, .samples = samples, .max_bounces = max_bounces, .n_threads = 1 };
  codin_shim_time = (i64)seed;
  render_thread_proc(&ctx);
  UNGUARD();
  return ctx.n_threads == 0 ? 0 : -3;
}

REF_API i32 ref_lightmap_bake(Image const *lightmap, Scene const *scene, isize samples, u32 state) {
  if (scene->bvh.nodes.len <= 0 || !scene->bvh.nodes.data) return -1;
  GUARDED(-2)
  random_state = state;
  lightmap_bake(lightmap, scene, samples);
  UNGUARD();
  return 0;
}

REF_API i32 ref_denoise_image(Image const *src, Image const *dst) {
  GUARDED(-2)
  denoise_image(src, dst, 1);
  UNGUARD();
  return 0;
}

/* scene_init with the default allocator; 0, or -2 when an assertion of the reference failed (ref_last_panic) */
REF_API i32 ref_scene_init(Scene *scene, Triangle const *triangles, isize n) {
  GUARDED(-2)
  Triangle_Slice s = { .data = (Triangle *)triangles, .len = n };
  Allocator a = { NULL, NULL };
  scene_init(scene, s, a);
  UNGUARD();
  return 0;
}

REF_API void ref_scene_free(Scene *scene) {
  free(scene->bvh.nodes.data);
  free(scene->triangles.x[0]);
  memset(&scene->bvh, 0, sizeof scene->bvh);
  memset(&scene->triangles, 0, sizeof scene->triangles);
}

REF_API void ref_sample_texture_bilinear(Image const *texture, f32 u, f32 v, f32 rgb[3]) {
  Color3 c = sample_texture_bilinear(texture, vec2(u, v));
  rgb[0] = c.r; rgb[1] = c.g; rgb[2] = c.b;
}

REF_API void ref_sample_background(Image const *image, f32 const dir[3], f32 rgb[3]) {
  Color3 c = sample_background(image, vec3(dir[0], dir[1], dir[2]));
  rgb[0] = c.r; rgb[1] = c.g; rgb[2] = c.b;
}

/* the addresses a Scene for libref.so carries in shader.proc / background.proc */
REF_API rawptr ref_proc_address(i32 which) {
  switch (which) {
  case 0: return (rawptr)disney_shader_proc;
  case 1: return (rawptr)debug_shader_proc;
  case 2: return (rawptr)sample_background;
  default: return NULL;
  }
}

REF_API void ref_sample_disney_brdf(f32 roughness, f32 metalness, f32 sheen, f32 sheen_tint, f32 aniso2,
                                    f32 const base_color[3], f32 const in_dir[3], u32 *state, f32 out_dir[3], f32 brdf[4]) {
  Disney_BRDF_Data d = { .roughness = roughness, .metalness = metalness, .sheen = sheen, .sheen_tint = sheen_tint,
                         .anisotropic_strength2 = aniso2, .base_color = vec3(base_color[0], base_color[1], base_color[2]) };
  Vec3 o = vec3(0);
  random_state = *state;
  Vec4 b = sample_disney_BRDF(&d, vec3(in_dir[0], in_dir[1], in_dir[2]), &o);
  *state = random_state;
  out_dir[0] = o.x; out_dir[1] = o.y; out_dir[2] = o.z;
  brdf[0] = b.r; brdf[1] = b.g; brdf[2] = b.b; brdf[3] = b.a;
}

/* which: 0 = disney_shader_proc, 1 = debug_shader_proc; on explicit RNG state, output zeroed first (raytracer.c:533) */
REF_API void ref_shade(i32 which, PBR_Shader_Data const *data, Shader_Input const *in, u32 *state, Shader_Output *out) {
  random_state = *state;
  *out = (Shader_Output){0};
  if (which == 0) disney_shader_proc((rawptr)data, in, out);
  else            debug_shader_proc((rawptr)data, in, out);
  *state = random_state;
}
