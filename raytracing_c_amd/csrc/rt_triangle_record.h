/* rt_triangle_record.h -- what ONE builder-input Triangle becomes in a slot of the triangle block, and its padded bounds.
 *
 * The one definition of the per-triangle arithmetic of triangles_insert (reference scene.c:105-155) and of
 * aabb_triangle (scene.c:165-178), for every unit that writes a slot: rt_scene_build.c and rt_scene_refit.c on the
 * host, rt_build.hip and rt_refit.hip on the device (RT_FN is __host__ __device__ under hipcc).  All of them are
 * built with -ffp-contract=off, so the same fp32 operations round the same way everywhere.
 */
#ifndef RT_TRIANGLE_RECORD_H
#define RT_TRIANGLE_RECORD_H

#include "../../include/rt_scene.h"
#include "../../include/rt_math.h"

/* scene.c:118-152: the face normal and the UV-aligned tangent frame of `t`, its vertex normals, UVs and Shader */
RT_FN void rt_triangle_record(Triangle const *t, Triangle_AOS *aos) {
  rt_v3 p0 = rt_v3_make(t->positions[0].x, t->positions[0].y, t->positions[0].z);
  rt_v3 p1 = rt_v3_make(t->positions[1].x, t->positions[1].y, t->positions[1].z);
  rt_v3 p2 = rt_v3_make(t->positions[2].x, t->positions[2].y, t->positions[2].z);
  rt_v3 edge1 = rt_v3_sub(p1, p0);
  rt_v3 edge2 = rt_v3_sub(p2, p0);

  f32 du1 = t->tex_coords[1].x - t->tex_coords[0].x, dv1 = t->tex_coords[1].y - t->tex_coords[0].y;
  f32 du2 = t->tex_coords[2].x - t->tex_coords[0].x, dv2 = t->tex_coords[2].y - t->tex_coords[0].y;

  f32 d = du1 * dv2 - du2 * dv1;
  if (rt_absf(d) < 0.0001f) d = (d < 0) ? -0.0001f : 0.0001f;
  f32 inv_d = 1.0f / d;

  rt_v3 tangent   = rt_v3_normalize_plain(rt_v3_scale(rt_v3_sub(rt_v3_scale(edge1, dv2), rt_v3_scale(edge2, dv1)), inv_d));
  rt_v3 bitangent = rt_v3_normalize_plain(rt_v3_scale(rt_v3_sub(rt_v3_scale(edge2, du1), rt_v3_scale(edge1, du2)), inv_d));
  rt_v3 normal    = rt_v3_normalize_plain(rt_v3_cross_plain(edge1, edge2));

  aos->shader       = t->shader;
  aos->normal.x     = normal.x;    aos->normal.y    = normal.y;    aos->normal.z    = normal.z;
  aos->normal_a     = t->normals[0];
  aos->normal_b     = t->normals[1];
  aos->normal_c     = t->normals[2];
  aos->tex_coords_a = t->tex_coords[0];
  aos->tex_coords_b = t->tex_coords[1];
  aos->tex_coords_c = t->tex_coords[2];
  aos->tangent.x    = tangent.x;   aos->tangent.y   = tangent.y;   aos->tangent.z   = tangent.z;
  aos->bitangent.x  = bitangent.x; aos->bitangent.y = bitangent.y; aos->bitangent.z = bitangent.z;
}

/* slot `slot` of a triangle block of `len` slots that starts at x0: the nine SoA coordinates (x[k] = x0 + len * k,
 * y[k] = x0 + len * (3 + k), z[k] = x0 + len * (6 + k), scene.c:84-98) */
RT_FN void rt_triangle_coordinates(Triangle const *t, f32 *x0, isize len, isize slot) {
  for (int k = 0; k < 3; k++) {
    x0[len * (0 + k) + slot] = t->positions[k].x;
    x0[len * (3 + k) + slot] = t->positions[k].y;
    x0[len * (6 + k) + slot] = t->positions[k].z;
  }
}

/* scene.c:165-178: min3 - EPSILON, max3 + EPSILON per axis, with these comparisons */
RT_FN f32 rt_min3f(f32 a, f32 b, f32 c) { f32 m = b < c ? b : c; return a < m ? a : m; }
RT_FN f32 rt_max3f(f32 a, f32 b, f32 c) { f32 m = b > c ? b : c; return a > m ? a : m; }

RT_FN void rt_triangle_bounds(Triangle const *t, f32 lo[3], f32 hi[3]) {
  for (int ax = 0; ax < 3; ax++) {
    lo[ax] = rt_min3f(t->positions[0].data[ax], t->positions[1].data[ax], t->positions[2].data[ax]) - RT_EPSILON;
    hi[ax] = rt_max3f(t->positions[0].data[ax], t->positions[1].data[ax], t->positions[2].data[ax]) + RT_EPSILON;
  }
}

#endif /* RT_TRIANGLE_RECORD_H */
