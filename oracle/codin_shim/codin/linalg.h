/* codin/linalg.h -- stand-in, written for this project (see codin.h).  Vec2/Vec3/Vec4/Matrix_4x4 come from
 * include/rt_types.h.
 *
 * ASSUMPTIONS about the real codin, with the reference line that uses each.  Every formula is the one include/rt_math.h
 * gives the same operation under contract v1 (two roundings per multiply-add), sums left to right:
 *   L1  vec2(..) vec3(..) vec4(..) build a value from positional or designated components, missing ones zero;
 *       a trailing comma is allowed                                                   common.h:32-36, raytracer.c:169-173, driver.c:178,302
 *   L2  vec3_broadcast(s) = (s, s, s)                                                  driver.c:209,292
 *   L3  vec3_add / _sub / _mul component-wise, vec3_scale(v, s) = v * s, vec2_sub, vec2_mul the same
 *                                                                                    raytracer.c:168,537,544, scene.c:125, raytracer.c:733
 *   L4  vec3_dot = a.x*b.x + a.y*b.y + a.z*b.z, vec3_length2(v) = vec3_dot(v, v)       raytracer.c:517, common.h:37
 *   L5  vec3_cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)   scene.c:144, driver.c:157
 *   L6  vec3_normalize(v) = v * (1 / sqrt(v.v))                                        raytracer.c:526, scene.c:139-144
 *   L7  vec3_lerp(a, b, t) = a * (1 - t) + b * t per component                         driver.c:90-92,182,292, denoiser.c:121
 *   L8  vec3_reflect(v, n) = v - 2 (v.n) n, evaluated as n * -(2 (v.n)) + v            driver.c:324
 *   L9  vec2_fract(v) = v - floor(v) per component                                     driver.c:56
 *   L10 matrix_4x4_mul_vec4(m, v): row i = sum_j m.rows[i][j] * v[j]                    raytracer.c:612
 *   L11 Matrix_3x3 has rows[3][3]; matrix_3x3_from_basis(t, b, n) has t, b, n as COLUMNS; matrix_3x3_transpose;
 *       matrix_3x3_mul_vec3(m, v): row i = m.rows[i][0]*v.x + m.rows[i][1]*v.y + m.rows[i][2]*v.z
 *                                                                                    driver.c:383-398
 */
#ifndef CODIN_SHIM_LINALG_H
#define CODIN_SHIM_LINALG_H

#include "codin.h"

#define vec2(...) ((Vec2){ __VA_ARGS__ })
#define vec3(...) ((Vec3){ __VA_ARGS__ })
#define vec4(...) ((Vec4){ __VA_ARGS__ })

typedef struct { f32 rows[3][3]; } Matrix_3x3;

static inline Vec3 vec3_broadcast(f32 s) { return vec3(s, s, s); }
static inline Vec3 vec3_add(Vec3 a, Vec3 b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline Vec3 vec3_sub(Vec3 a, Vec3 b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline Vec3 vec3_mul(Vec3 a, Vec3 b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline Vec3 vec3_scale(Vec3 a, f32 s) { return vec3(a.x * s, a.y * s, a.z * s); }
static inline Vec2 vec2_sub(Vec2 a, Vec2 b) { return vec2(a.x - b.x, a.y - b.y); }
static inline Vec2 vec2_mul(Vec2 a, Vec2 b) { return vec2(a.x * b.x, a.y * b.y); }
static inline Vec2 vec2_fract(Vec2 a) { return vec2(rt_fractf(a.x), rt_fractf(a.y)); }
static inline f32  vec3_dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline f32  vec3_length2(Vec3 a) { return vec3_dot(a, a); }
static inline Vec3 vec3_cross(Vec3 a, Vec3 b) {
  return vec3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
static inline Vec3 vec3_normalize(Vec3 v) { return vec3_scale(v, 1.0f / rt_sqrtf(vec3_dot(v, v))); }
static inline Vec3 vec3_lerp(Vec3 a, Vec3 b, f32 t) {
  return vec3(a.x * (1.0f - t) + b.x * t, a.y * (1.0f - t) + b.y * t, a.z * (1.0f - t) + b.z * t);
}
static inline Vec3 vec3_reflect(Vec3 v, Vec3 n) {
  f32 k = -(2.0f * vec3_dot(v, n));
  return vec3(n.x * k + v.x, n.y * k + v.y, n.z * k + v.z);
}
static inline Vec4 matrix_4x4_mul_vec4(Matrix_4x4 m, Vec4 v) {
  Vec4 r;
  for (int i = 0; i < 4; i++)
    r.data[i] = m.rows[i][0] * v.x + m.rows[i][1] * v.y + m.rows[i][2] * v.z + m.rows[i][3] * v.w;
  return r;
}
static inline Matrix_3x3 matrix_3x3_from_basis(Vec3 t, Vec3 b, Vec3 n) {
  Matrix_3x3 m = { { { t.x, b.x, n.x }, { t.y, b.y, n.y }, { t.z, b.z, n.z } } };
  return m;
}
static inline Matrix_3x3 matrix_3x3_transpose(Matrix_3x3 m) {
  Matrix_3x3 r;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.rows[i][j] = m.rows[j][i];
  return r;
}
static inline Vec3 matrix_3x3_mul_vec3(Matrix_3x3 m, Vec3 v) {
  return vec3(m.rows[0][0] * v.x + m.rows[0][1] * v.y + m.rows[0][2] * v.z,
              m.rows[1][0] * v.x + m.rows[1][1] * v.y + m.rows[1][2] * v.z,
              m.rows[2][0] * v.x + m.rows[2][1] * v.y + m.rows[2][2] * v.z);
}

#endif
