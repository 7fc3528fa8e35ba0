/* codin/codin.h -- stand-in for the core header of the third-party library "codin", written for this project.
 * It lets the reference's own hot-path sources (common.h, scene.h/.c, raytracer.h/.c, denoiser.c and the shading
 * stretch of driver.c) compile unchanged, so that oracle/oracle.c can be compared with THEIR text (oracle/ref_harness.c,
 * `make -C oracle ref`).  Types and layouts come from include/rt_types.h: libref.so and the library share one Scene.
 *
 * ASSUMPTIONS about the real codin (the checklist for a maintainer who has it), with the reference line that uses each:
 *   A1  base types u8 byte i32 u32 i64 u64 isize f32 f64 rawptr uintptr bool          common.h:13-23, scene.c:37
 *   A2  `internal` = static, `thread_local` = C11 _Thread_local, `nil` = NULL, `loop` = for (;;)
 *                                                                                    common.h:13,31, scene.c:399
 *   A3  size_of / count_of / type_of = sizeof / array length / __typeof__            scene.h:63, denoiser.c:49,109
 *   A4  U32_MAX = 4294967295 (so (f32)U32_MAX == 2^32), F32_INFINITY = +inf          common.h:23, raytracer.c:17
 *   A5  Slice(T) = { T *data; isize len; }; IDX(s, i) = element i                     scene.h:44,87, common.h:10-11
 *   A6  for_range(i, a, b): isize i from a while i < b, step 1                         scene.h:105, raytracer.c:459
 *   A7  slice_iter_v(s, v, i, body): i = 0 .. len-1, v a COPY of element i; `break` and `continue` in the body act on
 *       that loop                                                                     scene.c:109,193,383, denoiser.c:111
 *   A8  slice_array(T, arr) = slice over a whole C array                              scene.c:383, denoiser.c:49
 *   A9  slice_end(s, n) = the first n elements, slice_start(s, n) = the rest          scene.c:341-342
 *   A10 slice_to_bytes(s) = the bytes of the elements                                 scene.c:27
 *   A11 min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b (second operand on NaN), clamp(x, lo, hi) =
 *       x < lo ? lo : (x > hi ? hi : x); usual arithmetic conversions, so a double literal makes the result double
 *                                                                                    scene.c:166-186, driver.c:246,275,331-333,368
 *   A12 assert(c) stops the program when c is false                                   scene.c:106-107,324
 *   A13 Allocator by value; mem_alloc_aligned(size, align, a) returns ZEROED memory wrapped in a result that
 *       unwrap_err() opens; slice_init(&s, n, a) allocates n ZEROED elements; mem_free(p, size, a); mem_copy = memcpy;
 *       `context.allocator` / `context.temp_allocator` exist; a request for 0 bytes
 *       returns a block that can take the first task (scene.c:268-274 with no node)  scene.c:43,84,102,268,422
 *   A14 the math wrappers sqrt_f32 pow_f32 sin_f32 cos_f32 atan2_f32 asin_f32 abs_f32 are the correctly named libm
 *       functions in single precision.  THIS STAND-IN maps them to include/rt_math.h under numeric contract v1
 *       (-DRT_MATH_NO_FMA), which removes libm as a source of difference from liboracle_v1.so (deviation D5 stays
 *       unpinned); pow_f32(x, 5) and pow_f32(x, 2) are the plain products of oracle.c (D5); asin_f32 clamps (D4)
 *                                                                                    common.h:39,84-91, scene.c:129, driver.c:99-100,120-125,205-214
 *   A15 PI is a double constant                                                       driver.c:96-97,119,214,238
 *   A16 the type name Writer is visible through codin.h / image.h / linalg.h / sync.h alone (its functions: io.h)
 *                                                                                    scene.h:3-6,99
 */
#ifndef CODIN_SHIM_CODIN_H
#define CODIN_SHIM_CODIN_H

#include "../../../include/rt_types.h"
#ifndef RT_MATH_NO_FMA
#error "the codin stand-in maps the math wrappers to rt_math.h under contract v1: compile with -DRT_MATH_NO_FMA"
#endif
#include "../../../include/rt_math.h"

#include <stdlib.h>
#include <string.h>

typedef uintptr_t uintptr;

#define internal     static
#define thread_local _Thread_local
#define nil          NULL
#define loop         for (;;)

#define size_of(x)  ((isize)sizeof(x))
#define count_of(a) ((isize)(sizeof(a) / sizeof((a)[0])))
#define type_of(x)  __typeof__(x)

#define U32_MAX      4294967295u
#define F32_INFINITY __builtin_inff()
#define PI           3.14159265358979323846

#define IDX(arr, i) (arr).data[(i)]

#define for_range(i, a, b) for (isize i = (a); i < (b); i += 1)
#define slice_iter_v(s, v, i, ...) \
  for (isize i = 0; i < (s).len; i += 1) { type_of((s).data[0]) v = (s).data[i]; __VA_ARGS__ }
#define slice_array(T, arr)  ((T){ .data = (arr), .len = count_of(arr) })
#define slice_end(s, n)      ((type_of(s)){ .data = (s).data, .len = (n) })
#define slice_start(s, n)    ((type_of(s)){ .data = (s).data + (n), .len = (s).len - (n) })
#define slice_to_bytes(s)    ((Byte_Slice){ .data = (byte *)(s).data, .len = (s).len * size_of((s).data[0]) })

#define min(a, b)         ((a) < (b) ? (a) : (b))
#define max(a, b)         ((a) > (b) ? (a) : (b))
#define clamp(x, lo, hi)  ((x) < (lo) ? (lo) : ((x) > (hi) ? (hi) : (x)))

/* defined by whoever hosts the reference's sources (oracle/ref_harness.c) */
extern void codin_shim_panic(char const *what, char const *file, int line) __attribute__((noreturn));
#define assert(c) ((c) ? (void)0 : codin_shim_panic(#c, __FILE__, __LINE__))

static inline rawptr codin_shim_alloc(isize size, isize align, Allocator a) {
  rawptr p = NULL;
  /* never less than one cache line: with <= 8 triangles the reference sizes its task array by the node count, 0, and then
   * writes task 0 (scene.c:268-274); the slack keeps that write inside the block */
  if (size < 64) size = 64;
  if (a.proc) p = a.proc(a.user, size, align);
  else if (posix_memalign(&p, (size_t)(align < 64 ? 64 : align), (size_t)size) != 0) p = NULL;
  if (!p) codin_shim_panic("out of memory", __FILE__, __LINE__);
  memset(p, 0, (size_t)size);
  return p;
}
#define mem_alloc_aligned(size, align, a) codin_shim_alloc((size), (align), (a))
#define unwrap_err(x)                     (x)
#define mem_free(p, size, a)              do { if (!(a).proc) free(p); } while (0)
#define mem_copy(dst, src, n)             memcpy((dst), (src), (size_t)(n))
#define slice_init(s, n, a) \
  do { (s)->len = (n); (s)->data = (type_of((s)->data))codin_shim_alloc((n) * size_of((s)->data[0]), 64, (a)); } while (0)

typedef struct { void (*proc)(rawptr user, Byte_Slice bytes); rawptr user; } Writer;

typedef struct { Allocator allocator, temp_allocator; } Codin_Shim_Context;
static Codin_Shim_Context const context = { { NULL, NULL }, { NULL, NULL } };

static inline f32 sqrt_f32(f32 x) { return rt_sqrtf(x); }
static inline f32 abs_f32(f32 x) { return rt_absf(x); }
static inline f32 pow_f32(f32 x, f32 y) {
  if (y == 2.0f) return x * x;
  if (y == 5.0f) return x * x * x * x * x;
  return rt_powf(x, y);
}
static inline f32 sin_f32(f32 x) { f32 s, c; rt_sincosf(x, &s, &c); return s; }
static inline f32 cos_f32(f32 x) { f32 s, c; rt_sincosf(x, &s, &c); return c; }
static inline f32 atan2_f32(f32 y, f32 x) { return rt_atan2f(y, x); }
static inline f32 asin_f32(f32 x) { return rt_asinf(x); }

#endif
