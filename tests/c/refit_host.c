/* scene_refit / rt_scene_slot_map under AddressSanitizer + UBSan (CPU only; tests/test_refit_cpu.py builds and runs this,
 * linked with rt_scene_build.c and rt_scene_refit.c alone): build -> map -> refit -> refit back -> the rejections, for soups
 * with duplicates that hit depth 0, one node, an early-leaf chain and three levels, from both builders. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rt_scene.h"

static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s; }
static float frand(uint32_t *s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

static void token_shader(rawptr d, Shader_Input const *i, Shader_Output *o) { (void)d; (void)i; (void)o; }

static byte *snapshot(Scene const *scene, size_t *bytes) {
  size_t nb = (size_t)scene->bvh.nodes.len * sizeof(BVH_Node), tb = (size_t)TRIANGLES_ALLOCATION_SIZE(scene->triangles.len);
  byte *p = (byte *)malloc(nb + tb);
  if (nb) memcpy(p, scene->bvh.nodes.data, nb);
  memcpy(p + nb, scene->triangles.x[0], tb);
  *bytes = nb + tb;
  return p;
}

static int same(Scene const *scene, byte const *snap, size_t bytes) {
  size_t n = 0;
  byte *now = snapshot(scene, &n);
  int eq = n == bytes && memcmp(now, snap, n) == 0;
  free(now);
  return eq;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "n=%d sah=%d: %s failed (line %d)\n", n, sah, #c, __LINE__); return 1; } } while (0)

static int run_case(int n, int sah, uint32_t seed) {
  uint32_t s = seed;
  static int materials[2];
  Triangle *tris = (Triangle *)calloc((size_t)n + 1, sizeof *tris), *moved = (Triangle *)calloc((size_t)n + 1, sizeof *moved);
  for (int i = 0; i < n; i++) {
    float cx = frand(&s) * 4 - 2, cy = frand(&s) * 4 - 2, cz = frand(&s) * 4 - 2;
    for (int k = 0; k < 3; k++) {
      tris[i].positions[k].x = cx + frand(&s) * 0.5f;
      tris[i].positions[k].y = cy + frand(&s) * 0.5f;
      tris[i].positions[k].z = cz + frand(&s) * 0.5f;
      tris[i].normals[k].x = frand(&s); tris[i].normals[k].y = frand(&s); tris[i].normals[k].z = 1;
      tris[i].tex_coords[k].x = frand(&s); tris[i].tex_coords[k].y = frand(&s);
    }
    tris[i].shader.data = &materials[i & 1];
    tris[i].shader.proc = token_shader;
  }
  for (int i = 0; i < n / 4; i++) tris[n - 1 - i] = tris[i];                  /* byte-identical duplicates */
  for (int i = 0; i < n; i++) {
    moved[i] = tris[i];
    for (int k = 0; k < 3; k++) {
      moved[i].positions[k].x += frand(&s) * 0.1f;
      moved[i].positions[k].z -= frand(&s) * 0.1f;
      moved[i].tex_coords[k].y += frand(&s) * 0.1f;
    }
  }
  Scene scene;
  memset(&scene, 0, sizeof scene);
  Triangle_Slice src = { tris, n }, dst = { moved, n };
  Allocator none = { 0, 0 };
  if (sah) scene_init_sah(&scene, src, none); else scene_init(&scene, src, none);
  CHECK(scene.triangles.x[0] != NULL);

  size_t bytes = 0, bytes_moved = 0;
  byte *built = snapshot(&scene, &bytes);
  i32 *map = (i32 *)malloc((size_t)(n + 1) * sizeof *map);
  for (int i = 0; i <= n; i++) map[i] = -7;
  CHECK(rt_scene_slot_map(&scene, src, map) == n);
  CHECK(map[n] == -7);
  CHECK(rt_scene_slot_map(&scene, dst, map) == -1);                           /* the moved triangles have no slots yet */
  for (int i = 1; i < n; i++)
    if (memcmp(&tris[i], &tris[0], sizeof tris[0]) == 0) CHECK(map[i] > map[0]);

  CHECK(scene_refit(&scene, src, map) == 0);                                  /* the identity */
  CHECK(same(&scene, built, bytes));
  CHECK(scene_refit(&scene, dst, map) == 0);
  CHECK(!same(&scene, built, bytes));
  byte *after = snapshot(&scene, &bytes_moved);
  i32 *again = (i32 *)malloc((size_t)(n + 1) * sizeof *again);
  CHECK(rt_scene_slot_map(&scene, dst, again) == n);                          /* every triangle is still in its slot */
  if (n / 4 == 0) CHECK(memcmp(again, map, (size_t)n * sizeof *map) == 0);

  /* the rejections: nothing is written */
  Triangle_Slice fewer = { moved, n - 1 }, more = { moved, n + 1 };
  moved[n] = moved[0];
  map[n] = map[0];
  CHECK(scene_refit(&scene, fewer, map) == -1);
  CHECK(scene_refit(&scene, more, map) == -1);
  i32 keep = map[n - 1];
  map[n - 1] = -1;                    CHECK(scene_refit(&scene, dst, map) == -1);
  map[n - 1] = scene.triangles.len;   CHECK(scene_refit(&scene, dst, map) == -1);
  map[n - 1] = INT32_MAX;             CHECK(scene_refit(&scene, dst, map) == -1);
  if (n > 1) { map[n - 1] = map[0];   CHECK(scene_refit(&scene, dst, map) == -1); }
  map[n - 1] = keep;
  moved[n / 2].shader.data = &materials[(n / 2 + 1) & 1];
  CHECK(scene_refit(&scene, dst, map) == -1);
  moved[n / 2].shader.data = tris[n / 2].shader.data;
  CHECK(scene_refit(NULL, dst, map) == -1);
  CHECK(same(&scene, after, bytes_moved));

  CHECK(scene_refit(&scene, src, map) == 0);                                  /* and back */
  CHECK(same(&scene, built, bytes));

  free(built); free(after); free(map); free(again); free(tris); free(moved);
  rt_scene_free(&scene);
  printf("refit n=%d %s ok\n", n, sah ? "sah" : "reference");
  return 0;
}

int main(void) {
  static int const sizes[4] = {1, 9, 65, 513};
  for (int sah = 0; sah < 2; sah++)
    for (int k = 0; k < 4; k++)
      if (run_case(sizes[k], sah, 77u + (uint32_t)sizes[k])) return 1;
  return 0;
}
