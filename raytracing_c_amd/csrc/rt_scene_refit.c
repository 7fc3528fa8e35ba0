/* rt_scene_refit.c -- same topology, new geometry: refit the BVH of a deformed mesh in place, on the host.
 *
 * A deformation keeps every triangle in its slot.  What changes is the slot's nine coordinates, its Triangle_AOS
 * record (face normal, tangent frame, vertex normals, UVs), the box of its leaf group and the boxes above: one
 * bottom-up pass over a tree whose shape the implicit layout fixes (include/rt_scene.h).  On the output of scene_init
 * and scene_init_sah a refit with unmoved triangles is the identity: a child box there IS min / max over the
 * populated slots below it (min and max are exact, and no sign of a zero survives the +- EPSILON), a slot is populated
 * when its Shader has a proc, and unpopulated children are all-zero boxes.
 *
 *   rt_scene_slot_map   which slot holds which source triangle, for a Scene from any builder or from a .scene file
 *   scene_refit         validate, write the slots, recompute the boxes
 *   rt_refit_check      the validation alone, with the inverse map: what scene_refit_gpu (rt_extras.cpp) runs before
 *                       it launches anything
 */
#include "rt_triangle_record.h"

#include <stdlib.h>
#include <string.h>

extern void rt_scene_invalidate(Scene const *scene) __attribute__((weak));
/* the error text of rt_last_error() (rt_host.cpp); absent where this file is linked on its own (tests/c/) */
extern void rt_error_message(char const *message) __attribute__((weak));

int rt_refit_check(Scene const *scene, Triangle_Slice src, i32 const *slot_of_source, i32 *source_of_slot)
  __attribute__((visibility("hidden")));

static int refit_fail(char const *message) {
  if (rt_error_message) rt_error_message(message);
  return -1;
}

/* ---- the slot map ---------------------------------------------------------------------------------- */

/* the builder-input Triangle that slot `s` holds (Triangle has no padding: 112 bytes, all of them fields) */
static void slot_source(Triangles const *T, isize s, Triangle *t) {
  for (int k = 0; k < 3; k++) {
    t->positions[k].x = T->x[k][s];
    t->positions[k].y = T->y[k][s];
    t->positions[k].z = T->z[k][s];
  }
  Triangle_AOS const *a = &T->aos[s];
  t->normals[0] = a->normal_a; t->normals[1] = a->normal_b; t->normals[2] = a->normal_c;
  t->tex_coords[0] = a->tex_coords_a; t->tex_coords[1] = a->tex_coords_b; t->tex_coords[2] = a->tex_coords_c;
  t->shader = a->shader;
}

static u64 triangle_hash(Triangle const *t) {
  u64 w[sizeof(Triangle) / 8], h = 0x9E3779B97F4A7C15ull;
  memcpy(w, t, sizeof w);
  for (size_t i = 0; i < sizeof w / sizeof w[0]; i++) {
    h ^= w[i];
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
  }
  return h;
}

/* A chained hash table of the populated slots, keyed by the bytes of the Triangle a slot holds.  The slots are entered
 * in descending order at the head of their chain, so every chain lists them in ASCENDING order; a source triangle takes
 * the first slot of its chain with its bytes and unlinks it.  The k-th of several identical source triangles so gets
 * the k-th identical slot, and a run of duplicates is never walked twice: expected O(n) in all. */
isize rt_scene_slot_map(Scene const *scene, Triangle_Slice src, i32 *slot_of_source) {
  if (!scene || !slot_of_source || src.len < 0 || (src.len > 0 && !src.data)) return -1;
  Triangles const *T = &scene->triangles;
  if (T->len < 0 || (T->len > 0 && (!T->x[0] || !T->aos))) return -1;
  isize populated = 0;
  for (isize s = 0; s < T->len; s++) populated += T->aos[s].shader.proc != NULL;
  if (populated != src.len) return -1;
  if (src.len == 0) return 0;

  size_t n_buckets = 16;
  while (n_buckets < (size_t)populated * 2) n_buckets *= 2;
  i32 *head = (i32 *)malloc(n_buckets * sizeof *head);
  i32 *next = (i32 *)malloc((size_t)T->len * sizeof *next);
  i32 *map  = (i32 *)malloc((size_t)src.len * sizeof *map);
  isize result = -1;
  if (head && next && map) {
    for (size_t b = 0; b < n_buckets; b++) head[b] = -1;
    for (isize s = T->len - 1; s >= 0; s--) {
      if (T->aos[s].shader.proc == NULL) continue;
      Triangle t;
      slot_source(T, s, &t);
      size_t b = (size_t)triangle_hash(&t) & (n_buckets - 1);
      next[s] = head[b];
      head[b] = (i32)s;
    }
    isize i = 0;
    for (; i < src.len; i++) {
      size_t b = (size_t)triangle_hash(&src.data[i]) & (n_buckets - 1);
      i32 *link = &head[b];
      while (*link >= 0) {
        Triangle t;
        slot_source(T, *link, &t);
        if (memcmp(&t, &src.data[i], sizeof t) == 0) break;
        link = &next[*link];
      }
      if (*link < 0) break;                     /* no slot of its own */
      map[i] = *link;
      *link = next[*link];
    }
    if (i == src.len) {                         /* as many slots as triangles, each taken once: one to one and onto */
      memcpy(slot_of_source, map, (size_t)src.len * sizeof *map);
      result = src.len;
    }
  }
  free(head); free(next); free(map);
  return result;
}

/* ---- validation ------------------------------------------------------------------------------------ */

/* 0 when `scene` can take `src` through `slot_of_source`; -1 and a message otherwise.  Nothing of the scene is written.
 * source_of_slot (optional, scene->triangles.len entries): the inverse map, -1 for the padding slots. */
int rt_refit_check(Scene const *scene, Triangle_Slice src, i32 const *slot_of_source, i32 *source_of_slot) {
  if (!scene) return refit_fail("scene_refit: scene is NULL");
  if (src.len < 0 || (src.len > 0 && (!src.data || !slot_of_source))) return refit_fail("scene_refit: bad triangle slice or map");
  Triangles const *T = &scene->triangles;
  BVH const *bvh = &scene->bvh;
  isize const len = T->len;
  if (len <= 0 || !T->x[0] || !T->aos) return refit_fail("scene_refit: the scene has no triangle block");
  if (bvh->depth < 0 || bvh->depth > 9 /* (8^(depth + 1) slots in an i32) */ || len != bvh_n_leaf_nodes(bvh->depth) * RT_BVH_WIDTH ||
      bvh->nodes.len != bvh_n_internal_nodes(bvh->depth) || bvh->last_row_offset != bvh->nodes.len ||
      (bvh->nodes.len > 0 && !bvh->nodes.data))
    return refit_fail("scene_refit: the scene is not a complete 8-ary tree over its triangle block");
  for (int k = 0; k < 3; k++)                    /* one allocation that starts at x[0] (scene.c:84-98) */
    if (T->x[k] != T->x[0] + len * (0 + k) || T->y[k] != T->x[0] + len * (3 + k) || T->z[k] != T->x[0] + len * (6 + k))
      return refit_fail("scene_refit: the coordinate arrays are not one block");
  if ((void const *)T->aos != (void const *)(T->x[0] + len * 9)) return refit_fail("scene_refit: the coordinate arrays are not one block");

  isize populated = 0;
  for (isize s = 0; s < len; s++) populated += T->aos[s].shader.proc != NULL;
  if (populated != src.len) return refit_fail("scene_refit: src.len differs from the number of populated slots");

  i32 *inverse = source_of_slot ? source_of_slot : (i32 *)malloc((size_t)len * sizeof *inverse);
  if (!inverse) return refit_fail("scene_refit: out of memory");
  for (isize s = 0; s < len; s++) inverse[s] = -1;
  char const *why = NULL;
  for (isize i = 0; i < src.len && !why; i++) {
    i32 s = slot_of_source[i];
    if (s < 0 || s >= len) why = "scene_refit: the map names a slot outside the triangle block";
    else if (T->aos[s].shader.proc == NULL) why = "scene_refit: the map names a padding slot";
    else if (inverse[s] >= 0) why = "scene_refit: the map names a slot twice";
    else if (memcmp(&src.data[i].shader, &T->aos[s].shader, sizeof(Shader)) != 0)
      why = "scene_refit: a triangle's Shader differs from its slot's (a refit keeps the materials; rebuild instead)";
    else inverse[s] = (i32)i;
  }
  if (!source_of_slot) free(inverse);
  return why ? refit_fail(why) : 0;
}

/* ---- the refit ------------------------------------------------------------------------------------- */

typedef struct { f32 lo[3], hi[3]; } Box;

static void box_store(BVH_Node *node, int child, Box const *b) {
  node->min_x[child] = b->lo[0]; node->min_y[child] = b->lo[1]; node->min_z[child] = b->lo[2];
  node->max_x[child] = b->hi[0]; node->max_y[child] = b->hi[1]; node->max_z[child] = b->hi[2];
}

static void box_load(BVH_Node const *node, int child, Box *b) {
  b->lo[0] = node->min_x[child]; b->lo[1] = node->min_y[child]; b->lo[2] = node->min_z[child];
  b->hi[0] = node->max_x[child]; b->hi[1] = node->max_y[child]; b->hi[2] = node->max_z[child];
}

/* aabb_triangle_slice / aabb_grow of rt_scene_build.c: the first box as it is, every later one with `<` and `>` */
static void box_grow(Box *a, Box const *t, bool first) {
  if (first) { *a = *t; return; }
  for (int ax = 0; ax < 3; ax++) {
    if (t->lo[ax] < a->lo[ax]) a->lo[ax] = t->lo[ax];
    if (t->hi[ax] > a->hi[ax]) a->hi[ax] = t->hi[ax];
  }
}

int scene_refit(Scene *scene, Triangle_Slice src, i32 const *slot_of_source) {
  if (rt_refit_check(scene, src, slot_of_source, NULL) != 0) return -1;
  Triangles *T = &scene->triangles;
  isize const depth = scene->bvh.depth, n_internal = scene->bvh.nodes.len, n_groups = T->len / RT_BVH_WIDTH;
  /* populated[c] for the children c of the level being written: a flag per child, never a test for an all-zero box */
  bool *populated = depth > 0 ? (bool *)malloc((size_t)n_groups) : NULL;
  if (depth > 0 && !populated) return refit_fail("scene_refit: out of memory");

  for (isize i = 0; i < src.len; i++) {
    rt_triangle_coordinates(&src.data[i], T->x[0], T->len, slot_of_source[i]);
    rt_triangle_record(&src.data[i], &T->aos[slot_of_source[i]]);
  }

  if (depth > 0) {
    BVH_Node *nodes = scene->bvh.nodes.data;
    /* the last internal level: child c of node j is leaf group 8j + 1 + c - last_row_offset; its box comes from the
     * populated slots of the group, in slot order */
    isize first = bvh_n_internal_nodes(depth - 1), count = bvh_n_leaf_nodes(depth - 1);
    for (isize j = first; j < first + count; j++) {
      BVH_Node node;
      memset(&node, 0, sizeof node);
      for (int c = 0; c < RT_BVH_WIDTH; c++) {
        isize g = j * RT_BVH_WIDTH + 1 + c - n_internal;
        Box box = {{0, 0, 0}, {0, 0, 0}};
        isize n = 0;
        for (isize s = g * RT_BVH_WIDTH; s < (g + 1) * RT_BVH_WIDTH; s++) {
          if (T->aos[s].shader.proc == NULL) continue;
          Triangle t;
          Box b;
          slot_source(T, s, &t);
          rt_triangle_bounds(&t, b.lo, b.hi);
          box_grow(&box, &b, n == 0);
          n += 1;
        }
        populated[g] = n > 0;
        if (n > 0) box_store(&node, c, &box);
      }
      nodes[j] = node;
    }
    /* every level above: the union over the populated children of the child node, in child order.  populated[] is
     * indexed by the position in the level below and rewritten in place for this level: entries 8k .. 8k + 7 are all
     * read before entry k <= 8k is written */
    for (isize level = depth - 2; level >= 0; level--) {
      first = bvh_n_internal_nodes(level); count = bvh_n_leaf_nodes(level);
      isize below = bvh_n_internal_nodes(level + 1);
      for (isize j = first; j < first + count; j++) {
        BVH_Node node;
        memset(&node, 0, sizeof node);
        for (int c = 0; c < RT_BVH_WIDTH; c++) {
          isize m = j * RT_BVH_WIDTH + 1 + c;                 /* the child node; its children are below[(m - below) * 8 ..] */
          Box box = {{0, 0, 0}, {0, 0, 0}};
          isize n = 0;
          for (int q = 0; q < RT_BVH_WIDTH; q++) {
            if (!populated[(m - below) * RT_BVH_WIDTH + q]) continue;
            Box b;
            box_load(&nodes[m], q, &b);
            box_grow(&box, &b, n == 0);
            n += 1;
          }
          populated[m - below] = n > 0;
          if (n > 0) box_store(&node, c, &box);
        }
        nodes[j] = node;
      }
    }
  }
  free(populated);
  if (rt_scene_invalidate) rt_scene_invalidate(scene);       /* the device copies hold the old geometry */
  return 0;
}
