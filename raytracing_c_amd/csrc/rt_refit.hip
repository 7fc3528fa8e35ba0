// rt_refit.hip -- scene_refit() on the GPU, in place on the device copy of a scene (include/rt_hip.h: scene_refit_gpu).
//
// A deformation keeps every triangle in its slot, so nothing is sorted and nothing is planned: the implicit layout fixes
// which slots a leaf group holds and which eight children a node has.  Two kernels:
//
//   refit_leaf_kernel    one lane per slot.  The eight lanes of a leaf group sit together, a wave of 64 is the eight
//                        children of ONE node of the last internal level.  The lane gathers its 112-byte source Triangle
//                        through source_of_slot (-1: a padding slot), computes the slot's record with the arithmetic of
//                        scene_init (rt_triangle_record.h) and writes -- the wave's stores cover one contiguous range
//                        each; the coordinate, leaf-tile and node stores are also coalesced per instruction, the two
//                        records are per-lane stores at a stride of 112 bytes --
//                          - the host-layout slot (nine SoA floats + Triangle_AOS) into a staging block that goes back to
//                            the host Scene in one copy,
//                          - the device copy's 28-float shading record (the material id in r[3] stays: a refit keeps the
//                            materials) and its column of the 72-float leaf tile (a, b - a, c - a: plain fp32
//                            subtractions, as build_leaf_tile of rt_residency.cpp does).
//                        The lanes of a group reduce their padded bounds with cross-lane operations over the populated
//                        lanes; the wave writes the whole 192-byte BVH_Node of its parent straight into the copy's node
//                        array (BVH_Node as is: the host layout too) and a populated flag per group.  |edge component| is
//                        reduced within the wave and joins the scene's bound with ONE integer atomic max per wave on the
//                        bit pattern of the absolute value -- NaN patterns order above infinity, so a NaN sticks.
//   refit_levels_kernel  from the second-last internal level up to the root, one lane per (node, child): the union of the
//                        child node's populated boxes, and the child's populated flag.  A level of more than 512 lanes is
//                        one launch; the levels that fit one workgroup (the top three: 73 nodes) are ONE launch with
//                        barriers between the levels.  A refit is at most depth + 1 launches.
//
// min and max are exact and no box value is a zero whose sign could depend on the order (every value had EPSILON added or
// subtracted), so any reduction order gives scene_refit's boxes -- for numbers; a soup with a NaN position is refitted by
// scene_refit itself (rt_extras.cpp).  "Populated" is a flag per child, never a test for an all-zero box.
//
// Built with the flags of rt_build.hip (-ffp-contract=off).

#include <hip/hip_runtime.h>

#include "rt_triangle_record.h"

namespace {

constexpr int kLeafBlock = 256;       // four waves: four nodes of the last internal level
constexpr int kLevelBlock = 512;      // the lanes of level 2: 64 nodes x 8 children

__device__ inline float min_f(float a, float b) { return b < a ? b : a; }
__device__ inline float max_f(float a, float b) { return b > a ? b : a; }

__global__ __launch_bounds__(kLeafBlock) void refit_leaf_kernel(int len, int depth, int n_internal, const Triangle *src,
                                                                 const int *source_of_slot, float *block, float *nodes, float *leaves,
                                                                 float *tris, unsigned char *populated, unsigned int *max_edge_bits) {
  const int slot = blockIdx.x * kLeafBlock + threadIdx.x;
  const bool in_range = slot < len;                  // (a depth-0 scene has 8 slots: the other lanes only take part in the shuffles)
  const int s = in_range ? source_of_slot[slot] : -1;
  const bool has = s >= 0;

  Triangle t;
  Triangle_AOS aos;
  memset(&t, 0, sizeof t);
  memset(&aos, 0, sizeof aos);
  float lo[3] = {RT_INF, RT_INF, RT_INF}, hi[3] = {-RT_INF, -RT_INF, -RT_INF};
  if (has) {
    t = src[s];
    rt_triangle_record(&t, &aos);
    rt_triangle_bounds(&t, lo, hi);
  }
  unsigned int edge_bits = 0;
  if (in_range) {
    rt_triangle_coordinates(&t, block, len, slot);                                  // zeros for a padding slot
    reinterpret_cast<Triangle_AOS *>(block + (size_t)len * 9)[slot] = aos;
    // the device copy's shading record (build_tri_record of rt_residency.cpp) without r[3], the material id
    float *r = tris + (size_t)slot * 28;
    r[0] = aos.normal.x;    r[1] = aos.normal.y;    r[2] = aos.normal.z;
    r[4] = aos.normal_a.x;  r[5] = aos.normal_a.y;  r[6] = aos.normal_a.z;  r[7] = aos.tex_coords_a.x;
    r[8] = aos.normal_b.x;  r[9] = aos.normal_b.y;  r[10] = aos.normal_b.z; r[11] = aos.tex_coords_a.y;
    r[12] = aos.normal_c.x; r[13] = aos.normal_c.y; r[14] = aos.normal_c.z; r[15] = aos.tex_coords_b.x;
    r[16] = aos.tangent.x;  r[17] = aos.tangent.y;  r[18] = aos.tangent.z;  r[19] = aos.tex_coords_b.y;
    r[20] = aos.bitangent.x; r[21] = aos.bitangent.y; r[22] = aos.bitangent.z; r[23] = aos.tex_coords_c.x;
    r[24] = aos.tex_coords_c.y; r[25] = 0.0f; r[26] = 0.0f; r[27] = 0.0f;
    // its column of the leaf tile: 9 rows x 8 (build_leaf_tile)
    float *l = leaves + (size_t)(slot >> 3) * 72 + (slot & 7);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      const float a = t.positions[0].data[ax];
      const float e1 = t.positions[1].data[ax] - a, e2 = t.positions[2].data[ax] - a;
      l[(3 * ax + 0) * 8] = a;
      l[(3 * ax + 1) * 8] = e1;
      l[(3 * ax + 2) * 8] = e2;
      const unsigned int b1 = rt_f2u(e1) & 0x7fffffffu, b2 = rt_f2u(e2) & 0x7fffffffu;
      edge_bits = b1 > edge_bits ? b1 : edge_bits;
      edge_bits = b2 > edge_bits ? b2 : edge_bits;
    }
  }

  // the scene's edge bound: one atomic per wave
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned int o = (unsigned int)__shfl_xor((int)edge_bits, m);
    edge_bits = o > edge_bits ? o : edge_bits;
  }
  const int lane = threadIdx.x & 63;
  if (lane == 0 && edge_bits != 0) atomicMax(max_edge_bits, edge_bits);

  if (depth == 0) return;                            // no nodes: the render path tests the one group directly

  // the bounds of each leaf group: over its populated lanes (the others hold the identities)
#pragma unroll
  for (int m = 1; m <= 4; m <<= 1) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      lo[ax] = min_f(lo[ax], __shfl_xor(lo[ax], m));
      hi[ax] = max_f(hi[ax], __shfl_xor(hi[ax], m));
    }
  }
  const unsigned long long has_mask = __ballot(has);
  // lane 8 * row + child writes float `row` of child `child` of the wave's node: min x, y, z, max x, y, z (rows of 8)
  const int child = lane & 7, row = lane >> 3;
  float v[6];
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    v[ax] = __shfl(lo[ax], child * 8);
    v[3 + ax] = __shfl(hi[ax], child * 8);
  }
  const bool child_has = ((has_mask >> (child * 8)) & 0xffull) != 0;
  const int wave = slot >> 6;                                       // = position of the node in the last internal level
  const int node = n_internal - (len >> 6) + wave;                  // that level holds len / 64 nodes, the last of the array
  if (in_range && row < 6) {
    float out = v[0];
#pragma unroll
    for (int k = 1; k < 6; k++) out = row == k ? v[k] : out;
    nodes[(size_t)node * 48 + lane] = child_has ? out : 0.0f;
  }
  if (in_range && row == 6) populated[n_internal + wave * 8 + child] = child_has ? 1 : 0;     // indexed like the implicit tree
}

// Levels level_hi .. level_lo (level_hi >= level_lo; level L holds 8^L nodes, the first of them node (8^L - 1) / 7).  More than
// one level only in a launch of ONE workgroup.
__global__ __launch_bounds__(kLevelBlock) void refit_levels_kernel(int level_hi, int level_lo, float *nodes, unsigned char *populated) {
  for (int level = level_hi; level >= level_lo; level--) {
    const int n_lanes = 8 << (3 * level);                           // nodes of the level x 8 children
    const int first = ((1 << (3 * level)) - 1) / 7;
    for (int i = blockIdx.x * kLevelBlock + threadIdx.x; i < n_lanes; i += gridDim.x * kLevelBlock) {
      const int node = first + (i >> 3), c = i & 7;
      const int m = node * 8 + 1 + c;                               // the child node
      const float *b = nodes + (size_t)m * 48;
      float lo[3] = {RT_INF, RT_INF, RT_INF}, hi[3] = {-RT_INF, -RT_INF, -RT_INF};
      bool any = false;
      for (int q = 0; q < 8; q++) {
        if (!populated[m * 8 + 1 + q]) continue;
        any = true;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
          lo[ax] = min_f(lo[ax], b[ax * 8 + q]);
          hi[ax] = max_f(hi[ax], b[(3 + ax) * 8 + q]);
        }
      }
      float *out = nodes + (size_t)node * 48 + c;
#pragma unroll
      for (int ax = 0; ax < 3; ax++) {
        out[ax * 8] = any ? lo[ax] : 0.0f;
        out[(3 + ax) * 8] = any ? hi[ax] : 0.0f;
      }
      populated[m] = any ? 1 : 0;
    }
    if (level > level_lo) {                                         // (one workgroup: the level above reads what this one wrote)
      __threadfence();
      __syncthreads();
    }
  }
}

}  // namespace

// Enqueues the refit of a device copy on `stream`: len slots (8^(depth + 1)), n_internal nodes.  d_src: the source triangles;
// d_source_of_slot: len entries; d_block: the staging block (TRIANGLES_ALLOCATION_SIZE(len) bytes); d_nodes / d_leaves / d_tris:
// the copy's arrays; d_populated: n_internal + len / 8 bytes; d_max_edge_bits: one word, zero on entry.  Returns a hipError_t.
extern "C" int rt_launch_refit(int len, int depth, int n_internal, const void *d_src, const int *d_source_of_slot, float *d_block,
                               float *d_nodes, float *d_leaves, float *d_tris, unsigned char *d_populated,
                               unsigned int *d_max_edge_bits, hipStream_t stream) {
  hipLaunchKernelGGL(refit_leaf_kernel, dim3((unsigned)((len + kLeafBlock - 1) / kLeafBlock)), dim3(kLeafBlock), 0, stream, len, depth,
                     n_internal, (const Triangle *)d_src, d_source_of_slot, d_block, d_nodes, d_leaves, d_tris, d_populated,
                     d_max_edge_bits);
  int level = depth - 2;                                            // the leaf kernel wrote level depth - 1
  for (; level > 2; level--) {
    const int n_lanes = 8 << (3 * level);
    hipLaunchKernelGGL(refit_levels_kernel, dim3((unsigned)(n_lanes / kLevelBlock)), dim3(kLevelBlock), 0, stream, level, level,
                       d_nodes, d_populated);
  }
  if (level >= 0)
    hipLaunchKernelGGL(refit_levels_kernel, dim3(1), dim3(kLevelBlock), 0, stream, level, 0, d_nodes, d_populated);
  return (int)hipGetLastError();
}
