/* The HDR lightmap's sampler and product (include/rt_hip.h, "HDR lightmaps") over include/rt_math.h, for tests/_lightmap_hdr.py.
 * Reads whitespace-separated requests from stdin, prints one line per request:
 *   "d <seed, hex> <texel> <sample> <nx bits> <ny bits> <nz bits>"
 *        state = rt_path_seed(seed, texel, sample); directions by rt_rand_unit_vec3 until c = dot(d, normal) > 0, at most 64 tries.
 *        prints: the bits of the last direction tried (3 words), the bits of its c, the state behind it, the try count, 1 if accepted
 *   "q <float bits, hex> <float bits, hex>"   prints rt_accum_quantize(a * b), one f32 multiply */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_math.h"

int main(void) {
  char op[8];
  while (scanf("%7s", op) == 1) {
    if (strcmp(op, "d") == 0) {
      uint32_t seed, texel, sample, nb[3];
      if (scanf("%" SCNx32 " %" SCNu32 " %" SCNu32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &seed, &texel, &sample, &nb[0], &nb[1], &nb[2]) != 6)
        return 2;
      const rt_v3 normal = rt_v3_make(rt_u2f(nb[0]), rt_u2f(nb[1]), rt_u2f(nb[2]));
      uint32_t state = rt_path_seed(seed, texel, sample);
      rt_v3 d = rt_v3_make(0, 0, 0);
      float c = 0.0f;
      int tries = 0, accepted = 0;
      while (tries < 64 && !accepted) {
        d = rt_rand_unit_vec3(&state);
        c = rt_v3_dot(d, normal);
        tries++;
        accepted = c > 0.0f;
      }
      printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %d %d\n", rt_f2u(d.x), rt_f2u(d.y), rt_f2u(d.z),
             rt_f2u(c), state, tries, accepted);
    } else if (strcmp(op, "q") == 0) {
      uint32_t a, b;
      if (scanf("%" SCNx32 " %" SCNx32, &a, &b) != 2) return 2;
      printf("%016" PRIx64 "\n", rt_accum_quantize(rt_u2f(a) * rt_u2f(b)));
    } else {
      return 2;
    }
  }
  return 0;
}
