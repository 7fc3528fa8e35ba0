/* rt_rand_unit_vec3 / rt_sh9_basis / rt_accum_quantize_signed (include/rt_math.h) on the command line's values, for
 * tests/_probes.py and tests/test_probes_cpu.py:
 *   "s <seed, hex> <probe> <sample>"  prints one line: the bits of the direction (3 words), the RNG state after it, the bits of
 *                                     the nine basis values at that direction -- state = rt_path_seed(seed, probe, sample)
 *   "p <float bits, hex> <float bits, hex>"  prints rt_accum_quantize_signed(a * b), one f32 multiply
 *   "y <x bits> <y bits> <z bits>"    prints the bits of the nine basis values at the direction given */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_math.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc;) {
    if (strcmp(argv[i], "s") == 0 && i + 3 < argc) {
      uint32_t state = rt_path_seed((uint32_t)strtoul(argv[i + 1], NULL, 16), (uint32_t)strtoul(argv[i + 2], NULL, 10),
                                    (uint32_t)strtoul(argv[i + 3], NULL, 10));
      const rt_v3 d = rt_rand_unit_vec3(&state);
      float y[RT_SH9];
      rt_sh9_basis(d, y);
      printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32, rt_f2u(d.x), rt_f2u(d.y), rt_f2u(d.z), state);
      for (int k = 0; k < RT_SH9; k++) printf(" %08" PRIx32, rt_f2u(y[k]));
      printf("\n");
      i += 4;
    } else if (strcmp(argv[i], "p") == 0 && i + 2 < argc) {
      const float a = rt_u2f((uint32_t)strtoul(argv[i + 1], NULL, 16)), b = rt_u2f((uint32_t)strtoul(argv[i + 2], NULL, 16));
      printf("%016" PRIx64 "\n", rt_accum_quantize_signed(a * b));
      i += 3;
    } else if (strcmp(argv[i], "y") == 0 && i + 3 < argc) {
      float y[RT_SH9];
      rt_sh9_basis(rt_v3_make(rt_u2f((uint32_t)strtoul(argv[i + 1], NULL, 16)), rt_u2f((uint32_t)strtoul(argv[i + 2], NULL, 16)),
                              rt_u2f((uint32_t)strtoul(argv[i + 3], NULL, 16))), y);
      for (int k = 0; k < RT_SH9; k++) printf("%s%08" PRIx32, k ? " " : "", rt_f2u(y[k]));
      printf("\n");
      i += 4;
    } else {
      return 2;
    }
  }
  return 0;
}
