/* rt_accum_quantize_signed / rt_accum_resolve_signed (include/rt_math.h) on the command line's values, for
 * tests/test_features_cpu.py: "q <float bits, hex>" prints the quantised value, "r <sum, hex> <samples>" the bits of the mean. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_math.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc;) {
    if (strcmp(argv[i], "q") == 0 && i + 1 < argc) {
      printf("%016" PRIx64 "\n", rt_accum_quantize_signed(rt_u2f((uint32_t)strtoul(argv[i + 1], NULL, 16))));
      i += 2;
    } else if (strcmp(argv[i], "r") == 0 && i + 2 < argc) {
      printf("%08" PRIx32 "\n", rt_f2u(rt_accum_resolve_signed(strtoull(argv[i + 1], NULL, 16), (uint32_t)strtoul(argv[i + 2], NULL, 10))));
      i += 3;
    } else {
      return 2;
    }
  }
  return 0;
}
